"""
The convolution family under exact-size, poisoned, guarded memory (tests/hostile_mem.py): right numbers at wrong addresses
must not pass.

Part A runs the suite's existing runners twice -- plainly, and with ops._workspace replaced by hostile workspaces (a view of
exactly the bytes the library declares, every byte 0xFF = NaN, a guard band of the object's own size on both sides, poisoned
again at every request).  The hostile run meets the runner's oracle bars, equals the plain run bit for bit in every output,
and leaves every guard intact: no launch overruns dlwpcs_conv_workspace_bytes / dlwpcs_wgrad_batch_sizes, none reads a
workspace cell that no launch of the same call (or of the documented predecessor call: REUSE_DZ, DEFER_RING0, DEFER_REDUCE)
wrote.

Part B calls the C ABI with the OUTPUT tensors carved from the arena as well: after each call the outputs meet conv_check's
bars against the fp64 oracle (EPS = 2^-8 scaling for bf16, 1e-5 for fp32, 2e-5 for weight gradients; TOL = 2e-5 of
test_gpu_wgrad_batch.py), no output element is still poison, and all guards are intact -- the ragged-tile epilogues, the
scalar channel stores, the pooled second output, the direct-store data gradients, the ring fix-ups and the reductions into a
flat gradient buffer store nowhere else.  Every call is a documented, supported use, runs eagerly on the current stream, and
nothing is skipped.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import conv_check
import hostile_mem as hm
import test_gpu_conv_coverage as cov
import test_gpu_wgrad_batch as wb
from oracle import cs_oracle as orc

pytestmark = pytest.mark.gpu

EPS = conv_check.EPS
ALPHA, VMAX = conv_check.ALPHA, conv_check.VMAX


def _dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def _module_arena():
    """one 2 GiB arena for the module, given back when its last test is done"""
    a = hm.Arena(2 << 30, _dev())
    yield a
    torch.cuda.synchronize()
    a.buf = None
    torch.cuda.empty_cache()


@pytest.fixture
def arena(_module_arena):
    """the module's arena, poison again and empty at the start of every test"""
    torch.cuda.synchronize()
    _module_arena.reset()
    return _module_arena


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    assert torch.equal(a.contiguous().view(it), b.contiguous().view(it)), '%s: hostile run differs from the plain run' % (what,)


# ------------------------------------------------------------------------------------------------------------------ #
# Part A: the existing runners on hostile workspaces
# ------------------------------------------------------------------------------------------------------------------ #
def _n_out(c):
    B, N, C0, C1, Cout, k, halo = c.case[:7]
    No = N if halo else N - k + 1
    return B * No * No * Cout


def _select(cases):
    """for each distinct set of declared tags the case with the fewest output elements (the first of equals)"""
    best = {}
    for c in cases:
        key = frozenset(c.tags)
        if key not in best or _n_out(c) < _n_out(best[key]):
            best[key] = c
    return list(best.values())


SELECTED = _select(cov.CASES)


def test_selected_cases_cover_every_declared_tag():
    assert set().union(*[c.tags for c in SELECTED]) == set().union(*[c.tags for c in cov.CASES])


@pytest.mark.parametrize('c', SELECTED, ids=lambda c: c.name)
def test_fused_convolution_on_hostile_workspaces(c, arena, monkeypatch):
    ref = conv_check.reference(c.case, c.bf16)
    runs = []
    for hostile in (False, True):
        hw = hm.hostile_workspaces(monkeypatch, arena=arena) if hostile else None
        out = {}
        with conv_check.launched_tags() as tags:
            conv_check.check(c.case, c.bf16, device_mask=True, outputs=out, ref=ref, **c.kw)
        missing = sorted(set(c.tags) - tags)
        assert not missing, 'not launched: %s (launched: %s)' % (missing, sorted(tags))
        if hostile:
            hw.check()
            assert hw.requests, 'no workspace was asked for'
        runs.append(out)
    monkeypatch.undo()
    plain, host = runs
    assert sorted(plain) == sorted(host) and 'y' in plain
    for name in plain:
        _same_bits(plain[name], host[name], '%s of %s' % (name, c.name))


def _grads(lay):
    return [lay.dw[n] for n in sorted(lay.dw)] + [lay.db[n] for n in sorted(lay.db)]


def _wb_twice(make, arena, monkeypatch):
    """make() -> (layers, entries); ops.wgrad_batch on them plainly and on a hostile workspace"""
    from DLWP import ops
    runs = []
    for hostile in (False, True):
        hw = hm.hostile_workspaces(monkeypatch, arena=arena) if hostile else None
        lays, entries = make()
        for lay in lays:
            assert ops.wgrad_batch_supported(lay.d)
        ops.wgrad_batch(entries)
        torch.cuda.synchronize()
        if hostile:
            hw.check()
            assert [r for r, _ in hw.requests] == ['wgrad_batch']
        for lay in lays:
            lay.check()
        runs.append([g.cpu() for lay in lays for g in _grads(lay)])
    monkeypatch.undo()
    for i, (a, b) in enumerate(zip(*runs)):
        _same_bits(a, b, 'gradient tensor %d' % i)


@pytest.mark.parametrize('case', wb.CASES)
def test_batched_weight_gradient_on_a_hostile_workspace(case, arena, monkeypatch):
    def make():
        lay = wb.Layer(np.random.default_rng(abs(hash(case)) % (2 ** 31)), *case)
        return [lay], [lay.entry()]
    _wb_twice(make, arena, monkeypatch)


def test_batched_weight_gradient_layer_options_on_a_hostile_workspace(arena, monkeypatch):
    """the four layers of test_layer_options in one launch"""
    def make():
        rng = np.random.default_rng(5)
        lays = [wb.Layer(rng, 2, 12, 32, 0, 0, 32, 3, 1, flip=True, indep=True),
                wb.Layer(rng, 2, 12, 32, 0, 0, 64, 3, 1, flip=False, indep=False),
                wb.Layer(rng, 2, 12, 64, 0, 0, 64, 3, 1, flip=False, indep=True, bias=False),
                wb.Layer(rng, 3, 16, 8, 0, 0, 32, 3, 1, c0_valid=7)]
        return lays, [l.entry() for l in lays]
    _wb_twice(make, arena, monkeypatch)


@pytest.mark.parametrize('case', [(2, 48, 14, 0, 0, 32, 3, 1), (3, 16, 8, 0, 0, 32, 3, 1), (2, 24, 64, 0, 0, 64, 3, 1),
                                  (2, 12, 32, 0, 0, 64, 3, 1)])
def test_batched_weight_gradient_mask_on_load_on_a_hostile_workspace(case, arena, monkeypatch):
    """the cases of test_mask_on_load: the item carries y, the producers form dy * act'(y)"""
    from DLWP import _native as nat

    def make():
        rng = np.random.default_rng(abs(hash(case)) % (2 ** 31))
        lay = wb.Layer(rng, *case)
        y = wb._bf(rng.standard_normal(tuple(lay.dz.shape)) * 6.0)
        dy = lay.dz
        yf, gf = y.float().cpu().numpy(), dy.float().cpu().numpy()
        sl = np.where(yf < 0, np.float32(0.1), np.where((yf > 0) & (yf < 10.0), np.float32(1.0), np.float32(0.0)))
        lay.dz = torch.tensor(gf * sl).to(torch.bfloat16).to(_dev())        # what the reference sees
        d = nat.ConvDesc.from_buffer_copy(lay.d)
        d.act, d.alpha, d.vmax = nat.ACT_LEAKY_CLIP, 0.1, 10.0
        e = lay.entry()
        return [lay], [(d, e[1], e[2], dy, e[4], e[5], y)]
    _wb_twice(make, arena, monkeypatch)


@pytest.mark.parametrize('dtype,options', [('bfloat16', ''), ('bfloat16', 'dgrad_gather=0'), ('float32', ''),
                                           ('bfloat16', 'dgrad_gather=0,wgrad_batch=0')])
def test_whole_eager_step_on_hostile_workspaces(dtype, options, arena, monkeypatch):
    """`unet2`, base 32, 14 channels, N = 48, B = 2, eager: two training steps.  The one place where the ring, defer, batch and
    main roles interleave as in production; dgrad_gather=0 runs the padded-grid data gradients with folded ring fix-ups, wgrad_batch=0
    on top of it the per-layer weight gradients (REUSE_DZ pairs, deferred reductions)."""
    from DLWP.keras import backend
    from DLWP.model.cs_unet import build_cs_model
    dev = _dev()
    backend.set_device('cuda:0')
    N, C, B = 48, 14, 2
    rng = np.random.default_rng(7)
    adt = torch.bfloat16 if dtype == 'bfloat16' else torch.float32
    x = torch.tensor(rng.standard_normal((B, 6, N, N, C)), dtype=torch.float32, device=dev).to(adt)
    t = torch.tensor(rng.standard_normal((B, 6, N, N, C)), dtype=torch.float32, device=dev)
    w0, runs = None, []
    monkeypatch.setenv('DLWPCS_OPTIONS', options)
    for hostile in (False, True):
        hw = hm.hostile_workspaces(monkeypatch, arena=arena) if hostile else None
        backend.set_compute_dtype(dtype)
        try:
            np.random.seed(5)
            model = build_cs_model((6, N, N, C), C, 'unet2', base_filter_number=32)
        finally:
            backend.set_compute_dtype('float32')
        model.use_graphs = False
        model.compile(optimizer='adam', loss='mse', metrics=['mae'])
        if w0 is None:
            w0 = model.get_weights()
        model.set_weights(w0)
        stats = []
        for _ in range(2):
            stats.append(model.train_on_device_batch([x], [t]).clone())
        torch.cuda.synchronize()
        if hostile:
            hw.check()
            roles = set(r for r, _ in hw.requests)
            assert 'main' in roles, roles
            print('workspace roles of the step:', sorted(roles))
        moved = max(float(np.abs(a - b).max()) for a, b in zip(model.get_weights(), w0))
        assert moved > 0, 'two steps left the weights where they were'
        runs.append((model._flat_params.detach().cpu().clone(), [s.cpu() for s in stats]))
    monkeypatch.undo()
    (p_plain, s_plain), (p_host, s_host) = runs
    assert torch.isfinite(p_host).all() and all(torch.isfinite(s).all() for s in s_host)
    _same_bits(p_plain, p_host, 'flat parameters after two steps')
    for i, (a, b) in enumerate(zip(s_plain, s_host)):
        _same_bits(a, b, 'statistics of step %d' % i)



def test_two_ring_nodes_with_deferred_reductions_keep_their_partial_sums():
    """What the hostile step with dgrad_gather=0,wgrad_batch=0 found, in plain memory: both ring nodes of a `unet2` were given the
    role 'ring0' (the pooling adjoint takes its entry out of ops._pending_ring), and with the reduction deferred the second node's
    launches overwrote the partial sums the first node's reduce item still pointed to -- from the second step on, once the
    buffer no longer grew.  Folding the ring fix-ups or not must give the same parameters, bit for bit, as it does with the
    batched weight gradient (test_gpu_premask.py)."""
    from DLWP.keras import backend
    from DLWP.model.cs_unet import build_cs_model
    dev = _dev()
    backend.set_device('cuda:0')
    N, C, B = 48, 14, 2
    rng = np.random.default_rng(7)
    x = torch.tensor(rng.standard_normal((B, 6, N, N, C)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    t = torch.tensor(rng.standard_normal((B, 6, N, N, C)), dtype=torch.float32, device=dev)
    w0, out = None, []
    try:
        for fold in ('0', '1'):
            os.environ['DLWPCS_OPTIONS'] = 'dgrad_gather=0,wgrad_batch=0,fold_ring=' + fold
            backend.set_compute_dtype('bfloat16')
            try:
                np.random.seed(5)
                model = build_cs_model((6, N, N, C), C, 'unet2', base_filter_number=32)
            finally:
                backend.set_compute_dtype('float32')
            model.use_graphs = False
            model.compile(optimizer='adam', loss='mse', metrics=['mae'])
            if w0 is None:
                w0 = model.get_weights()
            model.set_weights(w0)
            assert len(model._defer_ring) == 2 and model.fold_ring == (fold == '1')
            for _ in range(3):
                stats = model.train_on_device_batch([x], [t])
            torch.cuda.synchronize()
            out.append((model._flat_params.detach().cpu().clone(), stats.cpu().clone()))
    finally:
        os.environ.pop('DLWPCS_OPTIONS', None)
    _same_bits(out[0][0], out[1][0], 'parameters with and without the folded ring fix-ups')
    _same_bits(out[0][1], out[1][1], 'statistics with and without the folded ring fix-ups')


# ------------------------------------------------------------------------------------------------------------------ #
# Part B: outputs under guard through the C ABI
# ------------------------------------------------------------------------------------------------------------------ #
def _desc(case, bf16, flags=0, c0_valid=0, act=None):
    from DLWP import _native as nat
    B, N, C0, C1, Cout, k, halo, up0, flip, indep, a = case
    a = a if act is None else act
    return nat.ConvDesc(B=B, N=N, C0=C0, C1=C1, Cout=Cout, ksize=k, halo=int(halo), up0=int(up0), flip_north_pole=int(flip),
                        act=nat.ACT_LEAKY_CLIP if a else nat.ACT_NONE, alpha=ALPHA if a else 0., vmax=VMAX if a else 0.,
                        dtype=nat.BF16 if bf16 else nat.F32, flags=flags, c0_valid=c0_valid)


class _Inputs(object):
    """device copies of a reference's inputs (plain allocations: only outputs and workspaces are hostile)"""

    def __init__(self, ref):
        dev = _dev()
        self.adt = torch.bfloat16 if ref.bf16 else torch.float32
        put = lambda a: None if a is None else torch.tensor(a, dtype=torch.float32).to(self.adt).to(dev)
        self.x0, self.x1, self.gy = put(ref.x0), put(ref.x1), put(ref.gy)
        self.w = {n: (None if v is None else torch.tensor(v, device=dev)) for n, v in ref.w.items()}
        self.b = {n: (None if v is None else torch.tensor(v, device=dev)) for n, v in ref.b.items()}

    def wargs(self):
        from DLWP._native import ptr
        return tuple(ptr(self.w[n]) for n in ('eq', 'pol', 'np')) + tuple(ptr(self.b[n]) for n in ('eq', 'pol', 'np'))


def _np64(t):
    return t.detach().to(torch.float64).cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def _rel(a, ref, floor=0.0):
    a, ref = _np64(a), _np64(ref)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    den = max(np.abs(ref).max(), floor)
    return np.abs(a - ref).max() / (den if den > 0 else 1.0)


def _settle(arena, outputs, what):
    """after a call: all guards intact, no output element still poison, every output within its bar
    outputs: [(name, device tensor, fp64 reference | None, bar, floor)]"""
    arena.assert_guards()
    for name, t, ref, bar, floor in outputs:
        left = int(hm.is_poison(t).sum())
        assert left == 0, '%s of %s: %d of %d elements were never written' % (name, what, left, t.numel())
        if ref is not None:
            e = _rel(t, ref, floor)
            print('%s %s: %.3g (bar %.3g)' % (what, name, e, bar))
            assert e <= bar, '%s of %s: %.3g > %.3g' % (name, what, e, bar)


def _ws(arena, d):
    from DLWP import _native as nat
    nbytes = nat.lib().dlwpcs_conv_workspace_bytes(ctypes.byref(d))
    return arena.carve(nbytes, name='workspace'), nbytes


def _case(B, N, C0, C1, Cout, k=3, halo=True, up0=False, flip=True, indep=False, act=True):
    return (B, N, C0, C1, Cout, k, halo, up0, flip, indep, act)


def _fwd(arena, case, bf16, c0_valid=0, flags=0, pool=False, what='conv_fwd'):
    """dlwpcs_conv_fwd / dlwpcs_conv_fwd_pool with y (and the pooled y) under guard -> (ref, inputs, y, y_pooled)"""
    from DLWP import _native as nat
    B, N, C0, C1, Cout, k, halo, up0, flip, indep, act = case
    ref = conv_check.reference(case, bf16, c0_valid)
    inp = _Inputs(ref)
    d = _desc(case, bf16, flags, c0_valid)
    rows = (Cout + 7) // 8 * 8 if flags & nat.CONV_OUT_PADDED else Cout
    y = arena.tensor((B, 6, ref.No, ref.No, rows), inp.adt, 'y')
    yp = arena.tensor((B, 6, ref.No // 2, ref.No // 2, Cout), inp.adt, 'pooled y') if pool else None
    ws, nbytes = _ws(arena, d)
    table = nat.halo_tables(N, 1, _dev())[0] if halo else None
    lib = nat.lib()
    if pool:
        nat.check(lib.dlwpcs_conv_fwd_pool(ctypes.byref(d), nat.ptr(inp.x0), nat.ptr(inp.x1), *inp.wargs(), nat.ptr(y), nat.ptr(yp),
                                           nat.ptr(table), nat.ptr(ws), nbytes, nat.stream_ptr()), 'conv_fwd_pool')
    else:
        nat.check(lib.dlwpcs_conv_fwd(ctypes.byref(d), nat.ptr(inp.x0), nat.ptr(inp.x1), *inp.wargs(), nat.ptr(y), nat.ptr(table),
                                      nat.ptr(ws), nbytes, nat.stream_ptr()), 'conv_fwd')
    yref = ref.yref.detach().numpy()
    outs = [('y', y[..., :Cout], yref, EPS if bf16 else 1e-5, 0.0)]
    if rows > Cout:
        outs.append(('padding channels', y[..., Cout:], None, 0.0, 0.0))
    if pool:
        # (conv_check: the device pools its fp32 results and rounds once -- 2 EPS of the pooled maximum)
        outs.append(('pooled y', yp, orc.avgpool_122(ref.yref).detach().numpy(), 2 * EPS if bf16 else 1e-5, 0.0))
    _settle(arena, outs, '%s %s %s' % (what, case, 'bf16' if bf16 else 'fp32'))
    return ref, inp, y, yp


FWD = [(_case(3, 10, 12, 0, 8), 0),                # ragged tiles, 4-channel vectors
       (_case(2, 12, 7, 0, 5, indep=True), 0),     # scalar channel stores
       (_case(2, 24, 64, 64, 64, up0=True), 0),
       (_case(2, 48, 32, 0, 32), 0),
       (_case(2, 14, 16, 0, 16, halo=False), 0)]   # halo-free: 12 x 12 outputs


@pytest.mark.parametrize('bf16', [True, False], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('case,c0_valid', FWD)
def test_conv_fwd_stores_only_its_output(case, c0_valid, bf16, arena):
    _fwd(arena, case, bf16, c0_valid)


def test_conv_fwd_with_padded_input_channels_stores_only_its_output(arena):
    _fwd(arena, _case(3, 16, 8, 0, 32), True, c0_valid=7)


@pytest.mark.parametrize('Cout', [26, 14])
def test_conv_fwd_out_padded_writes_zeros_into_the_padding(Cout, arena):
    from DLWP import _native as nat
    case = _case(2, 16, 32, 0, Cout, k=1, halo=False, act=False)
    ref, inp, y, _ = _fwd(arena, case, True, flags=nat.CONV_OUT_PADDED)
    assert y.shape[-1] == (Cout + 7) // 8 * 8 and float(y[..., Cout:].float().abs().max()) == 0.0


@pytest.mark.parametrize('bf16', [True, False], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('shape', [(1, 48, 32, 32), (2, 24, 32, 64), (2, 20, 8, 24)])
def test_conv_fwd_pool_stores_only_its_two_outputs(shape, bf16, arena):
    """pooled by the epilogue (N = 48 / 24) or by the launch behind (N = 20): the same bits as dlwpcs_conv_fwd +
    dlwpcs_avgpool2_fwd either way, the pooled output under a guard of its own"""
    from DLWP import _native as nat
    B, N, C0, Cout = shape
    case = _case(B, N, C0, 0, Cout)
    ref, inp, y, yp = _fwd(arena, case, bf16, pool=True, what='conv_fwd_pool')
    _, _, y0, _ = _fwd(arena, case, bf16)
    p0 = arena.tensor(yp.shape, yp.dtype, 'pooled by avgpool2_fwd')
    nat.check(nat.lib().dlwpcs_avgpool2_fwd(nat.ptr(y0), nat.ptr(p0), B, N, Cout, nat.BF16 if bf16 else nat.F32, nat.stream_ptr()),
              'avgpool2_fwd')
    _settle(arena, [('pooled y', p0, None, 0.0, 0.0)], 'avgpool2_fwd')
    _same_bits(y.cpu(), y0.cpu(), 'y of conv_fwd_pool')
    _same_bits(yp.cpu(), p0.cpu(), 'pooled y of conv_fwd_pool')


# ---- data gradients ----
def _premask_cases():
    import test_gpu_premask as pm
    cases = [c for c in pm.CONV_CASES if c[1] <= 24] + [(2, 48, 32, 0, 0, 32, 3, 1, True, False)]
    return cases


def _bwd_data(arena, pc, bf16, masked, flags, c0_valid=0, ring=False):
    """dlwpcs_conv_bwd_data (masked = False: a layer without activation, dy = dz) or dlwpcs_conv_bwd_data_masked (the sources'
    masks as the premask case names them) with both source gradients under guard; ring: DLWPCS_CONV_DEFER_RING0 and the pooling
    adjoint dlwpcs_avgpool2_bwd_ring behind it"""
    from DLWP import _native as nat
    B, N, C0, C1, up0, Cout, k, halo, mask0, mask1 = pc
    case = _case(B, N, C0, C1, Cout, k=k, halo=bool(halo), up0=bool(up0), act=False)
    what = '%s %s flags %d %s' % ('bwd_data_masked' if masked else 'bwd_data', pc, flags, 'bf16' if bf16 else 'fp32')
    ref = conv_check.reference(case, bf16, c0_valid)
    inp = _Inputs(ref)
    ref.backward()
    d = _desc(case, bf16, flags | (nat.CONV_DEFER_RING0 if ring else 0), c0_valid)
    dev = _dev()
    lib = nat.lib()
    inv = nat.halo_tables(N, 1, dev)[1] if halo else None
    if flags & nat.CONV_DGRAD_GATHER:
        assert nat.dgrad_gather_ready(N, 1, dev)
    g0 = arena.tensor(inp.x0.shape, inp.adt, 'dsrc0')
    g1 = arena.tensor(inp.x1.shape, inp.adt, 'dsrc1') if C1 else None
    ws, nbytes = _ws(arena, d)
    m0 = inp.x0 if (masked and mask0) else None
    m1 = inp.x1 if (masked and mask1 and C1) else None
    if masked:
        nat.check(lib.dlwpcs_conv_bwd_data_masked(ctypes.byref(d), nat.ptr(inp.gy), nat.ptr(inp.w['eq']), nat.ptr(inp.w['pol']), 0,
                                                  nat.ptr(g0), nat.ptr(g1), nat.ptr(m0), nat.ptr(m1), ALPHA, VMAX, nat.ptr(inv),
                                                  nat.ptr(ws), nbytes, nat.stream_ptr()), 'conv_bwd_data_masked')
    else:
        nat.check(lib.dlwpcs_conv_bwd_data(ctypes.byref(d), nat.ptr(inp.gy), 0, nat.ptr(inp.w['eq']), nat.ptr(inp.w['pol']), 0,
                                           nat.ptr(g0), nat.ptr(g1), nat.ptr(inv), nat.ptr(ws), nbytes, nat.stream_ptr()),
                  'conv_bwd_data')
    tol = ((5 if up0 else 3) * EPS) if bf16 else 1e-5
    r0 = ref.t0.grad.numpy() * (conv_check._slope(ref.x0) if m0 is not None else 1.0)
    outs = []
    if ring:
        # dsrc0 holds the interior contributions only; the pooling adjoint adds the ring from the workspace while it spreads
        # the gradient: dx = avgpool2_bwd(dsrc0 + ring) -- a quarter of the complete gradient in each of the 2 x 2 cells (the
        # scaling is exact in both formats: the data gradient's own bar holds)
        off, ch = ctypes.c_size_t(), ctypes.c_int()
        assert lib.dlwpcs_conv_ring_info(ctypes.byref(d), ctypes.byref(off), ctypes.byref(ch)) == 1
        dx = arena.tensor((B, 6, 2 * N, 2 * N, C0), inp.adt, 'dx of the pooling adjoint')
        nat.check(lib.dlwpcs_avgpool2_bwd_ring(nat.ptr(g0), 0, 0, nat.ptr(dx), B, 2 * N, C0, 0.0, 0.0, d.dtype,
                                               ws.data_ptr() + off.value, nat.ptr(inv), ch.value, 0, nat.stream_ptr()),
                  'avgpool2_bwd_ring')
        spread = np.repeat(np.repeat(r0, 2, axis=2), 2, axis=3) / 4.0
        outs += [('dsrc0 (interior)', g0, None, 0.0, 0.0), ('dx of the pooling adjoint', dx, spread, tol, 0.0)]
    else:
        outs.append(('dsrc0', g0, r0, tol, 0.0))
    if C1:
        r1 = ref.t1.grad.numpy() * (conv_check._slope(ref.x1) if m1 is not None else 1.0)
        outs.append(('dsrc1', g1, r1, tol, 0.0))
    _settle(arena, outs, what)
    if ring:
        n = N
        edge = np.zeros((n, n), bool)
        edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
        inner = _np64(g0)[:, :, ~edge]
        assert np.abs(inner - r0[:, :, ~edge]).max() <= tol * np.abs(r0).max()
    if c0_valid:
        assert float(g0[..., c0_valid:].float().abs().max()) == 0.0, 'padding channels of dsrc0 are zeros'
    return g0, g1


def _ring_ok(pc, bf16, flags):
    from DLWP import _native as nat
    B, N, C0, C1, up0, Cout, k, halo, mask0, mask1 = pc
    d = _desc(_case(B, N, C0, C1, Cout, k=k, halo=bool(halo), up0=bool(up0), act=False), bf16, flags | nat.CONV_DEFER_RING0)
    off, ch = ctypes.c_size_t(), ctypes.c_int()
    return nat.lib().dlwpcs_conv_ring_info(ctypes.byref(d), ctypes.byref(off), ctypes.byref(ch)) == 1


@pytest.mark.parametrize('bf16', [True, False], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('pc', _premask_cases())
def test_conv_bwd_data_stores_only_its_gradients(pc, bf16, arena):
    """each case plain (both entry points), in gather form where N > 16 (bf16; the flag is ignored where the kernel does not
    apply), and with the ring fix-up of source 0 left to the pooling adjoint where dlwpcs_conv_ring_info allows it"""
    from DLWP import _native as nat
    B, N, C0, C1, up0, Cout, k, halo, mask0, mask1 = pc
    _bwd_data(arena, pc, bf16, False, 0)
    arena.reset()
    _bwd_data(arena, pc, bf16, True, 0)
    if N > 16 and halo and nat.dgrad_gather_ready(N, 1, _dev()):
        for masked in (False, True):
            arena.reset()
            _bwd_data(arena, pc, bf16, masked, nat.CONV_DGRAD_GATHER)
    ringed = 0
    for masked, flags in ((False, 0), (True, 0)):
        # (source 0 must not be masked for the deferral: the masked entry point runs with the mask of source 1 only)
        rc = pc[:8] + (False, pc[9])
        if _ring_ok(rc, bf16, flags):
            arena.reset()
            _bwd_data(arena, rc, bf16, masked, flags, ring=True)
            ringed += 1
    print('%s %s: %d deferred-ring runs' % (pc, 'bf16' if bf16 else 'fp32', ringed))


def test_conv_bwd_data_writes_zeros_into_padded_input_channels(arena):
    _bwd_data(arena, (3, 16, 8, 0, 0, 32, 3, 1, False, False), True, False, 0, c0_valid=7)
    arena.reset()
    _bwd_data(arena, (3, 16, 8, 0, 0, 32, 3, 1, True, False), True, True, 0, c0_valid=7)


# ---- weight gradients, per layer ----
def _wgrad_outputs(arena, ref, fill=None):
    """the six gradient tensors under guard (None where the layer has no such parameter); fill: preset value"""
    dev_w, dev_b = {}, {}
    for n in ('eq', 'pol', 'np'):
        dev_w[n] = None if ref.w[n] is None else arena.tensor(ref.w[n].shape, torch.float32, 'dw_' + n)
        dev_b[n] = None if ref.b[n] is None else arena.tensor(ref.b[n].shape, torch.float32, 'db_' + n)
    if fill is not None:
        for t in list(dev_w.values()) + list(dev_b.values()):
            if t is not None:
                t.fill_(fill)
    return dev_w, dev_b


def _wgrad_checks(ref, dw, db, bf16, base=0.0):
    B, N = ref.case[0], ref.case[1]
    tol = 2e-5 if bf16 else 1e-5
    floor = float(np.sqrt(B * 6 * ref.No * ref.No))         # (conv_check: the natural scale of a bias gradient's fp32 sum)
    outs = []
    for n in ('eq', 'pol', 'np'):
        if dw[n] is not None:
            outs.append(('dW ' + n, dw[n] if not base else dw[n] - base, ref.tw[n].grad.numpy(), tol, 0.0))
            outs.append(('db ' + n, db[n] if not base else db[n] - base, ref.tb[n].grad.numpy(), tol, floor))
    return outs


def _gptrs(dw, db):
    from DLWP._native import ptr
    return tuple(ptr(dw[n]) for n in ('eq', 'pol', 'np')) + tuple(ptr(db[n]) for n in ('eq', 'pol', 'np'))


WGRAD = [_case(2, 12, 32, 0, 32, act=False), _case(3, 10, 16, 0, 24, act=False), _case(2, 12, 7, 0, 5, indep=True, act=False)]


@pytest.mark.parametrize('bf16', [True, False], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('mode', ['plain', 'accumulate', 'defer_reduce'])
@pytest.mark.parametrize('case', WGRAD)
def test_conv_bwd_weights_stores_only_its_gradients(case, mode, bf16, arena):
    """plain: dw_* / db_* are overwritten.  accumulate: ACCUMULATE_WGRAD adds to known values (0.5: the sum's rounding is 2^-24 of
    it, far inside the bar).  defer_reduce: the kernel leaves its partial sums in the workspace and touches no destination (they
    stay poison) until dlwpcs_wgrad_reduce_batch has run over the item."""
    from DLWP import _native as nat
    lib = nat.lib()
    B, N = case[0], case[1]
    what = 'bwd_weights %s %s %s' % (mode, case, 'bf16' if bf16 else 'fp32')
    ref = conv_check.reference(case, bf16)
    inp = _Inputs(ref)
    ref.backward()
    flags = {'plain': 0, 'accumulate': nat.CONV_ACCUMULATE_WGRAD, 'defer_reduce': nat.CONV_DEFER_REDUCE}[mode]
    d = _desc(case, bf16, flags)
    dw, db = _wgrad_outputs(arena, ref, fill=0.5 if mode == 'accumulate' else None)
    ws, nbytes = _ws(arena, d)
    table = nat.halo_tables(N, 1, _dev())[0]
    nat.check(lib.dlwpcs_conv_bwd_weights(ctypes.byref(d), nat.ptr(inp.x0), nat.ptr(inp.x1), nat.ptr(inp.gy), 0, *_gptrs(dw, db),
                                          nat.ptr(table), nat.ptr(ws), nbytes, nat.stream_ptr()), 'conv_bwd_weights')
    if mode == 'defer_reduce':
        arena.assert_guards()
        for t in list(dw.values()) + list(db.values()):
            assert t is None or bool(hm.is_poison(t).all()), 'DEFER_REDUCE touched a destination before the reduction'
        item = nat.ReduceItem()
        nat.check(lib.dlwpcs_conv_wgrad_reduce_item(ctypes.byref(d), *_gptrs(dw, db), nat.ptr(ws), nbytes, ctypes.byref(item)),
                  'conv_wgrad_reduce_item')
        host = (nat.ReduceItem * 1)(item)
        items_dev = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(_dev())
        nat.check(lib.dlwpcs_wgrad_reduce_batch(nat.ptr(items_dev), ctypes.addressof(host), 1, nat.stream_ptr()), 'wgrad_reduce_batch')
    _settle(arena, _wgrad_checks(ref, dw, db, bf16, base=0.5 if mode == 'accumulate' else 0.0), what)


@pytest.mark.parametrize('bf16', [True, False], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('case', [_case(2, 12, 32, 0, 32), _case(3, 10, 16, 0, 24), _case(2, 12, 7, 0, 5, indep=True)])
def test_conv_bwd_weights_hands_dz_over_to_conv_bwd_data(case, bf16, arena):
    """REUSE_DZ on both calls of an activated layer, the weight gradient first, the same descriptor and workspace: where the bf16
    weight-gradient kernel applies the data gradient reads dz from the workspace, elsewhere the flag is ignored"""
    from DLWP import _native as nat
    lib = nat.lib()
    B, N, C0, C1, Cout = case[:5]
    what = 'reuse_dz %s %s' % (case, 'bf16' if bf16 else 'fp32')
    ref, inp, y, _ = _fwd(arena, case, bf16)
    ref.backward(_np64(y), device_mask=True)
    d = _desc(case, bf16, nat.CONV_REUSE_DZ)
    dw, db = _wgrad_outputs(arena, ref)
    g0 = arena.tensor(inp.x0.shape, inp.adt, 'dsrc0')
    ws, nbytes = _ws(arena, d)
    table, inv = nat.halo_tables(N, 1, _dev())
    nat.check(lib.dlwpcs_conv_bwd_weights(ctypes.byref(d), nat.ptr(inp.x0), 0, nat.ptr(inp.gy), nat.ptr(y), *_gptrs(dw, db),
                                          nat.ptr(table), nat.ptr(ws), nbytes, nat.stream_ptr()), 'conv_bwd_weights')
    nat.check(lib.dlwpcs_conv_bwd_data(ctypes.byref(d), nat.ptr(inp.gy), nat.ptr(y), nat.ptr(inp.w['eq']), nat.ptr(inp.w['pol']),
                                       nat.ptr(inp.w['np']), nat.ptr(g0), 0, nat.ptr(inv), nat.ptr(ws), nbytes, nat.stream_ptr()),
              'conv_bwd_data')
    outs = _wgrad_checks(ref, dw, db, bf16) + [('dsrc0', g0, ref.t0.grad.numpy(), 3 * EPS if bf16 else 1e-5, 0.0)]
    _settle(arena, outs, what)


# ---- batched weight gradients into flat buffers ----
WB_LAYERS = [(2, 12, 32, 0, 0, 64, 3, 1), (2, 12, 64, 0, 0, 32, 3, 1), (2, 12, 32, 0, 0, 14, 1, 0)]
GAP = 64
HYPER = (1e-3, 0.9, 0.999, 1e-7, 0.5)


class _Flat(object):
    """p, g, m, v: four flat fp32 buffers under guard; every gradient tensor of the layers is a view into g at a 64-float
    aligned offset (the model's own layout) with a gap of at least 64 floats that no item covers behind it"""

    def __init__(self, arena, lays, rng):
        self.spans, off = [], 0
        for lay in lays:
            for kind, dct in (('dw', lay.dw), ('db', lay.db)):
                for n in sorted(dct):
                    self.spans.append((lay, kind, n, off, tuple(dct[n].shape), dct[n].numel()))
                    off = (off + dct[n].numel() + 63) // 64 * 64 + GAP
        self.n = off
        self.p, self.g, self.m, self.v = (arena.tensor((off,), torch.float32, name) for name in 'pgmv')
        self.covered = torch.zeros(off, dtype=torch.bool)
        for lay, kind, n, o, shape, numel in self.spans:
            self.covered[o:o + numel] = True
            getattr(lay, kind)[n] = self.g[o:o + numel].view(shape)
        cov = self.covered.to(_dev())
        self.p0 = torch.tensor(rng.standard_normal(off), dtype=torch.float32)
        # covered elements: parameters, zero gradients, zero moments; the gaps keep the arena's poison in all four
        self.p[cov] = self.p0.to(_dev())[cov]
        for t in (self.g, self.m, self.v):
            t[cov] = 0.0
        self.n_covered = int(self.covered.sum())

    def param(self, lay, kind, n):
        for l, k, nn, o, shape, numel in self.spans:
            if l is lay and k == kind and nn == n:
                return self.p[o:o + numel].view(shape)
        return None

    def assert_gaps_untouched(self, which='pgmv'):
        gap = (~self.covered).to(_dev())
        for name in which:
            t = getattr(self, name)
            assert bool(hm.is_poison(t)[gap].all()), 'elements of %s that no item covers were written' % name
            assert not bool(hm.is_poison(t)[~gap].any()), 'covered elements of %s hold poison' % name


def _wb_setup(arena, f32, seed=31):
    from DLWP import ops
    rng = np.random.default_rng(seed)
    lays = [wb.Layer(rng, *cfg, f32=f32) for cfg in WB_LAYERS]
    for lay in lays:
        assert ops.wgrad_batch_supported(lay.d)
    flat = _Flat(arena, lays, rng)
    entries = [l.entry() for l in lays]
    arr, key = ops._wb_items(entries)
    host, plan_dev, ws_bytes = ops._wb_plan(arr, len(entries), (str(_dev()), key), _dev())
    ws = arena.carve(ws_bytes, name='wgrad_batch workspace')
    return lays, flat, entries, arr, host, plan_dev, ws, ws_bytes


def _adam_reference(flat, g_dev, t):
    """orc.adam_step in fp64 on the covered elements, fed the device's own reduced gradient (times grad_scale) and the hyper-
    parameters as the fp32 numbers the kernel is given (test_gpu_parity.py: 1 - beta2 differs from 0.001 by 5e-5 of it in fp32)"""
    h = [float(np.float32(x)) for x in HYPER]
    cov = flat.covered
    p = flat.p0.double()[cov].clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    orc.adam_step(p, h[4] * g_dev.double().cpu()[cov], m, v, t, lr=h[0], b1=h[1], b2=h[2], eps=h[3])
    return p, m, v


def _check_adam(flat, g_dev, t):
    cov = flat.covered.to(_dev())
    assert float(flat.g[cov].abs().max()) == 0.0, 'g is zero where covered'
    pr, mr, vr = _adam_reference(flat, g_dev, t)
    for name, ref in (('p', pr), ('m', mr), ('v', vr)):
        e = _rel(getattr(flat, name)[cov], ref)
        print('adam %s: %.3g' % (name, e))
        assert e < 1e-6, (name, e)           # (the bar of test_gpu_parity.py's Adam tests against the same oracle)


def _reduced_gradient(f32):
    """the batch's gradient as dlwpcs_wgrad_batch leaves it in a flat buffer of the same layout (its own arena)"""
    from DLWP import _native as nat
    side = hm.Arena(512 << 20, _dev())
    lays, flat, entries, arr, host, plan_dev, ws, ws_bytes = _wb_setup(side, f32)
    nat.check(nat.lib().dlwpcs_wgrad_batch(arr, len(entries), host, nat.ptr(plan_dev), nat.ptr(ws), ws_bytes, nat.stream_ptr()),
              'wgrad_batch')
    side.assert_guards()
    return flat.g.clone()


@pytest.mark.parametrize('f32', [False, True], ids=['bf16', 'fp32'])
def test_wgrad_batch_reduces_into_views_of_a_flat_buffer(f32, arena):
    from DLWP import _native as nat
    lays, flat, entries, arr, host, plan_dev, ws, ws_bytes = _wb_setup(arena, f32)
    nat.check(nat.lib().dlwpcs_wgrad_batch(arr, len(entries), host, nat.ptr(plan_dev), nat.ptr(ws), ws_bytes, nat.stream_ptr()),
              'wgrad_batch')
    arena.assert_guards()
    flat.assert_gaps_untouched()
    for lay in lays:
        lay.check()                         # fp64 oracle, TOL = 2e-5 of test_gpu_wgrad_batch.py
    cov = flat.covered.to(_dev())
    assert torch.equal(flat.p[cov].cpu(), flat.p0[flat.covered]) and float(flat.m[cov].abs().max()) == 0.0


@pytest.mark.parametrize('f32', [False, True], ids=['bf16', 'fp32'])
def test_wgrad_batch_adam_updates_only_what_the_items_cover(f32, arena):
    from DLWP import _native as nat
    g_dev = _reduced_gradient(f32)
    lays, flat, entries, arr, host, plan_dev, ws, ws_bytes = _wb_setup(arena, f32)
    state = torch.zeros(2, dtype=torch.int32, device=_dev())
    hyper = torch.tensor(HYPER, dtype=torch.float32, device=_dev())
    nat.check(nat.lib().dlwpcs_wgrad_batch_adam(arr, len(entries), host, nat.ptr(plan_dev), nat.ptr(ws), ws_bytes, nat.ptr(flat.p),
                                                nat.ptr(flat.g), nat.ptr(flat.m), nat.ptr(flat.v), flat.n, nat.ptr(state),
                                                nat.ptr(hyper), nat.stream_ptr()), 'wgrad_batch_adam')
    arena.assert_guards()
    flat.assert_gaps_untouched()
    assert int(state[0]) == 1
    _check_adam(flat, g_dev, 1)


def _packs(arena, lays, flat, tag):
    """per layer the make_pack_items entry whose parameters are the views into flat.p, the packed operands under guard and
    filled by dlwpcs_pack_batch from the initial parameters"""
    from DLWP import _native as nat
    from DLWP import ops
    packs = []
    for lay in lays:
        B, N, C0, C1, up0, Cout, k, halo, flip, indep, bias, c0_valid = lay.cfg
        sizes = [t.numel() for t in ops.conv_packed_buffers(k, C0 + C1, Cout, tag, _dev())]
        bufs = tuple(arena.carve(n, name='packed operand %d of %r' % (i, lay.cfg)) for i, n in enumerate(sizes))
        packs.append((flat.param(lay, 'dw', 'eq'), flat.param(lay, 'dw', 'pol'), None, flat.param(lay, 'db', 'eq'),
                      flat.param(lay, 'db', 'pol'), None, bufs, k, flip, tag))
    return packs


def _pack_now(packs):
    from DLWP import ops
    ops.pack_batch(ops.make_pack_items(packs, _dev()), len(packs))
    torch.cuda.synchronize()


def _fresh_pack(packs):
    """what dlwpcs_pack_batch makes of the parameters as they are now, in plain buffers (0xFF where it writes nothing)"""
    fresh = [p[:6] + (tuple(torch.full_like(b, hm.POISON) for b in p[6]),) + p[7:] for p in packs]
    _pack_now(fresh)
    return [p[6] for p in fresh]


def test_wgrad_batch_adam_tail_refreshes_the_packed_operands(arena):
    """dlwpcs_wgrad_batch_adam_tail with pack items (bf16): the updated parameters also reach their places in the packed operands
    -- the bits dlwpcs_pack_batch makes of the updated parameters -- and nothing around the operands is written"""
    from DLWP import _native as nat
    from DLWP import ops
    g_dev = _reduced_gradient(False)
    lays, flat, entries, arr, host, plan_dev, ws, ws_bytes = _wb_setup(arena, False)
    packs = _packs(arena, lays, flat, nat.BF16)
    _pack_now(packs)
    arena.assert_guards()
    state = torch.zeros(2, dtype=torch.int32, device=_dev())
    hyper = torch.tensor(HYPER, dtype=torch.float32, device=_dev())
    nat.check(nat.lib().dlwpcs_wgrad_batch_adam_tail(arr, len(entries), host, nat.ptr(plan_dev), nat.ptr(ws), ws_bytes,
                                                     nat.ptr(flat.p), nat.ptr(flat.g), nat.ptr(flat.m), nat.ptr(flat.v), flat.n,
                                                     nat.ptr(state), nat.ptr(hyper), None, ops._pack_array(packs), nat.stream_ptr()),
              'wgrad_batch_adam_tail')
    arena.assert_guards()
    flat.assert_gaps_untouched()
    assert int(state[0]) == 1
    _check_adam(flat, g_dev, 1)
    for pk, fresh in zip(packs, _fresh_pack(packs)):
        for i, (a, b) in enumerate(zip(pk[6], fresh)):
            assert not bool((a == hm.POISON).all())
            assert torch.equal(a, b), 'packed operand %d differs from dlwpcs_pack_batch of the updated parameters' % i


@pytest.mark.parametrize('f32', [False, True], ids=['bf16', 'fp32'])
def test_wgrad_batch_apply_updates_only_what_the_items_cover(f32, arena):
    """the data-parallel tail: dlwpcs_wgrad_batch leaves the gradient in g, dlwpcs_wgrad_batch_apply consumes it (no workspace)"""
    from DLWP import _native as nat
    lays, flat, entries, arr, host, plan_dev, ws, ws_bytes = _wb_setup(arena, f32)
    nat.check(nat.lib().dlwpcs_wgrad_batch(arr, len(entries), host, nat.ptr(plan_dev), nat.ptr(ws), ws_bytes, nat.stream_ptr()),
              'wgrad_batch')
    torch.cuda.synchronize()
    g_dev = flat.g.clone()
    g_dev[~flat.covered.to(_dev())] = 0.0
    state = torch.zeros(2, dtype=torch.int32, device=_dev())
    hyper = torch.tensor(HYPER, dtype=torch.float32, device=_dev())
    nat.check(nat.lib().dlwpcs_wgrad_batch_apply(arr, len(entries), host, nat.ptr(plan_dev), nat.ptr(flat.p), nat.ptr(flat.g),
                                                 nat.ptr(flat.m), nat.ptr(flat.v), flat.n, nat.ptr(state), nat.ptr(hyper), None, None,
                                                 nat.stream_ptr()), 'wgrad_batch_apply')
    arena.assert_guards()
    flat.assert_gaps_untouched()
    assert int(state[0]) == 1
    _check_adam(flat, g_dev, 1)


# ---- generic convolution ----
@pytest.mark.parametrize('bf16', [True, False], ids=['bf16', 'fp32'])
def test_gconv_stores_only_its_outputs(bf16, arena):
    """3 x 3, stride 2, 'same', (2, H = W = 13, 5 -> 7), independent north pole: forward and all gradients under guard.  Reference and
    bars as in test_gconv_backward (fp32: 1e-5) and test_gconv_bf16 (one bf16 rounding for y and dx, 1e-5 for the fp32 sums)"""
    from DLWP import _native as nat
    from DLWP import ops
    lib = nat.lib()
    dev = _dev()
    rng = np.random.default_rng(21)
    B, H, Cin, Cout, k, s = 2, 13, 5, 7, 3, 2
    adt = torch.bfloat16 if bf16 else torch.float32
    rnd = (lambda a: torch.tensor(a, dtype=torch.float32).to(torch.bfloat16).double().numpy()) if bf16 else (lambda a: np.asarray(a, np.float64))
    x = rnd(rng.standard_normal((B, 6, H, H, Cin)))
    w = {n: (rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)).astype(np.float32) for n in ('eq', 'pol', 'np')}
    b = {n: (rng.standard_normal((Cout,)) * 0.1).astype(np.float32) for n in ('eq', 'pol', 'np')}
    t0 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tw = {n: torch.tensor(rnd(v), dtype=torch.float64, requires_grad=True) for n, v in w.items()}   # (bf16: the kernels round the weights)
    tb = {n: torch.tensor(v, dtype=torch.float64, requires_grad=True) for n, v in b.items()}
    yref = orc.cs_conv2d(t0, tw['eq'], tw['pol'], tw['np'], tb['eq'], tb['pol'], tb['np'], strides=(s, s), padding='same',
                         dilation=(1, 1), flip_north_pole=True, independent_north_pole=True)
    gy = rnd(rng.standard_normal(tuple(yref.shape)))
    yref.backward(torch.tensor(gy, dtype=torch.float64))
    pad, Ho = ops._same_pads(H, k, s, 1)
    assert tuple(yref.shape) == (B, 6, Ho, Ho, Cout)
    d = nat.GConvDesc(B=B, H=H, W=H, Cin=Cin, Cout=Cout, kh=k, kw=k, sh=s, sw=s, dh=1, dw=1, pad_t=pad, pad_l=pad, Ho=Ho, Wo=Ho,
                      flip_north_pole=1, dtype=nat.BF16 if bf16 else nat.F32)
    put = lambda a: torch.tensor(a, dtype=torch.float32).to(adt).to(dev)
    dx0, dgy = put(x), put(gy)
    dwt = {n: torch.tensor(v, device=dev) for n, v in w.items()}
    dbt = {n: torch.tensor(v, device=dev) for n, v in b.items()}
    y = arena.tensor((B, 6, Ho, Ho, Cout), adt, 'y')
    dx = arena.tensor(dx0.shape, adt, 'dx')
    gw = {n: arena.tensor(w[n].shape, torch.float32, 'dw_' + n) for n in w}
    gb = {n: arena.tensor(b[n].shape, torch.float32, 'db_' + n) for n in b}
    wp = [nat.ptr(dwt[n]) for n in ('eq', 'pol', 'np')]
    nat.check(lib.dlwpcs_gconv_fwd(ctypes.byref(d), nat.ptr(dx0), *wp, *[nat.ptr(dbt[n]) for n in ('eq', 'pol', 'np')], nat.ptr(y),
                                   nat.stream_ptr()), 'gconv_fwd')
    nat.check(lib.dlwpcs_gconv_bwd_data(ctypes.byref(d), nat.ptr(dgy), *wp, nat.ptr(dx), nat.stream_ptr()), 'gconv_bwd_data')
    nat.check(lib.dlwpcs_gconv_bwd_weights(ctypes.byref(d), nat.ptr(dx0), nat.ptr(dgy), *[nat.ptr(gw[n]) for n in ('eq', 'pol', 'np')],
                                           *[nat.ptr(gb[n]) for n in ('eq', 'pol', 'np')], nat.stream_ptr()), 'gconv_bwd_weights')
    bar = EPS if bf16 else 1e-5
    outs = [('y', y, yref.detach().numpy(), bar, 0.0), ('dx', dx, t0.grad.numpy(), bar, 0.0)]
    for n in ('eq', 'pol', 'np'):
        outs += [('dW ' + n, gw[n], tw[n].grad.numpy(), 1e-5, 0.0), ('db ' + n, gb[n], tb[n].grad.numpy(), 1e-5, 0.0)]
    _settle(arena, outs, 'gconv %s' % ('bf16' if bf16 else 'fp32'))


# ---- the pointwise output layer behind the last convolution ----
@pytest.mark.parametrize('B,N,cout2,padded,fold', [(1, 24, 26, True, True), (1, 12, 14, False, False)])
def test_conv_fwd_head_stores_only_its_outputs(B, N, cout2, padded, fold, arena):
    """32 -> 32 (3 x 3, activated) + head 32 -> cout2 on packed operands.  Folded (*fused = 1, rows of 32 channels): y_head complete,
    padding channels zero, y never written -- it stays poison.  Two launches (*fused = 0): y holds the layer's output.  Reference
    and bars of test_gpu_head_fold.py: the head of the bf16-rounded intermediate, two rounding steps of the head's scale."""
    import test_gpu_head_fold as hf
    from DLWP import _native as nat
    from DLWP import ops
    lib = nat.lib()
    dev = _dev()
    rng = np.random.default_rng(100 + N + cout2)
    w, h = hf._layers(rng, 32, 32, cout2, dev)
    x = torch.tensor(rng.standard_normal((B, 6, N, N, 32)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    table, keep, items = hf._prepack([(w, 3), (h, 1)], dev)
    pk, hk = table[id(w[0])], table[id(h[0])]
    d = ops._make_desc(B, N, 32, 0, 32, 3, True, False, True, nat.ACT_LEAKY_CLIP, ALPHA, VMAX, nat.BF16, 0)
    d.flags |= nat.CONV_PREPACKED
    dh = ops._make_desc(B, N, 32, 0, cout2, 1, False, False, True, nat.ACT_NONE, 0.0, 0.0, nat.BF16, 0)
    dh.flags |= nat.CONV_PREPACKED | (nat.CONV_OUT_PADDED if padded else 0)
    rows = (cout2 + 7) // 8 * 8 if padded else cout2
    y = arena.tensor((B, 6, N, N, 32), torch.bfloat16, 'y')
    yh = arena.tensor((B, 6, N, N, rows), torch.bfloat16, 'y_head')
    nbytes = max(lib.dlwpcs_conv_workspace_bytes(ctypes.byref(d)), lib.dlwpcs_conv_workspace_bytes(ctypes.byref(dh)))
    ws = arena.carve(nbytes, name='workspace')
    fused = ctypes.c_int(-1)
    nat.check(lib.dlwpcs_conv_fwd_head(ctypes.byref(d), nat.ptr(x), 0, nat.ptr(pk[1]), nat.ptr(pk[2]), ctypes.byref(dh), nat.ptr(hk[1]),
                                       nat.ptr(hk[2]), nat.ptr(y), nat.ptr(yh), nat.ptr(nat.halo_tables(N, 1, dev)[0]), nat.ptr(ws),
                                       nbytes, ctypes.byref(fused), nat.stream_ptr()), 'conv_fwd_head')
    assert fused.value == int(fold)
    ref = hf._oracle(x, None, False, w, h, True)
    outs = [('y_head', yh[..., :cout2], ref, 2.0 * EPS, 0.0)]
    if rows > cout2:
        outs.append(('padding channels of y_head', yh[..., cout2:], None, 0.0, 0.0))
    if not fold:
        t = lambda a: torch.tensor(hf._f32(a), dtype=torch.float64)
        yr = orc.relu_leaky_clip(orc.cs_conv2d(orc.cs_pad(t(x), 1), t(w[0]), t(w[1]), None, t(w[2]), t(w[3])), ALPHA, VMAX)
        outs.append(('y', y, yr.numpy(), EPS, 0.0))
    _settle(arena, outs, 'conv_fwd_head -> %d' % cout2)
    if fold:
        assert bool(hm.is_poison(y).all()), 'the folded call never writes y'
        assert float(yh[..., cout2:].float().abs().max()) == 0.0, 'padding channels are zero'
