"""
The small-face convolution kernel (csrc/conv_small.hip: dlwpcs_conv_small_fwd / dlwpcs_conv_small_bwd_data) against the general
entry points it stands in for: the SAME BITS in every output -- the forward output, the source's gradient (interior cells and,
after the fix-up, the border), the halo ring left in the workspace, masked and unmasked -- on the smallest shapes at which it
can go wrong: N = 8 (two M tiles: two of the four waves idle), 12 (the benchmark's coarsest level: 5 / 7 M tiles), 16 (8 / 11 M
tiles: three per wave in the data gradient); B = 3 (all six faces, a batch stride that is no power of two); one, four and
eight operand groups; one, two and four output-channel groups.  Inputs reach both clip branches of the activation
(conv_check.reference: |x| up to ~600 against max_value 10).  One case runs with every buffer carved from a poisoned, guarded
arena; one against the fp64 oracle at the bars of the other bf16 convolution tests; shapes outside the kernel's conditions
answer E_UNSUPPORTED and the engine falls back; and whole training steps with the option on and off end in the same parameters.
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_check
import hostile_mem as hm

pytestmark = pytest.mark.gpu

ALPHA, VMAX = conv_check.ALPHA, conv_check.VMAX
EPS = conv_check.EPS
SHAPES = [(N, ci, co) for N in (8, 12, 16) for ci, co in ((32, 32), (64, 128), (128, 64))]
B = 3


def _dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch.device('cuda', 0)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.element_size()]
    assert torch.equal(a.contiguous().view(it), b.contiguous().view(it)), '%s: the small-face kernel differs from the general one' % (what,)


def _case(N, ci, co, act, b=B):
    return (b, N, ci, 0, co, 3, True, False, True, False, bool(act))


_refs = {}


def _ref(case):
    """conv_check.reference of a case, computed once and shared (never modified: the tests only read its inputs / fp64 results)"""
    if case not in _refs:
        _refs[case] = conv_check.reference(case, True)
    return _refs[case]


def _desc(case, flags=0):
    from DLWP import _native as nat
    b, N, C0, C1, Cout, k, halo, up0, flip, indep, act = case
    return nat.ConvDesc(B=b, N=N, C0=C0, C1=C1, Cout=Cout, ksize=k, halo=int(halo), up0=int(up0), flip_north_pole=int(flip),
                        act=nat.ACT_LEAKY_CLIP if act else nat.ACT_NONE, alpha=ALPHA if act else 0., vmax=VMAX if act else 0.,
                        dtype=nat.BF16, flags=flags, c0_valid=0)


class _Inputs(object):
    def __init__(self, ref):
        dev = _dev()
        put = lambda a: None if a is None else torch.tensor(a, dtype=torch.float32).to(torch.bfloat16).to(dev)
        self.x0, self.gy = put(ref.x0), put(ref.gy)
        self.w = {n: (None if v is None else torch.tensor(v, device=dev)) for n, v in ref.w.items()}
        self.b = {n: (None if v is None else torch.tensor(v, device=dev)) for n, v in ref.b.items()}

    def wargs(self):
        from DLWP._native import ptr
        return tuple(ptr(self.w[n]) for n in ('eq', 'pol', 'np')) + tuple(ptr(self.b[n]) for n in ('eq', 'pol', 'np'))


def _alloc(arena, shape, dtype, name):
    if arena is not None:
        return arena.tensor(shape, dtype, name)
    return torch.full(tuple(shape), float('nan'), dtype=dtype, device=_dev())


def _workspace(arena, d):
    from DLWP import _native as nat
    n = nat.lib().dlwpcs_conv_workspace_bytes(ctypes.byref(d))
    if arena is not None:
        return arena.carve(n, name='workspace'), n
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=_dev()), n


def _fwd(small, case, arena=None):
    """(rc, y) of dlwpcs_conv_small_fwd / dlwpcs_conv_fwd on the case's inputs"""
    from DLWP import _native as nat
    ref = _ref(case)
    inp = _Inputs(ref)
    d = _desc(case)
    y = _alloc(arena, (case[0], 6, ref.No, ref.No, case[4]), torch.bfloat16, 'y')
    ws, n = _workspace(arena, d)
    table = nat.halo_tables(case[1], 1, _dev())[0]
    fn = nat.lib().dlwpcs_conv_small_fwd if small else nat.lib().dlwpcs_conv_fwd
    rc = fn(ctypes.byref(d), nat.ptr(inp.x0), None, *inp.wargs(), nat.ptr(y), nat.ptr(table), nat.ptr(ws), n, nat.stream_ptr())
    torch.cuda.synchronize()
    return rc, y


def _bwd(small, case, masked, defer, arena=None):
    """(rc, dsrc0, workspace) of dlwpcs_conv_small_bwd_data / dlwpcs_conv_bwd_data_masked: dz = the case's gy, the mask operand the
    source itself (values on both sides of 0 and of max_value)"""
    from DLWP import _native as nat
    ref = _ref(case)
    inp = _Inputs(ref)
    d = _desc(case, nat.CONV_DEFER_RING0 if defer else 0)
    d.act = nat.ACT_NONE
    dx = _alloc(arena, inp.x0.shape, torch.bfloat16, 'dsrc0')
    ws, n = _workspace(arena, d)
    inv = nat.halo_tables(case[1], 1, _dev())[1]
    fn = nat.lib().dlwpcs_conv_small_bwd_data if small else nat.lib().dlwpcs_conv_bwd_data_masked
    rc = fn(ctypes.byref(d), nat.ptr(inp.gy), *inp.wargs()[:3], nat.ptr(dx), None, nat.ptr(inp.x0) if masked else None, None,
            ALPHA, VMAX, nat.ptr(inv), nat.ptr(ws), n, nat.stream_ptr())
    torch.cuda.synchronize()
    return rc, dx, ws


@pytest.mark.parametrize('act', [True, False], ids=['act', 'linear'])
@pytest.mark.parametrize('N,ci,co', SHAPES)
def test_forward_is_bitwise_the_general_kernel(N, ci, co, act):
    case = _case(N, ci, co, act)
    rc0, y0 = _fwd(False, case)
    rc1, y1 = _fwd(True, case)
    assert rc0 == 0 and rc1 == 0, (rc0, rc1)
    assert not bool(torch.isnan(y1.float()).any()), 'an output cell was never written'
    if act:
        yf = y1.float()
        assert float(yf.max()) == VMAX and float(yf.min()) < 0, 'the inputs must reach both branches of the activation'
    _same_bits(y0, y1, 'y %s' % (case,))


@pytest.mark.parametrize('masked,defer', [(True, False), (False, True), (False, False)], ids=['masked', 'ring-deferred', 'plain'])
@pytest.mark.parametrize('N,ci,co', SHAPES)
def test_data_gradient_is_bitwise_the_general_kernel(N, ci, co, masked, defer):
    """interior cells (+ the fix-up's border), the ring in the workspace, the mask of the direct stores"""
    from DLWP import _native as nat
    case = _case(N, ci, co, False)
    rc0, dx0, ws0 = _bwd(False, case, masked, defer)
    rc1, dx1, ws1 = _bwd(True, case, masked, defer)
    assert rc0 == 0 and rc1 == 0, (rc0, rc1)
    assert not bool(torch.isnan(dx1.float()).any()), 'a gradient cell was never written'
    _same_bits(dx0, dx1, 'dsrc0 %s' % (case,))
    _same_bits(ws0, ws1, 'workspace (packed operands, halo ring) %s' % (case,))
    if masked:
        x = torch.tensor(_ref(case).x0)
        assert bool((x < 0).any()) and bool((x > VMAX).any()) and bool(((x > 0) & (x < VMAX)).any())
    if defer:
        d = _desc(case)
        off, ch = ctypes.c_size_t(), ctypes.c_int()
        assert nat.lib().dlwpcs_conv_ring_info(ctypes.byref(d), ctypes.byref(off), ctypes.byref(ch)) == 1 and ch.value == ci
        ring = ws1[off.value:off.value + B * 6 * (N + 2) * (N + 2) * ci * 2].view(torch.bfloat16).view(B, 6, N + 2, N + 2, ci)
        edge = torch.cat([ring[:, :, 0].reshape(-1), ring[:, :, -1].reshape(-1), ring[:, :, :, 0].reshape(-1), ring[:, :, :, -1].reshape(-1)])
        assert not bool(torch.isnan(edge.float()).any()), 'a ring cell was never written'
        assert bool(torch.isnan(ring[:, :, 1:-1, 1:-1].float()).all()), 'interior cells belong to dsrc0, not to the workspace'


def test_guarded_poisoned_exact_size_buffers():
    """N = 12, 64 -> 128: y, dsrc0 and the workspaces carved from a poisoned arena with guards -- nothing stored outside them, no
    output cell left unwritten, and the same bits as with plain allocations (a read of unwritten memory would be NaN)"""
    arena = hm.Arena(256 << 20, _dev())
    try:
        case = _case(12, 64, 128, True)
        rc, y = _fwd(True, case, arena)
        assert rc == 0
        arena.assert_guards()
        assert int(hm.is_poison(y).sum()) == 0
        _same_bits(_fwd(False, case)[1], y, 'y under guard')
        for masked, defer in ((True, False), (False, True)):
            rc, dx, ws = _bwd(True, _case(12, 64, 128, False), masked, defer, arena)
            assert rc == 0
            arena.assert_guards()
            assert int(hm.is_poison(dx).sum()) == 0
            _same_bits(_bwd(False, _case(12, 64, 128, False), masked, defer)[1], dx, 'dsrc0 under guard')
    finally:
        torch.cuda.synchronize()
        arena.buf = None
        torch.cuda.empty_cache()


def _count_calls(monkeypatch, name):
    """the library's entry point `name`, counting the calls that returned 0"""
    from DLWP import _native as nat
    handle, fn, n = nat.lib(), getattr(nat.lib(), name), [0]

    def counted(*a):
        rc = fn(*a)
        n[0] += rc == 0
        return rc
    monkeypatch.setattr(handle, name, counted)
    return n


def test_against_the_fp64_oracle(monkeypatch):
    """N = 12, 64 -> 128 through conv_check (y: EPS; dx0: 3 EPS, pre-masked), every cs_conv of the run offered to the small kernel"""
    from DLWP import ops
    orig = ops.cs_conv
    monkeypatch.setattr(ops, 'cs_conv', lambda *a, **k: orig(*a, small=True, **k))
    nf, nb = _count_calls(monkeypatch, 'dlwpcs_conv_small_fwd'), _count_calls(monkeypatch, 'dlwpcs_conv_small_bwd_data')
    for act in (True, False):
        errs = conv_check.check(_case(12, 64, 128, act, b=2), True, dgrad=True, wgrad=False, premask=True)
        print('small-face kernel against fp64, act=%s: %s' % (act, errs))
    assert nf[0] == 2 and nb[0] == 2, 'the small-face kernel did not serve the layer (%d forward, %d backward calls)' % (nf[0], nb[0])


@pytest.mark.parametrize('N,ci,co', [(24, 64, 64), (12, 14, 32), (12, 64, 48)])
def test_unsupported_shapes_are_refused_and_the_engine_falls_back(N, ci, co, monkeypatch):
    from DLWP import _native as nat, ops
    case = _case(N, ci, co, True, b=2)
    rc, _ = _fwd(True, case)
    assert rc == nat.E_UNSUPPORTED
    if ci % 8 == 0:
        rc, _, _ = _bwd(True, case, True, False)
        assert rc == nat.E_UNSUPPORTED
    ref = _ref(case)
    inp = _Inputs(ref)
    ys = [ops.cs_conv(inp.x0, inp.w['eq'], inp.w['pol'], None, inp.b['eq'], inp.b['pol'], None, act=nat.ACT_LEAKY_CLIP, alpha=ALPHA,
                      vmax=VMAX, small=s) for s in (False, True)]
    _same_bits(ys[0], ys[1], 'engine fall-back %s' % (case,))


def test_pooled_output_keeps_the_general_kernel(monkeypatch):
    from DLWP import _native as nat, ops
    case = _case(12, 64, 128, True, b=2)
    inp = _Inputs(_ref(case))
    nf = _count_calls(monkeypatch, 'dlwpcs_conv_small_fwd')
    out = []
    for s in (False, True):
        y = ops.cs_conv(inp.x0, inp.w['eq'], inp.w['pol'], None, inp.b['eq'], inp.b['pol'], None, act=nat.ACT_LEAKY_CLIP, alpha=ALPHA,
                        vmax=VMAX, small=s, want_pool=True)
        out.append((y, ops._POOLED.pop(y.data_ptr())))
    assert nf[0] == 0
    _same_bits(out[0][0], out[1][0], 'y beside a pooled output')
    _same_bits(out[0][1], out[1][1], 'pooled y')


# ---- whole training steps ----
def _train(N, C, base, b, options, graphs, monkeypatch, w0=None):
    from DLWP.keras import backend
    from DLWP.model.cs_unet import build_cs_model
    dev = _dev()
    backend.set_device('cuda:0')
    rng = np.random.default_rng(11)
    x = torch.tensor(rng.standard_normal((b, 6, N, N, C)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    t = torch.tensor(rng.standard_normal((b, 6, N, N, C)), dtype=torch.float32, device=dev)
    monkeypatch.setenv('DLWPCS_OPTIONS', options)
    backend.set_compute_dtype('bfloat16')
    try:
        np.random.seed(5)
        model = build_cs_model((6, N, N, C), C, 'unet2', base_filter_number=base)
    finally:
        backend.set_compute_dtype('float32')
    model.use_graphs = graphs
    model.compile(optimizer='adam', loss='mse', metrics=['mae'])
    if w0 is None:
        w0 = model.get_weights()
    model.set_weights(w0)
    for _ in range(3):
        model.train_on_device_batch([x], [t])
    torch.cuda.synchronize()
    return model._flat_params.detach().cpu().clone(), w0, model


@pytest.mark.parametrize('graphs', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('N,base,b,served', [(48, 8, 2, False), (24, 32, 2, True)], ids=['fallback-N12-c16', 'served-N6-c64'])
def test_training_steps_option_on_and_off_end_in_the_same_parameters(N, base, b, served, graphs, monkeypatch):
    """three steps of a small unet2: base 8 at N = 48 (coarsest level 16 / 32 channels at N = 12: not multiples of 32 throughout ->
    the general kernel) and base 32 at face 24 (coarsest level N = 6, 64 / 128 channels: served)"""
    nf, nb = _count_calls(monkeypatch, 'dlwpcs_conv_small_fwd'), _count_calls(monkeypatch, 'dlwpcs_conv_small_bwd_data')
    p_off, w0, m_off = _train(N, 14, base, b, 'small_conv=0', graphs, monkeypatch)
    assert m_off.small_conv is False and nf[0] == 0 and nb[0] == 0
    p_on, _, m_on = _train(N, 14, base, b, '', graphs, monkeypatch, w0)
    assert m_on.small_conv is True
    if served:
        assert nf[0] >= 2 and nb[0] >= 2, 'the coarsest level was not served by the small-face kernel (%d / %d calls)' % (nf[0], nb[0])
    assert torch.isfinite(p_on).all()
    _same_bits(p_off, p_on, 'flat parameters after three steps')
