"""
GPU tests of the pointwise output layer family (csrc/conv_mfma.hip: pw_fwd_kernel, pw_dgrad_kernel, pw_head_train_kernel,
pw_head_loss_kernel; k = 1, 32 -> even C_out in 8..32, bf16), called through the C ABI (DLWP._native): dlwpcs_conv_fwd,
dlwpcs_conv_bwd_data[_masked] and the fused training tail dlwpcs_head_mse_step[_masked] / dlwpcs_head_loss_step.

Reference: fp64 on the CPU from the bf16-rounded x, the bf16-rounded kernels (the header's bf16 contract) and the fp32
biases, with the face -> weight-group rule restated (faces 0-3 equatorial, 4 polar, 5 north pole when independent, else
polar; a 1 x 1 kernel has no rows to flip), evaluated sample by sample.  The operands come from ops.conv_packed_buffers /
make_pack_items / pack_batch, with separate equatorial, polar (and north-pole) kernels and biases.  Conventions of
tests/test_gpu_stream_ops.py: sentinel-filled outputs, untouched padding, one case table per entry point;
tests/test_loss_ref.py asserts on the CPU that the tables cover every output width, shape class and variant.

Bars (u = 2**-24; all magnitudes from the reference)
  forward      |y - ref| <= 2**-8 |ref| + 40 u (sum_c |w_c x_c| + |b|): one bf16 rounding of the stored value plus the fp32
               accumulation of 33 terms (the activation is 1-Lipschitz: the same bar behind it);
  data grad    the same form over the C_out terms; the masked result is BITWISE the unmasked one times act' of the
               pre-activation, rounded again;
  fused tail   (a) dy and dx bitwise equal to dlwpcs_conv_fwd -> dlwpcs_loss_fwd_bwd -> dlwpcs_conv_bwd_data[_masked] on the
               same operands; (b) dy against the fp64 gradient at the reference prediction, with the forward's bar
               propagated through the gradient plus one bf16 rounding of dy, and dx against the fp64 product of the device's
               own dy with the bf16 kernels; (c) loss_out within loss_ref.bar(k) of the fp64 loss of the unfused device
               prediction; (d) DLWPCS_HEAD_DEFER_STAGE2 leaves loss_out alone until the tail has run, then the same bits.

Shapes: N = 4 (one group per face: the face class changes on every group; B = 1 leaves a wave with an empty range), N = 8,
N = 12 (9 groups per face), and B = 10 at N = 96: 34560 groups of 16 pixels, more than the 32768 that 2048 workgroups of
4 waves take PW_U = 4 at a time, so every wave makes a second trip through its main loop with clamped loads.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import conv_check
import loss_ref as L
import stream_ref as R
import test_gpu_stream_ops as S

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
E8 = 2.0 ** -8
ALPHA, VMAX = 0.1, 10.0
PW_U = 4                              # 16-pixel groups a wave keeps in flight
CAP_BLOCKS = 2048                     # the documented grid rule: ceil(groups / (4 waves * PW_U)) workgroups, at most 2048
CAP_GROUPS = CAP_BLOCKS * 4 * PW_U


def _report(table, frac):
    print('%s: error / bar %.3f' % (table, frac))


def ngroups(B, N):
    return B * 6 * N * N // 16


def grid(B, N):
    return min((ngroups(B, N) + 4 * PW_U - 1) // (4 * PW_U), CAP_BLOCKS)


def groups_per_wave(B, N):
    return -(-ngroups(B, N) // (grid(B, N) * 4))


def mt(cout):
    """16-channel output tiles of a kernel instantiation"""
    return 1 if cout <= 16 else 2


# ------------------------------------------------------------------------------------------------------------------ #
# case tables
# ------------------------------------------------------------------------------------------------------------------ #
COUTS = tuple(range(8, 33, 2))
SHAPES = ((1, 4), (3, 4), (3, 8), (2, 12))
BIG = (10, 96)
BIG_COUTS = (12, 14, 30)
assert ngroups(*BIG) > CAP_GROUPS and groups_per_wave(*BIG) == PW_U + 1


def _geo(i, j):
    """flip_north_pole both ways, and an independent north pole on every third case"""
    return dict(flip=bool((i + j) % 2), indep=(i + j) % 3 == 0)


# forward: every (C_out, shape) runs with and without DLWPCS_CONV_OUT_PADDED; activation and PREPACKED alternate
FWD = [dict(Cout=co, B=B, N=N, act=bool((i + j + p) % 2), padded=bool(p), prepacked=bool((i // 2 + j + p) % 2), **_geo(i, j))
       for i, co in enumerate(COUTS) for j, (B, N) in enumerate(SHAPES) for p in (0, 1)]
FWD += [dict(Cout=co, B=BIG[0], N=BIG[1], act=bool(p), padded=bool(p), prepacked=not p, **_geo(i, 1))
        for i, co in enumerate(BIG_COUTS) for p in (0, 1)]
# data gradient: mask = None (dlwpcs_conv_bwd_data) or (m_alpha, m_vmax) of dlwpcs_conv_bwd_data_masked; 0.7 is no bf16 number
MASKS = (None, (0.1, 10.0), (0.1, 0.7))
DGRAD = [dict(Cout=co, B=B, N=N, mask=m, prepacked=bool((i + j + k) % 2), **_geo(i, j))
         for i, co in enumerate(COUTS) for j, (B, N) in enumerate(SHAPES) for k, m in enumerate(MASKS)]
DGRAD += [dict(Cout=co, B=BIG[0], N=BIG[1], mask=m, prepacked=True, **_geo(i, 0)) for i, co in enumerate(BIG_COUTS) for m in MASKS]
# fused tail: 16 variants {mse, mae} x {no weight, per-cell weight} x mask x bias; every C_out sees all 16 across its four
# shapes (four per shape), the case past the cap two per C_out plus the masked 'mse' entry point at C_out = 14 and 30
_VARIANTS = [(k, w, m, b) for k in (L.MSE, L.MAE) for w in (False, True) for m in (None, (ALPHA, VMAX)) for b in (True, False)]


def _entry(kind, w, mask, v):
    """which entry point: the 'mse' forms have their own (and also run through dlwpcs_head_loss_step on odd variants)"""
    if kind == L.MSE and not w and v % 2 == 0:
        return 'masked' if mask else 'mse'
    return 'loss'


def _head_case(co, B, N, v, i, j):
    kind, w, mask, bias = _VARIANTS[v % 16]
    return dict(Cout=co, B=B, N=N, kind=kind, w=w, mask=mask, bias=bias, entry=_entry(kind, w, mask, v // 4 + v),
                mode='overwrite' if (v + j) % 2 else 'accumulate', **_geo(i, j))


HEAD = [_head_case(co, B, N, 4 * ((j + i) % 4) + r, i, j) for i, co in enumerate(COUTS) for j, (B, N) in enumerate(SHAPES)
        for r in range(4)]
HEAD += [_head_case(co, BIG[0], BIG[1], v, i, 0) for i, co in enumerate(BIG_COUTS) for v in (0, 15 - 2 * i)]
HEAD += [_head_case(14, BIG[0], BIG[1], 2, 1, 0), _head_case(30, BIG[0], BIG[1], 2, 2, 0)]      # dlwpcs_head_mse_step_masked past the cap


# ------------------------------------------------------------------------------------------------------------------ #
# operands
# ------------------------------------------------------------------------------------------------------------------ #

def group_of_face(f, indep):
    return 0 if f < 4 else (2 if (f == 5 and indep) else 1)


class Layer(object):
    """fp32 parameters of one 32 -> C_out pointwise layer (three weight groups), on the device and packed"""

    def __init__(self, cout, flip, indep, seed):
        from DLWP import ops
        nat = S._nat()
        dev = S._dev()
        rng = np.random.default_rng(seed)
        self.cout, self.flip, self.indep = cout, flip, indep
        ng = 3 if indep else 2
        self.w = [(rng.standard_normal((1, 1, 32, cout)) / np.sqrt(32.0)).astype(np.float32) for _ in range(ng)]
        self.b = [(0.2 * rng.standard_normal(cout)).astype(np.float32) for _ in range(ng)]
        self.wd = [torch.from_numpy(a).to(dev) for a in self.w] + [None] * (3 - ng)
        self.bd = [torch.from_numpy(a).to(dev) for a in self.b] + [None] * (3 - ng)
        self.bufs = ops.conv_packed_buffers(1, 32, cout, nat.BF16, dev, bias=True)
        entries = [(self.wd[0], self.wd[1], self.wd[2], self.bd[0], self.bd[1], self.bd[2], self.bufs, 1, flip, nat.BF16)]
        self.items = ops.make_pack_items(entries, dev)
        ops.pack_batch(self.items, 1)
        torch.cuda.synchronize()
        # what the kernels multiply with: the kernels rounded to bf16, the biases as they are
        self.w64 = [R.store(a.reshape(32, cout), 'bf16').astype(np.float64) for a in self.w]
        self.b64 = [a.astype(np.float64) for a in self.b]

    def face(self, f, bias=True):
        g = group_of_face(f, self.indep)
        return self.w64[g], (self.b64[g] if bias else np.zeros(self.cout))

    def desc(self, B, N, act=False, flags=0):
        from DLWP import ops
        nat = S._nat()
        d = ops._make_desc(B, N, 32, 0, self.cout, 1, False, False, self.flip, nat.ACT_LEAKY_CLIP if act else nat.ACT_NONE,
                           ALPHA if act else 0.0, VMAX if act else 0.0, nat.BF16)
        d.flags = flags
        return d


@functools.lru_cache(maxsize=8)
def layer(cout, flip, indep):
    return Layer(cout, flip, indep, 1000 + cout)


def _blocked(rng, shape, fn):
    n = int(np.prod(shape))
    return np.resize(fn(rng, min(n, 1000003)).astype(np.float32), n).reshape(shape)


@functools.lru_cache(maxsize=2)
def activations(B, N, alpha, vmax, scale):
    """(p, x): pre-activations p ~ N(0, scale) and x = the stored bf16 output of ReLU(alpha, vmax) at p, shape (B, 6, N*N, 32).
    Where bf16 cannot represent max_value the stored output does not tell a clipped value from an un-clipped one within one bf16
    step of max_value: no pre-activation is put there (they are moved to 2 * max_value), so that act' of the pre-activation is
    what every element's mask must be."""
    rng = np.random.default_rng(B * 100 + N)
    p = _blocked(rng, (B, 6, N * N, 32), lambda r, m: scale * r.standard_normal(m))
    p = R.store(p, 'bf16')
    if R.bf16_floor(vmax) != float(np.float32(vmax)):
        p[np.abs(p.astype(np.float64) - vmax) <= R.bf16_ulp(vmax)] = np.float32(2 * vmax)
    x = R.act_fwd(p, alpha, vmax, 'bf16')
    s = R.act_slope(p, alpha, vmax)
    assert (s == np.float32(alpha)).any() and (s == 1).any() and (s == 0).any(), 'all three slope regions occur'
    return p, x


def head_input(B, N):
    return activations(B, N, ALPHA, VMAX, 6.0)


def cell_weight(cells):
    """per-cell loss weight in [0.5, 1.5]"""
    return (0.5 + np.random.default_rng(cells).random(cells)).astype(np.float32)


def _dev_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(S._dev()).to(torch.bfloat16)


PAD = 64


def _guarded(n, dt='bf16'):
    """(buffer, view): n elements with PAD sentinel elements in front and behind"""
    buf = S._out((n + 2 * PAD,), dt)
    return buf, buf[PAD:PAD + n]


def _guards_ok(buf, n):
    return S._untouched(buf[:PAD]) and S._untouched(buf[PAD + n:])


def _ws(d):
    n = S._nat().lib().dlwpcs_conv_workspace_bytes(ctypes.byref(d))
    return torch.empty(max(int(n), 256), dtype=torch.uint8, device=S._dev())


def _rc(name, *args):
    nat = S._nat()
    rc = getattr(nat.lib(), 'dlwpcs_' + name)(*args, nat.stream_ptr())
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------------------------------------------------------ #
# device calls
# ------------------------------------------------------------------------------------------------------------------ #

def conv_fwd(lay, B, N, xd, yv, act=False, padded=False, prepacked=True, bias=True):
    nat = S._nat()
    d = lay.desc(B, N, act, (nat.CONV_PREPACKED if prepacked else 0) | (nat.CONV_OUT_PADDED if padded else 0))
    ws = _ws(d)
    if prepacked:
        wargs = (S._p(lay.bufs[0]), 0, 0, S._p(lay.bufs[1]) if bias else 0, 0, 0)
    else:
        wargs = tuple(S._p(t) for t in lay.wd) + tuple(S._p(t) if bias else 0 for t in lay.bd)
    S._call('conv_fwd', ctypes.byref(d), S._p(xd), 0, *wargs, S._p(yv), 0, S._p(ws), ws.numel())


def conv_bwd_data(lay, B, N, dyd, dxv, mask=None, md=None, prepacked=True):
    nat = S._nat()
    d = lay.desc(B, N, False, nat.CONV_PREPACKED if prepacked else 0)
    ws = _ws(d)
    wargs = (S._p(lay.bufs[2]), 0, 0) if prepacked else tuple(S._p(t) for t in lay.wd)
    if mask is None:
        S._call('conv_bwd_data', ctypes.byref(d), S._p(dyd), 0, *wargs, S._p(dxv), 0, 0, S._p(ws), ws.numel())
    else:
        S._call('conv_bwd_data_masked', ctypes.byref(d), S._p(dyd), *wargs, S._p(dxv), 0, S._p(md), 0, mask[0], mask[1], 0,
                S._p(ws), ws.numel())


def loss_desc(c, lw, wd, N, overwrite):
    nat = S._nat()
    Ld = nat.LossDesc()
    Ld.kind = nat.LOSS_MSE if c['kind'] == L.MSE else nat.LOSS_MAE
    Ld.loss_weight = lw
    if wd is not None:
        Ld.weight, Ld.weight_div, Ld.weight_period = S._p(wd), c['Cout'], 6 * N * N
    Ld.overwrite = overwrite
    return Ld


def head_step(c, lay, d, xd, td, lw, wd, dyv, dxv, out, scratch, overwrite):
    """the fused tail through the entry point the case names; returns the return code"""
    bias = S._p(lay.bufs[1]) if c['bias'] else 0
    common = (ctypes.byref(d), S._p(xd), S._p(lay.bufs[0]), bias, S._p(lay.bufs[2]), S._p(td))
    if c['entry'] == 'mse':
        return _rc('head_mse_step', *common, lw, S._p(dyv), S._p(dxv), S._p(out), overwrite, S._p(scratch))
    if c['entry'] == 'masked':
        return _rc('head_mse_step_masked', *common, lw, S._p(dyv), S._p(dxv), S._p(out), overwrite, S._p(scratch), c['mask'][0],
                   c['mask'][1])
    Ld = loss_desc(c, lw, wd, d.N, overwrite)
    m = c['mask'] or (0.0, 0.0)
    return _rc('head_loss_step', common[0], ctypes.byref(Ld), *common[1:], S._p(dyv), S._p(dxv), S._p(out), S._p(scratch),
               int(c['mask'] is not None), m[0], m[1])


# ------------------------------------------------------------------------------------------------------------------ #
# fp64 references, sample by sample
# ------------------------------------------------------------------------------------------------------------------ #

def fwd_ref(lay, xs, bias=True):
    """xs (6, N*N, 32) stored values of one sample -> (z (6, N*N, C_out) fp64, sum_c |w_c x_c| + |b|)"""
    z = np.empty(xs.shape[:2] + (lay.cout,))
    mag = np.empty_like(z)
    for f in range(6):
        w, b = lay.face(f, bias)
        x64 = xs[f].astype(np.float64)
        z[f] = x64 @ w + b
        mag[f] = np.abs(x64) @ np.abs(w) + np.abs(b)
    return z, mag


def dgrad_ref(lay, dys):
    """dys (6, N*N, C_out) stored values of one sample -> (dx (6, N*N, 32) fp64, sum_c |w_c dy_c|)"""
    dx = np.empty(dys.shape[:2] + (32,))
    mag = np.empty_like(dx)
    for f in range(6):
        w, _ = lay.face(f)
        g64 = dys[f].astype(np.float64)
        dx[f] = g64 @ w.T
        mag[f] = np.abs(g64) @ np.abs(w).T
    return dx, mag


def act64(z):
    return np.where(z >= 0, np.minimum(z, VMAX), float(np.float32(ALPHA)) * z)


def _worst(err, tol):
    i = int(np.argmax(err - tol))
    return np.unravel_index(i, err.shape), float(err.reshape(-1)[i]), float(tol.reshape(-1)[i])


# ------------------------------------------------------------------------------------------------------------------ #
# forward
# ------------------------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize('case', FWD, ids=S._id)
def test_pointwise_forward_matches_fp64(case):
    c = case
    B, N, co = c['B'], c['N'], c['Cout']
    lay = layer(co, c['flip'], c['indep'])
    _, x = head_input(B, N)
    xd = _dev_bf16(x)
    rows = (co + 7) // 8 * 8 if c['padded'] else co
    npix = B * 6 * N * N
    ybuf, yv = _guarded(npix * rows)
    conv_fwd(lay, B, N, xd, yv, c['act'], c['padded'], c['prepacked'])
    assert _guards_ok(ybuf, npix * rows), 'nothing beyond the output rows is written'
    y = yv.float().cpu().numpy().reshape(B, 6, N * N, rows)
    if rows > co:
        assert np.all(y[..., co:] == 0.0), 'padding channels are exactly zero'
    frac = 0.0
    for b in range(B):
        z, mag = fwd_ref(lay, x[b])
        ref = act64(z) if c['act'] else z
        err, tol = np.abs(y[b, ..., :co] - ref), E8 * np.abs(ref) + 40 * U * mag
        assert np.all(err <= tol), ('sample %d' % b,) + _worst(err, tol)
        frac = max(frac, float(np.max(err / tol)))
    print('forward: worst error / bar %.3f' % frac)
    _report('forward', frac)


# ------------------------------------------------------------------------------------------------------------------ #
# data gradient
# ------------------------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize('case', DGRAD, ids=S._id)
def test_pointwise_data_gradient_matches_fp64_and_its_mask_is_bitwise(case):
    c = case
    B, N, co = c['B'], c['N'], c['Cout']
    lay = layer(co, c['flip'], c['indep'])
    npix = B * 6 * N * N
    rng = np.random.default_rng(co + N)
    dy = R.store(_blocked(rng, (B, 6, N * N, co), lambda r, m: r.standard_normal(m)), 'bf16')
    dyd = _dev_bf16(dy)
    dbuf, dxv = _guarded(npix * 32)
    conv_bwd_data(lay, B, N, dyd, dxv, prepacked=c['prepacked'])
    assert _guards_ok(dbuf, npix * 32)
    dx = dxv.float().cpu().numpy().reshape(B, 6, N * N, 32)
    frac = 0.0
    for b in range(B):
        ref, mag = dgrad_ref(lay, dy[b])
        err, tol = np.abs(dx[b] - ref), E8 * np.abs(ref) + 40 * U * mag
        assert np.all(err <= tol), ('sample %d' % b,) + _worst(err, tol)
        frac = max(frac, float(np.max(err / tol)))
    print('data gradient: worst error / bar %.3f' % frac)
    _report('dgrad', frac)
    if c['mask'] is None:
        return
    alpha, vmax = c['mask']
    p, m = activations(B, N, alpha, vmax, 6.0 if vmax > 1 else 0.6)
    md = _dev_bf16(m)
    mbuf, mxv = _guarded(npix * 32)
    conv_bwd_data(lay, B, N, dyd, mxv, c['mask'], md, prepacked=c['prepacked'])
    assert _guards_ok(mbuf, npix * 32)
    want = R.store(dx * R.act_slope(p, alpha, vmax), 'bf16')             # the ROUNDED gradient times the slope, rounded again
    bad = np.flatnonzero(S._bits(mxv) != S._ref_bits(want, 'bf16').reshape(-1))
    assert bad.size == 0, '%d of %d masked elements differ, first at %d' % (bad.size, npix * 32, bad[0])


# ------------------------------------------------------------------------------------------------------------------ #
# fused training tail
# ------------------------------------------------------------------------------------------------------------------ #

def head_k(B, N, cout):
    """fp32 additions of one lane into its loss sum: 4 channels per 16-channel tile and group"""
    return groups_per_wave(B, N) * 4 * mt(cout)


def _dy_bar(c, yref, mag, t, w, gs):
    """bar of dy against the fp64 gradient g at the REFERENCE prediction: the device forms it from its own bf16 prediction, which
    is within dlt = 2**-8 |y| + 40 u mag of the reference (the forward's bar), in fp32 (a few u) and rounds once to bf16.
      mse: g = gs w^2 (y - t): |dg| <= gs w^2 dlt;   mae: g = gs w sign(y - t): exact unless |y - t| <= dlt, where any sign may come"""
    dlt = E8 * np.abs(yref) + 40 * U * mag
    if c['kind'] == L.MSE:
        g = gs * w * w * (yref - t)
        a = gs * w * w * dlt
        return g, a + E8 * (np.abs(g) + a) + 8 * U * np.abs(g)
    g = gs * w * np.sign(yref - t)
    sure = np.abs(yref - t) > dlt
    return g, np.where(sure, (E8 + 8 * U) * np.abs(g), 2.0 * (1 + E8) * gs * np.abs(w))


@pytest.mark.parametrize('case', HEAD, ids=S._id)
def test_fused_tail_matches_the_unfused_sequence_and_fp64(case):
    c = case
    nat = S._nat()
    lib = nat.lib()
    B, N, co = c['B'], c['N'], c['Cout']
    lay = layer(co, c['flip'], c['indep'])
    npix, cells = B * 6 * N * N, 6 * N * N
    n = npix * co
    lw = 0.75
    p, x = head_input(B, N)
    xd = _dev_bf16(x)
    rng = np.random.default_rng(co * 7 + N)
    t = _blocked(rng, (B, 6, N * N, co), lambda r, m: 3.0 * r.standard_normal(m))
    td = torch.from_numpy(t).to(S._dev())
    wcell = cell_weight(cells) if c['w'] else None
    wd = None if wcell is None else torch.from_numpy(wcell).to(S._dev())
    d = lay.desc(B, N, False, nat.CONV_PREPACKED)
    nscr = lib.dlwpcs_head_mse_scratch_bytes() // 4
    g = grid(B, N)
    ow = int(c['mode'] == 'overwrite')

    def outputs():
        return _guarded(n), _guarded(npix * 32), S._out((4,), 'f32'), S._out((nscr + 64,), 'f32')

    def prefill(out):
        out[:2] = torch.tensor([np.nan, np.nan] if ow else [3.0, -2.0], device=out.device)

    # ---- the fused launch
    (dybuf, dyv), (dxbuf, dxv), out, scratch = outputs()
    prefill(out)
    assert head_step(c, lay, d, xd, td, lw, wd, dyv, dxv, out, scratch, ow) == 0, lib.dlwpcs_last_error()
    assert _guards_ok(dybuf, n) and _guards_ok(dxbuf, npix * 32) and S._untouched(out[2:])
    assert not bool((scratch[:2 * g].view(torch.int32) == S.SENT['f32']).any().item()) and S._untouched(scratch[2 * g:])
    # ---- (a) the unfused sequence on the same operands: same dy / dx bits
    ybuf, yv = _guarded(n)
    conv_fwd(lay, B, N, xd, yv, bias=c['bias'])
    (_, udy), (_, udx), uout, _ = outputs()
    uscr = S._out((lib.dlwpcs_loss_scratch_bytes() // 4,), 'f32')
    Ld = loss_desc(c, lw, wd, N, 1)
    S._call('loss_fwd_bwd', ctypes.byref(Ld), S._p(yv), S._p(td), S._p(udy), S._p(uout), n, nat.BF16 | nat.MSE_TARGET_F32, S._p(uscr))
    conv_bwd_data(lay, B, N, udy, udx, c['mask'], xd if c['mask'] else None)
    for what, a, b_ in (('dy', dyv, udy), ('dx', dxv, udx)):
        same = a.view(torch.int16) == b_.view(torch.int16)
        assert bool(same.all().item()), '%s: %d elements differ from the unfused sequence' % (what, int((~same).sum().item()))
    # ---- (c) the loss against fp64 of the unfused DEVICE prediction
    ydev = yv.float().cpu().numpy().reshape(B, 6, N * N, co)
    wfull = None if wcell is None else np.broadcast_to(np.tile(wcell, B).reshape(B, 6, N * N, 1), ydev.shape)
    v = L.loss_values(c['kind'], ydev, t, wfull, lw=lw)
    k = head_k(B, N, co)
    bk = L.bar(k)
    assert bk <= 1e-5
    got = out.cpu().numpy().astype(np.float64)
    for j, (ref, tol) in enumerate(((v['loss'], bk * v['sums']['loss'] / n * lw), (v['mae'], bk * v['sums']['mae'] / n))):
        base = 0.0 if ow else (3.0, -2.0)[j]
        tol += 0.0 if ow else float(L.ulp_half(abs(base + ref) + tol, 'f32'))     # accumulate: one more fp32 addition
        err = abs(got[j] - (base + ref))
        print('loss_out[%d] = %.9g  fp64 %.9g  error %.3g  bar %.3g' % (j, got[j], base + ref, err, tol))
        assert np.isfinite(got[j]) and err <= tol, (j, got[j], base + ref, err, tol)
        _report('head loss', err / tol)
    # ---- (d) the deferred second stage
    (_, dyv2), (_, dxv2), out2, scratch2 = outputs()
    prefill(out2)
    keep = out2.clone()
    assert head_step(c, lay, d, xd, td, lw, wd, dyv2, dxv2, out2, scratch2, ow | nat.HEAD_DEFER_STAGE2) == 0
    assert torch.equal(out2.view(torch.int32), keep.view(torch.int32)), 'loss_out waits for the tail'
    tail = nat.LossTail()
    assert lib.dlwpcs_head_mse_tail(ctypes.byref(d), lw, ow, S._p(scratch2), S._p(out2), ctypes.byref(tail)) == 0
    assert tail.nblocks == g
    assert _rc('loss_tail_run', ctypes.byref(tail)) == 0
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32)), 'deferred and undeferred loss: same bits'
    assert torch.equal(dyv2.view(torch.int16), dyv.view(torch.int16)) and torch.equal(dxv2.view(torch.int16), dxv.view(torch.int16))
    # ---- (b) against the independent reference, sample by sample
    dy = dyv.float().cpu().numpy().reshape(B, 6, N * N, co)
    dx = dxv.float().cpu().numpy().reshape(B, 6, N * N, 32)
    gs = lw * (2.0 if c['kind'] == L.MSE else 1.0) / n
    w1 = np.ones((6, N * N, 1)) if wcell is None else wcell.astype(np.float64).reshape(6, N * N, 1)
    fy = fx = 0.0
    for b in range(B):
        yref, mag = fwd_ref(lay, x[b], c['bias'])
        g64, tol = _dy_bar(c, yref, mag, t[b].astype(np.float64), w1, gs)
        err = np.abs(dy[b] - g64)
        assert np.all(err <= tol), ('dy, sample %d' % b,) + _worst(err, tol)
        fy = max(fy, float(np.max(err / np.maximum(tol, 1e-300))))
        ref, mag2 = dgrad_ref(lay, dy[b])
        tolx = E8 * np.abs(ref) + 40 * U * mag2
        if c['mask']:
            # the rounded gradient times act'(pre-activation), rounded again where the slope is neither 0 nor 1
            s = R.act_slope(p[b], *c['mask']).astype(np.float64)
            ref, tolx = ref * s, tolx * s + np.where((s != 0) & (s != 1), E8 * (np.abs(ref * s) + tolx * s), 0.0)
        errx = np.abs(dx[b] - ref)
        assert np.all(errx <= tolx), ('dx, sample %d' % b,) + _worst(errx, tolx)
        fx = max(fx, float(np.max(errx / np.maximum(tolx, 1e-300))))
    print('dy: worst error / bar %.3f   dx: %.3f' % (fy, fx))
    _report('head dy', fy)
    _report('head dx', fx)


# ------------------------------------------------------------------------------------------------------------------ #
# the kernels the cases are meant for
# ------------------------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize('cout', [14, 30])
def test_cases_launch_the_kernels_they_are_meant_for(cout):
    """(the launch profiler knows the 'mse' instantiations of the fused tail, pw_head_train_kernel<1|2>; the other losses' head
    kernels, pw_head_loss_kernel<...>, are not profiled, so no tag can be asserted for them)"""
    nat = S._nat()
    B, N = 3, 8
    lay = layer(cout, True, False)
    _, x = head_input(B, N)
    xd = _dev_bf16(x)
    npix = B * 6 * N * N
    m = mt(cout)
    td = torch.zeros(npix * cout, dtype=torch.float32, device=S._dev())

    def launched(fn):
        with conv_check.launched_tags() as tags:
            fn()
        return tags

    for act in (False, True):
        yv = S._out((npix * cout,), 'bf16')
        assert launched(lambda: conv_fwd(lay, B, N, xd, yv, act)) == {'pw_fwd_kernel<%s, %d>' % ('true' if act else 'false', m)}
    dyd = _dev_bf16(np.ones((npix, cout), dtype=np.float32))
    dxv = S._out((npix * 32,), 'bf16')
    assert launched(lambda: conv_bwd_data(lay, B, N, dyd, dxv)) == {'pw_dgrad_kernel<false>'}
    assert launched(lambda: conv_bwd_data(lay, B, N, dyd, dxv, (ALPHA, VMAX), xd)) == {'pw_dgrad_kernel<true>'}
    d = lay.desc(B, N, False, nat.CONV_PREPACKED)
    dyv, out = S._out((npix * cout,), 'bf16'), S._out((2,), 'f32')
    scratch = S._out((nat.lib().dlwpcs_head_mse_scratch_bytes() // 4,), 'f32')
    for entry, mask in (('mse', None), ('masked', (ALPHA, VMAX)), ('loss', None)):
        c = dict(Cout=cout, kind=L.MSE, bias=True, entry=entry, mask=mask)
        tags = launched(lambda: head_step(c, lay, d, xd, td, 1.0, None, dyv, dxv, out, scratch, 1))
        assert tags == {'pw_head_train_kernel<%d>' % m}, (entry, tags)


# ------------------------------------------------------------------------------------------------------------------ #
# refusals
# ------------------------------------------------------------------------------------------------------------------ #

def test_unserved_layers_are_refused_with_nothing_written():
    """DLWPCS_E_UNSUPPORTED (-2) and every output still holds its sentinels"""
    nat = S._nat()
    from DLWP import ops
    dev = S._dev()
    B = 1
    xd = torch.zeros(B * 6 * 12 * 12 * 32, dtype=torch.bfloat16, device=dev)
    td = torch.zeros(B * 6 * 12 * 12 * 34, dtype=torch.float32, device=dev)
    fld = torch.ones(6 * 12 * 12, dtype=torch.float32, device=dev)
    dyv, dxv = S._out((td.numel(),), 'bf16'), S._out((xd.numel(),), 'bf16')
    out = S._out((2,), 'f32')
    scratch = S._out((nat.lib().dlwpcs_head_mse_scratch_bytes() // 4,), 'f32')

    def refused(cout, N, act=False, entry='mse', kind=L.MSE, field=None):
        bufs = ops.conv_packed_buffers(1, 32, cout, nat.BF16, dev, bias=True)
        d = ops._make_desc(B, N, 32, 0, cout, 1, False, False, True, nat.ACT_LEAKY_CLIP if act else nat.ACT_NONE, ALPHA, VMAX, nat.BF16)
        d.flags = nat.CONV_PREPACKED
        common = (ctypes.byref(d), S._p(xd), S._p(bufs[0]), S._p(bufs[1]), S._p(bufs[2]), S._p(td))
        if entry == 'mse':
            rc = _rc('head_mse_step', *common, 1.0, S._p(dyv), S._p(dxv), S._p(out), 1, S._p(scratch))
        elif entry == 'masked':
            rc = _rc('head_mse_step_masked', *common, 1.0, S._p(dyv), S._p(dxv), S._p(out), 1, S._p(scratch), ALPHA, VMAX)
        elif entry == 'loss':
            Ld = nat.LossDesc()
            Ld.kind = {L.MSE: nat.LOSS_MSE, L.MAE: nat.LOSS_MAE, L.ACC: nat.LOSS_ACC}[kind]
            Ld.loss_weight, Ld.overwrite = 1.0, 1
            if field is not None:
                Ld.weight, Ld.weight_div, Ld.weight_period = S._p(fld), field[0], field[1]
            rc = _rc('head_loss_step', common[0], ctypes.byref(Ld), *common[1:], S._p(dyv), S._p(dxv), S._p(out), S._p(scratch), 0, 0.0, 0.0)
        else:                                                                       # dlwpcs_conv_fwd with DLWPCS_CONV_OUT_PADDED
            d.flags |= nat.CONV_OUT_PADDED
            ws = _ws(d)
            rc = _rc('conv_fwd', ctypes.byref(d), S._p(xd), 0, S._p(bufs[0]), 0, 0, S._p(bufs[1]), 0, 0, S._p(dyv), 0, S._p(ws), ws.numel())
        assert rc == -2, 'DLWPCS_E_UNSUPPORTED expected, got %d (%s)' % (rc, nat.lib().dlwpcs_last_error())
        assert S._untouched(dyv) and S._untouched(dxv) and S._untouched(out) and S._untouched(scratch)

    for entry in ('mse', 'masked', 'loss', 'fwd_padded'):
        for cout, N in ((13, 8), (6, 8), (34, 8), (14, 6), (14, 10)):               # odd, too narrow, too wide, N * N % 16 != 0
            refused(cout, N, entry=entry)
    for entry in ('mse', 'masked', 'loss'):
        refused(14, 8, act=True, entry=entry)                                       # an activation on the head step
    for field in ((1, 6 * 8 * 8 * 14), (14, 6 * 8 * 8 - 1), (7, 6 * 8 * 8), (14, 8 * 8)):
        refused(14, 8, entry='loss', field=field)                                   # not a per-cell field of this layer
    refused(14, 8, entry='loss', kind=L.ACC)
    refused(14, 8, entry='loss', kind=L.ACC, field=(14, 6 * 8 * 8))
