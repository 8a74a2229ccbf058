"""
GPU tests (`-m gpu`) of the generic per-face convolution (csrc/conv_generic.hip: dlwpcs_gconv_fwd / _bwd_data / _bwd_weights),
the kernels behind every CubeSphereConv2D that is not 1 x 1 or 3 x 3, stride 1, dilation 1, 'valid': one case table over the
option space the layer class accepts (per-axis kernel size, stride and dilation, 'same'), called through the C ABI
(DLWP._native) so that weight-group forms DLWP/ops.py never builds are reachable too.

Reference: oracle.cs_oracle.cs_conv2d in fp64 with autograd (per-axis strides / dilations, TF's asymmetric 'same' padding).
bf16: the oracle is evaluated on the bf16-rounded activations, upstream gradient and kernels (the device rounds the fp32
master kernels on the fly), as in test_gpu_wirings.py::test_gconv_bf16.

Bars (max|d| / max|ref|), the project's own: fp32 < 1e-5 for y, dx, every dW and db (RTOL of test_gpu_parity.py); bf16
<= 2**-8 for y and dx (one rounding) and < 1e-5 for the fp32 parameter gradients (test_gconv_bf16).  On top of them:

* every output (y, dx, each dw_*, each db_*) is pre-filled with a sentinel bit pattern (test_gpu_stream_ops.py) and none of
  its elements may keep it -- an element a kernel skips cannot be right by accident;
* wherever the oracle's dx is exactly 0 (an input pixel no output reads) the device's dx is +0 in every bit;
* a tensor whose pointer is passed as NULL has a sentinel-filled buffer of its own that is never passed, and is checked
  afterwards.

THE `wrap` ROW FOLLOWS sgrid()'s CAP of 4096 workgroups x 256 lanes (SWEEP below): it has to grow with it if the cap is ever
raised, or the grid-stride loops stop taking a second sweep (the assertion in test_gconv_case then fails).
"""
import ctypes
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import cs_oracle as orc

pytestmark = pytest.mark.gpu

SWEEP = 4096 * 256                                  # work items per sweep of gconv_fwd_kernel / gconv_bwd_data_kernel
RTOL = 1e-5
EPS = 2.0 ** -8
DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
IT = {'f32': torch.int32, 'bf16': torch.int16}
SENT = {'f32': -842150451, 'bf16': -12851}          # 0xCDCDCDCD / 0xCDCD: about -4.3e8 in either type
GROUPS = ('eq', 'pol', 'np')
E_INVALID = -1                                      # DLWPCS_E_INVALID (include/dlwpcs.h)


def _dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch.device('cuda', 0)


def rel_err(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    denom = np.abs(ref).max()
    return np.abs(a - ref).max() / (denom if denom > 0 else 1.0)


# ------------------------------------------------------------------------------------------------------------------ #
# case table: one row per branch, the smallest shape at which it exists.  shape = (B, H, W, Cin, Cout, kh, kw, sh, sw, dh, dw,
# padding); dx_zeros: how many elements of dx no output reads (None: not what the row is about).
# ------------------------------------------------------------------------------------------------------------------ #
Row = namedtuple('Row', 'name shape why dx_zeros')

ROWS = [
    Row('k1x3', (2, 7, 9, 3, 5, 1, 3, 1, 1, 1, 1, 'valid'), 'kh != kw, H != W', None),
    Row('k3x1_same', (1, 7, 9, 3, 5, 3, 1, 1, 1, 1, 1, 'same'), 'padding on one axis only', None),
    Row('k2_same', (2, 8, 8, 3, 4, 2, 2, 1, 1, 1, 1, 'same'), 'even kernel: total padding 1, pad_t = 0, the extra row goes after', None),
    Row('k4_same_s2', (1, 9, 9, 2, 3, 4, 4, 2, 2, 1, 1, 'same'), 'even kernel with stride, odd face', None),
    Row('k5_valid', (1, 12, 12, 3, 4, 5, 5, 1, 1, 1, 1, 'valid'), 'the 5 x 5 kernels of the wider wirings', None),
    Row('k2x3_same', (1, 9, 12, 3, 4, 2, 3, 1, 1, 1, 1, 'same'), 'even x odd kernel, H != W', None),
    Row('s2x1_same', (2, 11, 11, 3, 4, 3, 3, 2, 1, 1, 1, 'same'), 'sh != sw', None),
    Row('s1x3_valid', (1, 11, 11, 3, 4, 3, 3, 1, 3, 1, 1, 'valid'), 'sw > kw: input columns between and behind the windows', 396),
    Row('d2x1_valid', (1, 11, 11, 3, 4, 3, 3, 1, 1, 2, 1, 'valid'), 'dh != dw', None),
    Row('d1x3_same', (1, 11, 11, 3, 4, 3, 3, 1, 1, 1, 3, 'same'), "dilated 'same' on one axis", None),
    Row('s2_d2_same', (2, 11, 12, 3, 4, 3, 3, 2, 2, 2, 2, 'same'), 'stride and dilation together: one row / column parity is read', 3456),
    Row('s2_even_same', (1, 12, 12, 3, 4, 3, 3, 2, 2, 1, 1, 'same'), 'even face: total padding 1, pad_t = 0', None),
    Row('win_gt_in', (1, 3, 3, 2, 3, 3, 3, 1, 1, 2, 2, 'same'), 'dilated window (5) wider than the face (3): most taps in the padding', None),
    Row('s3_k1', (1, 10, 10, 3, 4, 1, 1, 3, 3, 1, 1, 'valid'), 'stride beyond the kernel', 1512),
    Row('s3_k2_tail', (1, 11, 11, 3, 4, 2, 2, 3, 3, 1, 1, 'valid'), 'stride beyond an even kernel: unread rows / columns 2, 5, 8, the last window ends on the edge (a trailing unread '
        'strip: s1x3_valid)', 1026),
    Row('one_out', (2, 5, 5, 3, 4, 5, 5, 1, 1, 1, 1, 'valid'), 'Ho = Wo = 1', None),
    Row('c1', (1, 6, 6, 1, 1, 3, 3, 1, 1, 1, 1, 'same'), 'one channel in, one out', None),
    Row('wrap', (2, 50, 50, 36, 40, 3, 3, 1, 1, 1, 1, 'valid'),
        'y and dx above SWEEP: second grid-stride sweep with a ragged end; 39 000 weight-gradient workgroups of 72 trips', None),
]

# weight-group forms: which of (w_np / dw_np), (b_* / db_*), (b_np / db_np) are given, and the north-pole flip
Form = namedtuple('Form', 'name indep bias bias_np flip why')

FORMS = [
    Form('indep_flip', True, True, True, 1, "today's form: three kernels, three biases"),
    Form('indep_noflip', True, True, True, 0, 'three groups, face 5 unflipped'),
    Form('shared_flip', False, True, False, 1, 'shared pole: the flipped face 5 is summed into dw_pol / db_pol'),
    Form('shared_noflip', False, True, False, 0, 'shared pole, face 5 unflipped'),
    Form('shared_nobias', False, False, False, 1, 'no biases (b_* = db_* = NULL), shared pole'),
    Form('indep_nobias', True, False, False, 1, 'no biases, independent pole'),
    Form('indep_sharedbias', True, True, False, 1, 'w_np given, b_np = db_np = NULL: db_pol is the sum over faces 4 AND 5'),
]
CROSSED = ('k2_same', 's2_d2_same', 's3_k2_tail')      # rows that run every form; the others run FORMS[0]

CASES = [(row, form) for row in ROWS for form in (FORMS if row.name in CROSSED else FORMS[:1])]


def test_case_table_is_complete():
    assert len({r.name for r in ROWS}) == len(ROWS) == 18 and all(r.why for r in ROWS)
    assert {r.name for r in ROWS} >= set(CROSSED)
    assert len(CASES) == len(ROWS) + len(CROSSED) * (len(FORMS) - 1)


# ------------------------------------------------------------------------------------------------------------------ #
# runner
# ------------------------------------------------------------------------------------------------------------------ #
def _rnd(dt):
    if dt == 'bf16':
        return lambda a: torch.tensor(np.asarray(a), dtype=torch.float32).to(torch.bfloat16).to(torch.float64).numpy()
    return lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)


def _out(shape, dt):
    t = torch.empty(tuple(shape), dtype=DT[dt], device=_dev())
    t.view(IT[dt]).fill_(SENT[dt])
    return t


def _bits(t):
    return t.contiguous().view(IT['bf16' if t.dtype == torch.bfloat16 else 'f32']).cpu().numpy()


def _p(t):
    return 0 if t is None else t.data_ptr()


def _reference(shape, form, dt, seed):
    """inputs (numpy, on the grid the device reads) and the oracle's fp64 forward and gradients"""
    B, H, W, Cin, Cout, kh, kw, sh, sw, dh, dw, padding = shape
    rng = np.random.default_rng(seed)
    rnd = _rnd(dt)
    x = rnd(rng.standard_normal((B, 6, H, W, Cin)))
    w = {n: (rng.standard_normal((kh, kw, Cin, Cout)) / np.sqrt(kh * kw * Cin)).astype(np.float32) for n in GROUPS}
    b = {n: (rng.standard_normal((Cout,)) * 0.1).astype(np.float32) for n in GROUPS}
    t0 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tw = {n: torch.tensor(rnd(v), dtype=torch.float64, requires_grad=True) for n, v in w.items()}
    tb = {n: torch.tensor(v, dtype=torch.float64, requires_grad=True) for n, v in b.items()}
    if form.bias:
        # an independent kernel with a shared bias: the polar bias serves face 5 too, so its gradient sums faces 4 and 5
        b5 = tb['np'] if form.bias_np else tb['pol']
        biases = (tb['eq'], tb['pol'], b5 if form.indep else None)
    else:
        biases = (None, None, None)
    yref = orc.cs_conv2d(t0, tw['eq'], tw['pol'], tw['np'] if form.indep else None, *biases, strides=(sh, sw), padding=padding,
                         dilation=(dh, dw), flip_north_pole=bool(form.flip), independent_north_pole=form.indep)
    gy = rnd(rng.standard_normal(tuple(yref.shape)))
    yref.backward(torch.tensor(gy, dtype=torch.float64))
    grads = {'dx': t0.grad.numpy()}
    for n in GROUPS:
        grads['dw_' + n] = None if tw[n].grad is None else tw[n].grad.numpy()
        grads['db_' + n] = None if tb[n].grad is None else tb[n].grad.numpy()
    return x, w, b, gy, yref.detach().numpy(), grads


def _desc(shape, form, dt, Ho, Wo):
    from DLWP import _native as nat
    from DLWP import ops
    B, H, W, Cin, Cout, kh, kw, sh, sw, dh, dw, padding = shape
    if padding == 'same':
        (pad_t, ho), (pad_l, wo) = ops._same_pads(H, kh, sh, dh), ops._same_pads(W, kw, sw, dw)
    else:
        pad_t, pad_l, ho, wo = 0, 0, ops._valid_len(H, kh, sh, dh), ops._valid_len(W, kw, sw, dw)
    assert (ho, wo) == (Ho, Wo), 'the launch geometry and the oracle disagree on the output size'
    return nat.GConvDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, kh=kh, kw=kw, sh=sh, sw=sw, dh=dh, dw=dw, pad_t=pad_t, pad_l=pad_l,
                         Ho=Ho, Wo=Wo, flip_north_pole=form.flip, dtype=nat.BF16 if dt == 'bf16' else nat.F32)


def _run(shape, form, dt, seed, dx_zeros=None):
    """One case through the three entry points.  Returns ({name: error}, {name: bar}, device outputs as CPU tensors); the
    bit-level properties (sentinels, exact zeros, untouched null tensors) are asserted here."""
    from DLWP import _native as nat
    lib = nat.lib()
    dev = _dev()
    B, H, W, Cin, Cout = shape[:5]
    x, w, b, gy, yref, ref = _reference(shape, form, dt, seed)
    Ho, Wo = yref.shape[2:4]
    assert yref.shape == (B, 6, Ho, Wo, Cout) and Ho >= 1 and Wo >= 1
    d = _desc(shape, form, dt, Ho, Wo)
    given = {'eq': (True, form.bias), 'pol': (True, form.bias), 'np': (form.indep, form.bias and form.bias_np)}
    # what the oracle differentiated is what the device is given
    for n in GROUPS:
        assert (ref['dw_' + n] is not None) == given[n][0] and (ref['db_' + n] is not None) == given[n][1], (n, form)
    put = lambda a: torch.tensor(a, dtype=torch.float32).to(DT[dt]).to(dev)                # noqa: E731
    dx0, dgy = put(x), put(gy)
    dwt = {n: torch.tensor(w[n], device=dev) for n in GROUPS}
    dbt = {n: torch.tensor(b[n], device=dev) for n in GROUPS}
    y, dx = _out(yref.shape, dt), _out(x.shape, dt)
    gw = {n: _out(w[n].shape, 'f32') for n in GROUPS}          # the buffers of the groups that are NOT given are never passed
    gb = {n: _out(b[n].shape, 'f32') for n in GROUPS}
    wp = [_p(dwt[n]) if given[n][0] else 0 for n in GROUPS]
    bp = [_p(dbt[n]) if given[n][1] else 0 for n in GROUPS]
    nat.check(lib.dlwpcs_gconv_fwd(ctypes.byref(d), _p(dx0), *wp, *bp, _p(y), nat.stream_ptr()), 'gconv_fwd')
    nat.check(lib.dlwpcs_gconv_bwd_data(ctypes.byref(d), _p(dgy), *wp, _p(dx), nat.stream_ptr()), 'gconv_bwd_data')
    nat.check(lib.dlwpcs_gconv_bwd_weights(ctypes.byref(d), _p(dx0), _p(dgy), *[_p(gw[n]) if given[n][0] else 0 for n in GROUPS],
                                           *[_p(gb[n]) if given[n][1] else 0 for n in GROUPS], nat.stream_ptr()),
              'gconv_bwd_weights')
    torch.cuda.synchronize()

    act_bar = EPS if dt == 'bf16' else RTOL
    outs = [('y', y, yref, act_bar), ('dx', dx, ref['dx'], act_bar)]
    for n in GROUPS:
        for kind, buf, on in (('dw_', gw[n], given[n][0]), ('db_', gb[n], given[n][1])):
            if on:
                outs.append((kind + n, buf, ref[kind + n], RTOL))
            else:
                assert bool((buf.view(torch.int32) == SENT['f32']).all()), '%s was passed as NULL and has been written' % (kind + n)
    errs, bars, host = {}, {}, {}
    for name, t, r, bar in outs:
        bits = _bits(t)
        sent = SENT['bf16' if t.dtype == torch.bfloat16 else 'f32']
        assert not (bits == sent).any(), '%s: %d elements keep the sentinel' % (name, int((bits == sent).sum()))
        host[name] = t.cpu()
        errs[name], bars[name] = rel_err(host[name].to(torch.float64).numpy(), r), bar
    zero = ref['dx'] == 0
    if dx_zeros is not None:
        assert int(zero.sum()) == dx_zeros, 'the oracle finds %d unread input elements, the table says %d' % (int(zero.sum()), dx_zeros)
    assert not _bits(dx)[zero].any(), 'dx is not +0 where no output reads the input'
    return errs, bars, host


def _assert_bars(errs, bars, what):
    print(what + ': ' + ', '.join('%s %.3g' % (k, v) for k, v in errs.items()))
    for name, e in errs.items():
        if bars[name] == EPS:
            assert e <= bars[name], '%s: %s %.3g > %.3g' % (what, name, e, bars[name])
        else:
            assert e < bars[name], '%s: %s %.3g >= %.3g' % (what, name, e, bars[name])


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('row,form', CASES, ids=['%s-%s' % (r.name, f.name) for r, f in CASES])
def test_gconv_case(row, form, dt):
    B, H, W, Cin, Cout = row.shape[:5]
    if row.name == 'wrap':
        # must grow with sgrid()'s cap: both loops take a second sweep that ends ragged
        n_dx = B * 6 * H * W * Cin
        n_y = B * 6 * (H - 2) * (W - 2) * Cout
        assert SWEEP < n_y < 2 * SWEEP and SWEEP < n_dx < 2 * SWEEP, (n_y, n_dx)
    seed = zlib.crc32(('%s-%s' % (row.name, form.name)).encode())
    errs, bars, _ = _run(row.shape, form, dt, seed, row.dx_zeros)
    _assert_bars(errs, bars, '%s-%s-%s' % (row.name, form.name, dt))


def test_gconv_refuses_half_given_biases():
    """b_eq / b_pol and db_eq / db_pol are both given or both null -- DLWPCS_E_INVALID otherwise, in the forward pass and in the
    weight gradient alike; db_np without db_eq / db_pol is the adjoint of nothing the forward pass does (it ignores b_np when
    there are no biases) and is refused too.  A refused call writes nothing."""
    from DLWP import _native as nat
    lib = nat.lib()
    row = ROWS[2]
    form = FORMS[0]
    x, w, b, gy, yref, _ = _reference(row.shape, form, 'f32', 1)
    d = _desc(row.shape, form, 'f32', *yref.shape[2:4])
    dev = _dev()
    dx0, dgy = torch.tensor(x, dtype=torch.float32, device=dev), torch.tensor(gy, dtype=torch.float32, device=dev)
    dwt = [torch.tensor(w[n], device=dev) for n in GROUPS]
    dbt = [torch.tensor(b[n], device=dev) for n in GROUPS]
    y = _out(yref.shape, 'f32')
    gw = [_out(w[n].shape, 'f32') for n in GROUPS]
    gb = [_out(b[n].shape, 'f32') for n in GROUPS]
    for mask in ((1, 0, 0), (0, 1, 0), (1, 0, 1), (0, 1, 1)):
        rc = lib.dlwpcs_gconv_fwd(ctypes.byref(d), _p(dx0), *[_p(t) for t in dwt], *[_p(t) if m else 0 for t, m in zip(dbt, mask)],
                                  _p(y), nat.stream_ptr())
        assert rc == E_INVALID, (mask, rc)
    for mask in ((1, 0, 0), (0, 1, 0), (1, 0, 1), (0, 1, 1), (0, 0, 1)):
        rc = lib.dlwpcs_gconv_bwd_weights(ctypes.byref(d), _p(dx0), _p(dgy), *[_p(t) for t in gw],
                                          *[_p(t) if m else 0 for t, m in zip(gb, mask)], nat.stream_ptr())
        assert rc == E_INVALID, (mask, rc)
    torch.cuda.synchronize()
    for t in [y] + gw + gb:
        assert bool((t.view(torch.int32) == SENT['f32']).all())


def test_cs_gconv_refuses_an_empty_output_on_the_device():
    from DLWP import ops
    x = torch.zeros((1, 6, 4, 4, 2), device=_dev())
    w = torch.zeros((3, 3, 2, 3), device=_dev())
    with pytest.raises(ValueError, match='empty output'):
        ops.cs_gconv(x, w, w, strides=(2, 2), padding='valid', dilation=(2, 2))


# ------------------------------------------------------------------------------------------------------------------ #
# the point where the layer class switches families: 3 x 3, stride 1, dilation 1, 'valid' through both
# ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_gconv_agrees_with_the_mfma_path(dt):
    """(2, 6, 14, 14, 8) -> 16 on an already padded tensor, independent pole, biases: dlwpcs_gconv_* and ops.cs_conv(halo=False)
    both within the bars of the oracle; fp32: within 2e-5 (the sum of the two bars) of each other"""
    from DLWP import ops
    shape = (2, 14, 14, 8, 16, 3, 3, 1, 1, 1, 1, 'valid')
    form = FORMS[0]
    seed = 77
    errs, bars, host = _run(shape, form, dt, seed)
    _assert_bars(errs, bars, 'generic-' + dt)
    x, w, b, gy, yref, ref = _reference(shape, form, dt, seed)
    dev = _dev()
    d0 = torch.tensor(x, dtype=torch.float32).to(DT[dt]).to(dev).requires_grad_(True)
    dw = {n: torch.tensor(w[n], device=dev).requires_grad_(True) for n in GROUPS}
    db = {n: torch.tensor(b[n], device=dev).requires_grad_(True) for n in GROUPS}
    y = ops.cs_conv(d0, dw['eq'], dw['pol'], dw['np'], db['eq'], db['pol'], db['np'], ksize=3, halo=False, flip_north_pole=True)
    assert y.dtype == DT[dt]
    y.backward(torch.tensor(gy, dtype=torch.float32).to(DT[dt]).to(dev))
    mfma = {'y': y.detach().cpu(), 'dx': d0.grad.cpu()}
    for n in GROUPS:
        mfma['dw_' + n], mfma['db_' + n] = dw[n].grad.cpu(), db[n].grad.cpu()
    want = dict(ref, y=yref)
    merrs = {k: rel_err(v.to(torch.float64).numpy(), want[k]) for k, v in mfma.items()}
    _assert_bars(merrs, bars, 'mfma-' + dt)
    if dt == 'f32':
        cross = {k: rel_err(mfma[k].double().numpy(), host[k].double().numpy()) for k in mfma}
        print('generic vs mfma: ' + ', '.join('%s %.3g' % kv for kv in cross.items()))
        for k, e in cross.items():
            assert e < 2e-5, (k, e)


# ------------------------------------------------------------------------------------------------------------------ #
# through the layer class: tuple options that end on the generic kernels
# ------------------------------------------------------------------------------------------------------------------ #
LAYER_CASES = [
    # id, kernel_size, strides, dilation_rate, padding, data_format, independent_north_pole, use_bias
    ('k2x3_s2x1_same-cl', (2, 3), (2, 1), 1, 'same', 'channels_last', False, True),
    ('k2x3_s2x1_same-cf', (2, 3), (2, 1), 1, 'same', 'channels_first', True, False),
    ('k5_valid-cl', 5, 1, 1, 'valid', 'channels_last', True, True),
    ('k5_valid-cf', 5, 1, 1, 'valid', 'channels_first', False, False),
    ('k3_d1x2_same-cl', 3, 1, (1, 2), 'same', 'channels_last', False, False),
    ('k3_d1x2_same-cf', 3, 1, (1, 2), 'same', 'channels_first', True, True),
    ('k1_s2_same-cl', 1, 2, 1, 'same', 'channels_last', True, False),
    ('k1_s2_same-cf', 1, 2, 1, 'same', 'channels_first', False, True),
]


@pytest.mark.parametrize('ksize,strides,dil,padding,df,indep,use_bias', [c[1:] for c in LAYER_CASES], ids=[c[0] for c in LAYER_CASES])
def test_layer_class_tuple_options(ksize, strides, dil, padding, df, indep, use_bias):
    """CubeSphereConv2D on a (2, 6, 10, 10, 3) input (or its channels-first transpose), fp32: output, compute_output_shape and
    the gradient of every weight the layer owns against the oracle at 1e-5 -- the shared-pole backward pass through autograd"""
    from DLWP.custom import CubeSphereConv2D
    from DLWP.keras import backend
    backend.set_device('cuda:0')
    dev = _dev()
    filters = 4
    lay = CubeSphereConv2D(filters, ksize, strides=strides, padding=padding, data_format=df, dilation_rate=dil, use_bias=use_bias,
                           flip_north_pole=True, independent_north_pole=indep)
    assert not lay._is_mfma_config()
    rng = np.random.default_rng(zlib.crc32(repr((ksize, strides, dil, padding, df)).encode()))
    x = rng.standard_normal((2, 6, 10, 10, 3))
    xin = x if df == 'channels_last' else np.ascontiguousarray(x.transpose(0, 4, 1, 2, 3))
    lay.build(xin.shape)
    kh, kw = lay.kernel_size
    names = ['eq', 'pol'] + (['np'] if indep else [])
    w = {n: (rng.standard_normal((kh, kw, 3, filters)) / np.sqrt(kh * kw * 3)).astype(np.float32) for n in names}
    b = {n: (rng.standard_normal((filters,)) * 0.1).astype(np.float32) for n in names} if use_bias else {}
    lay.set_weights([w[n] for n in names] + [b[n] for n in names if use_bias])
    owned = dict(zip(['w_' + n for n in names] + (['b_' + n for n in names] if use_bias else []), lay.weights))
    assert len(owned) == len(lay.weights) == len(names) * (2 if use_bias else 1)

    t0 = torch.tensor(xin, dtype=torch.float64)
    tw = {n: torch.tensor(v, dtype=torch.float64, requires_grad=True) for n, v in w.items()}
    tb = {n: torch.tensor(v, dtype=torch.float64, requires_grad=True) for n, v in b.items()}
    yref = orc.cs_conv2d(t0, tw['eq'], tw['pol'], tw.get('np'), tb.get('eq'), tb.get('pol'), tb.get('np'), strides=lay.strides,
                         padding=padding, dilation=lay.dilation_rate, data_format=df, flip_north_pole=True,
                         independent_north_pole=indep)
    gy = rng.standard_normal(tuple(yref.shape))
    yref.backward(torch.tensor(gy))

    y = lay(torch.tensor(xin, dtype=torch.float32, device=dev))
    assert tuple(y.shape) == tuple(lay.compute_output_shape(xin.shape)) == tuple(yref.shape)
    errs = {'y': rel_err(y.detach().cpu().numpy(), yref.detach().numpy())}
    y.backward(torch.tensor(gy, dtype=torch.float32, device=dev))
    for name, t in owned.items():
        assert t.grad is not None, name
        r = (tw if name[0] == 'w' else tb)[name[2:]].grad
        errs['d' + name] = rel_err(t.grad.cpu().numpy(), r.numpy())
    print(', '.join('%s %.3g' % kv for kv in errs.items()))
    for name, e in errs.items():
        assert e < RTOL, (name, e)
