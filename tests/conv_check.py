"""
Shared runner of the fused cubed-sphere convolution against the fp64 oracle (test_gpu_fuzz.py, test_gpu_conv_coverage.py):
one case = (B, N, C0, C1, Cout, k, halo, up0, flip, indep, act); forward, both source gradients, dW and db of every weight group,
compared at the suite's bars.  Not a test module: imported by the tests that share it.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from oracle import cs_oracle as orc

EPS = 2.0 ** -8
ALPHA, VMAX = 0.1, 10.0
KINKS = {}          # (device_mask: the last fp32 case's elements near a kink -- see errors())


@contextlib.contextmanager
def launched_tags():
    """The kernel tags (dlwpcs_prof_known_tag names) launched inside the block, through the library's per-launch profiler;
    the profiler is reset and switched off again whatever happens."""
    from DLWP import _native as nat
    lib = nat.lib()
    tags = set()
    lib.dlwpcs_prof_reset()
    lib.dlwpcs_prof_enable(1)
    try:
        yield tags
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(160)
        ms, fl, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        for i in range(lib.dlwpcs_prof_count()):
            nat.check(lib.dlwpcs_prof_get(i, buf, 160, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)), 'prof_get')
            tags.add(buf.value.decode())
    finally:
        lib.dlwpcs_prof_enable(0)
        lib.dlwpcs_prof_reset()


def _slope(a):
    # act'(.) of the leaky clipped ReLU at its own output a
    return np.where(a < 0, ALPHA, np.where((a > 0) & (a < VMAX), 1.0, 0.0))


class Reference(object):
    """reference() of one case: the inputs as numpy arrays (x0, x1, w, b, gy -- already on the bf16 grid where the device
    reads bf16), their fp64 leaves (t0, t1, tw, tb) and the oracle's fp64 pre-activation zref / output yref with the
    autograd graph behind them."""

    def leaves(self):
        return [t for t in [self.t0, self.t1] + list(self.tw.values()) + list(self.tb.values()) if t is not None]

    def backward(self, yd=None, device_mask=False, retain_graph=False):
        """The oracle's backward pass for the upstream gradient gy (the leaves' gradients are cleared first).  yd: the
        device's stored output as an fp64 array (activated cases).  bf16: the device derives act' from ITS stored output and
        rounds dz, so the oracle is fed the same dz.  fp32 with device_mask: see errors()."""
        for leaf in self.leaves():
            leaf.grad = None
        act, gy, zref, yref = self.case[10], self.gy, self.zref, self.yref
        if self.bf16 and act:
            zref.backward(torch.tensor(self.rnd(gy * _slope(yd)), dtype=torch.float64), retain_graph=retain_graph)
        elif act and device_mask:
            z, yr = zref.detach().numpy(), yref.detach().numpy()
            band = 1e-5 * np.abs(yr).max()          # (the fp32 forward's bar)
            near = (np.abs(z) <= band) | (np.abs(z - VMAX) <= band)
            s_ref, s_dev = _slope(yr), _slope(yd)
            KINKS.update(near=int(near.sum()), differ=int((near & (s_ref != s_dev)).sum()),
                         differ_outside=int((~near & (s_ref != s_dev)).sum()))
            zref.backward(torch.tensor(gy * np.where(near, s_dev, s_ref), dtype=torch.float64), retain_graph=retain_graph)
        else:
            yref.backward(torch.tensor(gy, dtype=torch.float64), retain_graph=retain_graph)


def reference(case, bf16, c0_valid=0):
    """Inputs and fp64 forward results of one case (shared by errors() and by the runners that call the C ABI themselves).
    c0_valid: source 0 is stored with C0 channels of which the first c0_valid are real (the rest zero; the kernels have
    c0_valid + C1 input channels).  The backward reference depends on what the device stored (see errors()): the caller
    runs it with Reference.backward()."""
    B, N, C0, C1, Cout, k, halo, up0, flip, indep, act = case
    rng = np.random.default_rng(abs(hash(case)) % (2 ** 31))
    rnd = (lambda a: torch.tensor(a, dtype=torch.float32).to(torch.bfloat16).to(torch.float64).numpy()) if bf16 else (lambda a: a)
    n0 = N // 2 if up0 else N
    x0 = rng.standard_normal((B, 6, n0, n0, C0)) * 3.0
    # every case also has inputs beyond +-100 (pre-activations far above max_value and alpha * x above it for the negative
    # side would be a different kernel bug each): the activation's clip region and its zero-gradient branch are always hit
    x0.reshape(-1)[::97] *= 60.0
    if c0_valid:
        x0[..., c0_valid:] = 0.0
    x0 = rnd(x0)
    x1 = rnd(rng.standard_normal((B, 6, N, N, C1))) if C1 else None
    cin = (c0_valid or C0) + C1
    w = {n: (rng.standard_normal((k, k, cin, Cout)) / np.sqrt(k * k * cin)).astype(np.float32) for n in ('eq', 'pol', 'np')}
    b = {n: (rng.standard_normal((Cout,)) * 0.1).astype(np.float32) for n in ('eq', 'pol', 'np')}
    if not indep:
        w['np'] = b['np'] = None
    No = N if halo else N - k + 1
    if No < 1:
        pytest.skip('empty output')
    gy = rnd(rng.standard_normal((B, 6, No, No, Cout)))
    t0 = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
    t1 = torch.tensor(x1, dtype=torch.float64, requires_grad=True) if C1 else None
    tw = {n: (None if v is None else torch.tensor(rnd(v), dtype=torch.float64, requires_grad=True)) for n, v in w.items()}
    tb = {n: (None if v is None else torch.tensor(v, dtype=torch.float64, requires_grad=True)) for n, v in b.items()}
    t = t0[..., :c0_valid] if c0_valid else t0
    t = orc.upsample_122(t) if up0 else t
    if C1:
        t = torch.cat([t, t1], dim=-1)
    if halo:
        t = orc.cs_pad(t, 1, 'channels_last')
    zref = orc.cs_conv2d(t, tw['eq'], tw['pol'], tw['np'], tb['eq'], tb['pol'], tb['np'], data_format='channels_last',
                         flip_north_pole=flip, independent_north_pole=indep)
    yref = orc.relu_leaky_clip(zref, ALPHA, VMAX) if act else zref
    r = Reference()
    r.case, r.bf16, r.c0_valid, r.No, r.rnd = case, bf16, c0_valid, No, rnd
    r.x0, r.x1, r.w, r.b, r.gy = x0, x1, w, b, gy
    r.t0, r.t1, r.tw, r.tb, r.zref, r.yref = t0, t1, tw, tb, zref, yref
    return r


def errors(case, bf16, dgrad=True, wgrad=True, premask=False, want_pool=False, device_mask=False, on_forward=None,
           outputs=None, ref=None):
    """Runs one case on cuda:0 and returns {quantity: max|device - oracle| / max|oracle|} (bias gradients with the floor
    below) together with the bars they must meet: ({name: err}, {name: bar}).  dgrad / wgrad: the sources / the weights and
    biases require gradients (either one alone is a different launch sequence: no dz hand-over between the two kernels);
    premask: both sources carry the pre-masked gradient convention (ops.cs_conv premask0 / premask1); want_pool: the 2 x 2
    average pooling of the output is asked for as a by-product and checked too.  on_forward(errs, bars): called with the
    forward's errors before any backward pass starts (check() asserts them there, so a refused backward pass cannot hide a
    wrong forward).  device_mask (fp32): where the oracle's pre-activation lies within the forward's bar of a kink of the
    activation (0 or max_value), the backward reference takes act' from the device's stored output -- the kernels derive
    act' from it, and within that band the fp32 forward's rounding may put it on the other side; everywhere else act' is
    the oracle's own.  KINKS records how many elements took the device's act' and how many of them differ.
    outputs: a dict that receives the device's results as CPU tensors under the names of the errors ('y', 'pool', 'dx0',
    'dx1', 'dW eq', 'db eq', ...), for a caller that compares two runs bit by bit.  ref: the reference() of this case, for
    a caller that runs it more than once (its leaves' gradients are cleared here)."""
    backward = dgrad or wgrad
    from DLWP import ops
    from DLWP._native import ACT_LEAKY_CLIP, ACT_NONE
    B, N, C0, C1, Cout, k, halo, up0, flip, indep, act = case
    dev = torch.device('cuda', 0)
    shared = ref is not None
    if ref is None:
        ref = reference(case, bf16)
    assert ref.case == case and ref.bf16 == bf16 and not ref.c0_valid
    rnd, No = ref.rnd, ref.No
    x0, x1, w, b, gy = ref.x0, ref.x1, ref.w, ref.b, ref.gy
    t0, t1, tw, tb, zref, yref = ref.t0, ref.t1, ref.tw, ref.tb, ref.zref, ref.yref
    adt = torch.bfloat16 if bf16 else torch.float32
    d0 = torch.tensor(x0, dtype=torch.float32).to(adt).to(dev).requires_grad_(dgrad)
    d1 = torch.tensor(x1, dtype=torch.float32).to(adt).to(dev).requires_grad_(dgrad) if C1 else None
    dw = {n: (None if v is None else torch.tensor(v, device=dev).requires_grad_(wgrad)) for n, v in w.items()}
    db = {n: (None if v is None else torch.tensor(v, device=dev).requires_grad_(wgrad)) for n, v in b.items()}
    pm = (ALPHA, VMAX) if premask else None
    y = ops.cs_conv(d0, dw['eq'], dw['pol'], dw['np'], db['eq'], db['pol'], db['np'], src1=d1, ksize=k, halo=halo, up0=up0,
                    flip_north_pole=flip, act=ACT_LEAKY_CLIP if act else ACT_NONE, alpha=ALPHA, vmax=VMAX,
                    premask0=pm, premask1=pm if C1 else None, want_pool=want_pool)

    def err(a, ref, floor=0.0, name=None):
        if outputs is not None and name is not None:
            outputs[name] = a.detach().cpu()
        a, ref = a.detach().to(torch.float64).cpu().numpy(), ref.detach().numpy() if isinstance(ref, torch.Tensor) else ref
        den = max(np.abs(ref).max(), floor)
        return np.abs(a - ref).max() / (den if den > 0 else 1.0)
    errs, bars = {}, {}
    errs['y'], bars['y'] = err(y, yref, name='y'), (EPS if bf16 else 1e-5)
    if want_pool:
        yp = ops._POOLED.pop(y.data_ptr(), None)
        assert yp is not None, 'want_pool: no pooled output parked'
        # (bf16: the device pools its fp32 outputs and rounds once; against the fp64 pooled reference that is one rounding
        # of a value up to 4x smaller than max|y| -- the bar is relative to the pooled maximum: 2 EPS)
        errs['pool'], bars['pool'] = err(yp, orc.avgpool_122(yref), name='pool'), (2 * EPS if bf16 else 1e-5)
    if on_forward is not None:
        on_forward(errs, bars)
    if not backward:
        return errs, bars
    # a bias gradient is a sum of B*6*No^2 terms of magnitude ~1 that cancel: with very few output channels max|ref| can be
    # far below the natural scale sqrt(#terms) of the fp32 summation error, so that scale is the floor of the denominator
    bias_floor = float(np.sqrt(B * 6 * No * No))
    ref.backward(y.detach().to(torch.float64).cpu().numpy() if act else None, device_mask=device_mask, retain_graph=shared)
    y.backward(torch.tensor(gy, dtype=torch.float32).to(adt).to(dev))
    tol_x = ((5 if up0 else 3) * EPS) if bf16 else 1e-5
    # bf16: the oracle is fed exactly the bf16 x and dz the device multiplies, partial sums are fp32 -> what is left is the
    # fp32 summation order (2e-5 of max|ref|, like the fp32 mode's 1e-5 plus the rounding of the bf16-rounded kernels)
    tol_w = 2e-5 if bf16 else 1e-5
    if dgrad:
        g0 = t0.grad.numpy() * _slope(x0) if premask else t0.grad
        errs['dx0'], bars['dx0'] = err(d0.grad, g0, name='dx0'), tol_x
    if dgrad and C1:
        g1 = t1.grad.numpy() * _slope(x1) if premask else t1.grad
        errs['dx1'], bars['dx1'] = err(d1.grad, g1, name='dx1'), tol_x
    for n in ('eq', 'pol', 'np'):
        if wgrad and dw[n] is not None:
            errs['dW ' + n], bars['dW ' + n] = err(dw[n].grad, tw[n].grad, name='dW ' + n), tol_w
            errs['db ' + n], bars['db ' + n] = err(db[n].grad, tb[n].grad, bias_floor, name='db ' + n), tol_w
    return errs, bars


def check(case, bf16, **kw):
    """errors() of one case, asserted against their bars -- the forward's before any backward pass runs."""
    def expect(errs, bars):
        for name, e in errs.items():
            assert e <= bars[name], '%s: %.3g > %.3g (case %s, %s)' % (name, e, bars[name], case, 'bf16' if bf16 else 'fp32')
    errs, bars = errors(case, bf16, on_forward=expect, **kw)
    expect(errs, bars)
    return errs
