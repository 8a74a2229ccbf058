"""
Plain numpy references of the training losses of libdlwpcs (include/dlwpcs.h: dlwpcs_loss_fwd_bwd, dlwpcs_mse_fwd_bwd and
the loss half of dlwpcs_head_*_step), written from the header's doc comments: keras 'mse' / 'mae' with an optional weight
field, and the anomaly-correlation loss with its regularisers.

Conventions (as tests/stream_ref.py)
  * a bf16 tensor is a float32 array whose values are bf16 values;
  * `loss_values` evaluates everything in fp64 on the STORED values and also returns the sum of the absolute values of
    the terms of every sum a kernel forms -- the error bars of tests/test_gpu_loss_ops.py scale with those;
  * `dy_f32` is the fp32 replica of the MSE / MAE gradient: products only, so nothing can be contracted into an FMA and
    the device result has to equal it bit for bit.

tests/test_loss_ref.py checks these references against fp64 autograd of tests/test_losses.py::restated_loss on the CPU.

ERROR BAR OF A REDUCTION  (u = 2**-24, the unit roundoff of fp32)
The kernels sum in three stages: every lane adds its k terms one after the other in fp32, the 256 lanes of a workgroup are
added by an 8-level fp32 tree, and ONE workgroup adds the workgroup sums in fp64 and scales the result.  For a sum of terms
x_i the computed value differs from the exact one by at most  e * sum|x_i|  with, to first order in u,
      k u      a term passes through at most k lane additions, each (1 + d), |d| <= u
    + 8 u      and through the 8 levels of the tree
    + 5 u      the term itself: d = y - t is one rounding, w * d a second, the square doubles both and adds a third
               (2 + 2 + 1; 'mae' and the unweighted forms have fewer; a contracted multiply-add has one fewer)
    + 3 u      inv_n = 1 / float(n) is rounded, the fp64 product is rounded to fp32, and the result is multiplied by the
               loss weight in fp32 (the fp64 second stage itself contributes ~256 * 2**-53: nothing)
    + 4 u      spare, for the second-order terms ((1 + u)**(k + 16) - 1 - (k + 16) u < u for k <= 4000)
    = (k + 20) u  = bar(k).
The largest case of the suite has k = 24 (three sweeps of an 8-wide lane): bar = 44 * 2**-24 = 2.6e-6.
"""
import numpy as np

import stream_ref as R

F32, BF16 = R.F32, R.BF16
MSE, MAE, ACC = 'mse', 'mae', 'acc'
REGS = (None, 'mse', 'mae', 'global')
U = 2.0 ** -24

# the documented launch geometry (csrc/elementwise.hip): 256 lanes per workgroup, at most LOSS_BLOCKS workgroups in the
# reduction launches and ACC_DY_BLOCKS in the launch that writes the anomaly-correlation gradient
LOSS_BLOCKS = 1024
ACC_DY_BLOCKS = 2048
SWEEP = LOSS_BLOCKS * 256
ACC_DY_SWEEP = ACC_DY_BLOCKS * 256
SCRATCH_STRIDE = {MSE: 2, MAE: 2, ACC: 8}       # floats per workgroup in the scratch


def bar(k):
    """relative error bar of a sum whose lanes add k terms each (derivation: module docstring)"""
    return (k + 20) * U


def field(p, div, period, n):
    """the header's field[(e / div) % period] for e = 0 .. n-1"""
    e = np.arange(n, dtype=np.int64)
    return np.asarray(p)[(e // int(div)) % int(period)]


# ------------------------------------------------------------------------------------------------------------------ #
# which kernel serves a call, and how much a lane adds (the documented dispatch rules)
# ------------------------------------------------------------------------------------------------------------------ #

def loss_vec(n, *byte_offsets):
    """MSE / MAE: the 8-wide kernel when n % 8 == 0 and y, t and dy all sit on 32-byte boundaries, else the scalar one"""
    return n % 8 == 0 and all(o % 32 == 0 for o in byte_offsets)


def loss_items(n, vec):
    return n // 8 if vec else n


def loss_grid(items):
    return min((items + 255) // 256, LOSS_BLOCKS)


def loss_k(n, vec):
    """fp32 additions a lane makes into one of its sums"""
    items = loss_items(n, vec)
    per_lane = -(-items // (loss_grid(items) * 256))
    return per_lane * (8 if vec else 1)


def size_class(items, sweep=SWEEP):
    """'tiny': less than one workgroup; 'ragged': more than one workgroup, not a multiple of 256, less than a sweep;
    'wrap': more than two capped sweeps plus a ragged third; None: none of them"""
    if items < 256:
        return 'tiny'
    if items % 256 == 0:
        return None
    if items < sweep:
        return 'ragged'
    return 'wrap' if 2 * sweep < items < 3 * sweep else None


# ------------------------------------------------------------------------------------------------------------------ #
# fp64 values
# ------------------------------------------------------------------------------------------------------------------ #

def loss_values(kind, y, t, w=None, c=None, reg=None, reverse=False, lw=1.0):
    """fp64 loss of the flat arrays y, t (w, c: full-length fields, e.g. from field(), or None).  Returns a dict:
         loss    lw * the loss                                  mae     mean |y - t| (unweighted)
         grad    d loss / d y (fp64, flat)
         sums    {name: sum of |term|} of every sum the kernels form ('loss' and 'mae' for mse / mae; 'X', 'P', 'T', 'r0', 'r1'
                 and 'mae' for the anomaly correlation)
       and for the anomaly correlation also the pieces its error bars need:
         a, m, q         correlation, regulariser, and (global) q = (sum w t - sum w y) / sum w t
         X, P, T, r0, r1 the sums themselves
         mag             per element |w cA t'| + |w cB p'| + |regulariser's term| of the gradient"""
    y = np.asarray(y, dtype=np.float64).ravel()
    t = np.asarray(t, dtype=np.float64).ravel()
    n = y.size
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64).ravel()
    c = np.zeros(n) if c is None else np.asarray(c, dtype=np.float64).ravel()
    lw = float(lw)
    d = y - t
    wd = w * d
    out = {'mae': np.abs(d).mean()}
    if kind == MSE:
        out.update(loss=lw * (wd ** 2).mean(), grad=lw * 2.0 * w * wd / n, sums={'loss': (wd ** 2).sum(), 'mae': np.abs(d).sum()})
        return out
    if kind == MAE:
        out.update(loss=lw * np.abs(wd).mean(), grad=lw * w * np.sign(wd) / n, sums={'loss': np.abs(wd).sum(), 'mae': np.abs(d).sum()})
        return out
    assert kind == ACC, kind
    pa, ta = w * y - c, w * t - c
    X, P, T = (pa * ta).sum(), (pa ** 2).sum(), (ta ** 2).sum()
    rt = np.sqrt(P * T)
    a = X / rt
    sa = -1.0 if reverse else 1.0
    sm = 0.0 if reg is None else (1.0 if reverse else -1.0)
    r0 = r1 = q = m = 0.0
    sums = {'X': np.abs(pa * ta).sum(), 'P': P, 'T': T, 'r0': 0.0, 'r1': 0.0, 'mae': np.abs(d).sum()}
    if reg == 'mse':
        r0 = (wd ** 2).sum(); m = r0 / n; gm = 2.0 * w * wd / n; sums['r0'] = r0
    elif reg == 'mae':
        r0 = np.abs(wd).sum(); m = r0 / n; gm = w * np.sign(wd) / n; sums['r0'] = r0
    elif reg == 'global':
        r0, r1 = (w * t).sum(), (w * y).sum()
        q = (r0 - r1) / r0
        m = abs(q)
        gm = -np.sign(q) * w / r0
        sums['r0'], sums['r1'] = np.abs(w * t).sum(), np.abs(w * y).sum()
    else:
        assert reg is None, reg
        gm = np.zeros(n)
    cA, cB = lw * sa / rt, -lw * sa * a / P
    out.update(loss=lw * (sm * m + sa * a), grad=w * (cA * ta + cB * pa) + lw * sm * gm, sums=sums,
               a=a, m=m, q=q, X=X, P=P, T=T, r0=r0, r1=r1,
               mag=np.abs(w * cA * ta) + np.abs(w * cB * pa) + np.abs(lw * sm * gm))
    return out


def acc_loss_bar(v, reg, k, lw, n):
    """absolute error bar of loss_out[0] of the anomaly-correlation loss, from loss_values' result v: bar(k) relative to the
    sum of |term| of X, P and T propagated through a = X / sqrt(P T), plus the regulariser's own sums.
      |dX| <= b S_X <= b sqrt(P T) (Cauchy-Schwarz),  |dP| <= b P,  |dT| <= b T  =>  |d sqrt(P T)| <= b sqrt(P T)
      =>  |da| <= |dX| / sqrt(P T) + |a| b <= 2 b; the bar takes 3 b for the second-order terms and the final cast."""
    b = bar(k)
    s = v['sums']
    da = 3.0 * b
    if reg is None:
        dm = 0.0
    elif reg in ('mse', 'mae'):                             # m = r0 / n
        dm = b * s['r0'] / n
    else:                                                   # 'global': m = |1 - r1 / r0|
        dm = b * (s['r1'] + s['r0'] * abs(v['r1'] / v['r0'])) / abs(v['r0'])
    return abs(lw) * (da + dm)


# ------------------------------------------------------------------------------------------------------------------ #
# the fp32 gradient of 'mse' / 'mae', bit for bit
# ------------------------------------------------------------------------------------------------------------------ #

def dy_f32(kind, y, t, w, lw, n, store):
    """fp32 replica of the MSE / MAE gradient of the flat stored arrays y, t (w: full-length fp32 field or None):
    d = f32(y) - f32(t), gscale = (lw * 2) / f32(n) or lw / f32(n), then products only; rounded once to `store`."""
    f = np.float32
    d = np.asarray(y, dtype=f).ravel() - np.asarray(t, dtype=f).ravel()
    if kind == MSE:
        gscale = (f(lw) * f(2.0)) / f(n)
        g = gscale * d if w is None else gscale * (np.asarray(w, dtype=f) * (np.asarray(w, dtype=f) * d))
    else:
        assert kind == MAE, kind
        gscale = f(lw) / f(n)
        wd = d if w is None else np.asarray(w, dtype=f) * d
        sg = np.sign(wd).astype(f)
        g = gscale * sg if w is None else gscale * (np.asarray(w, dtype=f) * sg)
    assert g.dtype == f
    return R.store(g, store)


def ulp_half(v, store):
    """half a unit in the last place of the storage type at |v| (one rounding to nearest)"""
    v = np.abs(np.asarray(v, dtype=np.float64))
    bits = 8 if store == BF16 else 24
    with np.errstate(divide='ignore'):
        e = np.floor(np.log2(np.maximum(v, 2.0 ** -126)))
    return 2.0 ** (e - bits)
