"""
Plain numpy references of the masked losses and of the missing-value fill of libdlwpcs (include/dlwpcs.h:
dlwpcs_loss_masked_fwd_bwd, dlwpcs_fill_missing), written from the header's text on top of tests/loss_ref.py.

  * an element is a HOLE iff its stored target is NaN; y is never inspected; at a hole d = 0 by a select and dy = +0.0;
  * `masked_values`: everything in fp64 on the stored values, with the sum of |term| of every sum over the valid elements
    (the error bars of tests/test_gpu_masked_loss.py scale with those: loss_ref.bar, no new tolerance);
  * `inv_f32`, `gscale_f32`: the fp32 coefficients of DLWPCS_NORM_VALID as the header forms them -- an fp64 quotient of two fp32
    values rounded once to fp32, i.e. the correctly rounded fp32 quotient, evaluated here in np.float32 arithmetic;
  * `dy_masked_f32`: the fp32 replica of the gradient, loss_ref.dy_f32 (products only) on the inputs with zeros at the
    holes and the divisor of the normalisation, +0.0 at the holes;
  * `fill_ref`: np.where(isnan(x), field, x).

tests/test_masked_loss_ref.py checks these against fp64 autograd of a restated nan-mean loss on the CPU, and that the case
tables cover what they are meant to cover.
"""
import numpy as np

import loss_ref as L
import stream_ref as R

ALL, VALID = 'all', 'valid'
NORMS = (ALL, VALID)
PAIRS = (('f32', 'f32'), ('bf16', 'bf16'), ('bf16', 'f32'))         # (storage of y and dy, storage of t)
DIV, PER = 14, 96                   # the per-cell weight field of the plain suite: C_out = 14 at N = 4
WRAP = 8 * (2 * L.SWEEP + 1001)     # the 8-wide kernel: two capped sweeps and a ragged third

# hole patterns: name -> what it is there for
PATTERNS = ('none', 'all', 'first', 'last', 'vector', 'lane', 'random', 'random_bad_y')


def holes(pattern, n, vec, seed=0):
    """boolean mask of the holes of an n-element case served by the 8-wide (vec) or the scalar kernel"""
    h = np.zeros(n, dtype=bool)
    if pattern == 'none':
        return h
    if pattern == 'all':
        h[:] = True
    elif pattern == 'first':
        h[0] = True
    elif pattern == 'last':
        h[n - 1] = True
    elif pattern == 'vector':               # one whole 8-element vector (not the first one)
        v = min(5, max(n // 8 - 1, 0))
        h[8 * v:8 * v + 8] = True
    elif pattern == 'lane':                 # every element lane 3 of workgroup 0 visits: its stride is grid * 256 items
        items = L.loss_items(n, vec)
        w = 8 if vec else 1
        for i in range(3, items, L.loss_grid(items) * 256):
            h[i * w:(i + 1) * w] = True
    else:
        assert pattern in ('random', 'random_bad_y'), pattern
        h = np.resize(np.random.default_rng(100 + seed).random(min(n, 1000003)) < 0.3, n)
    return h


def apply_holes(y, t, h, pattern):
    """(y, t) with NaN targets at the holes; 'random_bad_y': y = NaN on every other hole and +inf on the rest"""
    y, t = np.array(y, dtype=np.float32), np.array(t, dtype=np.float32)
    t[h] = np.nan
    if pattern == 'random_bad_y':
        at = np.flatnonzero(h)
        y[at[0::2]] = np.nan
        y[at[1::2]] = np.inf
    return y, t


def zeroed(y, t):
    """copies of y and t with zeros written at the holes: what DLWPCS_NORM_ALL equals the plain call on"""
    h = np.isnan(t)
    y0, t0 = np.array(y, dtype=np.float32), np.array(t, dtype=np.float32)
    y0[h] = 0.0
    t0[h] = 0.0
    return y0, t0


def masked_values(kind, y, t, w=None, lw=1.0, normalize=VALID):
    """fp64 masked loss of the flat stored arrays y, t (w: full-length field or None).  Returns a dict: loss (lw * S0 / D), mae
    (S1 / D), grad (d loss / d y, 0 at the holes), count, D, sums {'loss': sum |term|, 'mae': sum |d|} over the valid elements."""
    y = np.asarray(y, dtype=np.float64).ravel()
    t = np.asarray(t, dtype=np.float64).ravel()
    n = y.size
    h = np.isnan(t)
    count = int(n - h.sum())
    D = n if normalize == ALL else count
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64).ravel()
    with np.errstate(invalid='ignore'):
        d = np.where(h, 0.0, y - t)
    wd = w * d
    if kind == L.MSE:
        term, g = wd ** 2, 2.0 * w * wd
    else:
        assert kind == L.MAE, kind
        term, g = np.abs(wd), w * np.sign(wd)
    s0, s1 = term.sum(), np.abs(d).sum()
    if count == 0:
        return dict(loss=0.0, mae=0.0, grad=np.zeros(n), count=0, D=D, sums={'loss': 0.0, 'mae': 0.0})
    return dict(loss=float(lw) * s0 / D, mae=s1 / D, grad=np.where(h, 0.0, float(lw) * g / D), count=count, D=D,
                sums={'loss': s0, 'mae': s1})


def inv_f32(count):
    """(float)(1.0 / (double)(float)count) == the correctly rounded fp32 quotient 1.f / (float)count"""
    f = np.float32
    return f(1.0) / f(count)


def gscale_f32(kind, lw, count):
    """(float)((double)(lw * 2.f) / (double)(float)count) (MSE; lw for MAE) == the correctly rounded fp32 quotient"""
    f = np.float32
    return (f(lw) * f(2.0)) / f(count) if kind == L.MSE else f(lw) / f(count)


def dy_masked_f32(kind, y, t, w, lw, normalize, store):
    """fp32 replica of the stored gradient: +0.0 at the holes (and everywhere when nothing is valid), elsewhere
    loss_ref.dy_f32 -- gscale = the quotient above, then products only -- with the divisor of the normalisation."""
    t = np.asarray(t, dtype=np.float32).ravel()
    h = np.isnan(t)
    n = t.size
    D = n if normalize == ALL else int(n - h.sum())
    if D == 0:
        return np.zeros(n, dtype=np.float32)
    y0, t0 = zeroed(np.asarray(y, dtype=np.float32).ravel(), t)
    g = L.dy_f32(kind, y0, t0, w, lw, D, store)
    g[h] = 0.0
    return g


def fill_ref(x, fill, div, period):
    """x[e] = fill[(e / div) % period] where x[e] is NaN, flat float32 arrays (a bf16 case passes fill rounded to bf16)"""
    x = np.asarray(x, dtype=np.float32).ravel()
    return np.where(np.isnan(x), L.field(np.asarray(fill, dtype=np.float32), div, period, x.size), x).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ #
# case tables of tests/test_gpu_masked_loss.py
# ------------------------------------------------------------------------------------------------------------------ #
# Every case runs every hole pattern.  vec: n % 8 == 0 on 32-byte boundaries; scalar: the same n with one operand 16 bytes off a
# 32-byte boundary (`off`, in turn y, t, dy), or n % 8 != 0.  Sizes: 1000 (less than a workgroup of 8-wide items), 2408 (more than
# one workgroup, not a multiple of 256 items), and WRAP once per normalisation.  The tiny cases assign loss_out, the ragged
# ones add to it.
_OFFS = ((16, 0, 0), (0, 16, 0), (0, 0, 16))


def _cases():
    out, i = [], 0
    for kind in (L.MSE, L.MAE):
        for fld in (False, True):
            for pair in PAIRS:
                for norm in NORMS:
                    for cls, n in (('tiny', 1000), ('ragged', 2408)):
                        for path in ('vec', 'offset', 'odd'):
                            i += 1
                            out.append(dict(kind=kind, fld=fld, y=pair[0], t=pair[1], norm=norm, cls=cls,
                                            n=n - 3 if path == 'odd' else n, path=path,
                                            off=_OFFS[(i // 3) % 3] if path == 'offset' else (0, 0, 0),
                                            mode='overwrite' if cls == 'tiny' else 'accumulate', lw=0.75))
    return out


CASES = _cases()
WRAP_CASES = [dict(kind=L.MSE, fld=True, y='bf16', t='f32', norm=ALL, cls='wrap', n=WRAP, path='vec', off=(0, 0, 0),
                   mode='overwrite', lw=0.75),
              dict(kind=L.MAE, fld=False, y='f32', t='f32', norm=VALID, cls='wrap', n=WRAP, path='vec', off=(0, 0, 0),
                   mode='accumulate', lw=0.75)]


def case_vec(c):
    """the kernel the documented rule picks"""
    return L.loss_vec(c['n'], *c['off'])


# dlwpcs_fill_missing: dtype x (channels_last div = 1 | channels_first div = 6 N N, N = 2) x period x n x bytes past a 16-byte line.
# The launch has at most FILL_BLOCKS workgroups of 256 lanes with FILL_UNROLL 16-byte vectors each per sweep: FILL_WRAP vectors
# make the grid-stride loop go round twice and leave a ragged third sweep (the one size at which an index error of that loop shows).
FILL_BLOCKS, FILL_UNROLL = 2048, 4
FILL_SIZES = (1, 7, 1000, 2 * L.SWEEP + 1001)
FILL_WRAP = 2 * FILL_BLOCKS * 256 * FILL_UNROLL + 1001
FILL_CASES = [dict(dt=dt, div=div, per=per, n=n, off=off)
              for dt in ('f32', 'bf16') for div in (1, 24) for per in (3, 7) for n in FILL_SIZES
              for off in ((0, 4) if dt == 'f32' else (0, 4, 2))]
FILL_CASES += [dict(dt='f32', div=24, per=7, n=4 * FILL_WRAP + 3, off=4), dict(dt='bf16', div=1, per=3, n=8 * FILL_WRAP + 5, off=2)]


def fill_input(n, dt, seed=0):
    """stored values with NaNs of several payloads and either sign (about 30 %), -0.0, +-inf and subnormals among them"""
    rng = np.random.default_rng(seed + n % 9973)
    m = min(n, 1000003)
    x = R.store(rng.standard_normal(m).astype(np.float32), dt)
    r = rng.random(m)
    u = x.view(np.uint32)
    u[r < 0.10] = 0x7fc00000                        # the quiet NaN
    u[(r >= 0.10) & (r < 0.20)] = 0xffc10000        # negative, with a payload that survives bf16
    u[(r >= 0.20) & (r < 0.30)] = 0x7f810000        # signalling
    u[(r >= 0.30) & (r < 0.33)] = 0x80000000        # -0.0
    u[(r >= 0.33) & (r < 0.36)] = 0x7f800000        # +inf
    u[(r >= 0.36) & (r < 0.39)] = 0xff800000        # -inf
    u[(r >= 0.39) & (r < 0.42)] = 0x00010000        # subnormal (representable in bf16)
    return np.resize(x, n)
