"""
Reference and case tables of the zonal spectrum tests (test_spectrum.py, test_gpu_spectrum.py).  Not a test module.

reference(): the definition, in float64 -- np.fft.rfft of the input widened to float64, c_k, the rows that count, the weighted
mean -- written group by group with plain loops, independently of DLWP.verify's vectorised numpy twin.  It also returns the
scale `m` of the device bound: the weighted mean over a group's counted rows of mean_j(x_j^2).

bound(): |P_k - ref_k| <= 4 (L + 2) 2^-24 m, the worst-case rounding bound of an fp32 dot product of length L with correctly
rounded twiddles; co and quad use sqrt(m_f m_v).  With remove_mean, m is the anomaly's mean square for k >= 1.  k = 0 then holds
the zonal mean squared itself, which the kernel forms in fp64 and stores as fp32: its error is the one rounding of a number of
the size of the FULL mean square, whatever the anomaly is, so k = 0 keeps the full mean square as m (the anomaly's would ask for
more digits of 280 K squared than an fp32 result holds).
"""
import itertools

import numpy as np

EPS = 2.0 ** -24
GPU_L = [2, 3, 4, 5, 8, 9, 12, 31, 32, 33, 45, 360, 1440]
ROWS = [1, 2, 31, 32, 33, 65]
GROUPS = [1, 3, 70]
N_WAVE = [1, 2, 33, None]
WEIGHTS = [None, 'full', 'broadcast', 'zeros']
NAN_BITS = (0x7FC00000, 0x7FA00000, 0xFFC00000, 0xFF800001, 0x7F800000, 0xFF800000)       # NaN payloads and +-inf


def c_k(L, K):
    c = np.full(K, 2.0)
    c[0] = 1.0
    if L % 2 == 0 and K == L // 2 + 1:
        c[K - 1] = 1.0
    return c


def full_k(L):
    return L // 2 + 1


def clip_wave(n_wave, L):
    return None if n_wave is None or n_wave >= full_k(L) else n_wave


def reference(f, v=None, axis=(), weights=None, n_wave=None, remove_mean=False):
    """
    f, v: arrays (..., L); axis: the averaged leading axes; weights: None or an array broadcasting against the leading shape.
    Returns (out (nq, kept..., K) float64, skipped (kept...) int64, m (2, kept..., K) float64: the bound's scale for f and v).
    """
    f = np.asarray(f, dtype=np.float64)
    pair = v is not None
    v = np.asarray(v, dtype=np.float64) if pair else f
    L = f.shape[-1]
    K = full_k(L) if n_wave is None else n_wave
    lead = f.shape[:-1]
    axis = tuple(sorted(a % len(lead) for a in axis)) if lead else ()
    kept = [i for i in range(len(lead)) if i not in axis]
    w = np.broadcast_to(np.ones(()) if weights is None else np.asarray(weights, dtype=np.float64), lead)
    perm = kept + list(axis)
    n_groups = int(np.prod([lead[i] for i in kept], dtype=np.int64))
    fr = f.transpose(perm + [len(lead)]).reshape(n_groups, -1, L)
    vr = v.transpose(perm + [len(lead)]).reshape(n_groups, -1, L)
    wr = w.transpose(perm).reshape(n_groups, -1)
    ck = c_k(L, K)
    nq = 4 if pair else 1
    out = np.full((nq, n_groups, K), np.nan)
    m = np.full((2, n_groups, K), np.nan)
    skipped = np.zeros(n_groups, dtype=np.int64)
    for g in range(n_groups):
        acc, accm, sw = np.zeros((nq, K)), np.zeros((2, K)), 0.0
        for r in range(fr.shape[1]):
            x, y = fr[g, r], vr[g, r]
            if not (np.isfinite(x).all() and np.isfinite(y).all()):
                skipped[g] += 1
                continue
            mx, my = x.mean(), y.mean()
            if remove_mean:
                X, Y = np.fft.rfft(x - mx)[:K], np.fft.rfft(y - my)[:K]
            else:
                X, Y = np.fft.rfft(x)[:K], np.fft.rfft(y)[:K]
            q = [ck * np.abs(X) ** 2 / L ** 2]
            if pair:
                q += [ck * np.abs(Y) ** 2 / L ** 2, ck * (X * np.conj(Y)).real / L ** 2, ck * (X * np.conj(Y)).imag / L ** 2]
            q = np.array(q)
            ms = np.array([np.full(K, ((x - mx * remove_mean) ** 2).mean()), np.full(K, ((y - my * remove_mean) ** 2).mean())])
            if remove_mean:
                q[0, 0] = mx * mx
                if pair:
                    q[1:, 0] = my * my, mx * my, 0.0
                ms[0, 0], ms[1, 0] = (x ** 2).mean(), (y ** 2).mean()
            acc += wr[g, r] * q
            accm += abs(wr[g, r]) * ms
            sw += wr[g, r]
        if sw != 0.0:
            out[:, g], m[:, g] = acc / sw, accm / abs(sw)
    shape = tuple(lead[i] for i in kept)
    return out.reshape((nq,) + shape + (K,)), skipped.reshape(shape), m.reshape((2,) + shape + (K,))


def bound(L, m, nq):
    """(nq, ..., K): the largest allowed |device - reference| per quantity"""
    b = 4.0 * (L + 2) * EPS
    if nq == 1:
        return b * m[:1]
    return b * np.stack([m[0], m[1], np.sqrt(m[0] * m[1]), np.sqrt(m[0] * m[1])])


def make_weights(kind, rng, groups, rows):
    """row weights for a (groups, rows, L) input averaged over axis 1"""
    if kind is None:
        return None
    if kind == 'full':
        return rng.uniform(0.1, 1.0, (groups, rows)).astype(np.float32)
    if kind == 'broadcast':                             # one weight per row position, the same in every group: stride 0
        return rng.uniform(0.1, 1.0, (rows,)).astype(np.float32)
    w = rng.uniform(0.1, 1.0, (groups, rows)).astype(np.float32)
    w[:, ::2] = 0.0                                     # a band: zeros and ones times a smooth weight
    return w


def make_field(rng, shape, kind='white', offset=0.0):
    """float32 test rows: white noise, red noise (a random walk along longitude) or noise on a large offset"""
    x = rng.standard_normal(shape)
    if kind == 'red':
        x = np.cumsum(x, axis=-1)
    return (x + offset).astype(np.float32)


def grid_cases(L):
    """the (rows per group, groups) grid for one L with the options rotating through it: every value of every option occurs"""
    out = []
    for i, (rows, groups) in enumerate(itertools.product(ROWS, GROUPS)):
        out.append(dict(rows=rows, groups=groups, n_wave=clip_wave(N_WAVE[i % 4], L), weights=WEIGHTS[(i // 2) % 4],
                        pair=bool(i % 2), remove_mean=bool((i // 3) % 2), kind=('white', 'red')[(i // 5) % 2]))
    return out


def spectrum_dims_reference(shape, strides, reduced):
    """what ops.spectrum_dims must produce, by brute force: every element offset of every (group, row) per operand, with groups
    and rows enumerated row-major over the kept / averaged axes.  Returns (offsets (n_ops, groups, rows))"""
    shape = tuple(shape)
    kept = [i for i in range(len(shape)) if i not in reduced]
    red = [i for i in range(len(shape)) if i in reduced]
    offs = []
    for st in strides:
        o = np.zeros(shape, dtype=np.int64)
        for i, (e, s) in enumerate(zip(shape, st)):
            idx = [None] * len(shape)
            idx[i] = slice(None)
            o = o + (np.arange(e, dtype=np.int64) * s)[tuple(idx)]
        offs.append(o.transpose(kept + red).reshape(int(np.prod([shape[i] for i in kept], dtype=np.int64)), -1))
    return np.array(offs)


def dims_offsets(dims, n_ops):
    """the offsets the kernel derives from a spectrum_dims list: (n_ops, groups, rows)"""
    kept = [(e, st) for e, st, k in dims if k]
    red = [(e, st) for e, st, k in dims if not k]

    def walk(part):
        o = np.zeros((n_ops, 1), dtype=np.int64)
        for e, st in part:
            step = np.array(st, dtype=np.int64)[:, None] * np.arange(e, dtype=np.int64)[None, :]
            o = (o[:, :, None] + step[:, None, :]).reshape(n_ops, -1)
        return o
    return walk(kept)[:, :, None] + walk(red)[:, None, :]
