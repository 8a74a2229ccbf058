"""
Reference, case tables and series makers of the block-bootstrap tests (test_resample_ref.py, test_gpu_resample.py,
test_gpu_resample_verify.py).  Not a test module.

reference(): the definition of dlwpcs_row_resample (include/dlwpcs.h) restated in numpy, bit for bit: resample b draws, in this
order, for block j = 0 .. nb-1 the rows (starts[b, j] + i) mod T, i = 0 .. L-1, the last block cut after n_draw - (nb - 1) L rows;
a block's entries are added in row order into a float64 sum from +0 (float32 widened, an explicit loop over the rows: strictly
sequential, never np.sum, which is pairwise), the block sums are added in draw order into the float64 total from +0, the counts
the same way; a NaN entry is skipped and not counted, +-inf are values; the value is one float64 division rounded to float32
once, QNAN = 0x7fc00000 where the count is below max(min_count, 1) (SKIP) or below n_draw (PROPAGATE), and every NaN is QNAN.
The loops run over blocks and rows; what is vectorised (resamples, columns) shares no sum.  reference_loops() is the same
statement with plain Python loops per resample and column over the list of drawn rows, for small cases.
"""
import numpy as np

STAGED_ROWS = 1280                                  # DLWPCS_RESAMPLE_STAGED_ROWS: the cap the plan query reports
SKIP, PROPAGATE = 0, 1
QNAN = np.uint32(0x7fc00000)

ROWS = [1, 2, 7, 64]                                # and cap - 1, cap, cap + 1 (CAP_ROWS) in the device test
COLUMNS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000]     # around a chunk (4), a wave / tile (64) and four tiles
RESAMPLES = [1, 2, 63, 64, 65, 300]
NAN_PATTERNS = ['none', 'one percent', 'nan row', 'nan column', 'one valid']
MODES = [(SKIP, 1), (SKIP, 3), (PROPAGATE, 1)]
LENGTHS = ['1', '2', '5', 'T-1', 'T']
DRAWS = ['T', 'T-1', '2T+1']


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def cap_rows(cap=STAGED_ROWS):
    return [cap - 1, cap, cap + 1]


def block_length(T, name):
    """the block length a LENGTHS name stands for at T rows, clipped into 1 .. T"""
    L = {'1': 1, '2': 2, '5': 5, 'T-1': T - 1, 'T': T}[name]
    return min(max(L, 1), T)


def n_draw(T, name):
    return max({'T': T, 'T-1': T - 1, '2T+1': 2 * T + 1}[name], 1)


def cases():
    """The size cases of the device test: every (T, columns) of ROWS x COLUMNS, with the resample count, block length, draw count,
    NaN pattern and mode rotating at strides that are coprime to the table lengths, so that each value of each table occurs
    (test_resample_ref.py checks that).  dict(T, E, B, L, L_name, n_draw, draw_name, pattern, mode, min_count, seed)."""
    out = []
    for it, T in enumerate(ROWS):
        for ie, E in enumerate(COLUMNS):
            i = it * len(COLUMNS) + ie
            ln, dn = LENGTHS[i % len(LENGTHS)], DRAWS[(i // 2) % len(DRAWS)]
            mode, mc = MODES[(i // 3) % len(MODES)]
            out.append(dict(T=T, E=E, B=RESAMPLES[(i + it) % len(RESAMPLES)], L=block_length(T, ln), L_name=ln, n_draw=n_draw(T, dn),
                            draw_name=dn, pattern=NAN_PATTERNS[(i + i // 5) % len(NAN_PATTERNS)], mode=mode, min_count=mc, seed=500 + i))
    return out


def make_series(rng, T, E, pattern='none', offset=250.0, scale=5.0):
    """float32 (T, E): red noise on an offset with the NaN pattern"""
    x = rng.standard_normal((T, E))
    for t in range(1, T):
        x[t] += 0.7 * x[t - 1]
    x = (x * scale + offset).astype(np.float32)
    if pattern == 'one percent':
        x[rng.random((T, E)) < 0.01] = np.nan
        x[T // 2, 0] = np.nan                       # (at least one, whatever the size)
    elif pattern == 'nan row':
        x[T // 2] = np.nan
    elif pattern == 'nan column':
        x[:, E // 2] = np.nan
    elif pattern == 'one valid':
        keep = x[T - 1, E - 1]
        x[:, E - 1] = np.nan
        x[T - 1, E - 1] = keep
    elif pattern != 'none':
        raise ValueError(pattern)
    return x


def make_starts(rng, T, B, L, draws=None, circular=True):
    """(B, nb) int32 block starts; circular: uniform on 0 .. T-1 and T - 1 itself is among them (a block of L > 1 wraps there);
    else uniform on 0 .. T-L (no block wraps)"""
    nd = T if draws is None else draws
    nb = -(-nd // L)
    st = rng.integers(0, T if circular else T - L + 1, size=(B, nb)).astype(np.int32)
    if circular and st.size:
        st[B - 1, nb - 1] = T - 1
        st[0, 0] = T - 1
    return st


def reference(x, starts, L=1, draws=None, mode=SKIP, min_count=1):
    """(values float32 (B, E), counts int32 (B, E)) of the (T, E) float32 series x: the definition, see above"""
    x = np.asarray(x, dtype=np.float32)
    st = np.asarray(starts, dtype=np.int64)
    T, E = x.shape
    B, nb = st.shape
    nd = T if draws is None else int(draws)
    assert 1 <= L <= T and nb == -(-nd // L)
    tot = np.zeros((B, E), dtype=np.float64)
    cnt = np.zeros((B, E), dtype=np.int32)
    with np.errstate(all='ignore'):
        for j in range(nb):
            s = np.zeros((B, E), dtype=np.float64)
            n = np.zeros((B, E), dtype=np.int32)
            for i in range(L if j < nb - 1 else nd - (nb - 1) * L):
                v = x[(st[:, j] + i) % T]
                ok = ~np.isnan(v)
                s = np.where(ok, s + v.astype(np.float64), s)
                n = n + ok
            tot = tot + s
            cnt = cnt + n
        need = max(int(min_count), 1) if mode == SKIP else nd
        val = (tot / np.maximum(cnt, 1).astype(np.float64)).astype(np.float32)
    out = np.where(cnt >= need, val, np.float32(np.nan)).astype(np.float32)
    out = bits(out).copy()
    out[np.isnan(out.view(np.float32))] = QNAN
    return out.view(np.float32), cnt


def drawn_rows(starts_b, T, L, draws):
    """the rows resample b draws, in order, as a list of blocks (lists of rows)"""
    nb = len(starts_b)
    return [[(int(starts_b[j]) + i) % T for i in range(L if j < nb - 1 else draws - (nb - 1) * L)] for j in range(nb)]


def reference_loops(x, starts, L=1, draws=None, mode=SKIP, min_count=1):
    """reference() with plain Python adds per resample and column over the list of drawn rows (Python floats are float64)"""
    x = np.asarray(x, dtype=np.float32)
    T, E = x.shape
    B = len(starts)
    nd = T if draws is None else int(draws)
    out = np.zeros((B, E), dtype=np.float32)
    cnt = np.zeros((B, E), dtype=np.int32)
    for b in range(B):
        blocks = drawn_rows(starts[b], T, L, nd)
        assert sum(len(r) for r in blocks) == nd
        for e in range(E):
            tot, n = 0.0, 0
            for rows in blocks:
                s, m = 0.0, 0
                for r in rows:
                    v = float(x[r, e])
                    if v == v:
                        s = s + v
                        m = m + 1
                tot = tot + s
                n = n + m
            need = max(int(min_count), 1) if mode == SKIP else nd
            cnt[b, e] = n
            with np.errstate(all='ignore'):
                out[b, e] = np.float32(np.float64(tot) / np.float64(n)) if n >= need else np.float32(np.nan)
    o = bits(out).copy()
    o[np.isnan(out)] = QNAN
    return o.view(np.float32), cnt
