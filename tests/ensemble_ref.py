"""
The ensemble scores (csrc/ensemble.hip, include/dlwpcs.h dlwpcs_ensemble_stats) restated in fp64, the error bounds of the fp32
kernel, an fp32 emulation of its arithmetic, and the table of cases that pins every plan its planner can choose.  Not a test
module: imported by test_ensemble_ref.py, test_ensemble.py (CPU) and test_gpu_ensemble.py.

reference(): members sorted with np.sort in fp64; mean, spread, A = mean |x_i - y|, B in the sorted form
2 sum_i (2 i - M - 1) x_(i) / M^2 (/ (M (M - 1)) fair), crps = A - B / 2, rank = #{x_i < y}.  pair_sum_brute() restates B as the
double sum.  An element with a NaN or infinite member is NaN / rank -1 everywhere, a NaN or infinite y in crps and rank.

Bounds.  u = 2^-24; A, B, x-bar, s are the fp64 values of the fp32 inputs; D = max_i |x_i - x-bar|.
    |crps - ref|   <= K_crps u (A + B / 2)          K_crps   = M + 7
    |spread - ref| <= K_spread u s                  K_spread = M / 2 + sqrt(M) + 4     (variance: 2 K_spread u s^2)
    |mean - ref|   <= 2 u |x-bar| + K_mean u D      K_mean   = 2 M
every K at or below the cap 2 M + 8.  They count the roundings of the algorithm that was built:

  crps.  The kernel forms d_i = x_i - y (one rounding, |error| <= u |d_i|; the score moves by at most 2 / M per unit of one d_i,
  so these cost 2 u A), sorts them (exact) and adds non-negative terms only: per gap the part below zero times k^2 and the part
  above times (M - k)^2 (the parts: one rounding each; min / max are exact), each into its own fma chain of M - 1 links (one
  rounding per link on a partial sum that never exceeds the final one): M u relative per chain.  Then (below + above) / M^2 + tail:
  three more roundings, M^2 and the tail are exact.  All terms >= 0, so this is (M + 3) u crps_std <= (M + 3) u A.  The fair form
  subtracts P = sum_k k (M - k) gap_k / (M^2 (M - 1)) = B_fair / (2 M): gap, M - 1 links, one division (M^2 (M - 1) < 2^24 is
  exact): (M + 1) u P <= (M + 1) u B / 2, and the subtraction adds u |crps| <= u (A + B / 2).  Sum: at most (M + 6) u (A + B / 2);
  one more for the second-order terms.
  spread.  t_i = x_i - x_1 (u |t_i| each; |t_i| <= |dev_i| + |dev_1| and Cauchy-Schwarz make that 2 (1 + sqrt(M)) u of the
  variance), tbar from a sequential sum (a shift c of tbar changes sum (t_i - tbar)^2 by M c^2 only: below u for M <= 128),
  dv_i = t_i - tbar (2 u), an fma chain of M squares (M u), the division (u): (M + 2 sqrt(M) + 5) u of the variance, half of it
  for the root, plus the root's own rounding and one for the second order.
  mean.  x_1 + tbar: the t_i cost 2 u D after averaging (|t_i| <= 2 D), the M - 2 additions 2 (M - 2) u D, the division u D,
  the last addition u |x-bar| (its operand errors are already counted): u |x-bar| + (2 M - 1) u D; one more for the second order.
test_ensemble_ref.py runs emulate_fp32() -- the same operations in numpy float32, with every fma split into a product and a sum,
which only adds roundings -- against all three bounds before any other test depends on them.

CASES: name, memory shape (contiguous), the permutation that makes the logical view, the member axis of that view, the byte skew
of the base pointer, how valid is given, and the plan tag (class, 16-byte loads, valid form, LDS) dlwpcs_ensemble_plan_info must
report.
"""
import itertools

import numpy as np

U = 2.0 ** -24
MAX_M = 128
CLASSES = (4, 8, 16, 32, 64, 128)
VEC_MAX_CLASS = 16
GPU_M = (2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65, 100, 128)      # the issue's list and both sides of every class boundary
GPU_E = (1, 63, 64, 65, 255, 257, 1000)


def class_of(M):
    return next(c for c in CLASSES if M <= c)


def k_crps(M):
    return M + 7.0


def k_spread(M):
    return M / 2.0 + np.sqrt(M) + 4.0


def k_mean(M):
    return 2.0 * M


# --------------------------------------------------------------------------------------------------------------------- #
# fp64 reference
# --------------------------------------------------------------------------------------------------------------------- #

def pair_sum_sorted(xs):
    """sum_ij |x_i - x_j| of members sorted along axis 0: 2 sum_i (2 i - M - 1) x_(i), i = 1..M"""
    M = xs.shape[0]
    coef = (2.0 * np.arange(1, M + 1) - M - 1).reshape((M,) + (1,) * (xs.ndim - 1))
    return 2.0 * (coef * xs).sum(axis=0)


def pair_sum_brute(x):
    """the same as the double sum, no sorting"""
    return np.abs(x[:, None] - x[None, :]).sum(axis=(0, 1))


def reference(x, y=None, fair=False, ddof=1, variance=False):
    """x (M, ...) float32 members first, y (...) float32 or None.  dict of fp64 fields: mean, spread, crps, rank (int32), and
    the quantities the bounds need: A, B, s, D, bad (member missing), miss (crps / rank missing)."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    M = x.shape[0]
    with np.errstate(invalid='ignore'):
        x64 = x.astype(np.float64)
    bad = ~np.isfinite(x64).all(axis=0)
    xs = np.sort(np.where(bad, 0.0, x64), axis=0)
    mean = xs.mean(axis=0)
    var = ((xs - mean) ** 2).sum(axis=0) / (M - ddof)
    out = {'bad': bad, 's': np.sqrt(var), 'D': np.abs(xs - mean).max(axis=0),
           'mean': np.where(bad, np.nan, mean), 'spread': np.where(bad, np.nan, var if variance else np.sqrt(var))}
    if y is not None:
        y = np.asarray(y)
        assert y.dtype == np.float32
        with np.errstate(invalid='ignore'):
            y64 = np.broadcast_to(y.astype(np.float64), x.shape[1:])
        miss = bad | ~np.isfinite(y64)
        y0 = np.where(miss, 0.0, y64)
        A = np.abs(xs - y0).mean(axis=0)
        B = pair_sum_sorted(xs) / (M * (M - 1) if fair else M * M)
        out.update(miss=miss, A=A, B=B, crps=np.where(miss, np.nan, A - B / 2.0),
                   rank=np.where(miss, -1, (xs < y0).sum(axis=0)).astype(np.int32))
    return out


def bounds(ref, M, variance=False):
    """dict of the bounds of mean, spread and (when the reference has it) crps"""
    b = {'mean': 2.0 * U * np.abs(np.where(ref['bad'], 0.0, ref['mean'])) + k_mean(M) * U * ref['D'],
         'spread': (2.0 * k_spread(M) * U * ref['s'] ** 2) if variance else k_spread(M) * U * ref['s']}
    if 'A' in ref:
        b['crps'] = k_crps(M) * U * (ref['A'] + ref['B'] / 2.0)
    return b


# --------------------------------------------------------------------------------------------------------------------- #
# the kernel's arithmetic in numpy float32, and its sorting network
# --------------------------------------------------------------------------------------------------------------------- #

def emulate_fp32(x, y=None, fair=False, ddof=1, variance=False):
    """mean, spread, crps as csrc/ensemble.hip forms them, operation by operation in float32 (fma = product then sum: two
    roundings where the kernel has one).  Finite inputs."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    M = x.shape[0]
    p = x[0]
    s = np.zeros(x.shape[1:], f)
    for i in range(1, M):
        s = s + (x[i] - p)
    tbar = s / f(M)
    q = np.zeros(x.shape[1:], f)
    for i in range(M):
        dv = (x[i] - p) - tbar
        q = q + dv * dv
    var = q / f(M - ddof)
    out = {'mean': p + tbar, 'spread': var if variance else np.sqrt(var)}
    if y is not None:
        d = np.sort(x - np.asarray(y, dtype=f), axis=0)
        zero = f(0)
        below = np.zeros(x.shape[1:], f)
        above = np.zeros(x.shape[1:], f)
        pair = np.zeros(x.shape[1:], f)
        for k in range(1, M):
            lo, hi = d[k - 1], d[k]
            below = below + f(k * k) * (np.minimum(hi, zero) - np.minimum(lo, zero))
            above = above + f((M - k) * (M - k)) * (np.maximum(hi, zero) - np.maximum(lo, zero))
            pair = pair + f(k * (M - k)) * (hi - lo)
        m2 = f(M * M)
        c = (np.maximum(d[0], zero) + np.maximum(-d[M - 1], zero)) + (below + above) / m2
        out['crps'] = c - pair / (m2 * f(M - 1)) if fair else c
    assert all(v.dtype == f for v in out.values())
    return out


def network(MC):
    """the compare-exchange passes of the kernel's bitonic network on MC slots (all ascending: a flip pass, then half-cleaners):
    a list of passes, each a list of (low slot, high slot)"""
    passes = []
    k = 2
    while k <= MC:
        passes.append([(i, i ^ (k - 1)) for i in range(MC) if (i ^ (k - 1)) > i])
        j = k // 4
        while j > 0:
            passes.append([(i, i ^ j) for i in range(MC) if (i ^ j) > i])
            j //= 2
        k *= 2
    return passes


def sort_lds_form(cols, run=32):
    """the LDS classes' order of the columns of cols (MC, n): runs of `run` slots through the network, then the stream merge --
    one head per run, the smallest leaves, ties go to the first run -- restated slot by slot"""
    MC, n = cols.shape
    runs = [apply_network(network(run), cols[r:r + run]) for r in range(0, MC, run)]
    out = np.empty_like(cols)
    for c in range(n):
        pos = [0] * len(runs)
        for k in range(MC):
            heads = [rn[p, c] if p < run else np.inf for rn, p in zip(runs, pos)]
            hi = min(heads)
            r = next(i for i, h in enumerate(heads) if h == hi and pos[i] < run) if any(p < run for p in pos) else None
            out[k, c] = hi
            if r is not None:
                pos[r] += 1
    return out


def apply_network(passes, cols):
    """cols (MC, n): run the passes on every column"""
    cols = np.array(cols, copy=True)
    for ps in passes:
        lo = np.array([a for a, _ in ps])
        hi = np.array([b for _, b in ps])
        a, b = cols[lo], cols[hi]
        cols[lo], cols[hi] = np.minimum(a, b), np.maximum(a, b)
    return cols


# --------------------------------------------------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------------------------------------------------- #

KINDS = ('white 0 / 0.01', 'white 280 / 0.01', 'white 0 / 30', 'white 280 / 30', 'ties', 'y is a member', 'y below all',
         'y above all', 'identical', 'nan member', 'inf member', 'nan y', '-inf y', 'nan member and inf y')
FINITE_KINDS = 9


def make_elements(rng, M, E, kinds=None, shift=0):
    """x (M, E) float32, y (E,) float32, kind (E,): element e is of kind kinds[(e + shift) % len(kinds)] (default: all KINDS)"""
    kinds = tuple(range(len(KINDS))) if kinds is None else tuple(kinds)
    kind = np.array([kinds[(e + shift) % len(kinds)] for e in range(E)])
    off = np.where(np.isin(kind, (1, 3)), 280.0, np.where(kind >= 4, rng.choice([0.0, 280.0, -55.0], E), 0.0))
    sc = np.where(np.isin(kind, (0, 1)), 0.01, np.where(np.isin(kind, (2, 3)), 30.0, 1.0))
    x = (off + sc * rng.standard_normal((M, E))).astype(np.float32)
    y = (off + sc * rng.standard_normal(E)).astype(np.float32)
    t = kind == 4
    x[:, t] = (off[t] + np.round(2.0 * rng.standard_normal((M, int(t.sum()))))).astype(np.float32)       # few distinct values
    y[t] = (off[t] + np.round(2.0 * rng.standard_normal(int(t.sum())))).astype(np.float32)
    pick = rng.integers(0, M, E)
    cols = np.arange(E)
    t = kind == 5
    y[t] = x[pick[t], cols[t]]
    t = kind == 6
    y[t] = x[:, t].min(axis=0) - np.float32(1.5)
    t = kind == 7
    y[t] = x[:, t].max(axis=0) + np.float32(1.5)
    t = kind == 8
    x[:, t] = x[0, t]
    xb, yb = x.view(np.uint32), y.view(np.uint32)
    for e in cols[np.isin(kind, (9, 13))]:
        xb[pick[e], e] = (0x7fc00001, 0xffc12345, 0x7f800001)[e % 3]                                     # NaN payloads
    for e in cols[kind == 10]:
        xb[pick[e], e] = (0x7f800000, 0xff800000)[e % 2]
    for e in cols[kind == 11]:
        yb[e] = (0x7fc00000, 0xffffffff)[e % 2]
    yb[kind == 12] = 0xff800000
    yb[kind == 13] = 0x7f800000
    return x, y, kind


# --------------------------------------------------------------------------------------------------------------------- #
# the case table
# --------------------------------------------------------------------------------------------------------------------- #

ABSENT, ELEM, VEC16 = -1, 0, 1


class Case(object):
    """mem: shape of the contiguous memory; perm: the permutation that gives the logical view; axis: the member axis of that
    view; skew: bytes added to the ensemble's 256-byte aligned base; valid: None, 'full' (contiguous, the logical element shape),
    or ('bcast', i): extent 1 at element dim i;  vskew likewise for valid.  tag = (class, vec, valid form, lds)."""

    def __init__(self, name, mem, perm, axis, tag, skew=0, valid='full', vskew=0):
        self.name, self.mem, self.perm, self.axis, self.tag = name, tuple(mem), tuple(perm), axis, tuple(tag)
        self.skew, self.valid, self.vskew = skew, valid, vskew

    def __repr__(self):
        return 'Case(%s)' % self.name

    @property
    def shape(self):
        return tuple(self.mem[p] for p in self.perm)

    @property
    def strides(self):
        st, n = [], 1
        for e in reversed(self.mem):
            st.insert(0, n)
            n *= e
        return tuple(st[p] for p in self.perm)

    @property
    def M(self):
        return self.shape[self.axis]

    @property
    def eshape(self):
        return tuple(e for i, e in enumerate(self.shape) if i != self.axis)

    @property
    def vshape(self):
        if self.valid is None:
            return None
        es = list(self.eshape)
        if self.valid != 'full':
            es[self.valid[1]] = 1
        return tuple(es)

    @property
    def vstrides(self):
        if self.valid is None:
            return None
        st, n = [], 1
        for e in reversed(self.vshape):
            st.insert(0, n)
            n *= e
        return tuple(st)


CASES = [
    # members first: the 16-byte form of every class that has one, its scalar twin by extent, by skew, by stride
    Case('first M=3 vec', (3, 5, 64), (0, 1, 2), 0, (4, 1, VEC16, 0)),
    Case('first M=4 odd extent', (4, 5, 63), (0, 1, 2), 0, (4, 0, ELEM, 0)),
    Case('first M=8 vec no valid', (8, 3, 68), (0, 1, 2), 0, (8, 1, ABSENT, 0), valid=None),
    Case('first M=7 skewed base', (7, 3, 68), (0, 1, 2), 0, (8, 0, ELEM, 0), skew=4),
    Case('first M=16 vec valid skewed', (16, 2, 132), (0, 1, 2), 0, (16, 1, ELEM, 0), vskew=4),
    Case('first M=15 vec valid broadcast rows', (15, 6, 44), (0, 1, 2), 0, (16, 1, VEC16, 0), valid=('bcast', 0)),
    Case('first M=15 vec valid broadcast lanes', (15, 6, 44), (0, 1, 2), 0, (16, 1, ELEM, 0), valid=('bcast', 1)),
    Case('first M=9 odd extent', (9, 257), (0, 1), 0, (16, 0, ELEM, 0)),
    Case('first M=17', (17, 4, 64), (0, 1, 2), 0, (32, 0, ELEM, 0)),
    Case('first M=32 no valid', (32, 255), (0, 1), 0, (32, 0, ABSENT, 0), valid=None),
    Case('first M=33', (33, 300), (0, 1), 0, (64, 0, ELEM, 1)),
    Case('first M=64 no valid', (64, 2, 129), (0, 1, 2), 0, (64, 0, ABSENT, 1), valid=None),
    Case('first M=65', (65, 130), (0, 1), 0, (128, 0, ELEM, 1)),
    Case('first M=128 valid broadcast', (128, 3, 50), (0, 1, 2), 0, (128, 0, ELEM, 1), valid=('bcast', 0)),
    # members in the middle and last
    Case('middle M=5 vec', (6, 5, 32), (0, 1, 2), 1, (8, 1, VEC16, 0)),
    Case('middle M=12 odd extent', (3, 12, 7, 9), (0, 1, 2, 3), 1, (16, 0, ELEM, 0)),
    Case('middle M=40', (3, 40, 70), (0, 1, 2), 1, (64, 0, ELEM, 1)),
    Case('last M=4', (9, 31, 4), (0, 1, 2), 2, (4, 0, ELEM, 0)),
    Case('last M=8', (5, 40, 8), (0, 1, 2), 2, (8, 0, ELEM, 0)),
    Case('last M=20', (7, 33, 20), (0, 1, 2), 2, (32, 0, ELEM, 0)),
    Case('last M=100', (130, 100), (0, 1), 1, (128, 0, ELEM, 1)),
    # permuted views: memory (b, M, a) seen as (a, M, b); memory (M, c, a, b) seen as (a, b, M, c)
    Case('permuted M=6 vec', (36, 6, 8), (2, 1, 0), 1, (8, 1, ELEM, 0)),
    Case('permuted M=10 vec', (10, 3, 4, 16), (2, 3, 0, 1), 2, (16, 1, ELEM, 0)),
    Case('permuted M=70', (66, 70, 3), (2, 1, 0), 1, (128, 0, ELEM, 1)),
]


# the valid form does not change the ensemble's path; the table need not cross it with every class, but every class and load form
# appears, and every valid form appears with both load forms that can carry it
def required_coverage():
    return {'class %d %s' % (c, 'vec' if v else 'scalar'): (lambda t, c=c, v=v: t[0] == c and t[1] == v)
            for c in CLASSES for v in ((0, 1) if c <= VEC_MAX_CLASS else (0,))} | \
           {'valid form %d with vec=%d' % (vm, v): (lambda t, vm=vm, v=v: t[2] == vm and t[1] == v)
            for v in (0, 1) for vm in ((ABSENT, ELEM, VEC16) if v else (ABSENT, ELEM))} | \
           {'lds %d' % l: (lambda t, l=l: t[3] == l) for l in (0, 1)}


def missing_coverage(cases):
    return [name for name, pred in required_coverage().items() if not any(pred(c.tag) for c in cases)]


def plan_of(case):
    """the tag dlwpcs_ensemble_plan_info reports for the case (host only)"""
    from DLWP import ops
    p = ops.ensemble_plan(case.shape, case.strides, case.axis, case.vshape, case.vstrides, ens_ptr=(1 << 20) + case.skew,
                          valid_ptr=None if case.valid is None else (1 << 21) + case.vskew)
    return (p['m_class'], int(p['vec']), p['valid'], int(p['lds'])), p


def case_arrays(case, rng):
    """(memory array of the ensemble, logical view, valid array or None, members-first view, valid broadcast to the elements)"""
    M = case.M
    n_el = int(np.prod(case.eshape))
    x, y, _ = make_elements(rng, M, n_el)
    logical = np.moveaxis(x.reshape((M,) + case.eshape), 0, case.axis)                  # logical view's values
    inv = np.argsort(case.perm)
    mem = np.ascontiguousarray(np.transpose(logical, inv))
    assert mem.shape == case.mem
    view = np.transpose(mem, case.perm)
    valid = None
    if case.valid is not None:
        valid = y.reshape(case.eshape)
        if case.valid != 'full':
            valid = np.ascontiguousarray(np.take(valid, [0], axis=case.valid[1]))
    return mem, view, valid


def subsets():
    names = ('mean', 'spread', 'crps', 'rank')
    return [c for r in range(1, 5) for c in itertools.combinations(names, r)]
