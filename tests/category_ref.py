"""
The category scores of an ensemble (csrc/category.hip, include/dlwpcs.h dlwpcs_ensemble_category) restated in fp64, a float32
emulation of the kernel's arithmetic that reproduces its bits, the error bounds of the fp32 fields against fp64, the inputs and
the table of cases that pins every plan the planner can choose.  Not a test module: imported by test_category_ref.py,
test_category.py (CPU) and test_gpu_category.py.

Definition.  Per element with members x_1..x_M, thresholds t_0..t_{Q-1} and verification y: k_j = #{i : x_i <= t_j},
o_j = 1{y <= t_j};  prob_j = k_j / M;  brier_j = ((k_j - o_j M) / M)^2;  rps = sum_j brier_j, fair: minus
P = sum_j k_j (M - k_j) / (M^2 (M - 1));  rps_ref = sum_j (ref_j - o_j)^2;  code_j = 2 k_j + o_j.  A NaN or infinite member: NaN /
-1 everywhere; a NaN or infinite y: in brier, rps, rps_ref and code; a NaN t_j: in threshold j's outputs and in rps and rps_ref.

emulate_fp32() performs the header's operations one by one in numpy float32 -- (float)k / (float)M; (float)(k - o M) / (float)M,
squared; the sums from 0.f in threshold order; (float)pair / ((float)(M M) * (float)(M - 1)) -- every one rounded once, none
contracted: the kernel's bits.

Bounds of the fp32 fields against fp64, u = 2^-24, derived from those roundings (the integers k, o, M, k - o M, the pair sum
below 2^24 and M^2 <= 2^20 are exact in fp32):
    prob     one division:                                                  u prob
    brier    the division, then the square of a value that is off by u:     (1 + u)^3 - 1 < 3 u + second order  ->  4 u brier
    rps      Q terms of 3 u each, Q - 1 additions of non-negative terms (the first, to 0, is exact), one rounding per addition
             on a partial sum that never exceeds the final one:             (Q + 2) u S, S the standard score;
             fair: P costs the product M^2 (M - 1) (below 2^30: one rounding) and the division, 2 u P, and the subtraction
             u |S - P| <= u (S + P):                                        (Q + 3) u S + 3 u P
             and one more u (S + P) for the second order                    ->  (Q + 4) u S + 4 u P
    rps_ref  ref_j - o_j (one rounding), squared (3 u in all), Q - 1 additions:  (Q + 2) u R  ->  (Q + 3) u R
    code     exact.
test_category_ref.py holds the emulation against these bounds before any other test depends on them.

CASES: name, memory shape (contiguous), the permutation that makes the logical view, the member axis of that view, Q, how the
thresholds and the verification are given, byte skews of the three base pointers, and the plan tag (Q class, 16-byte loads of the
ensemble, valid form, threshold form) dlwpcs_ensemble_category_plan_info must report.
"""
import itertools

import numpy as np

U = 2.0 ** -24
MAX_M, MAX_Q = 1024, 16
Q_CLASSES = (1, 2, 4, 8, 16)
VEC_MAX_CLASS = 8
NAMES = ('prob', 'brier', 'rps', 'rps_ref', 'code')
PER_THRESHOLD = ('prob', 'brier', 'code')
GPU_M = (1, 2, 3, 5, 32, 33, 100, 320, 1024)
GPU_Q = (1, 2, 3, 4, 5, 8, 9, 16)
GPU_E = (1, 63, 64, 65, 257, 1000)
QNAN = np.uint32(0x7fc00000)


def class_of(Q):
    return next(c for c in Q_CLASSES if Q <= c)


def ref_probs(Q):
    """the climatological probabilities of Q equally likely category boundaries, as the float32 the descriptor carries"""
    return (np.arange(1, Q + 1) / (Q + 1.0)).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------------- #
# fp64 reference and the float32 emulation
# --------------------------------------------------------------------------------------------------------------------- #

def _counts(x, y, t):
    """k (Q, ...), o (Q, ...) or None, and the masks: bad (...) member missing, ybad (...), tnan (Q, ...)"""
    x, t = np.asarray(x), np.asarray(t)
    assert x.dtype == np.float32 and t.dtype == np.float32
    Q = t.shape[0]
    t = np.broadcast_to(t, (Q,) + x.shape[1:])
    with np.errstate(invalid='ignore'):
        bad = ~np.isfinite(x).all(axis=0)
        k = np.stack([(x <= t[j]).sum(axis=0) for j in range(Q)]).astype(np.int64)
        tnan = np.isnan(t)
        o = ybad = None
        if y is not None:
            y = np.broadcast_to(np.asarray(y), x.shape[1:])
            assert y.dtype == np.float32
            ybad = ~np.isfinite(y)
            o = (y[None] <= t).astype(np.int64)
    return k, o, bad, ybad, tnan


def reference(x, y, t, fair=False, ref_prob=None):
    """x (M, ...) float32 members first, y (...) float32 or None, t (Q, ...) float32 (broadcast against the elements), ref_prob
    (Q,) float32 or None.  dict of fp64 fields (code int32) with NaN / -1 where the definition says, and S, P, R without."""
    M = x.shape[0]
    k, o, bad, ybad, tnan = _counts(x, y, t)
    Q = k.shape[0]
    miss = bad[None] | tnan
    out = {'prob': np.where(miss, np.nan, k / float(M))}
    if y is None:
        return out
    ymiss = miss | ybad[None]
    whole = ymiss.any(axis=0)
    brier = ((k - o * M) / float(M)) ** 2
    S = brier.sum(axis=0)
    P = (k * (M - k)).sum(axis=0) / (float(M) * M * (M - 1)) if fair else np.zeros(S.shape)
    out.update(brier=np.where(ymiss, np.nan, brier), rps=np.where(whole, np.nan, S - P), S=S, P=P,
               code=np.where(ymiss, -1, 2 * k + o).astype(np.int32))
    if ref_prob is not None:
        rp = np.asarray(ref_prob)                   # as the caller holds them: float32 in the descriptor, float64 on the host path
        R = ((rp.astype(np.float64).reshape((Q,) + (1,) * (k.ndim - 1)) - o) ** 2).sum(axis=0)
        out.update(rps_ref=np.where(whole, np.nan, R), R=R)
    return out


def bounds(ref, Q):
    """dict of the bounds of the float fields the reference holds"""
    nz = lambda a: np.where(np.isnan(a), 0.0, a)      # noqa: E731
    b = {'prob': U * nz(ref['prob'])}
    if 'brier' in ref:
        b['brier'] = 4.0 * U * nz(ref['brier'])
        b['rps'] = (Q + 4.0) * U * ref['S'] + 4.0 * U * ref['P']
    if 'R' in ref:
        b['rps_ref'] = (Q + 3.0) * U * ref['R']
    return b


def _nan32(a, mask):
    a = np.array(a, dtype=np.float32, copy=True)
    a.view(np.uint32)[np.broadcast_to(mask, a.shape)] = QNAN
    return a


def emulate_fp32(x, y, t, fair=False, ref_prob=None):
    """the fields as csrc/category.hip forms them, operation by operation in numpy float32; NaN (0x7fc00000) / -1 where the
    definition says.  The kernel must give these bits."""
    f = np.float32
    M = x.shape[0]
    k, o, bad, ybad, tnan = _counts(x, y, t)
    Q = k.shape[0]
    fm = f(M)
    miss = bad[None] | tnan
    out = {'prob': _nan32(k.astype(f) / fm, miss)}
    if y is None:
        return out
    ymiss = miss | ybad[None]
    whole = ymiss.any(axis=0)
    e = (k - o * M).astype(f) / fm
    brier = e * e
    rps = np.zeros(k.shape[1:], f)
    for j in range(Q):
        rps = rps + brier[j]
    if fair:
        pair = (k * (M - k)).sum(axis=0)
        assert pair.max(initial=0) < 2 ** 24
        rps = rps - pair.astype(f) / (f(M * M) * f(M - 1))
    out.update(brier=_nan32(brier, ymiss), rps=_nan32(rps, whole), code=np.where(ymiss, -1, 2 * k + o).astype(np.int32))
    if ref_prob is not None:
        rp = np.asarray(ref_prob, dtype=f)
        ref = np.zeros(k.shape[1:], f)
        for j in range(Q):
            d = rp[j] - o[j].astype(f)
            ref = ref + d * d
        out['rps_ref'] = _nan32(ref, whole)
    assert all(v.dtype == (np.int32 if n == 'code' else f) for n, v in out.items())
    return out


# --------------------------------------------------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------------------------------------------------- #

KINDS = ('plain', 'y on a threshold', 'a member on a threshold', 'y below all', 'y above all', 'identical members',
         'infinite thresholds', 'nan member', 'inf member', 'nan y', 'inf y', 'nan threshold', 'nan member and nan threshold')
FINITE_KINDS = 7


def make_elements(rng, M, Q, E, kinds=None, shift=0, shared_thresholds=False):
    """x (M, E), y (E,), t (Q, E) float32 and kind (E,): element e is of kind kinds[(e + shift) % len(kinds)].  Every value lies
    on a grid of 0.25 around an offset, so that x == t and y == t happen by themselves and a `<` written for `<=` shows; the
    thresholds rise along Q (with ties).  shared_thresholds: one threshold vector for every element (the kinds that edit
    thresholds then fall back to 'plain')."""
    kinds = tuple(range(len(KINDS))) if kinds is None else tuple(kinds)
    kind = np.array([kinds[(e + shift) % len(kinds)] for e in range(E)])
    if shared_thresholds:
        kind[np.isin(kind, (6, 11, 12))] = 0
    off = rng.choice([0.0, 280.0, -55.0], 1 if shared_thresholds else E)
    grid = lambda a: (off + np.round(4.0 * a) / 4.0).astype(np.float32)      # noqa: E731
    x = grid(rng.standard_normal((M, E)))
    y = grid(rng.standard_normal(E))
    t = np.sort(grid(0.8 * rng.standard_normal((Q, 1 if shared_thresholds else E))), axis=0)
    t = np.array(np.broadcast_to(t, (Q, E)))
    cols = np.arange(E)
    pm, pq = rng.integers(0, M, E), rng.integers(0, Q, E)
    s = kind == 1
    y[s] = t[pq[s], cols[s]]
    s = kind == 2
    x[pm[s], cols[s]] = t[pq[s], cols[s]]
    s = kind == 3
    y[s] = np.minimum(x[:, s].min(axis=0), t[0, s]) - np.float32(1.0)
    s = kind == 4
    y[s] = np.maximum(x[:, s].max(axis=0), t[-1, s]) + np.float32(1.0)
    s = kind == 5
    x[:, s] = x[0, s]
    s = kind == 6
    t[0, s] = -np.inf
    t[-1, s & (cols % 2 == 0)] = np.inf
    xb, yb, tb = x.view(np.uint32), y.view(np.uint32), t.view(np.uint32)
    for e in cols[np.isin(kind, (7, 12))]:
        xb[pm[e], e] = (0x7fc00001, 0xffc12345, 0x7f800001)[e % 3]
    for e in cols[kind == 8]:
        xb[pm[e], e] = (0x7f800000, 0xff800000)[e % 2]
    for e in cols[kind == 9]:
        yb[e] = (0x7fc00000, 0xffffffff)[e % 2]
    for e in cols[kind == 10]:
        yb[e] = (0x7f800000, 0xff800000)[e % 2]
    for e in cols[np.isin(kind, (11, 12))]:
        tb[pq[e], e] = (0x7fc00000, 0xffc00001)[e % 2]
    return x, y, t, kind


def subsets():
    return [c for r in range(1, len(NAMES) + 1) for c in itertools.combinations(NAMES, r)]


# --------------------------------------------------------------------------------------------------------------------- #
# the case table
# --------------------------------------------------------------------------------------------------------------------- #

ABSENT, ELEM, VEC16, UNIFORM = -1, 0, 1, 2


def _contiguous(shape):
    st, n = [], 1
    for e in reversed(shape):
        st.insert(0, n)
        n *= e
    return tuple(st)


class Case(object):
    """mem: shape of the contiguous memory of the ensemble; perm: the permutation that gives the logical view; axis: the member
    axis of that view; Q; thr: 'full' (contiguous, threshold axis first, then the logical element shape), 'last' (the same with
    the threshold axis last), 'vector' (a bare (Q,) vector) or ('bcast', i): 'full' with extent 1 at element dim i; valid: None,
    'full' or ('bcast', i); skew / vskew / tskew: bytes added to the 256-byte aligned bases.
    tag = (Q class, vec, valid form, threshold form)."""

    def __init__(self, name, mem, perm, axis, Q, tag, thr='full', valid='full', skew=0, vskew=0, tskew=0):
        self.name, self.mem, self.perm, self.axis, self.Q, self.tag = name, tuple(mem), tuple(perm), axis, Q, tuple(tag)
        self.thr, self.valid, self.skew, self.vskew, self.tskew = thr, valid, skew, vskew, tskew

    def __repr__(self):
        return 'Case(%s)' % self.name

    @property
    def shape(self):
        return tuple(self.mem[p] for p in self.perm)

    @property
    def strides(self):
        st = _contiguous(self.mem)
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
    def tshape(self):
        if self.thr == 'vector':
            return (self.Q,)
        es = list(self.eshape)
        if isinstance(self.thr, tuple):
            es[self.thr[1]] = 1
        return tuple(es) + (self.Q,) if self.thr == 'last' else (self.Q,) + tuple(es)

    @property
    def taxis(self):
        return -1 if self.thr == 'last' else 0


CASES = [
    # members first: the 16-byte form of every class that has one, its scalar twin by extent, by skew, by class
    Case('first M=5 Q=2 vec', (5, 3, 64), (0, 1, 2), 0, 2, (2, 1, VEC16, VEC16)),
    Case('first M=3 Q=1 odd extent', (3, 5, 63), (0, 1, 2), 0, 1, (1, 0, ELEM, ELEM)),
    Case('first M=2 Q=1 vec', (2, 2, 64), (0, 1, 2), 0, 1, (1, 1, VEC16, VEC16)),
    Case('first M=33 Q=3 one threshold vector', (33, 4, 68), (0, 1, 2), 0, 3, (4, 1, VEC16, UNIFORM), thr='vector'),
    Case('first M=8 Q=9 class without a 16-byte form', (8, 2, 64), (0, 1, 2), 0, 9, (16, 0, ELEM, ELEM)),
    Case('first M=100 Q=8 skewed base', (100, 3, 68), (0, 1, 2), 0, 8, (8, 0, ELEM, ELEM), skew=4),
    Case('first M=7 Q=4 thresholds skewed', (7, 2, 132), (0, 1, 2), 0, 4, (4, 1, VEC16, ELEM), tskew=4),
    Case('first M=6 Q=5 valid skewed', (6, 3, 44), (0, 1, 2), 0, 5, (8, 1, ELEM, VEC16), vskew=4),
    Case('first M=9 Q=2 no valid', (9, 257), (0, 1), 0, 2, (2, 0, ABSENT, ELEM), valid=None),
    Case('first M=4 Q=8 vec no valid', (4, 3, 64), (0, 1, 2), 0, 8, (8, 1, ABSENT, VEC16), valid=None),
    Case('first M=12 Q=2 thresholds broadcast rows', (12, 6, 44), (0, 1, 2), 0, 2, (2, 1, VEC16, VEC16), thr=('bcast', 0)),
    Case('first M=12 Q=2 thresholds broadcast lanes', (12, 6, 44), (0, 1, 2), 0, 2, (2, 1, VEC16, ELEM), thr=('bcast', 1)),
    Case('first M=12 Q=4 valid broadcast lanes', (12, 6, 44), (0, 1, 2), 0, 4, (4, 1, ELEM, VEC16), valid=('bcast', 1)),
    Case('first M=5 Q=3 threshold axis last', (5, 4, 32), (0, 1, 2), 0, 3, (4, 1, VEC16, ELEM), thr='last'),
    Case('first M=320 Q=9', (320, 130), (0, 1), 0, 9, (16, 0, ELEM, ELEM)),
    Case('first M=1024 Q=16 one threshold vector', (1024, 65), (0, 1), 0, 16, (16, 0, ELEM, UNIFORM), thr='vector'),
    # members in the middle and last
    Case('middle M=5 Q=2 vec', (6, 5, 32), (0, 1, 2), 1, 2, (2, 1, VEC16, VEC16)),
    Case('middle M=40 Q=5 odd extent', (3, 40, 7, 9), (0, 1, 2, 3), 1, 5, (8, 0, ELEM, ELEM)),
    Case('last M=4 Q=4', (9, 31, 4), (0, 1, 2), 2, 4, (4, 0, ELEM, ELEM)),
    Case('last M=100 Q=16', (130, 100), (0, 1), 1, 16, (16, 0, ELEM, ELEM)),
    # permuted views: memory (b, M, a) seen as (a, M, b); valid and the thresholds are contiguous in the logical order
    Case('permuted M=6 Q=2 vec', (36, 6, 8), (2, 1, 0), 1, 2, (2, 1, ELEM, ELEM)),
    Case('permuted M=70 Q=3', (66, 70, 3), (2, 1, 0), 1, 3, (4, 0, ELEM, ELEM)),
]


def required_coverage():
    return {'class %d %s' % (c, 'vec' if v else 'scalar'): (lambda t, c=c, v=v: t[0] == c and t[1] == v)
            for c in Q_CLASSES for v in ((0, 1) if c <= VEC_MAX_CLASS else (0,))} | \
           {'valid form %d with vec=%d' % (vm, v): (lambda t, vm=vm, v=v: t[2] == vm and t[1] == v)
            for v in (0, 1) for vm in ((ABSENT, ELEM, VEC16) if v else (ABSENT, ELEM))} | \
           {'threshold form %d with vec=%d' % (tm, v): (lambda t, tm=tm, v=v: t[3] == tm and t[1] == v)
            for v in (0, 1) for tm in ((ELEM, VEC16, UNIFORM) if v else (ELEM, UNIFORM))}


def missing_coverage(cases):
    return [name for name, pred in required_coverage().items() if not any(pred(c.tag) for c in cases)]


def plan_of(case):
    """the tag dlwpcs_ensemble_category_plan_info reports for the case (host only)"""
    from DLWP import ops
    p = ops.ensemble_category_plan(case.shape, case.strides, case.tshape, _contiguous(case.tshape), case.axis, case.taxis,
                                   case.vshape, None if case.valid is None else _contiguous(case.vshape),
                                   ens_ptr=(1 << 20) + case.skew, valid_ptr=None if case.valid is None else (1 << 21) + case.vskew,
                                   thr_ptr=(1 << 22) + case.tskew)
    return (p['q_class'], int(p['vec']), p['valid'], p['thr']), p


def case_arrays(case, rng):
    """(memory array of the ensemble, its logical view, valid array or None, threshold array)"""
    M, Q = case.M, case.Q
    n_el = int(np.prod(case.eshape))
    x, y, t, _ = make_elements(rng, M, Q, n_el, shared_thresholds=case.thr == 'vector')
    logical = np.moveaxis(x.reshape((M,) + case.eshape), 0, case.axis)
    mem = np.ascontiguousarray(np.transpose(logical, np.argsort(case.perm)))
    assert mem.shape == case.mem
    view = np.transpose(mem, case.perm)
    valid = None
    if case.valid is not None:
        valid = y.reshape(case.eshape)
        if case.valid != 'full':
            valid = np.ascontiguousarray(np.take(valid, [0], axis=case.valid[1]))
    if case.thr == 'vector':
        thr = np.ascontiguousarray(t[:, 0])
    else:
        thr = t.reshape((Q,) + case.eshape)
        if isinstance(case.thr, tuple):
            thr = np.ascontiguousarray(np.take(thr, [0], axis=1 + case.thr[1]))
        if case.thr == 'last':
            thr = np.ascontiguousarray(np.moveaxis(thr, 0, -1))
    assert thr.shape == case.tshape
    return mem, view, valid, thr


def case_operands(case, view, valid, thr):
    """members first, the verification and the thresholds (threshold first) broadcast to the element shape: what reference() and
    emulate_fp32() take"""
    x = np.ascontiguousarray(np.moveaxis(view, case.axis, 0))
    y = None if valid is None else np.ascontiguousarray(np.broadcast_to(valid, case.eshape))
    if case.thr == 'vector':
        t = thr.reshape((case.Q,) + (1,) * len(case.eshape))
    else:
        t = np.moveaxis(thr, -1, 0) if case.thr == 'last' else thr
    return x, y, np.ascontiguousarray(np.broadcast_to(t, (case.Q,) + case.eshape))
