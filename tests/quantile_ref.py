"""
The grouped quantiles (csrc/quantile.hip, include/dlwpcs.h dlwpcs_group_quantile) restated column by column in fp64, the class
table of the planner, the inputs and the table of layout cases.  Not a test module: imported by test_quantile_ref.py,
test_quantile.py (CPU) and test_gpu_quantile.py.

Definition (the header's).  The members of a column are its entries that are not NaN, n of them; +-inf are values like any other,
-0 enters as +0.  n = 0: the quiet NaN 0x7fc00000, count 0.  Otherwise with the members sorted, in fp64 and without contraction,
    h = (n - 1) p;  j = floor(h);  g = h - j;  v = x_(j) if g == 0 else x_(j) + g (x_(j+1) - x_(j))
and v is rounded to fp32 once; a NaN v (inf - inf) is stored as 0x7fc00000.  Nothing is left to measure: the kernel selects
exactly x_(j) and x_(j+1) and performs these operations, so the tests compare bits.

CLASSES: rows x lanes of the staged form in the planner's order (the smallest that holds the longest group is taken), beyond the
last the long form.  P_CLASSES: the probability slots of an instantiation.

CASES: name, memory shape (contiguous), the permutation that makes the logical view, the row axis of that view, out_perm, the byte
skew of the base pointer, the group lengths, the number of probabilities, and the plan tag dlwpcs_group_quantile_plan_info must
report: (form, rows, lanes, probability class, grid).
"""
import numpy as np

CLASSES = ((64, 256), (128, 128), (256, 64), (640, 64))
P_CLASSES = (1, 2, 4, 8, 16)
LONG_THREADS = 256
MAX_PROBS = 16
STAGED, LONG = 0, 1
QNAN = np.uint32(0x7fc00000)

# both neighbours of every class boundary, the smallest groups and one long group; element counts around a wave and a workgroup
GPU_ROWS = (1, 2, 3, 63, 64, 65, 128, 129, 256, 257, 640, 641, 1500)
GPU_E = (1, 63, 64, 65, 257)
GPU_PROBS = {1: (0.5,), 2: (1. / 3., 2. / 3.), 3: (0., 1. / 3., 1.), 5: (0., 0.1, 1. / 3., 0.9, 1.),
             16: tuple(np.linspace(0., 1., 16))}


def class_of(rows, n_probs):
    """(form, rows of the class, lanes, probability class) the planner takes for a longest group of `rows` rows"""
    pc = next(c for c in P_CLASSES if n_probs <= c)
    for r, l in CLASSES:
        if rows <= r:
            return (STAGED, r, l, pc)
    return (LONG, 0, LONG_THREADS, pc)


def grid_of(n_groups, inner, lanes):
    n = n_groups * (-(-inner // lanes))
    gx = min(n, 65536)
    return (gx, -(-n // gx)) if n else (0, 0)


# --------------------------------------------------------------------------------------------------------------------- #
# fp64 reference
# --------------------------------------------------------------------------------------------------------------------- #

def quantile_column(col, probs):
    """the definition on one column of float32: (fp64 values before the rounding, n)"""
    col = np.asarray(col)
    assert col.dtype == np.float32
    m = np.sort(col[~np.isnan(col)].astype(np.float64) + 0.0)
    n = m.size
    out = np.full(len(probs), np.nan)
    if n:
        with np.errstate(invalid='ignore'):
            for q, p in enumerate(probs):
                h = np.float64(n - 1) * np.float64(p)
                j = np.floor(h)
                g = h - j
                xj = m[int(j)]
                out[q] = xj if g == 0 else xj + g * (m[int(j) + 1] - xj)
    return out, n


def to_fp32(v):
    """the one rounding, NaN made the quiet NaN"""
    with np.errstate(over='ignore', invalid='ignore'):
        r = np.asarray(v, dtype=np.float64).astype(np.float32)
    b = r.view(np.uint32).copy()
    b[np.isnan(r)] = QNAN
    return b.view(np.float32)


def reference(x, group_start, row_index, probs):
    """x (R, E) float32, CSR of groups of its rows: (quantiles (P, K, E) float32, counts (K, E) int32)"""
    x = np.asarray(x)
    R, E = x.shape
    K = len(group_start) - 1
    v = np.empty((len(probs), K, E), dtype=np.float64)
    cnt = np.empty((K, E), dtype=np.int32)
    for k in range(K):
        rows = x[np.asarray(row_index[group_start[k]:group_start[k + 1]], dtype=np.int64)]
        for e in range(E):
            v[:, k, e], cnt[k, e] = quantile_column(rows[:, e], probs)
    return to_fp32(v), cnt


# --------------------------------------------------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------------------------------------------------- #

KINDS = ('white', 'white 10 % NaN', 'ties 10 % NaN', 'all NaN', 'one member', 'zeros and denormals', 'infinities', 'negative 10 % NaN')
FINITE_KINDS = (0, 1, 2, 5, 7)          # every member finite (NaN entries are no members)


def make_columns(rng, R, E, shift=0):
    """x (R, E) float32, kind (E,): column e is of kind (e + shift) % len(KINDS)"""
    kind = np.array([(e + shift) % len(KINDS) for e in range(E)])
    x = (10.0 * rng.standard_normal((R, E))).astype(np.float32)
    holes = rng.random((R, E)) < 0.1
    rows = np.arange(R)
    for e in range(E):
        k = kind[e]
        if k == 2:
            x[:, e] = np.round(2.0 * x[:, e] / 10.0) * 0.5                      # values on a grid of 0.5: heavy ties
        elif k == 5:
            x[:, e] = rng.choice(np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000,
                                           0x3f800000, 0xbf800000], dtype=np.uint32), R).view(np.float32)
        elif k == 6:
            pick = rng.random(R)
            x[pick < 0.2, e] = np.inf
            x[pick > 0.8, e] = -np.inf
        elif k == 7:
            x[:, e] -= np.float32(280.0)
        if k in (1, 2, 6, 7):
            x[holes[:, e], e] = np.nan
        elif k == 3:
            x[:, e] = np.nan
        elif k == 4:
            keep = rng.integers(0, R)
            x[rows != keep, e] = np.nan
    xb = x.view(np.uint32)
    nanb = np.isnan(x)
    xb[nanb & (rng.random((R, E)) < 0.5)] = 0xffc12345                          # NaN payloads and signs
    return x, kind


def make_groups(rng, R, lens):
    """CSR of len(lens) groups of the R rows with these lengths (at most R each): rows drawn without order inside a group, and a
    row of the first non-empty group repeated as the first row of the next non-empty one (a row shared by two groups)"""
    start, index, shared = [0], [], None
    for n in lens:
        rows = rng.permutation(R)[:n]
        if n and shared is not None:
            rows[0] = shared
            shared = None
        elif n and not index:
            shared = int(rows[-1])
        index.extend(int(r) for r in rows)
        start.append(len(index))
    return np.array(start, dtype=np.int64), np.array(index, dtype=np.int64)


# --------------------------------------------------------------------------------------------------------------------- #
# the case table
# --------------------------------------------------------------------------------------------------------------------- #

class Case(object):
    """mem: shape of the contiguous memory; perm: the permutation that gives the logical view; axis: the row axis of that view;
    out_perm: the order of the logical dims in the output (None: unchanged); skew: bytes added to the 256-byte aligned base;
    lens: the group lengths; n_probs; tag = (form, rows, lanes, probability class, grid)."""

    def __init__(self, name, mem, perm, axis, lens, n_probs, tag, out_perm=None, skew=0):
        self.name, self.mem, self.perm, self.axis, self.lens, self.n_probs = name, tuple(mem), tuple(perm), axis, tuple(lens), n_probs
        self.tag, self.out_perm, self.skew = tuple(tag), out_perm, skew

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
    def inner(self):
        return int(np.prod([e for i, e in enumerate(self.shape) if i != self.axis]))


CASES = [
    Case('rows first, an empty group', (70, 3, 65), (0, 1, 2), 0, (64, 0, 5), 2, (STAGED, 64, 256, 2, (3, 1))),
    Case('rows in the middle', (3, 130, 65), (0, 1, 2), 1, (129,), 3, (STAGED, 256, 64, 4, (4, 1))),
    Case('rows last: lanes with a stride', (5, 9, 66), (0, 1, 2), 2, (65, 1), 1, (STAGED, 128, 128, 1, (2, 1))),
    Case('permuted view', (65, 40, 4), (2, 1, 0), 1, (33, 7), 5, (STAGED, 64, 256, 8, (4, 1))),
    Case('channels first to last', (20, 4, 6, 6), (0, 1, 2, 3), 0, (20,), 16, (STAGED, 64, 256, 16, (1, 1)), out_perm=(0, 2, 3, 1)),
    Case('skewed base', (10, 257), (0, 1), 0, (3, 2, 5), 2, (STAGED, 64, 256, 2, (6, 1)), skew=4),
    Case('largest staged class', (300, 70), (0, 1), 0, (257, 300), 2, (STAGED, 640, 64, 2, (4, 1))),
    Case('long form', (700, 67), (0, 1), 0, (700, 12), 3, (LONG, 0, 256, 4, (2, 1))),
    Case('long form, permuted', (67, 650), (1, 0), 0, (641,), 1, (LONG, 0, 256, 1, (1, 1))),
]


def plan_of(case):
    """the tag dlwpcs_group_quantile_plan_info reports for the case (host only)"""
    from DLWP import ops
    p = ops.group_quantile_plan(case.shape, case.strides, len(case.lens), max(case.lens), case.n_probs, row_axis=case.axis,
                                out_perm=case.out_perm)
    return (LONG if p['form'] == 'long' else STAGED, p['rows'], p['lanes'], p['p_class'], tuple(p['grid'])), p


def case_arrays(case, rng):
    """(memory array, logical view, group_start, row_index, probabilities)"""
    R, E = case.shape[case.axis], case.inner
    x, _ = make_columns(rng, R, E)
    eshape = tuple(e for i, e in enumerate(case.shape) if i != case.axis)
    logical = np.moveaxis(x.reshape((R,) + eshape), 0, case.axis)
    mem = np.ascontiguousarray(np.transpose(logical, np.argsort(case.perm)))
    assert mem.shape == case.mem
    gs, ri = make_groups(rng, R, case.lens)
    return mem, np.transpose(mem, case.perm), gs, ri, GPU_PROBS.get(case.n_probs, tuple(np.linspace(0., 1., case.n_probs)))


def case_reference(case, view, gs, ri, probs):
    """(quantiles (P,) + the output's shape, counts the output's shape) of the logical view"""
    R = case.shape[case.axis]
    eshape = tuple(e for i, e in enumerate(case.shape) if i != case.axis)
    q, c = reference(np.moveaxis(view, case.axis, 0).reshape(R, -1), gs, ri, probs)
    K = len(gs) - 1
    q = np.moveaxis(q.reshape((len(probs), K) + eshape), 1, case.axis + 1)
    c = np.moveaxis(c.reshape((K,) + eshape), 0, case.axis)
    if case.out_perm is not None:
        q = q.transpose((0,) + tuple(a + 1 for a in case.out_perm))
        c = c.transpose(case.out_perm)
    return np.ascontiguousarray(q), np.ascontiguousarray(c)
