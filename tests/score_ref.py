"""
The score reduction (csrc/verify.hip, include/dlwpcs.h dlwpcs_score) restated in fp64, and the table of cases that pins every plan
the kernel's planner can choose.  Not a test module: imported by test_score_plan.py (CPU) and test_gpu_score_plans.py.

reference() is the header's addressing formula and per-method definitions, literally: strided fp64 views
(numpy.lib.stride_tricks.as_strided) over flat host copies of the buffers the kernel sees, so overlapping and stride-0 operands
are what they are in the kernel; n_f = clamp(min(t_len, t_cap - t_slope * f), 0); every term counts its own non-NaN entries;
an empty count is NaN; COS skips nothing.  It returns the value and the error bound of each output.

The bound is derived from the code, not measured.  u = 2^-24.  A term costs at most 4 fp32 roundings (ACC: two differences,
two products).  Terms are added in fp32 runs of at most 4 per slot in the row forms (SC_UNROLL: 3 additions) and at most 16 in
the column form (15 additions); everything after that is fp64.  So moment i is off by at most
    m_i = K * u * sum|term_i| / n_i,    K = 20 >= 4 + 15   (one K for all three forms; the column form sets it)
and MSE / MAE / MEAN are off by m_0, RMSE by m_0 / (2 rmse), ACC and COS by the first-order propagation
    m_0 / sqrt(M_1 M_2) + |r| (m_1 / M_1 + m_2 / M_2) / 2,
doubled for the neglected second order.  An fp32 output adds u * |value|.

CASES: every entry is a descriptor recipe (extents, one memory layout per operand), pointer skews in bytes, and the plan tag
    (form, slabs > 1, kc, cmode, wmode, indexed operand, grid y > 1)
the planner must report for it (dlwpcs_score_plan_info).  cmode / wmode are how the 16-byte form reads c / w; the other two forms
read every operand element by element whatever the mode says, so there a present operand is written AUX_ELEM.  Buffers are
exactly as large as the largest offset the descriptor reaches, plus one.  Shapes are the smallest that take the path:
column form when elems * kc < 256 or (n_out >= 131072 and elems <= 4096); several slabs need chunks >= 2 * 4096 and few
groups; a second grid dimension needs more than 65536 workgroups.
"""
import ctypes

import numpy as np
from numpy.lib.stride_tricks import as_strided

from DLWP import _native as nat

MSE, RMSE, MAE, ACC, COS, MEAN = nat.SCORE_MSE, nat.SCORE_RMSE, nat.SCORE_MAE, nat.SCORE_ACC, nat.SCORE_COS, nat.SCORE_MEAN
METHOD_NAMES = {MSE: 'mse', RMSE: 'rmse', MAE: 'mae', ACC: 'acc', COS: 'cos', MEAN: 'mean'}
ROW_SCALAR, ROW_VECTOR, COLUMN = 0, 1, 2
FORM_NAMES = {ROW_SCALAR: 'row scalar', ROW_VECTOR: 'row vector', COLUMN: 'column'}
AUX_ABSENT, AUX_ELEM, AUX_VEC, AUX_CELL = -1, 0, 1, 2
AUX_NAMES = {AUX_ABSENT: 'absent', AUX_ELEM: 'AUX_ELEM', AUX_VEC: 'AUX_VEC', AUX_CELL: 'AUX_CELL'}
OPS = 'abcw'
U = 2.0 ** -24
K_BOUND = 20
SC_NM = 6
CHUNK_ELEMS = 1 << 22              # reference: terms materialised at a time


def idx_operand(method):
    """the operand the indexed form looks up: 'c' for ACC / COS, else 'a'"""
    return 'c' if method in (ACC, COS) else 'a'


# --------------------------------------------------------------------------------------------------------------------- #
# The reference
# --------------------------------------------------------------------------------------------------------------------- #

def n_f_of(d, f):
    return max(min(int(d.t_len), int(d.t_cap) - int(d.t_slope) * f), 0)


def _dims(d, op, n_f):
    """(shape, strides in elements) of the view (keep..., kc, t < n_f, red...) of operand op for one lead"""
    shape = [int(d.keep_ext[i]) for i in range(d.n_keep)] + [int(d.kc), n_f] + [int(d.red_ext[i]) for i in range(d.n_red)]
    strides = [int(d.keep_stride[op][i]) for i in range(d.n_keep)] + [int(d.kc_stride[op]), int(d.t_stride[op])] + \
              [int(d.red_stride[op][i]) for i in range(d.n_red)]
    return shape, strides


def _reach(shape, strides):
    """largest element offset the view reaches (-1: it has no element)"""
    if any(e == 0 for e in shape):
        return -1
    assert all(s >= 0 for s in strides)
    return sum((e - 1) * s for e, s in zip(shape, strides))


def _view(buf, base, shape, strides):
    """bounds-checked strided view of the flat array buf"""
    r = _reach(shape, strides)
    assert r < 0 or base + r < buf.size, 'the descriptor reaches element %d of a buffer of %d' % (base + r, buf.size)
    if r < 0:
        return np.zeros(shape, buf.dtype)
    return as_strided(buf[base:], shape=shape, strides=[s * buf.itemsize for s in strides], writeable=False)


def lead_view(d, op, buf, f, rows=None, table_stride=0):
    """operand op (0..3) of lead f as a (keep..., kc, n_f, red...) array; rows: op is the indexed operand"""
    n_f = n_f_of(d, f)
    shape, strides = _dims(d, op, n_f)
    if rows is None:
        return _view(buf, f * int(d.lead_stride[op]), shape, strides)
    it = d.n_keep + 1
    r = np.asarray(rows, dtype=np.int64).reshape(d.n_lead, d.t_len)[f, :n_f]
    if n_f == 0 or _reach(shape, strides) < 0:
        return np.zeros(shape, buf.dtype)
    one = shape[:it] + shape[it + 1:]
    st = strides[:it] + strides[it + 1:]
    tab = _view(buf, 0, [int(r.max()) + 1] + one, [int(table_stride)] + st)
    return np.moveaxis(tab[r], 0, it)


def _moment(term, axes, skip):
    if skip:
        ok = ~np.isnan(term)
        t = np.where(ok, term, 0.0)
        return t.sum(axis=axes), np.abs(t).sum(axis=axes), ok.sum(axis=axes).astype(np.float64)
    n = 1
    for a in axes:
        n *= term.shape[a]
    s = term.sum(axis=axes)
    return s, np.abs(term).sum(axis=axes), np.full(s.shape, float(n))


def _finish(method, mom, out_f32):
    """value and bound from [(sum, sum of magnitudes, count)] per moment"""
    with np.errstate(invalid='ignore', divide='ignore'):
        M = [s / n for s, _, n in mom]
        m = [K_BOUND * U * sa / n for _, sa, n in mom]
        if method in (MSE, MAE, MEAN):
            val, bound = M[0], m[0]
        elif method == RMSE:
            val = np.sqrt(M[0])
            bound = m[0] / (2.0 * val)
        else:
            den = np.sqrt(M[1]) * np.sqrt(M[2]) if method == COS else np.sqrt(M[1] * M[2])
            val = M[0] / den
            bound = 2.0 * (m[0] / den + np.abs(val) * (m[1] / M[1] + m[2] / M[2]) / 2.0)
        if out_f32:
            bound = bound + U * np.abs(val)
    return val, bound


def reference(desc, a, b, c, w, rows=None, table_stride=0, out_f32=False):
    """(value, bound): fp64 arrays of n_out entries in the kernel's output order (f, keep..., k).
    a, b, c, w: flat host copies of the buffers the kernel is handed (None: absent); rows: the row table of the indexed form."""
    d = desc
    method = int(d.method)
    bufs = [None if x is None else np.asarray(x).astype(np.float64).reshape(-1) for x in (a, b, c, w)]
    iop = OPS.index(idx_operand(method)) if rows is not None else -1
    keep_total = 1
    for i in range(d.n_keep):
        keep_total *= int(d.keep_ext[i])
    per_lead = keep_total * int(d.kc)
    val = np.empty(d.n_lead * per_lead)
    bound = np.empty(d.n_lead * per_lead)
    nk = d.n_keep
    for f in range(d.n_lead):
        n_f = n_f_of(d, f)
        shape, _ = _dims(d, 0, n_f)
        axes = tuple(range(nk + 1, len(shape)))
        inner = int(np.prod(shape[1:], dtype=np.int64)) if nk else int(np.prod(shape, dtype=np.int64))
        k0 = shape[0] if nk else 1
        step = max(1, CHUNK_ELEMS // max(inner, 1))
        vals, bounds = [], []
        ops = []
        for op in range(4):
            if bufs[op] is None or (method == MEAN and op == 0):
                ops.append(None)
            else:
                ops.append(lead_view(d, op, bufs[op], f, rows if op == iop else None, table_stride))
        for lo in range(0, k0, step):
            sl = slice(lo, lo + step) if nk else Ellipsis
            y = ops[1][sl]
            x = ops[0][sl] if ops[0] is not None else None
            cv = ops[2][sl] if ops[2] is not None else 0.0
            wv = ops[3][sl] if ops[3] is not None else 1.0
            if method == MEAN:
                mom = [_moment(y + 0.0, axes, True)]
            elif method in (MSE, RMSE):
                mom = [_moment((y - x) ** 2 * wv, axes, True)]
            elif method == MAE:
                mom = [_moment(np.abs((y - x) * wv), axes, True)]
            elif method == ACC:
                av, af = y - cv, x - cv
                mom = [_moment(av * af * wv, axes, True), _moment(av * av * wv, axes, True), _moment(af * af * wv, axes, True)]
            else:
                av, af = y - cv, x - cv
                mom = [_moment(af * (av * wv), axes, False), _moment((af * wv) ** 2, axes, False),
                       _moment((av * wv) ** 2, axes, False)]
            v, bd = _finish(method, mom, out_f32)
            vals.append(np.asarray(v).reshape(-1))
            bounds.append(np.asarray(bd).reshape(-1))
        val[f * per_lead:(f + 1) * per_lead] = np.concatenate(vals)
        bound[f * per_lead:(f + 1) * per_lead] = np.concatenate(bounds)
    return val, bound


# --------------------------------------------------------------------------------------------------------------------- #
# Case recipes
# --------------------------------------------------------------------------------------------------------------------- #

class Case(object):
    """One recipe.  Logical dims are named f, t, k0.., r0.., c (the kc channels).  Every present operand has a layout:
         order   the dims in memory, outermost first (default f t k.. r.. c: channels last)
         zero    dims the operand is broadcast over (stride 0, no memory)
         pad     {dim: elements added to the dim's natural stride}
         same    {dim: other}: the dim takes the other dim's stride and no memory of its own (a continuous series: f like t)
         strides {dim: stride}: given outright (overlapping windows)
       tag = (form, slabs > 1, kc, cmode, wmode, indexed operand or None, grid y > 1)."""

    def __init__(self, name, method, tag, f=1, t=1, cap=None, slope=0, keep=(), red=(), kc=1, a=None, b=None, c=None, w=None,
                 skew=None, f32=False, idx=None, nan_group=None, plain=False):
        self.name, self.method, self.tag = name, method, tuple(tag)
        self.f, self.t, self.cap, self.slope = f, t, (t if cap is None else cap), slope
        self.keep, self.red, self.kc = tuple(keep), tuple(red), kc
        self.lay = {'a': a if method != MEAN else None, 'b': b if b is not None else {}, 'c': c, 'w': w}
        if method != MEAN and a is None:
            self.lay['a'] = {}
        self.skew = dict(skew or {})
        self.f32 = f32
        self.idx = idx                      # None or (table rows K, table row stride or None: the row span rounded up to 4)
        self.nan_group = nan_group          # output group whose b is all NaN
        self.plain = plain                  # expressible as contiguous arrays for DLWP.verify's numpy path

    def __repr__(self):
        return 'Case(%s)' % self.name

    @property
    def ext(self):
        e = {'f': self.f, 't': self.t, 'c': self.kc}
        e.update(('k%d' % i, x) for i, x in enumerate(self.keep))
        e.update(('r%d' % i, x) for i, x in enumerate(self.red))
        return e

    @property
    def dims(self):
        return ['f', 't'] + ['k%d' % i for i in range(len(self.keep))] + ['r%d' % i for i in range(len(self.red))] + ['c']

    def strides(self, op):
        lay = self.lay[op]
        ext = self.ext
        order = list(lay.get('order', self.dims))
        assert sorted(order) == sorted(self.dims), (self.name, op, order)
        zero, pad, same, given = set(lay.get('zero', ())), lay.get('pad', {}), lay.get('same', {}), lay.get('strides', {})
        st, run = {}, 1
        for n in reversed(order):
            if n in zero or n in same:
                st[n] = 0
                continue
            if n in given:
                st[n] = given[n]
                run = max(run, st[n] * max(ext[n], 1))
                continue
            st[n] = run + pad.get(n, 0)
            run = st[n] * max(ext[n], 1)
        for n, o in same.items():
            st[n] = st[o]
        return st


class Built(object):
    """a case made concrete: descriptor, host buffers (float32, None when absent), row table, sizes"""
    pass


def n_out_of(case):
    n = case.f * case.kc
    for e in case.keep:
        n *= e
    return n


def make_desc(case, method=None):
    d = nat.ScoreDesc()
    d.method = case.method if method is None else method
    d.n_lead, d.t_len, d.t_cap, d.t_slope = case.f, case.t, case.cap, case.slope
    d.n_keep, d.n_red, d.kc = len(case.keep), len(case.red), case.kc
    for i, e in enumerate(case.keep):
        d.keep_ext[i] = e
    for i, e in enumerate(case.red):
        d.red_ext[i] = e
    for k, op in enumerate(OPS):
        if case.lay[op] is None:
            continue
        st = case.strides(op)
        d.lead_stride[k], d.t_stride[k], d.kc_stride[k] = st['f'], st['t'], st['c']
        for i in range(len(case.keep)):
            d.keep_stride[k][i] = st['k%d' % i]
        for i in range(len(case.red)):
            d.red_stride[k][i] = st['r%d' % i]
    return d


def _size(d, op, table=None):
    """elements of operand op's buffer: the largest offset any lead reaches, plus one; table = (K, row stride)"""
    top = -1
    for f in range(d.n_lead):
        shape, strides = _dims(d, op, n_f_of(d, f))
        if table is not None:
            it = d.n_keep + 1
            shape, strides = shape[:it] + shape[it + 1:], strides[:it] + strides[it + 1:]
            r = _reach(shape, strides) if n_f_of(d, f) else -1
            if r >= 0:
                top = max(top, (table[0] - 1) * table[1] + r)
            continue
        r = _reach(shape, strides)
        if r >= 0:
            top = max(top, f * int(d.lead_stride[op]) + r)
    return top + 1


def row_span(case, op):
    """elements one table row spans (every dim but f and t)"""
    st, ext = case.strides(op), case.ext
    return 1 + sum((max(ext[n], 1) - 1) * st[n] for n in case.dims if n not in ('f', 't'))


def build(case, seed=None):
    """descriptor and seeded inputs of a case: normal values that differ element by element, positive weights, about 3 % NaN in
    b for the NaN-skipping methods, none for COS"""
    B = Built()
    B.case = case
    B.desc = d = make_desc(case)
    B.out_f32 = case.f32
    B.n_out = n_out_of(case)
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name)) if seed is None else seed)
    iop = idx_operand(case.method) if case.idx is not None else None
    B.rows, B.table_stride = None, 0
    if case.idx is not None:
        K, ts = case.idx
        B.table_stride = ts if ts is not None else -(-row_span(case, iop) // 4) * 4
        rows = rng.integers(0, K, case.f * case.t).astype(np.int32)
        rows[rng.integers(0, rows.size)] = K - 1
        B.rows = rows
    B.buf = {}
    for k, op in enumerate(OPS):
        if case.lay[op] is None:
            B.buf[op] = None
            continue
        n = _size(d, k, (case.idx[0], B.table_stride) if op == iop else None)
        x = rng.standard_normal(n).astype(np.float32)
        if op == 'w':
            x = (0.5 + np.abs(x)).astype(np.float32)
        B.buf[op] = x
    if case.method != COS:
        bb = B.buf['b']
        bb[rng.random(bb.size) < 0.03] = np.nan
        if case.nan_group is not None:
            g = case.nan_group
            kt = B.n_out // (case.f * case.kc)
            f, ko = divmod(g, kt)
            shape, strides = _dims(d, 1, n_f_of(d, f))
            v = as_strided(bb[f * int(d.lead_stride[1]):], shape=shape, strides=[s * 4 for s in strides])
            v[np.unravel_index(ko, case.keep) if case.keep else ()] = np.nan
    return B


def twin(case):
    """the COS twin of a non-COS case: the same extents, layouts, skews and row table scored as COS on NaN-free inputs, where a
    single read outside an operand (poison is NaN) makes the output NaN.  MEAN has no a: the twin's a is laid out like b.  An
    indexed a has no COS counterpart (COS looks up c): the table's layout and skew move to c, and a is laid out like b."""
    assert case.method != COS
    lay = dict(case.lay)
    skew = dict(case.skew)
    if case.method == MEAN:
        lay['a'] = dict(lay['b'])
        if 'b' in skew:
            skew['a'] = skew['b']
    if case.idx is not None and idx_operand(case.method) == 'a':
        lay['c'] = lay['a']
        lay['a'] = dict(lay['b'])
        if 'a' in skew:
            skew['c'] = skew.pop('a')
    t = Case(case.name + '-cos', COS, case.tag, f=case.f, t=case.t, cap=case.cap, slope=case.slope, keep=case.keep, red=case.red,
             kc=case.kc, a=lay['a'], b=lay['b'], c=lay['c'], w=lay['w'], skew=skew, f32=case.f32, idx=case.idx)
    return t


def materialised(B):
    """the indexed case with its table operand laid out over (lead, time): whole table rows copied in row-table order, so the
    strides keep their residues mod 4 and dlwpcs_score chooses the plan dlwpcs_score_indexed chose"""
    case = B.case
    op = idx_operand(case.method)
    k = OPS.index(op)
    ts = B.table_stride
    tab = B.buf[op]
    mat = np.zeros((B.rows.size, ts), np.float32)
    for i, r in enumerate(B.rows):
        row = tab[r * ts:(r + 1) * ts]
        mat[i, :row.size] = row
    M = Built()
    M.case, M.out_f32, M.n_out, M.rows, M.table_stride = case, B.out_f32, B.n_out, None, 0
    M.desc = make_desc(case)
    M.desc.lead_stride[k], M.desc.t_stride[k] = case.t * ts, ts
    M.buf = dict(B.buf)
    span = row_span(case, op)
    M.buf[op] = mat.reshape(-1)[:(B.rows.size - 1) * ts + span].copy()
    return M


def fake_pointers(case):
    """addresses with the residues the skews ask for (never dereferenced: dlwpcs_score_plan_info looks at NULL and alignment)"""
    return [None if case.lay[op] is None else 0x100000 * (k + 1) + case.skew.get(op, 0) for k, op in enumerate(OPS)]


def plan_info(lib, desc, ptrs, indexed, table_stride):
    info = (ctypes.c_int32 * 8)(*([-7] * 8))
    rc = lib.dlwpcs_score_plan_info(ctypes.byref(desc), ptrs[0], ptrs[1], ptrs[2], ptrs[3], 1 if indexed else 0,
                                    int(table_stride), info)
    return rc, list(info)


def tag_of(info, case, method=None):
    """the plan tag of a dlwpcs_score_plan_info answer, in the form the case table states it"""
    form = info[0]
    aux = [m if form == ROW_VECTOR or m < 0 else AUX_ELEM for m in info[2:4]]
    idx = idx_operand(case.method if method is None else method) if case.idx is not None else None
    return (form, info[1] > 1, case.kc, aux[0], aux[1], idx, info[5] > 1)


# --------------------------------------------------------------------------------------------------------------------- #
# The table
# --------------------------------------------------------------------------------------------------------------------- #

S, V, C = ROW_SCALAR, ROW_VECTOR, COLUMN
NO, EL, VE, CE = AUX_ABSENT, AUX_ELEM, AUX_VEC, AUX_CELL


def T(form, kc, c=NO, w=NO, multi=False, idx=None, gy=False):
    return (form, multi, kc, c, w, idx, gy)


SPATIAL = {'zero': ('f', 't', 'k0', 'c')}          # a field over the reduced dims only (latitude weights)
CELLS = {'zero': ('f', 't', 'c')}                  # a field over the kept and reduced dims, constant along the channels
CHANNELS = {'zero': ('f', 't')}                    # a field with channels, the same for every lead and time (a climatology)
FIRST = {'order': ['f', 't', 'c', 'k0', 'r0', 'r1']}    # channels first
VSHAPE = dict(f=2, t=3, keep=(2,), red=(5, 24))    # 360 elements per output: a workgroup per group, rows of whole float4s
SSHAPE = dict(f=2, t=3, keep=(2,), red=(5, 23))    # rows of 23 (x kc 1 or 2): no float4 rows
CSHAPE = dict(f=2, t=2, keep=(3,), red=(3, 5))     # 30 elements per output: a lane per output

CASES = []


def _add(*args, **kw):
    CASES.append(Case(*args, **kw))


# ---- every method on every form, kc 1 / 2 / 4 on every form, both output types
_add('vector_mse_kc1', MSE, T(V, 1, w=VE), w=SPATIAL, plain=True, **VSHAPE)
_add('vector_rmse_kc2', RMSE, T(V, 2), kc=2, f32=True, plain=True, **VSHAPE)
_add('vector_mae_kc4', MAE, T(V, 4, w=CE), kc=4, w=SPATIAL, plain=True, **VSHAPE)
_add('vector_acc_kc1', ACC, T(V, 1, c=VE, w=VE), c={}, w=SPATIAL, f32=True, plain=True, **VSHAPE)
_add('vector_cos_kc2', COS, T(V, 2, c=VE, w=EL), kc=2, c=CHANNELS, w=SPATIAL, plain=True, **VSHAPE)
_add('vector_mean_kc4', MEAN, T(V, 4), kc=4, f32=True, **VSHAPE)
_add('scalar_mse_kc2', MSE, T(S, 2, w=EL), kc=2, w=SPATIAL, f32=True, plain=True, **SSHAPE)
_add('scalar_rmse_kc4', RMSE, T(S, 4), kc=4, a=FIRST, **VSHAPE)
_add('scalar_mae_kc1', MAE, T(S, 1, w=EL), w=SPATIAL, f32=True, plain=True, **SSHAPE)
_add('scalar_acc_kc4', ACC, T(S, 4, c=EL, w=EL), kc=4, a=FIRST, c=CHANNELS, w=CELLS, **VSHAPE)
_add('scalar_cos_kc1', COS, T(S, 1, c=EL, w=EL), c=CHANNELS, w=SPATIAL, f32=True, plain=True, **SSHAPE)
_add('scalar_mean_kc2', MEAN, T(S, 2), kc=2, **SSHAPE)
_add('column_mse_kc4', MSE, T(C, 4, w=EL), kc=4, w=SPATIAL, plain=True, **CSHAPE)
_add('column_rmse_kc1', RMSE, T(C, 1), f32=True, plain=True, **CSHAPE)
_add('column_mae_kc2', MAE, T(C, 2, w=EL), kc=2, w=CELLS, plain=True, **CSHAPE)
_add('column_acc_kc2', ACC, T(C, 2, c=EL, w=EL), kc=2, c=CHANNELS, w=SPATIAL, f32=True, plain=True, **CSHAPE)
_add('column_cos_kc4', COS, T(C, 4, c=EL), kc=4, c={}, b=FIRST, **CSHAPE)
_add('column_mean_kc1', MEAN, T(C, 1), f32=True, **CSHAPE)

# ---- several slabs: Q = chunks of a group is divisible neither by the 3 slabs nor by 256, so slab edges fall inside rows
_add('slabs_scalar', MSE, T(S, 1, multi=True), red=(53, 233))                                   # Q = 12349
_add('slabs_scalar_kc2', RMSE, T(S, 2, multi=True), f=2, kc=2, red=(55, 113), f32=True)         # Q = 12430, rows of 226
_add('slabs_vector', ACC, T(V, 1, c=VE, multi=True), f=2, red=(211, 236), c={})                 # Q = 211 * 59 = 12449
_add('slabs_vector_kc4', MAE, T(V, 4, w=CE, multi=True), kc=4, red=(211, 59), w=SPATIAL, f32=True)

# ---- rows shorter than a workgroup's stride (row += col / cpr advances many rows at once): 300 rows, so that every lane
# ---- takes several chunks and the advance is used (with fewer than 256 chunks a lane never advances)
for _n in (3, 5, 7):
    _add('short_rows_%d_scalar' % _n, MSE, T(S, 1), f=2, keep=(2,), red=(300, _n))
    _add('short_rows_%d_vector' % _n, MAE, T(V, 4), f=2, kc=4, keep=(2,), red=(300, _n))

# ---- how the 16-byte form reads c and w
_add('aux_vec_vec_kc4', ACC, T(V, 4, c=VE, w=VE), kc=4, c={}, w=CHANNELS, **VSHAPE)
_add('aux_cell_cell', ACC, T(V, 4, c=CE, w=CE), kc=4, c=CELLS, w=CELLS, **VSHAPE)
_add('aux_elem_elem', ACC, T(V, 2, c=EL, w=EL), kc=2, c=CELLS, w={'zero': ('f',), 'pad': {'r0': 1}}, **VSHAPE)
_add('aux_broadcast_lead_or_time', COS, T(V, 1, c=VE, w=VE), c={'zero': ('f',)}, w={'zero': ('t',)}, **VSHAPE)
_add('aux_c_only_elem', ACC, T(V, 1, c=EL), c={'pad': {'k0': 2}}, **VSHAPE)
_add('aux_w_only_cell', MSE, T(V, 4, w=CE), kc=4, w=CELLS, **VSHAPE)

# ---- the silent scalar path: nothing is refused, 16-byte loads are just not possible
_add('quiet_row_not_x4', MSE, T(S, 2), t=3, kc=2, red=(4, 35))                                  # rows of 70, all contiguous
_add('quiet_odd_kept_stride', MSE, T(S, 1), a={'pad': {'k0': 1}}, **VSHAPE)
_add('quiet_odd_outer_stride', MSE, T(S, 1), b={'pad': {'r0': 1}}, **VSHAPE)
_add('quiet_odd_time_stride', MAE, T(S, 1), a={'pad': {'t': 3}}, **VSHAPE)
for _s in (4, 8, 12):
    _add('skew_a_%d' % _s, MSE, T(S, 1, w=EL), w=SPATIAL, skew={'a': _s}, **VSHAPE)
    _add('skew_b_%d' % _s, MSE, T(S, 1, w=EL), w=SPATIAL, skew={'b': _s}, **VSHAPE)
    _add('skew_c_%d' % _s, ACC, T(V, 1, c=EL, w=VE), c={}, w=SPATIAL, skew={'c': _s}, **VSHAPE)
    _add('skew_w_%d' % _s, ACC, T(V, 1, c=VE, w=EL), c={}, w=SPATIAL, skew={'w': _s}, **VSHAPE)
_add('skew_mean_b_4', MEAN, T(S, 1), skew={'b': 4}, **VSHAPE)

# ---- dimension structure
_add('outer0_keep1', MSE, T(V, 1), keep=(3,), red=(260,))
_add('outer3_no_merge', MAE, T(V, 1), t=3, keep=(2,), red=(2, 3, 2, 24), a={'pad': {'r0': 4, 'r1': 8, 'r2': 4}},
     b={'pad': {'r0': 8, 'r1': 4, 'r2': 4}})
_add('outer3_one_odd', MAE, T(S, 1), t=3, keep=(2,), red=(2, 3, 2, 24), a={'pad': {'r0': 4, 'r1': 1, 'r2': 4}},
     b={'pad': {'r0': 8, 'r1': 4, 'r2': 4}})
_add('keep0_column', COS, T(C, 1), t=2, red=(3, 5))
_add('keep0_vector', RMSE, T(V, 1), t=3, red=(5, 24))
_add('keep3_vector', RMSE, T(V, 1), f=2, t=3, keep=(2, 3, 2), red=(5, 24), a={'pad': {'k0': 4, 'k1': 8, 'k2': 4}},
     b={'pad': {'k0': 8, 'k1': 4, 'k2': 8}})
_add('keep3_column', MSE, T(C, 1), f=2, keep=(2, 3, 2), red=(7,), a={'pad': {'k0': 1, 'k1': 2, 'k2': 3}},
     b={'order': ['f', 't', 'r0', 'k2', 'k0', 'k1', 'c']})
_add('nred0_column', MSE, T(C, 2), f=2, t=3, keep=(5,), kc=2)
_add('nred0_rows', MAE, T(S, 1), f=2, t=300, keep=(2,))
_add('extent0_inner', ACC, T(C, 1, c=EL), f=2, t=2, keep=(3,), red=(5, 0), c={})
_add('extent0_outer', MSE, T(C, 1), f=2, t=2, keep=(3,), red=(0, 24))
_add('extent0_cos', COS, T(C, 1), f=2, t=2, keep=(3,), red=(0, 24))
_add('all_nan_group_vector', MSE, T(V, 1), nan_group=1, **VSHAPE)
_add('all_nan_group_scalar', ACC, T(S, 1, c=EL), c=CHANNELS, nan_group=2, **SSHAPE)
_add('all_nan_group_column', MAE, T(C, 1), nan_group=4, **CSHAPE)

# ---- lag: n_f = min(4, 5 - f) is 4 (clamped by t_len), 4, 3, 2, 1, 0, 0 (NaN); b is a continuous series (lead stride = time stride)
SERIES = {'same': {'f': 't'}}
_add('lag_vector', RMSE, T(V, 1), f=7, t=4, cap=5, slope=1, keep=(2,), red=(3, 24), b=SERIES)
_add('lag_scalar', MSE, T(S, 1, w=EL), f=7, t=4, cap=5, slope=1, keep=(2,), red=(3, 23), b=SERIES, w=SPATIAL)
_add('lag_column', MAE, T(C, 1), f=7, t=4, cap=5, slope=1, keep=(2,), red=(3, 5), b=SERIES)
_add('lag_slabs_vector', RMSE, T(V, 1, multi=True), f=4, t=5, cap=5, slope=2, red=(37, 236), b=SERIES)   # Q = 10915, 6549, 2183, 0
_add('lag_slope2_vector', ACC, T(V, 1, c=VE), f=4, t=3, cap=6, slope=2, keep=(2,), red=(4, 24), b=SERIES, c=CHANNELS)

# ---- indexed form: a of MSE / RMSE / MAE, c of ACC / COS, is a table of 5 rows looked up per (lead, time)
TABLE = {'zero': ('f', 't')}
for _m, _nm in ((MSE, 'mse'), (MAE, 'mae'), (ACC, 'acc'), (COS, 'cos')):
    _o = idx_operand(_m)
    _kw = {_o: TABLE}
    _aux = (lambda m: {'c': m}) if _o == 'c' else (lambda m: {})
    _add('indexed_%s_column' % _nm, _m, T(C, 1, idx=_o, **_aux(EL)), f=2, t=4, keep=(3,), red=(3, 5), idx=(5, None), **_kw)
    _add('indexed_%s_scalar' % _nm, _m, T(S, 1, idx=_o, **_aux(EL)), f=2, t=4, keep=(3,), red=(4, 23), idx=(5, None), **_kw)
    _add('indexed_%s_vector' % _nm, _m, T(V, 1, idx=_o, **_aux(VE)), f=2, t=4, keep=(3,), red=(4, 24), idx=(5, None), **_kw)
    _add('indexed_%s_slabs' % _nm, _m, T(V, 1, idx=_o, multi=True, **_aux(VE)), t=7, red=(31, 236), idx=(5, None), **_kw)
_add('indexed_rmse_slabs_scalar', RMSE, T(S, 1, idx='a', multi=True), t=7, red=(31, 59), kc=1, a=TABLE, idx=(4, None),
     b={'pad': {'r0': 1}}, f32=True)                                                           # Q = 217 * 59 = 12803
_add('indexed_a_stride_not_x4', MSE, T(S, 1, idx='a'), f=2, t=4, keep=(3,), red=(4, 24), idx=(5, 3 * 4 * 24 + 1), a=TABLE)
_add('indexed_c_stride_not_x4', ACC, T(V, 1, c=EL, idx='c'), f=2, t=4, keep=(3,), red=(4, 24), idx=(5, 3 * 4 * 24 + 2), c=TABLE)
_add('indexed_c_kc4', ACC, T(V, 4, c=VE, w=CE, idx='c'), f=2, t=4, kc=4, keep=(3,), red=(4, 6), idx=(5, None), c=TABLE, w=CELLS)

# ---- a second grid dimension: more than 65536 workgroups, small in memory through overlapping windows
WINDOW = {'strides': {'k0': 1, 'r0': 1}}
WINDOW4 = {'strides': {'k0': 4, 'r0': 1}}
GRID2_COLUMN_OUTPUTS = 65536 * 256 + 1
_add('grid2_column', MSE, T(C, 1, gy=True), keep=(GRID2_COLUMN_OUTPUTS,), red=(3,), a=WINDOW, b=WINDOW, f32=True)
_add('grid2_row_scalar', MSE, T(S, 1, gy=True), keep=(65600,), red=(256,), a=WINDOW, b=WINDOW)
_add('grid2_row_vector', MAE, T(V, 1, gy=True), keep=(65600,), red=(256,), a=WINDOW4, b=WINDOW4, f32=True)

GRID2 = ('grid2_column', 'grid2_row_scalar', 'grid2_row_vector')
BY_NAME = dict((c.name, c) for c in CASES)
assert len(BY_NAME) == len(CASES)


def required_combinations():
    """{description: predicate over a case} of every plan combination the table has to hold"""
    req = {}
    for form in (S, V, C):
        for m in (MSE, RMSE, MAE, ACC, COS, MEAN):
            req['%s form x %s' % (FORM_NAMES[form], METHOD_NAMES[m])] = \
                (lambda c, form=form, m=m: c.tag[0] == form and c.method == m)
        for kc in (1, 2, 4):
            req['%s form x kc %d' % (FORM_NAMES[form], kc)] = (lambda c, form=form, kc=kc: c.tag[0] == form and c.tag[2] == kc)
        for o in ('a', 'c'):
            req['indexed %s x %s form' % (o, FORM_NAMES[form])] = (lambda c, form=form, o=o: c.tag[0] == form and c.tag[5] == o)
        req['grid y > 1 x %s form' % FORM_NAMES[form]] = (lambda c, form=form: c.tag[0] == form and c.tag[6])
    for form in (S, V):
        for multi in (False, True):
            req['%s form x %s' % (FORM_NAMES[form], 'several slabs' if multi else '1 slab')] = \
                (lambda c, form=form, multi=multi: c.tag[0] == form and c.tag[1] == multi)
    for mode in (NO, EL, VE, CE):
        req['row vector form x cmode %s' % AUX_NAMES[mode]] = (lambda c, mode=mode: c.tag[0] == V and c.tag[3] == mode)
        req['row vector form x wmode %s' % AUX_NAMES[mode]] = (lambda c, mode=mode: c.tag[0] == V and c.tag[4] == mode)
    for o in ('a', 'c'):
        req['indexed %s x several slabs' % o] = (lambda c, o=o: c.tag[5] == o and c.tag[1])
    for f32 in (False, True):
        req['out_f32 = %d' % f32] = (lambda c, f32=f32: c.f32 == f32)
    return req


def missing_combinations(cases):
    return sorted(name for name, pred in required_combinations().items() if not any(pred(c) for c in cases))
