"""
Every plan of the score reduction (csrc/verify.hip) on the device against the fp64 reference of score_ref.py, through the C ABI.

One test per case of score_ref.CASES, and one per COS twin of every non-COS case.  a, b, c, w, the row table, the scratch
(exactly dlwpcs_score_scratch_bytes) and out (exactly n_out elements) are carved from one hostile_mem.Arena -- exact size,
poisoned (every byte 0xFF: NaN), a guard band on both sides -- with the pointer skews applied inside the carve.  After the call:
the plan dlwpcs_score_plan_info reports for the real pointers is the case's tag; the NaN pattern is the reference's; every finite
output is within the reference's bound (score_ref.py: derived from the code, K = 20); no output element is still poison
(bitwise: a genuine NaN result is not poison); no guard byte changed; a second call gives the same bits.  An indexed case is
also compared bitwise with dlwpcs_score on the materialised operand.

Poison is NaN and five methods skip NaN, so a read outside an operand could pass unseen: the COS twin (score_ref.twin) scores the
same extents, layouts, skews and row table as COS on NaN-free inputs, where one such read makes the output NaN.  The non-COS
sizes are small enough that a dropped term moves the mean by more than the bound; the three cases with a second grid dimension
are the exception and rely on their twin and on the guards.

Every test prints `score-plan-fraction <case> <form> <largest |got - ref| / bound>`.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hostile_mem as H      # noqa: E402
import score_ref as R        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ARENA_BYTES = 900 << 20      # grid2_column: a, b and out of 64 MiB each between guards of 32 MiB

RUNS = []
for _c in R.CASES:
    RUNS.append((_c, None))
    if _c.method != R.COS:
        RUNS.append((R.twin(_c), _c))


@pytest.fixture(scope='module')
def arena():
    return H.Arena(ARENA_BYTES, DEV)


@pytest.fixture(scope='module')
def lib():
    from DLWP import _native as nat
    return nat.lib()


class _Placed(object):
    """the operands of a built case in the arena: device addresses, and the views the checks read"""

    def __init__(self, arena, B):
        self.ptr, self.raw = {}, {}
        case = B.case
        for op in R.OPS:
            buf = B.buf[op]
            if buf is None:
                self.ptr[op] = None
                continue
            sk = case.skew.get(op, 0)
            raw = arena.carve(buf.nbytes + sk, name='%s of %s' % (op, case.name))
            if buf.nbytes:
                raw[sk:].copy_(torch.from_numpy(buf).view(torch.uint8))
            self.ptr[op] = arena.base + arena.objects[-1].start + sk
            self.raw[op] = raw
            assert self.ptr[op] % 16 == sk % 16
        self.rows = None
        if B.rows is not None:
            raw = arena.carve(B.rows.nbytes, name='row table of %s' % case.name)
            raw.copy_(torch.from_numpy(B.rows).view(torch.uint8))
            self.rows = arena.base + arena.objects[-1].start
        self.skew = dict((op, case.skew.get(op, 0)) for op in self.raw)

    def pointers(self):
        return [self.ptr[op] for op in R.OPS]

    def assert_skew_bytes_untouched(self):
        for op, raw in self.raw.items():
            if self.skew[op]:
                assert bool(H.is_poison(raw[:self.skew[op]]).all()), 'the bytes in front of the skewed %s changed' % op


def _call(lib, arena, B, P, desc=None):
    """carve scratch and out, call the entry point twice; returns the output (numpy) after checking poison and repeatability"""
    from DLWP import _native as nat
    desc = B.desc if desc is None else desc
    nbytes = int(lib.dlwpcs_score_scratch_bytes(ctypes.byref(desc)))
    scratch = arena.carve(nbytes, name='scratch') if nbytes else None
    sp = arena.base + arena.objects[-1].start if nbytes else None
    out = arena.carve(B.n_out * (4 if B.out_f32 else 8), name='out')
    op_ = arena.base + arena.objects[-1].start
    p = P.pointers()
    bits = []
    for _ in range(2):
        out.fill_(H.POISON)
        if scratch is not None:
            scratch.fill_(H.POISON)
        with torch.cuda.device(DEV):
            if P.rows is not None:
                rc = lib.dlwpcs_score_indexed(ctypes.byref(desc), p[0], p[1], p[2], p[3], P.rows, int(B.table_stride), op_,
                                              1 if B.out_f32 else 0, sp, nbytes, nat.stream_ptr())
            else:
                rc = lib.dlwpcs_score(ctypes.byref(desc), p[0], p[1], p[2], p[3], op_, 1 if B.out_f32 else 0, sp, nbytes,
                                      nat.stream_ptr())
        assert rc == 0, lib.dlwpcs_last_error()
        torch.cuda.synchronize()
        bits.append(out.clone())
    assert torch.equal(bits[0], bits[1]), 'a second call gave other bits'
    view = out.view(torch.float32 if B.out_f32 else torch.float64)
    still = H.is_poison(view)
    assert not bool(still.any()), 'output element %d was never written' % int(torch.nonzero(still)[0])
    return view.cpu().numpy().astype(np.float64), bits[0]


@pytest.mark.parametrize('case,twin_of', RUNS, ids=[c.name for c, _ in RUNS])
def test_plan_against_fp64(lib, arena, case, twin_of):
    arena.reset()
    B = R.build(case)
    P = _Placed(arena, B)
    rc, info = R.plan_info(lib, B.desc, P.pointers(), case.idx is not None, B.table_stride)
    assert rc == 0, lib.dlwpcs_last_error()
    tag = R.tag_of(info, case)
    if twin_of is None:
        assert tag == case.tag, 'plan_info %s' % info
    else:
        assert tag[6] == case.tag[6]
        if not (case.idx is not None and R.idx_operand(twin_of.method) == 'a'):      # (that twin's a is laid out like b)
            assert (tag[0], tag[1]) == (case.tag[0], case.tag[1]), 'plan_info %s' % info
    val, bound = R.reference(B.desc, B.buf['a'], B.buf['b'], B.buf['c'], B.buf['w'], B.rows, B.table_stride, B.out_f32)
    got, bits = _call(lib, arena, B, P)
    assert got.shape == val.shape
    nan = np.isnan(val)
    assert np.array_equal(np.isnan(got), nan), 'NaN pattern: first difference at output %d (got %r, reference %r)' % (
        int(np.nonzero(np.isnan(got) != nan)[0][0]), got[np.nonzero(np.isnan(got) != nan)[0][0]],
        val[np.nonzero(np.isnan(got) != nan)[0][0]])
    if case.method == R.COS and not any(e == 0 for e in case.red) and case.slope == 0:
        assert not nan.any()                             # a twin's inputs hold no NaN: the reference has none to hand on
    ok = ~nan
    frac = 0.0
    if ok.any():
        assert (bound[ok] > 0).all()
        fr = np.abs(got[ok] - val[ok]) / bound[ok]
        frac = float(fr.max())
        i = int(np.argmax(fr))
        print('score-plan-fraction %s %s %.4f' % (case.name, R.FORM_NAMES[info[0]].replace(' ', '-'), frac))
        assert frac <= 1.0, 'output %d: got %.17g, reference %.17g, bound %.3g' % (
            np.nonzero(ok)[0][i], got[ok][i], val[ok][i], bound[ok][i])
    if case.idx is not None:
        M = R.materialised(B)
        PM = _Placed(arena, M)
        _, bits_m = _call(lib, arena, M, PM)
        assert torch.equal(bits, bits_m), 'the indexed form and dlwpcs_score on the materialised operand differ bitwise'
    P.assert_skew_bytes_untouched()
    arena.assert_guards()
