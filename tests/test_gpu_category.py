"""
dlwpcs_ensemble_category on the device against the float32 emulation of category_ref.py, bit for bit: every fp32 operation of
the definition happens once and in the order the header states, so every float output, the codes and the NaN / -1 placement are
compared exactly.  Inputs, outputs and guards live in exact-size poisoned memory (hostile_mem.Arena): every output element must
have lost its poison and no guard byte may change.  Shapes: every M and Q of the lists in category_ref.py (both sides of every
class boundary) by element counts around a wave and a workgroup; thresholds per element, broadcast and as one bare vector; the
case table for the layouts; every subset of the outputs; the 16-byte form against the scalar form.
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
import category_ref as R     # noqa: E402
import score_ref as S        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def arena():
    return H.Arena(256 << 20, DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _place(arena, a, skew=0):
    """the contiguous numpy array a under guard, its first byte `skew` bytes behind a 256-byte line"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not skew:
        return arena.place(t.to(DEV))
    raw = arena.carve(a.nbytes + skew)
    v = raw[skew:].view(t.dtype).view(t.shape)
    v.copy_(t)
    return v


def _native(arena, ens, valid, thr, axis=0, taxis=0, want=None, fair=False, ref_prob=None):
    """dlwpcs_ensemble_category on guarded operands with poisoned exact-size outputs: dict of numpy fields, (Q,) + the element
    shape for the per-threshold ones"""
    from DLWP import ops
    from DLWP import _native as nat
    if want is None:
        want = ('prob',) if valid is None else tuple(n for n in R.NAMES if n != 'rps_ref' or ref_prob is not None)
    M, ms, Q, qs, eshape, order, merged = ops.category_layout(ens.shape, ens.stride(), thr.shape, thr.stride(), axis, taxis,
                                                              None if valid is None else valid.shape,
                                                              None if valid is None else valid.stride())
    d = ops.category_desc(M, ms, Q, qs, merged, fair, ref_prob)
    n = int(np.prod(eshape))
    outs = {k: arena.tensor((Q * n,) if k in R.PER_THRESHOLD else (n,), torch.int32 if k == 'code' else torch.float32, name=k)
            for k in want}
    p = lambda k: outs[k].data_ptr() if k in outs else None      # noqa: E731
    with torch.cuda.device(ens.device):
        nat.check(nat.lib().dlwpcs_ensemble_category(ctypes.byref(d), ens.data_ptr(), None if valid is None else valid.data_ptr(),
                                                     thr.data_ptr(), p('prob'), p('brier'), p('rps'), p('rps_ref'), p('code'),
                                                     torch.cuda.current_stream().cuda_stream), 'dlwpcs_ensemble_category')
    arena.assert_guards()
    res = {}
    perm = [order.index(i) for i in sorted(order)]
    for k, t in outs.items():
        if k != 'code':
            assert not bool(H.is_poison(t).any()), '%s: an element was never written' % k
        lead = (Q,) if k in R.PER_THRESHOLD else ()
        a = t.cpu().numpy().reshape(lead + tuple(eshape[i] for i in order))
        a = np.transpose(a, list(range(len(lead))) + [len(lead) + q for q in perm]) if order else a
        res[k] = a.reshape(lead + tuple(eshape))
    return res


def _same(got, emu, what):
    """every field the same bits as the emulation (NaN is the quiet NaN 0x7fc00000 there, the codes are int32)"""
    for k, g in got.items():
        e = emu[k]
        assert g.shape == e.shape and g.dtype == e.dtype, (what, k, g.shape, e.shape)
        if k == 'code':
            assert np.array_equal(g, e), '%s: code' % what
        else:
            assert np.array_equal(np.isnan(g), np.isnan(e)), '%s: NaN placement of %s' % (what, k)
            assert np.array_equal(_bits(g), _bits(e)), '%s: %d of %d values of %s differ' % (what, int((_bits(g) != _bits(e)).sum()), e.size, k)


@pytest.mark.parametrize('M', R.GPU_M)
def test_members_by_thresholds_by_elements(arena, M):
    rng = np.random.default_rng(M)
    for i, Q in enumerate(R.GPU_Q):
        E = R.GPU_E[(i + R.GPU_M.index(M)) % len(R.GPU_E)]
        arena.reset()
        x, y, t, _ = R.make_elements(rng, M, Q, E, shift=i)
        rp = R.ref_probs(Q)
        ens, val, thr = _place(arena, x), _place(arena, y), _place(arena, t)
        got = _native(arena, ens, val, thr, ref_prob=rp)
        _same(got, R.emulate_fp32(x, y, t, False, rp), 'M=%d Q=%d E=%d' % (M, Q, E))
        if M > 1:
            fair = _native(arena, ens, val, thr, want=('rps',), fair=True)
            _same(fair, R.emulate_fp32(x, y, t, True), 'fair M=%d Q=%d E=%d' % (M, Q, E))
        alone = _native(arena, ens, None, thr)
        _same(alone, R.emulate_fp32(x, None, t), 'prob alone M=%d Q=%d E=%d' % (M, Q, E))


@pytest.mark.parametrize('Q', R.GPU_Q)
def test_the_16_byte_form_gives_the_scalar_forms_bits(arena, Q):
    """every element count of the list that allows it (a multiple of 4) and 260, 1000: aligned (16-byte loads up to class 8) against
    the same operands 4 bytes off (one element per lane); thresholds per element and as one vector"""
    from DLWP import ops
    rng = np.random.default_rng(100 + Q)
    for E in (64, 260, 1000):
        for shared in (False, True):
            arena.reset()
            x, y, t, _ = R.make_elements(rng, 7, Q, E, shared_thresholds=shared)
            thr = np.ascontiguousarray(t[:, 0]) if shared else t
            a = _native(arena, _place(arena, x), _place(arena, y), _place(arena, thr), fair=True, ref_prob=R.ref_probs(Q))
            e4, v4, t4 = _place(arena, x, 4), _place(arena, y, 4), _place(arena, thr, 4)
            pa = ops.ensemble_category_plan(x.shape, e4.stride(), thr.shape, t4.stride(), valid_shape=y.shape, valid_strides=v4.stride())
            pb = ops.ensemble_category_plan(x.shape, e4.stride(), thr.shape, t4.stride(), valid_shape=y.shape, valid_strides=v4.stride(),
                                            ens_ptr=e4.data_ptr(), valid_ptr=v4.data_ptr(), thr_ptr=t4.data_ptr())
            assert pa['vec'] == (R.class_of(Q) <= R.VEC_MAX_CLASS) and not pb['vec'] and pa['q_class'] == pb['q_class'] == R.class_of(Q)
            b = _native(arena, e4, v4, t4, fair=True, ref_prob=R.ref_probs(Q))
            emu = R.emulate_fp32(x, y, t, True, R.ref_probs(Q))
            _same(a, emu, 'aligned Q=%d E=%d' % (Q, E))
            _same(b, emu, 'skewed Q=%d E=%d' % (Q, E))


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.name)
def test_layouts(arena, case):
    from DLWP import ops
    arena.reset()
    rng = np.random.default_rng(len(case.name) + case.M)
    mem, view, valid, thr = R.case_arrays(case, rng)
    ens = _place(arena, mem, case.skew).permute(case.perm)
    val = None if valid is None else _place(arena, valid, case.vskew)
    tt = _place(arena, thr, case.tskew)
    assert tuple(ens.shape) == case.shape and tuple(ens.stride()) == case.strides
    p = ops.ensemble_category_plan(ens.shape, ens.stride(), tt.shape, tt.stride(), case.axis, case.taxis,
                                   None if val is None else val.shape, None if val is None else val.stride(),
                                   ens_ptr=ens.data_ptr(), valid_ptr=None if val is None else val.data_ptr(), thr_ptr=tt.data_ptr())
    assert (p['q_class'], int(p['vec']), p['valid'], p['thr']) == case.tag
    rp = None if val is None else R.ref_probs(case.Q)
    fair = case.M > 1 and val is not None
    got = _native(arena, ens, val, tt, case.axis, case.taxis, fair=fair, ref_prob=rp)
    x, y, t = R.case_operands(case, view, valid, thr)
    emu = R.emulate_fp32(x, y, t, fair, rp)
    _same(got, emu, case.name)
    # the glue hands back the same bits, shaped like the ensemble without its member axis behind the threshold dim
    glue = ops.ensemble_category(ens, val, tt, member_axis=case.axis, threshold_axis=case.taxis, fair=fair, ref_prob=rp)
    assert set(glue) == set(got)
    for k, g in glue.items():
        assert tuple(g.shape) == emu[k].shape and np.array_equal(_bits(g.cpu().numpy()), _bits(emu[k])), k


@pytest.mark.parametrize('M,Q,E', [(5, 2, 256), (5, 3, 257), (33, 9, 65), (320, 16, 130)])
def test_every_subset_of_the_outputs(arena, M, Q, E):
    arena.reset()
    x, y, t, _ = R.make_elements(np.random.default_rng(M + E), M, Q, E)
    rp = R.ref_probs(Q)
    ens, val, thr = _place(arena, x), _place(arena, y), _place(arena, t)
    full = _native(arena, ens, val, thr, fair=True, ref_prob=rp)
    _same(full, R.emulate_fp32(x, y, t, True, rp), 'all outputs M=%d' % M)
    for want in R.subsets():
        got = _native(arena, ens, val, thr, want=want, fair=True, ref_prob=rp)
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(_bits(got[k]), _bits(full[k])), (want, k)


def test_refusals_launch_nothing(arena):
    from DLWP import ops
    arena.reset()
    x, y, t, _ = R.make_elements(np.random.default_rng(9), 4, 2, 64, kinds=range(R.FINITE_KINDS))
    ens, val, thr = _place(arena, x), _place(arena, y), _place(arena, t)
    for want in (('brier',), ('rps',), ('code',), ('prob', 'rps_ref')):
        with pytest.raises(ValueError, match='verification'):
            _native(arena, ens, None, thr, want=want, ref_prob=R.ref_probs(2))
    with pytest.raises(ValueError, match='verification'):
        ops.ensemble_category(ens, None, thr, want=('brier',))
    with pytest.raises(ValueError, match='ref_prob'):
        ops.ensemble_category(ens, val, thr, want=('rps_ref',))
    with pytest.raises(NotImplementedError, match='1024'):
        ops.ensemble_category(torch.zeros(1025, 4, device=DEV), None, thr[:, :4])
    with pytest.raises(NotImplementedError, match='16'):
        ops.ensemble_category(ens, None, torch.zeros(17, device=DEV))
    with pytest.raises(ValueError, match='fair'):
        ops.ensemble_category(ens[:1], val, thr, fair=True)
    with pytest.raises(TypeError):
        ops.ensemble_category(ens.double(), val, thr)
    out = ops.ensemble_category(torch.zeros(4, 0, 3, device=DEV), torch.zeros(0, 3, device=DEV), torch.zeros(2, device=DEV))
    assert out['prob'].shape == (2, 0, 3) and out['rps'].shape == (0, 3)
    arena.assert_guards()


def test_grand_ensemble_end_to_end():
    """320 members against climatological terciles on the device, through the public interface, against the host path: the
    fields' derived bounds (category_ref) carried through the weighted means, plus the score reduction's K u mean |term|
    (score_ref.K_BOUND, two more for the weight's rounding to fp32 and the product with it); the counts are exact."""
    from DLWP import verify as V
    from DLWP.model.extensions import Forecast
    rng = np.random.default_rng(21)
    dims = ('f_hour', 'time', 'face', 'height', 'width', 'varlev')
    shape = (2, 3, 6, 4, 4, 2)
    Mg, Q = 320, 2
    co = {d: np.arange(n) for d, n in zip(dims, shape)}
    g = lambda a: (280 + np.round(8 * a) / 8).astype(np.float32)      # noqa: E731
    truth, x = g(2 * rng.standard_normal(shape)), g(2 * rng.standard_normal((Mg,) + shape) + 0.3)
    t = np.sort(g(1.2 * rng.standard_normal((Q,) + shape)), axis=0)
    x[7, 1, 2, 3, 1, 1, 0] = np.nan
    truth[0, 1, 5, 3, 3, 1] = np.nan
    t[1, 1, 0, 0, 2, 2, 1] = np.nan
    lat = Forecast(rng.uniform(-85, 85, (6, 4, 4)), dims[2:5], {d: co[d] for d in dims[2:5]})

    def make(up):
        val = Forecast(up(truth), dims, co)
        val.lat = lat
        ens = Forecast(up(x), ('member',) + dims, dict(co, member=np.arange(Mg)))
        return ens, val, Forecast(up(t), ('quantile',) + dims, dict(co, quantile=np.array([0.25, 0.75])))

    host, dev = make(lambda a: a), make(lambda a: torch.from_numpy(a).to(DEV))
    ax = (1, 2, 3, 4)
    w = np.cos(np.deg2rad(lat.values))
    w = (w / w.mean()).reshape(1, 1, 6, 4, 4, 1)
    nm = lambda a: V._nanmean(a * w, ax)      # noqa: E731
    KU = (S.K_BOUND + 2) * S.U
    rp = np.array([0.25, 0.75], dtype=np.float32)                     # exact in fp32: both paths hold the same reference forecast
    lim = {}
    for fair in (False, True):
        ref = R.reference(x, truth, t, fair, rp)
        bd = R.bounds(ref, Q)
        hole = np.isnan(ref['rps'])
        e_rps = nm(np.where(hole, np.nan, bd['rps'])) + KU * nm(np.abs(ref['rps']))
        e_ref = nm(np.where(hole, np.nan, bd['rps_ref'])) + KU * nm(ref['rps_ref'])
        a, b = nm(ref['rps']), nm(ref['rps_ref'])
        pre = 'fair_' if fair else ''
        lim[pre + 'rps'] = e_rps
        lim[pre + 'rpss'] = 1.01 * (e_rps / b + np.abs(a) * e_ref / b ** 2)
        if not fair:
            lim['brier'] = np.stack([nm(np.where(np.isnan(ref['brier'][j]), np.nan, bd['brier'][j])) + KU * nm(ref['brier'][j])
                                     for j in range(Q)], axis=-1)
    for m in V._CAT_METHODS:
        kw = dict(axis=ax, weighted=True, probabilities=(0.25, 0.75) if m.endswith('rpss') else None)
        want, got = V.categorical_error(*host, m, **kw), V.categorical_error(*dev, m, **kw)
        assert got.dtype == np.float64 and got.shape == want.shape == ((2, 2, Q) if m == 'brier' else (2, 2)) and np.isfinite(got).all()
        err = np.abs(got - want)
        print('%s: largest |error| / bound = %.4f' % (m, float((err / lim[m]).max())))
        assert (err <= lim[m]).all(), m
    # fields come back on the device, labelled; the reliability counts are exact
    b = V.brier_score(*dev)
    assert isinstance(b, Forecast) and b.dims == ('quantile',) + dims and b.values.is_cuda and tuple(b.values.shape) == (Q,) + shape
    emu = R.emulate_fp32(x, truth, t)
    assert np.array_equal(_bits(b.values.cpu().numpy()), _bits(emu['brier']))
    p = V.ensemble_probability(dev[0], dev[2])
    assert p.values.is_cuda and np.array_equal(_bits(p.values.cpu().numpy()), _bits(emu['prob']))
    r = V.ranked_probability_score(*dev)
    assert r.dims == dims and np.array_equal(_bits(r.values.cpu().numpy()), _bits(emu['rps']))
    cd, ch = V.reliability_counts(*dev, axis=ax), V.reliability_counts(*host, axis=ax)
    assert cd.dims == ch.dims == ('f_hour', 'varlev', 'threshold', 'members_below', 'observed') and cd.values.dtype == np.int64
    assert np.array_equal(cd.values, ch.values) and cd.values.shape == (2, 2, Q, Mg + 1, 2)
    assert cd.values[:, :, 0].sum() == truth.size - 2 and cd.values[:, :, 1].sum() == truth.size - 3
