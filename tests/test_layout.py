"""
DLWP/layout.py: merge_dims against a plain enumeration of the offsets a walk reaches, on seeded random layouts, and
element_layout on a hand-written case.  No device, no library.
"""
import itertools
import random

import numpy as np
import pytest

from DLWP import layout

N_LAYOUTS = 200


def _operand_strides(rng, shape):
    """element strides of a view of `shape`: contiguous, permuted, sliced with step 2, or broadcast along some dims"""
    nd = len(shape)
    kind = rng.choice(['contiguous', 'permuted', 'sliced', 'broadcast'])
    if kind == 'permuted':
        p = list(range(nd))
        rng.shuffle(p)
        a = np.empty([shape[i] for i in p], dtype=np.float32).transpose(np.argsort(p))
    elif kind == 'sliced':
        step = [rng.choice([1, 2]) for _ in range(nd)]
        a = np.empty([e * s for e, s in zip(shape, step)], dtype=np.float32)[tuple(slice(None, None, s) for s in step)]
    elif kind == 'broadcast':
        a = np.broadcast_to(np.empty([e if rng.random() < 0.5 else 1 for e in shape], dtype=np.float32), shape)
    else:
        a = np.empty(shape, dtype=np.float32)
    assert a.shape == tuple(shape)
    return tuple(s // a.itemsize for s in a.strides)


def _layouts():
    rng = random.Random(20241)
    for _ in range(N_LAYOUTS):
        nd = rng.randint(0, 6)
        shape = tuple(rng.randint(1, 4) for _ in range(nd))
        n_op = rng.randint(1, 3)
        per_op = [_operand_strides(rng, shape) for _ in range(n_op)]
        # tags in runs, as the callers use them (kept / averaged, before / after the row axis); one tag in a third of the layouts
        tags = [0 if rng.random() < 0.33 else None] * nd
        for i in range(nd):
            if tags[i] is None:
                tags[i] = rng.choice([False, True]) if i == 0 or rng.random() < 0.4 else tags[i - 1]
        yield [(shape[i], tuple(st[i] for st in per_op), tags[i]) for i in range(nd)]


def _walk(dims, n_op):
    """the offset tuples (one offset per operand) a row-major walk over `dims` reaches, in order"""
    return [tuple(sum(c * d[1][op] for c, d in zip(idx, dims)) for op in range(n_op))
            for idx in itertools.product(*[range(d[0]) for d in dims])]


LAYOUTS = list(_layouts())


def test_the_layouts_cover_what_they_should():
    assert len(LAYOUTS) == N_LAYOUTS
    assert any(len(d) == 0 for d in LAYOUTS) and any(len(d) == 6 for d in LAYOUTS)
    assert {len(d[0][1]) for d in LAYOUTS if d} == {1, 2, 3}
    assert any(0 in d[1] for dims in LAYOUTS for d in dims), 'a broadcast stride'
    assert any(len(layout.merge_dims(dims)) < sum(1 for d in dims if d[0] != 1) for dims in LAYOUTS), 'something merges'


def test_merge_dims_reaches_the_same_offsets_in_the_same_order():
    for dims in LAYOUTS:
        merged = layout.merge_dims(dims)
        n_op = len(dims[0][1]) if dims else 1
        assert _walk(merged, n_op) == _walk(dims, n_op), dims
        assert all(isinstance(e, int) and isinstance(st, tuple) and e != 1 for e, st, _ in merged)


def test_merge_dims_leaves_nothing_mergeable():
    for dims in LAYOUTS:
        merged = layout.merge_dims(dims)
        for (e0, s0, t0), (e1, s1, t1) in zip(merged[:-1], merged[1:]):
            assert t0 != t1 or any(a != b * e1 for a, b in zip(s0, s1)), (dims, merged)


def test_merge_dims_never_merges_across_tags():
    for dims in LAYOUTS:
        merged = layout.merge_dims(dims)
        # the runs of equal tags survive in order, and each run keeps its number of elements
        def runs(ds):
            return [(tag, int(np.prod([d[0] for d in grp]))) for tag, grp in
                    ((t, list(g)) for t, g in itertools.groupby([d for d in ds if d[0] != 1], key=lambda d: d[2]))]
        assert runs(merged) == runs(dims), (dims, merged)
    # two dims that one tag would merge stay apart under two
    assert layout.merge_dims([(3, (4,), 'a'), (4, (1,), 'a')]) == [(12, (1,), 'a')]
    assert layout.merge_dims([(3, (4,), 'a'), (4, (1,), 'b')]) == [(3, (4,), 'a'), (4, (1,), 'b')]
    # every operand has to allow it
    assert layout.merge_dims([(3, (4, 4), 0), (4, (1, 2), 0)]) == [(3, (4, 4), 0), (4, (1, 2), 0)]
    # a unit dim in between is dropped first
    assert layout.merge_dims([(3, (4,), 0), (1, (99,), 0), (4, (1,), 0)]) == [(12, (1,), 0)]


def test_element_layout_orders_by_stride_and_broadcasts_unit_dims():
    # an ensemble stored (lat = 5, member = 3, lon = 4, level = 2) contiguous, seen as (member, level, lat, lon)
    stored = np.empty((5, 3, 4, 2), dtype=np.float32)
    ens = stored.transpose(1, 3, 0, 2)
    shape, strides = ens.shape, tuple(s // 4 for s in ens.strides)
    assert shape == (3, 2, 5, 4) and strides == (8, 1, 24, 2)
    # the verification: (level, 1, lon) contiguous, its unit latitude broadcast
    valid = np.empty((2, 1, 4), dtype=np.float32)
    vstr = tuple(s // 4 for s in valid.strides)
    M, ms, eshape, order, merged = layout.element_layout(shape, strides, 0, [(valid.shape, vstr)], 'test')
    assert (M, ms, eshape) == (3, 8, (2, 5, 4))
    assert order == [1, 2, 0]                       # lat (24), lon (2), level (1): the contiguous dim last
    assert merged == [(5, (24, 0)), (4, (2, 1)), (2, (1, 4))]
    # no verification: strides of 0; lon and level now merge (2 == 1 * 2 on the ensemble, 0 == 0 * 2 on the other)
    _, _, _, order, merged = layout.element_layout(shape, strides, 0, [(None, None)], 'test')
    assert order == [1, 2, 0] and merged == [(5, (24, 0)), (8, (1, 0))]
    # a negative member axis, a third operand given by its strides, unit element dims left out of the order
    M, ms, eshape, order, merged = layout.element_layout((4, 1, 6), (6, 6, 1), -1, [((1, 1), (7, 7)), (None, (2, 0))], 'test', 1)
    assert (M, ms, eshape, order) == (6, 1, (4, 1), [0]) and merged == [(4, (6, 0, 2))]
    with pytest.raises(ValueError, match='test: member axis 3 out of range of 3 axes'):
        layout.element_layout((4, 1, 6), (6, 6, 1), 3, [], 'test')
    with pytest.raises(ValueError, match=r'test: 1 members \(at least 2\)'):
        layout.element_layout((4, 1, 6), (6, 6, 1), 1, [], 'test')
    with pytest.raises(ValueError, match='test: the verification'):
        layout.element_layout((4, 1, 6), (6, 6, 1), 0, [((1, 5), (5, 1))], 'test')
    with pytest.raises(NotImplementedError, match='more than 1 element dims'):
        layout.element_layout(shape, strides, 0, [(valid.shape, vstr)], 'test', max_dims=1)


def test_layout_is_pure_python():
    assert not {'torch', 'ctypes', 'np', 'numpy'} & set(vars(layout))
