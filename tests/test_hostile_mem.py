"""
The guarded arena of hostile_mem.py must be able to fail: on CPU tensors, a write one byte in front of an object, one byte
behind it and at the far end of a guard is reported each time and names the object and the offset; writes inside an object
are not reported; poison reads as NaN; objects are disjoint and aligned; the workspace stand-in hands out exact sizes.
"""
import pytest
import torch

import hostile_mem as hm


def _arena():
    return hm.Arena(16 << 20)


def test_guard_size_rule():
    assert hm.guard_bytes(1) == 1 << 20
    assert hm.guard_bytes((1 << 20) + 1) == (1 << 20) + 256
    assert hm.guard_bytes(5 << 20) == 5 << 20
    assert hm.guard_bytes(1 << 30) == 32 << 20


@pytest.mark.parametrize('nbytes', [1, 1000, 4096 + 3, (1 << 20) + 7])
def test_writes_outside_an_object_are_reported(nbytes):
    a = _arena()
    a.carve(512, name='before')
    v = a.carve(nbytes, name='victim')
    a.carve(512, name='after')
    o = a.objects[1]
    g = hm.guard_bytes(nbytes)
    assert o.start - o.lo >= g and o.hi - (o.start + nbytes) >= g
    a.assert_guards()
    v.fill_(0)                                  # every byte of the object, first and last included
    a.assert_guards()
    for off in (o.start - 1, o.start + nbytes, o.lo, o.hi - 1, o.start - g, o.start + nbytes + g - 1):
        a.buf[off] = 0
        with pytest.raises(AssertionError) as e:
            a.assert_guards()
        assert 'victim' in str(e.value) and 'before' not in str(e.value) and 'after' not in str(e.value)
        rel = off - o.start
        assert (('%d bytes in front' % -rel) if rel < 0 else ('offset %d,' % rel)) in str(e.value)
        a.buf[off] = hm.POISON
        a.assert_guards()


def test_a_write_through_the_view_one_element_too_far_is_reported():
    a = _arena()
    t = a.tensor((3, 5), torch.float32, name='t')
    flat = torch.as_strided(t, (16,), (1,))     # one float past the end
    flat[15] = 1.0
    assert a.dirty_guards() == [('t', 60, 60)]


def test_poison_reads_as_nan():
    a = _arena()
    f = a.tensor((7, 3), torch.float32)
    b = a.tensor((5,), torch.bfloat16)
    assert torch.isnan(f).all() and torch.isnan(b).all()
    assert hm.is_poison(f).all() and hm.is_poison(b).all()
    f[2, 1] = 0.5
    b[4] = float('nan')                         # a NaN the code computed is not the poison pattern
    assert int(hm.is_poison(f).sum()) == 20 and int(hm.is_poison(b).sum()) == 4


def test_objects_are_disjoint_and_aligned():
    a = hm.Arena(32 << 20)
    sizes = [1, 255, 256, 257, 70000, 3, (1 << 20) + 1]
    views = [a.carve(n) for n in sizes]
    spans = []
    for v, n, o in zip(views, sizes, a.objects):
        assert v.numel() == n and v.data_ptr() % 256 == 0
        assert v.data_ptr() == a.base + o.start
        spans.append((o.lo, o.hi))
        assert o.lo <= o.start and o.start + n <= o.hi
    for (l0, h0), (l1, h1) in zip(spans, spans[1:]):
        assert h0 <= l1                         # guards included: no byte belongs to two objects
    assert a.carve(64, align=4096).data_ptr() % 4096 == 0
    for i, v in enumerate(views):
        v.fill_(i)
    for i, v in enumerate(views):
        assert bool((v == i).all())
    a.assert_guards()


def test_place_copies_and_reset_poisons_again():
    a = _arena()
    x = torch.arange(12, dtype=torch.float32).view(3, 4)
    v = a.place(x, 'x')
    assert torch.equal(v, x)
    a.reset()
    assert not a.objects and a.top == 0
    assert hm.is_poison(a.tensor((3, 4), torch.float32)).all()


def test_a_full_arena_raises():
    a = hm.Arena(4 << 20)
    a.carve(100)
    with pytest.raises(MemoryError):
        a.carve(3 << 20)


def test_workspace_stand_in_hands_out_exact_poisoned_views():
    a = _arena()
    hw = hm.HostileWorkspaces(a)
    w = hw(1000, 'cpu')
    assert w.numel() == 1000 and w.data_ptr() % 256 == 0 and bool((w == hm.POISON).all())
    w.fill_(1)
    hw.check()
    w2 = hw(1000, 'cpu')                        # same role, same size: same bytes, poisoned again
    assert w2.data_ptr() == w.data_ptr() and bool((w2 == hm.POISON).all())
    side = hw(300, 'cpu', role='ring0')
    assert side.data_ptr() != w.data_ptr()
    small = hw(600, 'cpu')                      # smaller: the guard begins right behind its last byte
    assert small.numel() == 600 and small.data_ptr() == w.data_ptr()
    w.fill_(2)                                  # the old, longer view now overruns
    with pytest.raises(AssertionError) as e:
        hw.check()
    assert "'main'" in str(e.value) and 'offset 600,' in str(e.value)
    big = hw(5000, 'cpu')                       # larger: a new slot, the old one is guard as a whole
    assert big.numel() == 5000 and bool((big == hm.POISON).all())
    hw.check()
    small.fill_(3)
    with pytest.raises(AssertionError):
        hw.check()
    assert hw.requests == [('main', 1000), ('main', 1000), ('ring0', 300), ('main', 600), ('main', 5000)]


def test_workspace_stand_in_replaces_ops_workspace(monkeypatch):
    from DLWP import ops
    a = _arena()
    hw = hm.hostile_workspaces(monkeypatch, arena=a)
    assert ops._workspace is hw
    assert ops._workspace(128, torch.device('cpu'), 'main').numel() == 128
    with pytest.raises(RuntimeError):
        hw(128, torch.device('meta'))
    monkeypatch.undo()
    assert ops._workspace is not hw
