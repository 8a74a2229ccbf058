"""
Exact-size, poisoned, guarded memory for the GPU tests: written for the convolution family (test_hostile_mem.py,
test_gpu_hostile_mem.py, whose workspaces hostile_workspaces() replaces), and shared by the tests of the analysis families
(ensemble, category, quantile, spectrum, the spherical transforms, the time filters and regressions, the score plans), which
place their operands and results in an Arena.  Not a test module: imported by the tests that share it.

Arena: one uint8 buffer (device or CPU), every byte 0xFF -- NaN as fp32 and as bf16, -1 as int32.  carve() hands out views
whose first and last byte are exactly the object's; a guard band lies in front of and behind each.  The guard is as large
as the object it protects (rounded up to 256 B, at least 1 MiB, at most 32 MiB): an index that is off by one row, one face
or one sample lands within one object size of the object, so any index error below a factor of two hits a guard.  That is
a design condition, not a measurement.  assert_guards() compares every guard band bitwise with the poison and names the
object and the first offending byte.

hostile_workspaces(monkeypatch) replaces ops._workspace: every request gets a view of EXACTLY the bytes asked for, poisoned
again at the request, with the guard beginning at its last byte + 1.  Only floating data may be poisoned this way (the seven
regions of ws_layout() in conv_mfma.hip and the float partials of wgrad_batch.hip hold nothing else: no poisoned word can
become an address); plans, tables and descriptor arrays never come from here.
"""
import torch

POISON = 0xFF
MIN_GUARD, MAX_GUARD = 1 << 20, 32 << 20


def _up(n, a):
    return -(-n // a) * a


def guard_bytes(nbytes):
    """the guard band of an object of nbytes: its own size (256-B units) within [1 MiB, 32 MiB]"""
    return min(max(_up(int(nbytes), 256), MIN_GUARD), MAX_GUARD)


class _Object(object):
    __slots__ = ('name', 'lo', 'start', 'nbytes', 'cap', 'hi')

    def __init__(self, name, lo, start, nbytes, hi):
        self.name, self.lo, self.start, self.nbytes, self.cap, self.hi = name, lo, start, nbytes, nbytes, hi


class Arena(object):
    """bump allocator over one poisoned uint8 buffer; offsets below are bytes from the buffer's start"""

    def __init__(self, capacity, device='cpu'):
        self.device = torch.device(device)
        self.buf = torch.full((int(capacity) + 256,), POISON, dtype=torch.uint8, device=self.device)
        self.base = self.buf.data_ptr()
        self.top = 0
        self.objects = []

    # ---- allocation ----
    def _carve(self, nbytes, align, name):
        nbytes = int(nbytes)
        if nbytes < 0 or align < 1:
            raise ValueError('carve(%d, align=%d)' % (nbytes, align))
        g = guard_bytes(nbytes)
        lo = self.top
        start = _up(self.base + lo + g, align) - self.base
        hi = _up(start + nbytes + g, 256)
        if hi > self.buf.numel():
            raise MemoryError('arena of %d bytes is full (%d in use, %d + 2 x %d asked for)' % (self.buf.numel(), lo, nbytes, g))
        obj = _Object(name if name is not None else 'object %d' % len(self.objects), lo, start, nbytes, hi)
        self.top = hi
        self.objects.append(obj)
        return obj

    def _view(self, obj):
        return self.buf[obj.start:obj.start + obj.nbytes]

    def carve(self, nbytes, align=256, name=None):
        """uint8 view of exactly nbytes (poison), its first byte aligned to `align`, guards on both sides"""
        return self._view(self._carve(nbytes, align, name))

    def tensor(self, shape, dtype, name=None):
        """a poisoned tensor of the given shape and dtype under guard"""
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        return self.carve(n * torch.empty((), dtype=dtype).element_size(), name=name).view(dtype).view(shape)

    def place(self, t, name=None):
        """a copy of t under guard"""
        v = self.tensor(t.shape, t.dtype, name)
        v.copy_(t)
        return v

    def reset(self):
        """forget every object; the used part is poison again"""
        self.buf[:self.top].fill_(POISON)
        self.top = 0
        del self.objects[:]

    # ---- checking ----
    def _first_dirty(self, lo, hi):
        """offset of the first byte of [lo, hi) that is not poison, or None.  The 4-byte aligned core is compared as int32
        with -1, the (at most 3 + 3) bytes around it as uint8."""
        if hi <= lo:
            return None
        off0 = self.buf.storage_offset()
        a, b = min(_up(lo + off0, 4) - off0, hi), max((hi + off0) // 4 * 4 - off0, lo)
        if b <= a:
            a = b = hi
        for x, y in ((lo, a), (b, hi)):
            if y > x:
                bad = self.buf[x:y] != POISON
                if bool(bad.any()):
                    return x + int(torch.nonzero(bad)[0])
        if b > a:
            bad = self.buf[a:b].view(torch.int32) != -1
            if bool(bad.any()):
                w = a + 4 * int(torch.nonzero(bad)[0])
                chunk = self.buf[w:w + 4] != POISON
                return w + int(torch.nonzero(chunk)[0])
        return None

    def dirty_guards(self):
        """[(object name, byte offset relative to the object's first byte)]: the first overwritten byte of every guard band
        that is not intact (negative: in front of the object; >= its size: behind it)"""
        out = []
        for o in self.objects:
            for lo, hi in ((o.lo, o.start), (o.start + o.nbytes, o.hi)):
                at = self._first_dirty(lo, hi)
                if at is not None:
                    out.append((o.name, at - o.start, o.nbytes))
        return out

    def assert_guards(self):
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)
        hits = self.dirty_guards()
        assert not hits, '; '.join(
            '%s (%d bytes): %s' % (name, n, ('written %d bytes in front of its start' % -at) if at < 0 else
                                   ('written at offset %d, %d bytes past its end' % (at, at - n + 1)))
            for name, at, n in hits)


def is_poison(t):
    """elementwise: is this element still the poison pattern? (bitwise, through an integer view)"""
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.contiguous().view(it) == (POISON if t.element_size() == 1 else -1)


class HostileWorkspaces(object):
    """stand-in for ops._workspace(nbytes, device, role): per (device, role) a view of exactly nbytes that ends where its
    guard begins, poisoned again at every request.  A request that outgrows its slot gets a new one; the old one becomes
    guard as a whole.  (A node of ops.py asks once and keeps the tensor across the calls that share it -- the REUSE_DZ
    pair, the ring role until the pooling adjoint, the defer role until the batched reduction: poisoning at request time
    honours the hand-over contracts of include/dlwpcs.h.)"""

    def __init__(self, arena):
        self.arena = arena
        self.slots = {}
        self.requests = []          # (role, nbytes) of every request, in order

    def __call__(self, nbytes, device, role='main'):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('hostile workspaces poison at request time: not usable while a stream is capturing')
        device = torch.device(device)
        if device.type != self.arena.device.type or (device.index not in (None, self.arena.device.index)
                                                     and self.arena.device.index is not None):
            raise RuntimeError('hostile workspaces live on %s, asked for %s' % (self.arena.device, device))
        nbytes = int(nbytes)
        key = (str(device), role)
        obj = self.slots.get(key)
        if obj is None or nbytes > obj.cap:
            if obj is not None:
                self.arena.buf[obj.start:obj.start + obj.cap].fill_(POISON)
                obj.nbytes = 0
            obj = self.slots[key] = self.arena._carve(nbytes, 256, 'workspace %r' % (role,))
        # (a smaller request keeps its first byte; what lies behind its last byte is guard from now on)
        obj.nbytes = nbytes
        self.arena.buf[obj.start:obj.start + obj.cap].fill_(POISON)
        self.requests.append((role, nbytes))
        return self.arena._view(obj)

    def check(self):
        self.arena.assert_guards()


def hostile_workspaces(monkeypatch, capacity=1 << 30, device='cuda:0', arena=None):
    """ops._workspace becomes hostile until monkeypatch undoes it; returns the HostileWorkspaces (check(): all guards)."""
    from DLWP import ops
    hw = HostileWorkspaces(arena if arena is not None else Arena(capacity, device))
    monkeypatch.setattr(ops, '_workspace', hw)
    return hw
