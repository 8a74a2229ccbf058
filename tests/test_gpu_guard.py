"""
Placement independence.  Every tensor the kernels READ (inputs, saved output, upstream gradient, weights, halo tables) is
moved to the very END of a dedicated device buffer and the results must be bit-identical to the regular placement.  This is
a weak out-of-bounds canary only (the caching allocator usually keeps slack mapped behind a buffer, and it did NOT catch the
one real over-read found this round: dead gather slots of a short band indexing past the halo table -- that one showed up
as a rare memory fault when the GPU suite was looped on fresh boxes, see conv_mfma.hip `lookup`); what it does pin is that
no kernel depends on what lies behind or before its operands, nor on their position inside an allocation.

What the kernels WRITE -- outputs, workspaces, the flat gradient buffer -- is pinned by test_gpu_hostile_mem.py: exact-size
workspaces and output tensors, poisoned with NaN and surrounded by guard bands that are checked after every call
(tests/hostile_mem.py).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GRANULE = 2 << 20


def _at_end(t):
    """copy of t whose last byte is the last byte of a dedicated allocation"""
    nbytes = t.numel() * t.element_size()
    total = -(-max(nbytes, 1) // GRANULE) * GRANULE
    buf = torch.empty(total, dtype=torch.uint8, device=t.device)
    view = buf[total - nbytes:].view(t.dtype).view(t.shape)
    view.copy_(t)
    view._keep = buf
    return view


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
@pytest.mark.parametrize('shape', [(2, 24, 32, 0, 64, False), (3, 24, 16, 16, 32, True), (2, 20, 8, 0, 24, False),
                                   (1, 48, 14, 0, 32, False), (2, 12, 64, 0, 128, False)])
def test_conv_reads_stay_inside_their_tensors(shape, dtype):
    from DLWP import _native as nat
    from DLWP import ops
    B, N, C0, C1, Cout, up0 = shape
    dev = torch.device('cuda', 0)
    adt = torch.bfloat16 if dtype == 'bfloat16' else torch.float32
    g = torch.Generator(device='cpu').manual_seed(N * 100 + C0)
    n0 = N // 2 if up0 else N
    x0 = torch.randn(B, 6, n0, n0, C0, generator=g).to(adt).to(dev)
    x1 = torch.randn(B, 6, N, N, C1, generator=g).to(adt).to(dev) if C1 else None
    w = [(torch.randn(3, 3, C0 + C1, Cout, generator=g) / (3 * (C0 + C1) ** 0.5)).to(dev) for _ in range(2)]
    b = [(torch.randn(Cout, generator=g) * 0.1).to(dev) for _ in range(2)]
    gy = torch.randn(B, 6, N, N, Cout, generator=g).to(adt).to(dev)

    def run(guard):
        key = (N, 1, str(dev))
        saved = nat._table_cache.get(key)
        tabs = nat.halo_tables(N, 1, dev)
        if guard:
            nat._table_cache[key] = tuple(_at_end(t) for t in tabs)
        try:
            place = _at_end if guard else (lambda t: t.clone())
            a0 = place(x0).requires_grad_(True)
            a1 = place(x1).requires_grad_(True) if C1 else None
            ww = [place(t).requires_grad_(True) for t in w]
            bb = [place(t).requires_grad_(True) for t in b]
            y = ops.cs_conv(a0, ww[0], ww[1], None, bb[0], bb[1], None, src1=a1, ksize=3, halo=True, up0=up0,
                            act=nat.ACT_LEAKY_CLIP, alpha=0.1, vmax=10.0)
            y.backward(place(gy))
            torch.cuda.synchronize()
            outs = [y.detach(), a0.grad, ww[0].grad, ww[1].grad, bb[0].grad, bb[1].grad] + ([a1.grad] if C1 else [])
            return [o.float().cpu() for o in outs]
        finally:
            if saved is not None:
                nat._table_cache[key] = saved
            else:
                nat._table_cache.pop(key, None)
    ref, got = run(False), run(True)
    for r, o in zip(ref, got):
        assert torch.equal(r, o)
