#!/usr/bin/env python3
"""Time each coarsest-level layer of the bf16 `unet2` step alone (N = 12, batch 32: 64 -> 128 and 128 -> 64, forward and data
gradient) on both paths: the persistent kernel (dlwpcs_conv_fwd / dlwpcs_conv_bwd_data_masked) and the small-face kernel
(dlwpcs_conv_small_fwd / dlwpcs_conv_small_bwd_data).  Packed operands, 20 calls captured into one hipGraph and replayed: the
figure is device time per launch, back to back (the data gradient's figure includes its ring fix-up launch on both paths).
Environment: N, B to change the face / batch."""
import ctypes
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'dlwp-cs_amd'))
import torch
from DLWP import _native as nat
from DLWP import ops

dev = torch.device('cuda', 0)
B, N = int(os.environ.get('B', '32')), int(os.environ.get('N', '12'))
ALPHA, VMAX = 0.1, 10.0
lib = nat.lib()


def timed_graph(fn, calls=20, reps=20):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * calls)


def layer(ci, co):
    w = [torch.randn(3, 3, ci, co, device=dev) / (9 * ci) ** 0.5 for _ in range(2)]
    b = [torch.randn(co, device=dev) * 0.1 for _ in range(2)]
    bufs = ops.conv_packed_buffers(3, ci, co, nat.BF16, dev)
    items = ops.make_pack_items([(w[0], w[1], None, b[0], b[1], None, bufs, 3, True, nat.BF16)], dev)
    ops.pack_batch(items, 1)
    x = (torch.randn(B, 6, N, N, ci, device=dev) * 3).to(torch.bfloat16)
    dz = torch.randn(B, 6, N, N, co, device=dev).to(torch.bfloat16)
    y, dx = torch.empty(B, 6, N, N, co, dtype=torch.bfloat16, device=dev), torch.empty_like(x)
    d = nat.ConvDesc(B=B, N=N, C0=ci, C1=0, Cout=co, ksize=3, halo=1, up0=0, flip_north_pole=1, act=nat.ACT_LEAKY_CLIP, alpha=ALPHA,
                     vmax=VMAX, dtype=nat.BF16, flags=nat.CONV_PREPACKED, c0_valid=0)
    dn = nat.ConvDesc.from_buffer_copy(d)
    dn.act = nat.ACT_NONE
    n = lib.dlwpcs_conv_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    table, inv = nat.halo_tables(N, 1, dev)
    sp = nat.stream_ptr
    out = {}
    for name, fwd, bwd in (('persistent', lib.dlwpcs_conv_fwd, lib.dlwpcs_conv_bwd_data_masked),
                           ('small-face', lib.dlwpcs_conv_small_fwd, lib.dlwpcs_conv_small_bwd_data)):
        def f():
            nat.check(fwd(ctypes.byref(d), nat.ptr(x), None, nat.ptr(bufs[0]), None, None, nat.ptr(bufs[1]), None, None, nat.ptr(y),
                          nat.ptr(table), nat.ptr(ws), n, sp()), name + ' forward')

        def g():
            nat.check(bwd(ctypes.byref(dn), nat.ptr(dz), nat.ptr(bufs[2]), None, None, nat.ptr(dx), None, nat.ptr(x), None, ALPHA, VMAX,
                          nat.ptr(inv), nat.ptr(ws), n, sp()), name + ' data gradient')
        with torch.no_grad():
            out[name] = (timed_graph(f), timed_graph(g), y.clone(), dx.clone())
    same = torch.equal(out['persistent'][2].view(torch.int16), out['small-face'][2].view(torch.int16)) and \
        torch.equal(out['persistent'][3].view(torch.int16), out['small-face'][3].view(torch.int16))
    for name in ('persistent', 'small-face'):
        print('N=%d B=%d %3d -> %3d  %-10s  forward %6.1f us   data gradient + ring fix-up (masked) %6.1f us' %
              (N, B, ci, co, name, out[name][0], out[name][1]))
    print('    outputs bitwise equal: %s' % same)


for ci, co in ((64, 128), (128, 64)):
    layer(ci, co)
