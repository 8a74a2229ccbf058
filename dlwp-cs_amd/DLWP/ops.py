"""
torch.autograd glue over the C ABI (include/dlwpcs.h).  Every function here launches hand-written HIP kernels from
libdlwpcs.so on torch's current stream; torch only provides storage and the autograd tape.  All tensors on this level
are channels_last `(B, 6, H, W, C)` on a HIP device, float32 or bfloat16 (activations only; parameters, their gradients
and the optimizer state are always float32 -- see the dtype note in include/dlwpcs.h).
"""
import ctypes
import os

import numpy as np
import torch

from . import _native as nat
from .layout import element_layout, member_split, merge_dims
from .options import option
from ._native import ConvDesc, GConvDesc, check, lib, ptr, require_device, stream_ptr

# When True, convolution backward accumulates weight gradients directly into the parameters' preset `.grad` buffers
# (DLWP.keras.Model turns this on around its training step; plain autograd use keeps the standard semantics).
DIRECT_PARAM_GRADS = False

# Pre-packed weights (dlwpcs_pack_batch): id(equatorial kernel tensor) -> (dtype tag, wpk_fwd, bias_pk | None, wpk_bwd).
# DLWP.keras.Model fills this around its forward pass after packing every layer with ONE launch; a convolution whose
# kernel is not listed (or listed for another dtype) packs its weights itself, per call, into the workspace.
PREPACKED = {}

# When True (DLWP.keras.Model training step), weight-gradient kernels are enqueued on a second HIP stream: they depend
# only on (src, dy) and nothing before the optimizer consumes them, so they overlap the data-gradient chain of the layers
# below (fills launch gaps and the tails of the persistent kernels).  Whoever sets this must call join_side_stream()
# before the gradients are read.
WGRAD_SIDE_STREAM = False
_side_streams = {}


def side_stream(device):
    key = str(device)
    st = _side_streams.get(key)
    if st is None:
        st = torch.cuda.Stream(device=device)
        _side_streams[key] = st
    return st


def join_side_stream(device):
    """Make the current stream wait for everything enqueued on the weight-gradient side stream."""
    st = _side_streams.get(str(device))
    if st is not None:
        torch.cuda.current_stream(device).wait_stream(st)


# workspace: one growing byte buffer per (device, role) (caller-owned from the library's point of view)
_workspaces = {}
_retired_workspaces = []    # outgrown buffers stay allocated: hipGraphs captured earlier have their addresses baked in


def _workspace(nbytes, device, role='main'):
    key = (str(device), role)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        if torch.cuda.is_current_stream_capturing():
            raise nat.NativeError('workspace would have to grow during graph capture; run one eager step first')
        if ws is not None:
            _retired_workspaces.append(ws)
        ws = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


# Deferred weight-gradient reduction (DLWPCS_CONV_DEFER_REDUCE): while the flag is on, every fused-conv backward node
# that accumulates straight into preset .grad buffers leaves its per-worker partials in a workspace of its own and
# queues a dlwpcs_reduce_item; flush_deferred_reduce() then sums ALL layers' partials with one launch (one per
# application round of shared layers) instead of one small launch per layer.  Whoever sets the flag must flush before
# the gradients are read.
DEFER_WGRAD_REDUCE = False
_deferred = []              # [(ReduceItem, workspace tensor)] of the backward pass in flight
_reduce_tables = {}         # (device, raw item bytes) -> device copy of the item table


def drop_deferred_reduce():
    del _deferred[:]


def flush_deferred_reduce(device):
    if not _deferred:
        return
    pending = list(_deferred)
    del _deferred[:]
    # items whose destinations coincide (a layer applied twice) go into successive launches
    rounds, seen = [], {}
    for item, ws in pending:
        k = seen.get(item.dw_eq, 0)
        seen[item.dw_eq] = k + 1
        while len(rounds) <= k:
            rounds.append([])
        rounds[k].append(item)
    for items in rounds:
        host = (nat.ReduceItem * len(items))(*items)
        raw = bytes(host)
        key = (str(device), raw)
        table = _reduce_tables.get(key)
        if table is None:
            if torch.cuda.is_current_stream_capturing():
                raise nat.NativeError('reduce-item table would have to be uploaded during graph capture; run one eager '
                                      'step first')
            table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
            _reduce_tables[key] = table
        check(lib().dlwpcs_wgrad_reduce_batch(ptr(table), ctypes.addressof(host), len(items), stream_ptr()),
              'dlwpcs_wgrad_reduce_batch')


# ------------------------------------------------------------------------------------------------------------------ #
# Batched weight gradients (dlwpcs_wgrad_batch): ONE persistent launch + one reduction for all layers of a backward pass
# ------------------------------------------------------------------------------------------------------------------ #
_wb_plans = {}              # geometry key -> (host plan buffer, device plan tensor, workspace bytes)


# When True (DLWP.keras.Model training step) a convolution's backward node does not launch its weight gradient: it queues
# (descriptor, inputs, dz, gradient buffers) and flush_wgrad_batch() runs ALL queued layers with one launch after the last
# data gradient (the weight gradients are off the critical path of the backward pass).  Needs DIRECT_PARAM_GRADS (the
# gradients are accumulated into the parameters' preset .grad buffers); whoever sets the flag must flush.
WGRAD_BATCH = False
_wb_pending = []


def wgrad_batch_supported(d):
    return bool(lib().dlwpcs_wgrad_batch_supported(ctypes.byref(d)))


_wb_flushed = []            # the entries flush_wgrad_batch() has run since the last drop (apply_wgrad_batch names their gradients)


def drop_wgrad_batch():
    del _wb_pending[:]
    del _wb_flushed[:]


# The fused head's loss is finished (second stage of its reduction) by the LAST launch of the training step when that is the
# fused weight-gradient reduction + optimizer (dlwpcs_wgrad_batch_adam_tail): DEFER_LOSS_TAIL is set by DLWP.keras.Model for such
# steps, _HeadMSE.forward then leaves a dlwpcs_loss_tail here; whoever ends the step without that launch runs finish_loss_tail().
DEFER_LOSS_TAIL = False
_pending_tail = []


def finish_loss_tail():
    """Run a deferred loss tail as a launch of its own (no fused reduction + optimizer launch took it)."""
    while _pending_tail:
        tail, keep = _pending_tail.pop()
        check(lib().dlwpcs_loss_tail_run(ctypes.byref(tail), stream_ptr()), 'dlwpcs_loss_tail_run')


PACK_FUSED = False          # did the last flush_wgrad_batch refresh the packed operands inside its optimizer launch?


def flush_wgrad_batch(adam=None, pack_lookup=None):
    """Run the queued layers.  adam = (flat params, flat grads, m, v, state {t-1, ticket}, hyper {lr, b1, b2, eps, scale},
    number of parameter elements) asks for the optimizer fused into the reduction (dlwpcs_wgrad_batch_adam): done -- and True
    returned -- when the queued layers cover every parameter exactly once; otherwise the gradients are left in the flat buffer
    as usual and the caller runs its optimizer launch.  pack_lookup (with adam): address of a layer's equatorial-kernel gradient
    -> its make_pack_items entry; when every queued layer has one, the launch also refreshes the packed bf16 operands
    (PACK_FUSED says whether it did)."""
    global PACK_FUSED
    PACK_FUSED = False
    if not _wb_pending:
        return False
    pending = list(_wb_pending)
    del _wb_pending[:]
    _wb_flushed.extend(pending)
    if adam is not None and len(pending) <= nat.WGRAD_BATCH_MAX:
        p, g, m, v, state, hyper, n_elems = adam
        if _wb_covers(pending, n_elems):
            packs = None
            if pack_lookup is not None:
                packs = [pack_lookup(ent[5][0].data_ptr()) for ent in pending]
                if any(pk is None for pk in packs):
                    packs = None
            wgrad_batch(pending, adam=(p, g, m, v, state, hyper), packs=packs)
            PACK_FUSED = packs is not None
            return True
    wgrad_batch(pending)
    return False


def _wb_covers(entries, n_elems):
    """do the gradient tensors of `entries` cover n_elems parameter elements?  A layer applied more than once (integration_steps
    = 2 in the reference scripts) names its tensors once per application: the library reduces such items in successive launches
    and lets the optimizer consume a tensor in the launch of its last item."""
    seen, covered = set(), 0
    for ent in entries:
        for t in ent[5]:
            if t is not None and t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                covered += t.numel()
    return covered == n_elems


_wb_anchor = {}


def flushed_wgrad_entries():
    """the entries run by flush_wgrad_batch() since the last drop, for a caller that applies the update after the backward pass's
    clean-up (apply_wgrad_batch / prepare_wgrad_plan) -- WITHOUT the layers' saved inputs, outputs and output gradients: the
    apply launch names the layers' descriptors and gradient views only, and a model that kept the full entries would hold one
    step's activations until the end of the next one (twice the peak memory of eager steps).  dz / y are replaced by a one-element
    tensor of the same device (the plan key asks which device, and whether a layer masks on load)."""
    out = []
    for ent in _wb_flushed:
        dev = ent[3].device
        a = _wb_anchor.get(dev)
        if a is None:
            a = _wb_anchor[dev] = torch.zeros(1, dtype=torch.uint8, device=dev)
        slim = (ent[0], None, None, a, ent[4], ent[5])
        if len(ent) > 6:
            slim += ((a if ent[6] is not None else None),)
        out.append(slim)
    return out


def apply_wgrad_batch(adam, pack_lookup=None, entries=None):
    """Data-parallel tail of a training step (dlwpcs_wgrad_batch_apply): the layers flush_wgrad_batch() has run since the last
    drop left their finished gradients in the flat buffer, the caller has summed it over the ranks; ONE launch now applies
    grad_scale + Adam, clears the gradients, refreshes the packed bf16 operands (pack_lookup as for flush_wgrad_batch) and
    finishes a deferred loss.  adam = (p, g, m, v, state {t, ticket}, hyper, number of parameter elements).  Returns False --
    nothing launched -- when those layers do not cover every parameter exactly once (the caller runs its optimizer launch)."""
    global PACK_FUSED
    PACK_FUSED = False
    entries = list(_wb_flushed) if entries is None else list(entries)
    p, g, m, v, state, hyper, n_elems = adam
    if not entries or len(entries) > nat.WGRAD_BATCH_MAX or not _wb_covers(entries, n_elems):
        return False
    dev = entries[0][3].device
    arr, key = _wb_items(entries)
    hit = _wb_plan(arr, len(entries), (str(dev), key), dev)
    host, plan_dev, _ = hit
    packs = None
    if pack_lookup is not None:
        packs = [pack_lookup(ent[5][0].data_ptr()) for ent in entries]
        if any(pk is None for pk in packs):
            packs = None
    tail = None
    if len(_pending_tail) == 1:
        tail, keep = _pending_tail.pop()                        # the step's loss is finished by this launch
    check(lib().dlwpcs_wgrad_batch_apply(arr, len(entries), host, ptr(plan_dev), ptr(p), ptr(g), ptr(m), ptr(v), g.numel(),
                                         ptr(state), ptr(hyper), ctypes.byref(tail) if tail is not None else None,
                                         _pack_array(packs) if packs is not None else None, stream_ptr()),
          'dlwpcs_wgrad_batch_apply')
    PACK_FUSED = packs is not None
    return True


def prepare_wgrad_plan(entries, n_elems):
    """Build (and upload) the plan of an item list outside a graph capture, so that a captured apply_wgrad_batch() of the same
    layers finds it (the two-bucket step flushes its halves separately: their union is first needed by the captured update)."""
    entries = list(entries)
    if not entries or len(entries) > nat.WGRAD_BATCH_MAX or not _wb_covers(entries, n_elems):
        return
    dev = entries[0][3].device
    arr, key = _wb_items(entries)
    _wb_plan(arr, len(entries), (str(dev), key), dev)


def _pack_array(packs):
    pk_arr = (nat.PackItem * len(packs))()
    for it, (we, wp, wn, be, bp, bn, bufs, ksize, flip, tag) in zip(pk_arr, packs):
        it.w_eq, it.w_pol, it.w_np = ptr(we), ptr(wp), ptr(wn)
        it.b_eq, it.b_pol, it.b_np = ptr(be), ptr(bp), ptr(bn)
        it.wpk_fwd, it.bias_pk, it.wpk_bwd = ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2])
        it.ksize, it.Cin, it.Cout = int(ksize), int(we.shape[2]), int(we.shape[3])
        it.flip_north_pole, it.dtype, it.reserved = int(flip), int(tag), 0
    return pk_arr


def _wb_plan(arr, n, key, dev):
    """(host plan buffer, device plan tensor, workspace bytes) of an item list, built once per geometry"""
    hit = _wb_plans.get(key)
    if hit is None:
        if torch.cuda.is_current_stream_capturing():
            raise nat.NativeError('the weight-gradient plan would have to be uploaded during graph capture; run one eager '
                                  'step first')
        pb, wb = ctypes.c_size_t(), ctypes.c_size_t()
        check(lib().dlwpcs_wgrad_batch_sizes(arr, n, ctypes.byref(pb), ctypes.byref(wb)), 'dlwpcs_wgrad_batch_sizes')
        host = (ctypes.c_char * pb.value)()
        check(lib().dlwpcs_wgrad_batch_plan(arr, n, host, pb.value), 'dlwpcs_wgrad_batch_plan')
        plan_dev = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)
        hit = (host, plan_dev, wb.value)
        _wb_plans[key] = hit
    return hit


def _wb_items(entries):
    arr = (nat.WgradItem * len(entries))()
    key = []
    for it, ent in zip(arr, entries):
        d, src0, src1, dz, table, grads = ent[:6]
        y = ent[6] if len(ent) > 6 else None
        it.d = d
        it.src0, it.src1, it.dz, it.y, it.table_dev = ptr(src0), ptr(src1), ptr(dz), ptr(y), ptr(table)
        it.dw_eq, it.dw_pol, it.dw_np, it.db_eq, it.db_pol, it.db_np = [ptr(g) for g in grads]
        key.append((d.B, d.N, d.C0, d.C1, d.Cout, d.ksize, d.halo, d.up0, d.flip_north_pole, d.dtype, d.c0_valid,
                    tuple(g is not None for g in grads), None if y is None else (d.act, d.alpha, d.vmax)))
    return arr, tuple(key)


def wgrad_batch(entries, adam=None, packs=None):
    """entries: [(ConvDesc, src0, src1 | None, dz, halo table | None, (dw_eq, dw_pol, dw_np, db_eq, db_pol, db_np)[, y])] with
    fp32 gradient tensors that are ACCUMULATED into (None where the layer has no such parameter).  dz is the gradient
    w.r.t. the layer's pre-activation output (already masked) -- or, with the optional 7th element y (the layer's saved
    output, desc.act = LEAKY_CLIP), the plain gradient dy, masked by the kernel on load.  The plan of a layer list is built
    once and cached."""
    if not entries:
        return
    dev = entries[0][3].device
    for lo in range(0, len(entries), nat.WGRAD_BATCH_MAX):
        chunk = entries[lo:lo + nat.WGRAD_BATCH_MAX]
        arr, key = _wb_items(chunk)
        host, plan_dev, ws_bytes = _wb_plan(arr, len(chunk), (str(dev), key), dev)
        ws = _workspace(ws_bytes, dev, 'wgrad_batch')
        if adam is not None:
            p, g, m, v, state, hyper = adam
            tail = None
            if len(_pending_tail) == 1:
                tail, keep = _pending_tail.pop()            # the step's loss is finished by this launch
            if tail is not None or packs is not None:
                pk_arr = _pack_array(packs[lo:lo + len(chunk)]) if packs is not None else None
                check(lib().dlwpcs_wgrad_batch_adam_tail(arr, len(chunk), host, ptr(plan_dev), ptr(ws), ws.numel(), ptr(p), ptr(g),
                                                         ptr(m), ptr(v), g.numel(), ptr(state), ptr(hyper),
                                                         ctypes.byref(tail) if tail is not None else None, pk_arr, stream_ptr()),
                      'dlwpcs_wgrad_batch_adam_tail')
                continue
            check(lib().dlwpcs_wgrad_batch_adam(arr, len(chunk), host, ptr(plan_dev), ptr(ws), ws.numel(), ptr(p), ptr(g), ptr(m),
                                                ptr(v), g.numel(), ptr(state), ptr(hyper), stream_ptr()),
                  'dlwpcs_wgrad_batch_adam')
            continue
        check(lib().dlwpcs_wgrad_batch(arr, len(chunk), host, ptr(plan_dev), ptr(ws), ws.numel(), stream_ptr()),
              'dlwpcs_wgrad_batch')


# Deferred ring fix-up (DLWPCS_CONV_DEFER_RING0): a data-gradient call whose source 0 is a pooled tensor with no other
# consumer leaves the halo ring of that source in its workspace; the pooling adjoint that receives the gradient next adds it
# while it spreads the gradient (dlwpcs_avgpool2_bwd_ring) -- one launch less per pooling level.  Keyed by the address of the
# gradient tensor the convolution's backward returns; DLWP.keras.Model asks for it only where its plan guarantees that the next
# reader of that tensor is the pooling node, and clears the table around every backward pass.
_pending_ring = {}
# Pooled by-products of the convolutions that ran with want_pool (dlwpcs_conv_fwd_pool), keyed by the address of the full-size
# output; the pooling node that follows takes its entry (DLWP.keras.Model asks for it only when the next reader of that
# output is such a node, and clears the table at the start of every forward pass).
_POOLED = {}


def drop_pending_rings():
    _pending_ring.clear()


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------------------------------ #
# CubeSpherePadding2D  (reference DLWP/custom.py:1082-1308)
# ------------------------------------------------------------------------------------------------------------------ #

class _CSPad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        require_device(x, 'cs_pad')
        x = _c(x)
        B, F6, N, N2, C = x.shape
        if F6 != 6 or N != N2:
            raise ValueError('cs_pad: expected (B, 6, N, N, C), got %s' % (tuple(x.shape),))
        table, inv = nat.halo_tables(N, p, x.device)
        y = torch.empty((B, 6, N + 2 * p, N + 2 * p, C), dtype=x.dtype, device=x.device)
        check(lib().dlwpcs_pad_fwd(ptr(x), ptr(y), B, N, C, p, nat.dtype_tag(x), ptr(table), stream_ptr()),
              'dlwpcs_pad_fwd')
        ctx.p, ctx.shape = p, (B, N, C)
        ctx.inv = inv
        return y

    @staticmethod
    def backward(ctx, dy):
        B, N, C = ctx.shape
        dy = _c(dy)
        dx = torch.empty((B, 6, N, N, C), dtype=dy.dtype, device=dy.device)
        check(lib().dlwpcs_pad_bwd(ptr(dy), ptr(dx), B, N, C, ctx.p, nat.dtype_tag(dy), ptr(ctx.inv), stream_ptr()),
              'dlwpcs_pad_bwd')
        return dx, None


def cs_pad(x, p):
    """Halo-pad a cubed-sphere tensor (B,6,N,N,C) -> (B,6,N+2p,N+2p,C)."""
    return _CSPad.apply(x, int(p))


# ------------------------------------------------------------------------------------------------------------------ #
# Fused cubed-sphere convolution (reference DLWP/custom.py:921-1002 + :1082-1308 + Keras ReLU/UpSampling3D/concatenate)
# ------------------------------------------------------------------------------------------------------------------ #

def _make_desc(B, N, C0, C1, Cout, ksize, halo, up0, flip, act, alpha, vmax, dtype=nat.F32, c0_valid=0):
    return ConvDesc(B=B, N=N, C0=C0, C1=C1, Cout=Cout, ksize=ksize, halo=int(halo), up0=int(up0),
                    flip_north_pole=int(flip), act=int(act), alpha=float(alpha), vmax=float(vmax), dtype=int(dtype),
                    flags=0, c0_valid=int(c0_valid))


class _PadChannels(torch.autograd.Function):
    """(…, C) -> (…, Cp): zero channels appended (dlwpcs_pad_channels); the backward slices them off again."""

    @staticmethod
    def forward(ctx, x, cp):
        require_device(x, 'pad_channels')
        x = _c(x)
        C = x.shape[-1]
        rows = x.numel() // C if C else 0
        y = torch.empty(tuple(x.shape[:-1]) + (cp,), dtype=x.dtype, device=x.device)
        check(lib().dlwpcs_pad_channels(ptr(x), ptr(y), rows, C, cp, nat.dtype_tag(x), stream_ptr()), 'dlwpcs_pad_channels')
        ctx.c = C
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _c(dy)
        cp = dy.shape[-1]
        rows = dy.numel() // cp
        dx = torch.empty(tuple(dy.shape[:-1]) + (ctx.c,), dtype=dy.dtype, device=dy.device)
        check(lib().dlwpcs_slice_channels(ptr(dy), ptr(dx), rows, cp, ctx.c, nat.dtype_tag(dy), stream_ptr()),
              'dlwpcs_slice_channels')
        return dx, None


def pad_channels(x, cp):
    """Append zero channels up to `cp` (no-op when the tensor already has cp channels)."""
    if x.shape[-1] == cp:
        return x
    if x.shape[-1] > cp:
        raise ValueError('pad_channels: tensor has %d channels, asked for %d' % (x.shape[-1], cp))
    return _PadChannels.apply(x, int(cp))


def channel_vector(dtype):
    """channels per 16-B vector of an activation dtype: the alignment the fast kernel paths want"""
    return 8 if dtype == torch.bfloat16 else 4


def padded_channels(c, dtype, even_too=None):
    """Physical channel count the engine stores a c-channel NETWORK INPUT with: odd counts (7 variables) are always padded
    to the next 16-B vector (the scalar-load kernel paths spill registers and run at a fraction of the vector paths); even
    counts that are not vector multiples (14 = 7 x 2) only when asked to (they have 4-B-vector / shifted-tail paths)."""
    v = channel_vector(dtype)
    if c % v == 0:
        return c
    if c % 2 == 1 or even_too:
        return (c + v - 1) // v * v
    return c


def _f32_param(t, what):
    if t is not None and t.dtype != torch.float32:
        raise TypeError('%s: parameters must be float32 master copies, got %s' % (what, t.dtype))


def _weight_gradients(d, src0, src1, dy, y, params, table, ws, nbytes, direct, defer, need, has_np, has_bias, has_bnp,
                      batch_mask_ok=False):
    """Weight / bias gradients of one fused convolution (shared by _CSConv.backward and the fused head + loss step).
    direct: accumulate straight into the parameters' preset .grad buffers (views of the model's flat gradient buffer, zeroed
    once per step): no temporaries, no AccumulateGrad add kernels; shared layers simply accumulate twice.  Returns the six
    gradient tensors (None in direct mode)."""
    dev = dy.device
    w_eq, w_pol, w_np = params[0], params[1], params[2]
    dw_eq = dw_pol = dw_np = db_eq = db_pol = db_np = None
    if (direct and WGRAD_BATCH and d.B > 0 and not WGRAD_SIDE_STREAM and wgrad_batch_supported(d)
            and (d.act == nat.ACT_NONE or (batch_mask_ok and d.ksize == 3 and y is not None))):
        # dy IS dz (no activation, or the gradient arrived pre-masked) -- or the batched kernel masks on load (a layer whose
        # inputs need no gradient: nobody else wants dz): queue the layer for the batched launch
        pe, pp, pn, be, bp, bn = params
        d2 = ConvDesc.from_buffer_copy(d)
        _wb_pending.append((d2, src0, src1, dy, table,
                            (pe.grad, pp.grad, None if pn is None else pn.grad, None if be is None else be.grad,
                             None if bp is None else bp.grad, None if bn is None else bn.grad),
                            None if d.act == nat.ACT_NONE else y))
        return dw_eq, dw_pol, dw_np, db_eq, db_pol, db_np
    if direct:
        pe, pp, pn, be, bp, bn = params
        d2 = ConvDesc.from_buffer_copy(d)
        d2.flags = d.flags | nat.CONV_ACCUMULATE_WGRAD | (nat.CONV_DEFER_REDUCE if defer else 0)
        grads = (ptr(pe.grad), ptr(pp.grad), ptr(None if pn is None else pn.grad),
                 ptr(None if be is None else be.grad), ptr(None if bp is None else bp.grad),
                 ptr(None if bn is None else bn.grad))

        def launch(wsx):
            check(lib().dlwpcs_conv_bwd_weights(ctypes.byref(d2), ptr(src0), ptr(src1), ptr(dy), ptr(y), *grads,
                                                ptr(table), ptr(wsx), wsx.numel(), stream_ptr()),
                  'dlwpcs_conv_bwd_weights')
            if defer:
                item = nat.ReduceItem()
                check(lib().dlwpcs_conv_wgrad_reduce_item(ctypes.byref(d2), *grads, ptr(wsx), wsx.numel(),
                                                          ctypes.byref(item)), 'dlwpcs_conv_wgrad_reduce_item')
                _deferred.append((item, wsx))
        if WGRAD_SIDE_STREAM:
            side = side_stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))      # dy and the saved activations are ready
            ws2 = _workspace(nbytes, dev, 'side')                 # own workspace: the main stream keeps using `ws`
            with torch.cuda.stream(side):
                launch(ws2)
            for t in (src0, src1, dy, y):                         # keep their memory until the side stream is done
                if t is not None:
                    t.record_stream(side)
        else:
            launch(ws)
    elif any(need):
        dw_eq, dw_pol = torch.empty_like(w_eq), torch.empty_like(w_pol)
        dw_np = torch.empty_like(w_np) if has_np else None
        if has_bias:
            db_eq = torch.empty(d.Cout, dtype=torch.float32, device=dev)
            db_pol = torch.empty(d.Cout, dtype=torch.float32, device=dev)
            db_np = torch.empty(d.Cout, dtype=torch.float32, device=dev) if has_bnp else None
        check(lib().dlwpcs_conv_bwd_weights(ctypes.byref(d), ptr(src0), ptr(src1), ptr(dy), ptr(y), ptr(dw_eq),
                                            ptr(dw_pol), ptr(dw_np), ptr(db_eq), ptr(db_pol), ptr(db_np),
                                            ptr(table), ptr(ws), ws.numel(), stream_ptr()),
              'dlwpcs_conv_bwd_weights')
    return dw_eq, dw_pol, dw_np, db_eq, db_pol, db_np


class _CSConv(torch.autograd.Function):
    """
    y = act(conv(halo_pad(concat(up?(src0), src1))) + bias); see dlwpcs_conv_fwd in include/dlwpcs.h.
    Inputs that may be None: src1, w_np, b_eq, b_pol, b_np.
    """

    @staticmethod
    def forward(ctx, src0, src1, w_eq, w_pol, w_np, b_eq, b_pol, b_np, ksize, halo, up0, flip, act, alpha, vmax,
                c0_valid=0, premask0=None, premask1=None, dy_premasked=False, defer_ring0=False, want_pool=False,
                out_padded=False, small=False):
        """small (engine option small_conv): layers the small-face kernel serves (_small_conv_ok) try dlwpcs_conv_small_fwd /
        dlwpcs_conv_small_bwd_data first -- the same bits -- and take the general entry point when it answers E_UNSUPPORTED.
        out_padded (inference only, the pointwise bf16 output layer): y gets ceil8(C_out) channels per pixel, the padding
        zero (DLWPCS_CONV_OUT_PADDED) -- what the first layer takes back as a padded source in a rollout.
        want_pool: the 2x2 average pooling of y is produced as a by-product (dlwpcs_conv_fwd_pool) and parked in _POOLED for
        the pooling node that follows (avgpool2_skip), which then launches nothing in its forward pass.
        defer_ring0: the gradient of source 0 goes to a pooling node that adds the halo ring itself (see _pending_ring).
        premask0 / premask1 = (negative_slope, max_value) | None: src0 / src1 is the output of an activated layer that expects
        its gradient PRE-MASKED (multiplied by act'(src)): the backward applies it to dsrc0 / dsrc1.  dy_premasked: the gradient
        THIS node receives is already dz = dy * act'(y) (every consumer of y honours premask).  See dlwpcs_conv_bwd_data_masked."""
        require_device(src0, 'cs_conv')
        src0 = _c(src0)
        B = src0.shape[0]
        if src0.dim() != 5 or src0.shape[1] != 6 or src0.shape[2] != src0.shape[3]:
            raise ValueError('cs_conv: expected (B, 6, N, N, C), got %s' % (tuple(src0.shape),))
        N = src0.shape[2] * (2 if up0 else 1)
        C0 = src0.shape[4]
        C1 = 0
        if src1 is not None:
            require_device(src1, 'cs_conv')
            src1 = _c(src1)
            if tuple(src1.shape[:4]) != (B, 6, N, N):
                raise ValueError('cs_conv: src1 shape %s does not match (B,6,%d,%d,*)' % (tuple(src1.shape), N, N))
            C1 = src1.shape[4]
            if src1.dtype != src0.dtype:
                raise TypeError('cs_conv: src0 is %s but src1 is %s' % (src0.dtype, src1.dtype))
        for prm in (w_eq, w_pol, w_np, b_eq, b_pol, b_np):
            _f32_param(prm, 'cs_conv')
        kh, kw, cin, Cout = w_eq.shape
        if kh != ksize or kw != ksize or cin != (c0_valid or C0) + C1:
            raise ValueError('cs_conv: kernel shape %s does not match ksize=%d, C_in=%d' % (tuple(w_eq.shape), ksize,
                                                                                          (c0_valid or C0) + C1))
        w_eq, w_pol = _c(w_eq), _c(w_pol)
        w_np = _c(w_np) if w_np is not None else None
        d = _make_desc(B, N, C0, C1, Cout, ksize, halo, up0, flip, act, alpha, vmax, nat.dtype_tag(src0), c0_valid)
        No = N if halo else N - ksize + 1
        if out_padded:
            if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (src0, src1, w_eq)):
                raise RuntimeError('cs_conv: out_padded is an inference-only layout')
            d.flags |= nat.CONV_OUT_PADDED
        y = torch.empty((B, 6, No, No, (Cout + 7) // 8 * 8 if out_padded else Cout), dtype=src0.dtype, device=src0.device)
        table = inv = None
        if halo:
            table, inv = nat.halo_tables(N, (ksize - 1) // 2, src0.device)
        nbytes = lib().dlwpcs_conv_workspace_bytes(ctypes.byref(d))
        ws = _workspace(nbytes, src0.device)
        packed = PREPACKED.get(id(w_eq))
        if packed is not None and packed[0] != d.dtype:
            packed = None
        yp = None
        if want_pool and halo and No % 2 == 0:
            yp = torch.empty((B, 6, No // 2, No // 2, Cout), dtype=src0.dtype, device=src0.device)
        wargs = ((ptr(packed[1]), 0, 0, ptr(packed[2]) if b_eq is not None else 0, 0, 0) if packed is not None else
                 (ptr(w_eq), ptr(w_pol), ptr(w_np), ptr(b_eq), ptr(b_pol), ptr(b_np)))
        if packed is not None:
            d.flags |= nat.CONV_PREPACKED
        small = bool(small) and _small_conv_ok(d)
        if yp is not None:
            check(lib().dlwpcs_conv_fwd_pool(ctypes.byref(d), ptr(src0), ptr(src1), *wargs, ptr(y), ptr(yp), ptr(table), ptr(ws),
                                             ws.numel(), stream_ptr()), 'dlwpcs_conv_fwd_pool')
            _POOLED[y.data_ptr()] = yp
        else:
            rc = nat.E_UNSUPPORTED
            if small:
                rc = lib().dlwpcs_conv_small_fwd(ctypes.byref(d), ptr(src0), ptr(src1), *wargs, ptr(y), ptr(table), ptr(ws),
                                                 ws.numel(), stream_ptr())
            if rc == nat.E_UNSUPPORTED:
                rc = lib().dlwpcs_conv_fwd(ctypes.byref(d), ptr(src0), ptr(src1), *wargs, ptr(y), ptr(table), ptr(ws),
                                           ws.numel(), stream_ptr())
            check(rc, 'dlwpcs_conv_fwd')
        ctx.small = small
        if premask0 is not None and premask1 is not None and tuple(premask0) != tuple(premask1):
            raise ValueError('cs_conv: both sources must share the activation parameters of their masks')
        ctx.premask = (premask0, premask1)
        ctx.dy_premasked = bool(dy_premasked) and act != nat.ACT_NONE
        ctx.defer_ring0 = bool(defer_ring0)
        ctx.packed = packed
        ctx.desc = d
        ctx.tables = (table, inv)
        ctx.has = (src1 is not None, w_np is not None, b_eq is not None, b_np is not None)
        # parameter objects (leaves whose .grad may be a view into the model's flat gradient buffer, see backward)
        ctx.params = (w_eq, w_pol, w_np, b_eq, b_pol, b_np)
        ctx.save_for_backward(src0, src1, w_eq, w_pol, w_np, y if act != nat.ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        src0, src1, w_eq, w_pol, w_np, y = ctx.saved_tensors
        d = ctx.desc
        table, inv = ctx.tables
        has_src1, has_np, has_bias, has_bnp = ctx.has
        dy = _c(dy)
        dev = dy.device
        nbytes = lib().dlwpcs_conv_workspace_bytes(ctypes.byref(d))
        need = ctx.needs_input_grad
        dsrc0 = torch.empty_like(src0) if need[0] else None
        dsrc1 = torch.empty_like(src1) if (has_src1 and need[1]) else None
        want_w = any(need[2:8])
        direct = DIRECT_PARAM_GRADS and (need[2] or need[3]) and all(
            p is None or (p.is_leaf and p.grad is not None and p.grad.is_contiguous()) for p in ctx.params)
        pm0, pm1 = ctx.premask
        if dsrc0 is None:
            pm0 = None
        if dsrc1 is None:
            pm1 = None
        masked_io = ctx.dy_premasked or pm0 is not None or pm1 is not None
        if masked_io:
            # Pre-masked gradient convention.  dy_premasked: dy is dz already -> both gradient kernels run as for a layer
            # without activation and never read y.  Otherwise (only the sources want masks) dz is formed once, elementwise.
            if ctx.dy_premasked or d.act == nat.ACT_NONE:
                dz = dy
            else:
                dz = torch.empty_like(dy)
                check(lib().dlwpcs_act_bwd(ptr(dy), ptr(y), ptr(dz), dy.numel(), nat.ACT_LEAKY_CLIP, d.alpha, d.vmax,
                                           nat.dtype_tag(dy), stream_ptr()), 'dlwpcs_act_bwd')
            dn = ConvDesc.from_buffer_copy(d)
            dn.act = nat.ACT_NONE
            dn.flags = (d.flags & nat.CONV_PREPACKED) | _gather_flag(d, dev)
            batching = (direct and WGRAD_BATCH and d.B > 0 and not WGRAD_SIDE_STREAM and wgrad_batch_supported(dn))
            defer = direct and DEFER_WGRAD_REDUCE and not WGRAD_SIDE_STREAM and d.B > 0 and not batching
            ws = _workspace(nbytes, dev, 'defer%d' % len(_deferred)) if defer else _workspace(nbytes, dev)
            ring = None
            if ctx.defer_ring0 and dsrc0 is not None and pm0 is None and halo_ring_info(dn) is not None:
                ring = halo_ring_info(dn)
                dn.flags |= nat.CONV_DEFER_RING0
                # The ring stays intact until the pooling adjoint ran.  A node that also defers its reduction keeps the workspace
                # of its 'defer' role, which lives until flush_deferred_reduce(): the adjoint takes its entry out of _pending_ring,
                # so the next ring node is given the same 'ring' role again -- its launches would overwrite the partial sums a
                # reduce item of this node still points to.
                if not defer:
                    ws = _workspace(nbytes, dev, 'ring%d' % len(_pending_ring))
            if dsrc0 is not None or dsrc1 is not None:
                wq = ctx.packed[3] if ctx.packed is not None else w_eq
                pm = pm0 if pm0 is not None else pm1
                ma, mv = (float(pm[0]), float(pm[1])) if pm is not None else (0.0, 0.0)
                bargs = (ctypes.byref(dn), ptr(dz), ptr(wq), ptr(w_pol), ptr(w_np), ptr(dsrc0), ptr(dsrc1),
                         ptr(src0 if pm0 is not None else None), ptr(src1 if pm1 is not None else None), ma, mv, ptr(inv), ptr(ws),
                         ws.numel(), stream_ptr())
                rc = nat.E_UNSUPPORTED
                if ctx.small and dsrc0 is not None and dsrc1 is None:
                    rc = lib().dlwpcs_conv_small_bwd_data(*bargs)
                if rc == nat.E_UNSUPPORTED:
                    rc = lib().dlwpcs_conv_bwd_data_masked(*bargs)
                check(rc, 'dlwpcs_conv_bwd_data_masked')
                if ring is not None:
                    _pending_ring[dsrc0.data_ptr()] = (ws, ring[0], ring[1], nat.halo_tables(d.N, 1, dev)[1])
                    dn.flags &= ~nat.CONV_DEFER_RING0
            dw_eq, dw_pol, dw_np, db_eq, db_pol, db_np = _weight_gradients(
                dn, src0, src1, dz, None, ctx.params, table, ws, nbytes, direct, defer, need[2:8], has_np, has_bias, has_bnp)
            return (dsrc0, dsrc1, dw_eq, dw_pol, dw_np, db_eq, db_pol, db_np) + (None,) * 15
        no_dgrad = dsrc0 is None and dsrc1 is None        # (first layer: the batched kernel applies act' itself)
        # (exact-fp32 mode: the batched kernel forms dz = dy * act'(y) on load in every 3x3 layer -- exact in fp32, so the
        #  data-gradient kernel forming its own copy changes no bits -- and no dz hand-over is written at all)
        mask_on_load = d.ksize == 3 and (no_dgrad or d.dtype == nat.F32)
        batching = (direct and WGRAD_BATCH and d.B > 0 and not WGRAD_SIDE_STREAM and wgrad_batch_supported(d)
                    and (d.act == nat.ACT_NONE or mask_on_load))
        defer = direct and DEFER_WGRAD_REDUCE and not WGRAD_SIDE_STREAM and d.B > 0 and not batching
        # deferred reduction: the partials (and the dz hand-over next to them) live in this node's own workspace
        ws = _workspace(nbytes, dev, 'defer%d' % len(_deferred)) if defer else _workspace(nbytes, dev)
        reuse_dz = ((dsrc0 is not None or dsrc1 is not None) and want_w and d.act != nat.ACT_NONE
                    and not WGRAD_SIDE_STREAM and not batching)
        if reuse_dz:
            # the weight-gradient kernel computes dz = dy * act'(y) anyway: launched FIRST, it leaves dz in the workspace
            # for the data-gradient kernel right behind it (which then reads neither y nor does the act' arithmetic)
            d.flags |= nat.CONV_REUSE_DZ

        def run_bwd_data():
            if dsrc0 is not None or dsrc1 is not None:
                # (d.flags carries CONV_PREPACKED from the forward when packed buffers were used)
                wq = ctx.packed[3] if ctx.packed is not None else w_eq
                d.flags |= _gather_flag(d, dev)         # (honoured where the gradient needs no mask on load: layers without activation)
                check(lib().dlwpcs_conv_bwd_data(ctypes.byref(d), ptr(dy), ptr(y), ptr(wq), ptr(w_pol), ptr(w_np),
                                                 ptr(dsrc0), ptr(dsrc1), ptr(inv), ptr(ws), ws.numel(), stream_ptr()),
                      'dlwpcs_conv_bwd_data')
                d.flags &= ~nat.CONV_DGRAD_GATHER
        if not reuse_dz:
            run_bwd_data()
        dw_eq, dw_pol, dw_np, db_eq, db_pol, db_np = _weight_gradients(
            d, src0, src1, dy, y, ctx.params, table, ws, nbytes, direct, defer, need[2:8], has_np, has_bias, has_bnp,
            batch_mask_ok=mask_on_load)
        if reuse_dz:
            run_bwd_data()
        return (dsrc0, dsrc1, dw_eq, dw_pol, dw_np, db_eq, db_pol, db_np) + (None,) * 15


def _small_conv_ok(d):
    """Layers worth offering to the small-face kernel (the library decides: it answers E_UNSUPPORTED for what it does not serve)."""
    return (d.dtype == nat.BF16 and d.ksize == 3 and d.halo and d.C1 == 0 and not d.up0 and d.c0_valid == 0
            and d.N * d.N <= 320 and d.C0 % 32 == 0 and d.Cout % 32 == 0 and d.B > 0)


_ring_info_cache = {}

# Data gradient in gather form (dlwpcs.h: DLWPCS_CONV_DGRAD_GATHER; the adjoint of CubeSpherePadding2D, DLWP/custom.py:1198-1308, folded
# into the data-gradient kernel): bf16 3x3 halo layers whose gradient arrives as dz compute every border cell completely inside the
# kernel -- no halo ring is materialised, no fix-up launch, one rounding per cell (tests/test_gpu_dgrad_gather.py: <= 1 bf16 ulp against
# the fp64 oracle); window_src 2 x 2 sums for upsampled sources.  Default since round 5 (weight substitution inside the matrix phase:
# as fast as the padded-grid kernel + the fix-up launches it replaces, 24 instead of 31 launches per unet2 step); faces whose tile
# holds both edge rows (N <= 16) and the exact-fp32 mode keep the padded-grid path.  Engine option dgrad_gather=0 (DLWP/options.py)
# restores it everywhere.


def _gather_flag(d, dev):
    if option('dgrad_gather') and d.halo and d.ksize == 3 and d.dtype == nat.BF16 and nat.dgrad_gather_ready(d.N, 1, dev):
        return nat.CONV_DGRAD_GATHER
    return 0


def halo_ring_info(d):
    """(byte offset of the padded gradient in the workspace, its channel count) if a data-gradient call on `d` with
    CONV_DEFER_RING0 leaves the fix-up of source 0 to the caller, else None (dlwpcs_conv_ring_info)."""
    key = (d.B, d.N, d.C0, d.C1, d.Cout, d.ksize, d.halo, d.up0, d.dtype, d.c0_valid, d.flags & nat.CONV_DGRAD_GATHER)
    if key not in _ring_info_cache:
        off, ch = ctypes.c_size_t(), ctypes.c_int()
        ok = lib().dlwpcs_conv_ring_info(ctypes.byref(d), ctypes.byref(off), ctypes.byref(ch))
        _ring_info_cache[key] = (off.value, ch.value) if ok else None
    return _ring_info_cache[key]


def conv_packed_buffers(ksize, cin, cout, dtype_tag, device, bias=True):
    """Allocate (wpk_fwd, bias_pk | None, wpk_bwd) for one layer; sizes from dlwpcs_conv_packed_bytes."""
    d = _make_desc(1, max(ksize, 2), cin, 0, cout, ksize, False, False, True, nat.ACT_NONE, 0.0, 0.0, dtype_tag)
    out = []
    for which in (nat.PACK_FWD, nat.PACK_BIAS, nat.PACK_BWD):
        n = lib().dlwpcs_conv_packed_bytes(ctypes.byref(d), which)
        if n == 0:
            check(-1, 'dlwpcs_conv_packed_bytes')
        out.append(torch.empty(n, dtype=torch.uint8, device=device))
    if not bias:
        out[1] = None
    return tuple(out)


def make_pack_items(entries, device):
    """
    entries: list of (w_eq, w_pol, w_np, b_eq, b_pol, b_np, (wpk_fwd, bias_pk, wpk_bwd), ksize, flip, dtype_tag).
    Returns the device-resident dlwpcs_pack_item array (uint8 tensor) for dlwpcs_pack_batch.
    """
    arr = (nat.PackItem * len(entries))()
    for it, (we, wp, wn, be, bp, bn, bufs, ksize, flip, tag) in zip(arr, entries):
        it.w_eq, it.w_pol, it.w_np = ptr(we), ptr(wp), ptr(wn)
        it.b_eq, it.b_pol, it.b_np = ptr(be), ptr(bp), ptr(bn)
        it.wpk_fwd, it.bias_pk, it.wpk_bwd = ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2])
        it.ksize, it.Cin, it.Cout = int(ksize), int(we.shape[2]), int(we.shape[3])
        it.flip_north_pole, it.dtype, it.reserved = int(flip), int(tag), 0
    raw = bytes(arr)
    host = torch.frombuffer(bytearray(raw), dtype=torch.uint8) if raw else torch.empty(0, dtype=torch.uint8)
    return host.to(device)


def pack_batch(items_dev, n_items):
    check(lib().dlwpcs_pack_batch(ptr(items_dev), int(n_items), stream_ptr()), 'dlwpcs_pack_batch')


def cs_conv(src0, w_eq, w_pol, w_np=None, b_eq=None, b_pol=None, b_np=None, src1=None, ksize=3, halo=True, up0=False,
            flip_north_pole=True, act=nat.ACT_NONE, alpha=0.0, vmax=0.0, premask0=None, premask1=None, dy_premasked=False,
            defer_ring0=False, want_pool=False, out_padded=False, small=False):
    """small: offer the layer to the small-face kernel first (the engine passes its option small_conv; direct callers keep the
    general kernel unless they ask)."""
    if (w_np is None) != (b_np is None) and b_eq is not None:
        raise ValueError('cs_conv: north-pole kernel and bias must be given together')
    # Network inputs with a channel count that is not a multiple of the 16-B vector (7 variables; optionally 14 = 7 x 2):
    # stored with zero channels up to the vector width (dlwpcs_conv_desc.c0_valid), so that every kernel takes its vector
    # path.  A caller that already holds the padded layout (Model pads its static input buffers once, the device batch feed
    # gathers straight into it) passes it as is.
    c0_valid = 0
    cin_w = w_eq.shape[2]
    if src1 is None and not up0:
        c_phys = src0.shape[-1]
        if c_phys == cin_w:
            cp = padded_channels(c_phys, src0.dtype)
            if cp != c_phys:
                src0 = pad_channels(src0, cp)
                c0_valid = cin_w
        elif cin_w < c_phys <= (cin_w + channel_vector(src0.dtype) - 1) // channel_vector(src0.dtype) * channel_vector(src0.dtype):
            c0_valid = cin_w
    return _CSConv.apply(src0, src1, w_eq, w_pol, w_np, b_eq, b_pol, b_np, int(ksize), bool(halo), bool(up0),
                         bool(flip_north_pole), int(act), float(alpha), float(vmax), int(c0_valid), premask0, premask1,
                         bool(dy_premasked), bool(defer_ring0), bool(want_pool), bool(out_padded), bool(small))


def cs_conv_head_applicable(src0, src1, w_eq, head_w_eq, out_padded):
    """True when dlwpcs_conv_fwd_head can serve (last 3x3 layer, pointwise head) of an inference pass: bf16 device tensors, both
    layers' operands packed for this pass (PREPACKED), 32 channels between them and head rows of 32 channels."""
    if torch.is_grad_enabled() or not src0.is_cuda or src0.dtype != torch.bfloat16:
        return False
    pk, hk = PREPACKED.get(id(w_eq)), PREPACKED.get(id(head_w_eq))
    if pk is None or hk is None or pk[0] != nat.BF16 or hk[0] != nat.BF16:
        return False
    cout2 = head_w_eq.shape[3]
    rows = (cout2 + 7) // 8 * 8 if out_padded else cout2
    c0, c1 = src0.shape[-1], (src1.shape[-1] if src1 is not None else 0)
    if c0 % 8 or c1 % 8 or c0 + c1 != w_eq.shape[2]:
        return False
    return (tuple(w_eq.shape[:2]) == (3, 3) and w_eq.shape[3] == 32 and tuple(head_w_eq.shape[:3]) == (1, 1, 32) and rows == 32
            and cout2 % 2 == 0 and cout2 >= 8)


def cs_conv_head(src0, w_eq, b_eq, head_w_eq, head_b_eq, src1=None, up0=False, flip_north_pole=True, act=nat.ACT_NONE,
                 alpha=0.0, vmax=0.0, out_padded=False):
    """Inference: y_head = conv1x1(act(conv3x3(halo_pad(concat(up?(src0), src1))) + b)) + b_head through dlwpcs_conv_fwd_head --
    the pointwise output layer folded into the epilogue of the convolution in front of it (Azure/train_cs.py:300-305).  The
    weights are identified by the layers' equatorial kernels (their packed operands of this pass: PREPACKED).  No autograd."""
    require_device(src0, 'cs_conv_head')
    src0 = _c(src0)
    B = src0.shape[0]
    N = src0.shape[2] * (2 if up0 else 1)
    C0, C1 = src0.shape[4], 0
    if src1 is not None:
        src1 = _c(src1)
        C1 = src1.shape[4]
    Cout, cout2 = w_eq.shape[3], head_w_eq.shape[3]
    pk, hk = PREPACKED[id(w_eq)], PREPACKED[id(head_w_eq)]
    d = _make_desc(B, N, C0, C1, Cout, 3, True, up0, flip_north_pole, act, alpha, vmax, nat.BF16, 0)
    d.flags |= nat.CONV_PREPACKED
    dh = _make_desc(B, N, Cout, 0, cout2, 1, False, False, flip_north_pole, nat.ACT_NONE, 0.0, 0.0, nat.BF16, 0)
    dh.flags |= nat.CONV_PREPACKED | (nat.CONV_OUT_PADDED if out_padded else 0)
    rows = (cout2 + 7) // 8 * 8 if out_padded else cout2
    y = torch.empty((B, 6, N, N, Cout), dtype=src0.dtype, device=src0.device)
    yh = torch.empty((B, 6, N, N, rows), dtype=src0.dtype, device=src0.device)
    table = nat.halo_tables(N, 1, src0.device)[0]
    nbytes = max(lib().dlwpcs_conv_workspace_bytes(ctypes.byref(d)), lib().dlwpcs_conv_workspace_bytes(ctypes.byref(dh)))
    ws = _workspace(nbytes, src0.device)
    fused = ctypes.c_int(0)
    check(lib().dlwpcs_conv_fwd_head(ctypes.byref(d), ptr(src0), ptr(src1), ptr(pk[1]), ptr(pk[2]) if b_eq is not None else 0,
                                     ctypes.byref(dh), ptr(hk[1]), ptr(hk[2]) if head_b_eq is not None else 0, ptr(y), ptr(yh),
                                     ptr(table), ptr(ws), ws.numel(), ctypes.byref(fused), stream_ptr()), 'dlwpcs_conv_fwd_head')
    global HEAD_FOLDED
    HEAD_FOLDED = bool(fused.value)
    return yh


HEAD_FOLDED = False     # (what the last cs_conv_head call did: tests / diagnostics)


# ------------------------------------------------------------------------------------------------------------------ #
# Generic per-face convolution for the off-hot-path layer options (strides, dilation, 'same')
# ------------------------------------------------------------------------------------------------------------------ #

def _same_pads(n, k, s, dil):
    out = -(-n // s)
    total = max((out - 1) * s + (k - 1) * dil + 1 - n, 0)
    return total // 2, out


def _valid_len(n, k, s, dil):
    """output length of a 'valid' axis; < 1 when the dilated window does not fit (cs_gconv then raises)"""
    return (n - (k - 1) * dil - 1) // s + 1


class _GConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_eq, w_pol, w_np, b_eq, b_pol, b_np, strides, padding, dilation, flip):
        require_device(x, 'cs_gconv')
        for prm in (w_eq, w_pol, w_np, b_eq, b_pol, b_np):
            _f32_param(prm, 'cs_gconv')
        x, w_eq, w_pol = _c(x), _c(w_eq), _c(w_pol)
        w_np = _c(w_np) if w_np is not None else None
        B, F6, H, W, Cin = x.shape
        kh, kw, cin, Cout = w_eq.shape
        if F6 != 6 or cin != Cin:
            raise ValueError('cs_gconv: bad shapes x=%s kernel=%s' % (tuple(x.shape), tuple(w_eq.shape)))
        sh, sw = strides
        dh, dw = dilation
        if padding == 'same':
            pad_t, Ho = _same_pads(H, kh, sh, dh)
            pad_l, Wo = _same_pads(W, kw, sw, dw)
        elif padding == 'valid':
            pad_t = pad_l = 0
            Ho = _valid_len(H, kh, sh, dh)
            Wo = _valid_len(W, kw, sw, dw)
        else:
            raise ValueError('padding must be "valid" or "same"')
        if Ho < 1 or Wo < 1:
            raise ValueError('cs_gconv: empty output')
        d = GConvDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, kh=kh, kw=kw, sh=sh, sw=sw, dh=dh, dw=dw, pad_t=pad_t,
                      pad_l=pad_l, Ho=Ho, Wo=Wo, flip_north_pole=int(flip), dtype=nat.dtype_tag(x))
        y = torch.empty((B, 6, Ho, Wo, Cout), dtype=x.dtype, device=x.device)
        check(lib().dlwpcs_gconv_fwd(ctypes.byref(d), ptr(x), ptr(w_eq), ptr(w_pol), ptr(w_np), ptr(b_eq), ptr(b_pol),
                                     ptr(b_np), ptr(y), stream_ptr()), 'dlwpcs_gconv_fwd')
        ctx.desc = d
        ctx.has = (w_np is not None, b_eq is not None, b_np is not None)
        ctx.save_for_backward(x, w_eq, w_pol, w_np)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w_eq, w_pol, w_np = ctx.saved_tensors
        d = ctx.desc
        has_np, has_bias, has_bnp = ctx.has
        dy = _c(dy)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            check(lib().dlwpcs_gconv_bwd_data(ctypes.byref(d), ptr(dy), ptr(w_eq), ptr(w_pol), ptr(w_np), ptr(dx),
                                              stream_ptr()), 'dlwpcs_gconv_bwd_data')
        dw_eq, dw_pol = torch.empty_like(w_eq), torch.empty_like(w_pol)
        dw_np = torch.empty_like(w_np) if has_np else None
        db_eq = db_pol = db_np = None
        if has_bias:
            db_eq = torch.empty(d.Cout, dtype=torch.float32, device=dy.device)
            db_pol = torch.empty_like(db_eq)
            db_np = torch.empty_like(db_eq) if has_bnp else None
        check(lib().dlwpcs_gconv_bwd_weights(ctypes.byref(d), ptr(x), ptr(dy), ptr(dw_eq), ptr(dw_pol), ptr(dw_np),
                                             ptr(db_eq), ptr(db_pol), ptr(db_np), stream_ptr()),
              'dlwpcs_gconv_bwd_weights')
        return dx, dw_eq, dw_pol, dw_np, db_eq, db_pol, db_np, None, None, None, None


def cs_gconv(x, w_eq, w_pol, w_np=None, b_eq=None, b_pol=None, b_np=None, strides=(1, 1), padding='valid',
             dilation=(1, 1), flip_north_pole=True):
    return _GConv.apply(x, w_eq, w_pol, w_np, b_eq, b_pol, b_np, tuple(strides), padding, tuple(dilation),
                        bool(flip_north_pole))


# ------------------------------------------------------------------------------------------------------------------ #
# Keras stock ops of the U-Net (Azure/train_cs.py:197-199)
# ------------------------------------------------------------------------------------------------------------------ #

class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, alpha, vmax):
        require_device(x, 'leaky_clip_relu')
        x = _c(x)
        y = torch.empty_like(x)
        check(lib().dlwpcs_act_fwd(ptr(x), ptr(y), x.numel(), nat.ACT_LEAKY_CLIP, alpha, vmax, nat.dtype_tag(x),
                                   stream_ptr()),
              'dlwpcs_act_fwd')
        ctx.alpha, ctx.vmax = alpha, vmax
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _c(dy)
        dx = torch.empty_like(dy)
        check(lib().dlwpcs_act_bwd(ptr(dy), ptr(y), ptr(dx), dy.numel(), nat.ACT_LEAKY_CLIP, ctx.alpha, ctx.vmax,
                                   nat.dtype_tag(dy), stream_ptr()), 'dlwpcs_act_bwd')
        return dx, None, None


def leaky_clip_relu(x, negative_slope=0.0, max_value=None):
    vmax = float('inf') if max_value is None else float(max_value)
    return _Act.apply(x, float(negative_slope), vmax)


def _bnc(x, what):
    require_device(x, what)
    if x.dim() != 5 or x.shape[1] != 6 or x.shape[2] != x.shape[3]:
        raise ValueError('%s: expected (B, 6, N, N, C), got %s' % (what, tuple(x.shape)))
    return x.shape[0], x.shape[2], x.shape[4]


class _AvgPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, premask=None):
        B, N, C = _bnc(x, 'avgpool2')
        if N % 2:
            raise ValueError('avgpool2: odd face size %d' % N)
        x = _c(x)
        y = torch.empty((B, 6, N // 2, N // 2, C), dtype=x.dtype, device=x.device)
        check(lib().dlwpcs_avgpool2_fwd(ptr(x), ptr(y), B, N, C, nat.dtype_tag(x), stream_ptr()), 'dlwpcs_avgpool2_fwd')
        ctx.shape = (B, N, C)
        ctx.premask = premask
        if premask is not None:
            ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, N, C = ctx.shape
        dy = _c(dy)
        dx = torch.empty((B, 6, N, N, C), dtype=dy.dtype, device=dy.device)
        if ctx.premask is not None:
            (x,) = ctx.saved_tensors
            check(lib().dlwpcs_avgpool2_bwd_masked(ptr(dy), 0, ptr(x), ptr(dx), B, N, C, float(ctx.premask[0]),
                                                   float(ctx.premask[1]), nat.dtype_tag(dy), stream_ptr()),
                  'dlwpcs_avgpool2_bwd_masked')
            return dx, None
        check(lib().dlwpcs_avgpool2_bwd(ptr(dy), ptr(dx), B, N, C, nat.dtype_tag(dy), stream_ptr()),
              'dlwpcs_avgpool2_bwd')
        return dx, None


class _AvgPool2Skip(torch.autograd.Function):
    """(pooled, alias of x): x feeds the pooling AND later consumers (a U-Net skip connection).  Routing those consumers
    through the alias hands this node both gradients at once, so the backward is ONE pass
    dx = d_alias + avgpool2_bwd(d_pooled) instead of avgpool2_bwd + autograd's elementwise add."""

    @staticmethod
    def forward(ctx, x, premask=None):
        """premask = (negative_slope, max_value) | None: x is the output of an activated layer that expects its gradient
        pre-masked; the backward then writes act'(x) * (d_alias + avgpool2_bwd(d_pooled)) (the alias itself is NOT premask: its
        consumers hand back plain gradients)."""
        B, N, C = _bnc(x, 'avgpool2')
        if N % 2:
            raise ValueError('avgpool2: odd face size %d' % N)
        x = _c(x)
        y = _POOLED.pop(x.data_ptr(), None)         # the producing convolution pooled in its epilogue (want_pool)
        if y is None or tuple(y.shape) != (B, 6, N // 2, N // 2, C) or y.dtype != x.dtype:
            y = torch.empty((B, 6, N // 2, N // 2, C), dtype=x.dtype, device=x.device)
            check(lib().dlwpcs_avgpool2_fwd(ptr(x), ptr(y), B, N, C, nat.dtype_tag(x), stream_ptr()), 'dlwpcs_avgpool2_fwd')
        ctx.shape = (B, N, C)
        ctx.dtype = x.dtype
        ctx.premask = premask
        if premask is not None:
            ctx.save_for_backward(x)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dskip):
        B, N, C = ctx.shape
        if ctx.premask is not None:
            (x,) = ctx.saved_tensors
            if dy is None:
                dx = _c(dskip).clone()
                check(lib().dlwpcs_act_bwd(ptr(dx), ptr(x), ptr(dx), dx.numel(), nat.ACT_LEAKY_CLIP, float(ctx.premask[0]),
                                           float(ctx.premask[1]), nat.dtype_tag(dx), stream_ptr()), 'dlwpcs_act_bwd')
                return dx, None
            ring = _pending_ring.pop(dy.data_ptr(), None)
            dy = _c(dy)
            dskip = _c(dskip) if dskip is not None else None
            dx = torch.empty((B, 6, N, N, C), dtype=dy.dtype, device=dy.device)
            if ring is not None:
                # dy holds the interior contributions of its producer's data gradient; the halo ring is still in that call's
                # workspace: added here, no fix-up launch
                rws, roff, rch, rinv = ring
                check(lib().dlwpcs_avgpool2_bwd_ring(ptr(dy), ptr(dskip), ptr(x), ptr(dx), B, N, C, float(ctx.premask[0]),
                                                     float(ctx.premask[1]), nat.dtype_tag(dy), rws.data_ptr() + roff, ptr(rinv),
                                                     rch, 0, stream_ptr()), 'dlwpcs_avgpool2_bwd_ring')
                return dx, None
            check(lib().dlwpcs_avgpool2_bwd_masked(ptr(dy), ptr(dskip), ptr(x), ptr(dx), B, N, C, float(ctx.premask[0]),
                                                   float(ctx.premask[1]), nat.dtype_tag(dy), stream_ptr()),
                  'dlwpcs_avgpool2_bwd_masked')
            return dx, None
        if dy is None:
            return dskip, None
        dy = _c(dy)
        dx = torch.empty((B, 6, N, N, C), dtype=dy.dtype, device=dy.device)
        if dskip is None:
            check(lib().dlwpcs_avgpool2_bwd(ptr(dy), ptr(dx), B, N, C, nat.dtype_tag(dy), stream_ptr()),
                  'dlwpcs_avgpool2_bwd')
        else:
            dskip = _c(dskip)
            check(lib().dlwpcs_avgpool2_bwd_add(ptr(dy), ptr(dskip), ptr(dx), B, N, C, nat.dtype_tag(dy), stream_ptr()),
                  'dlwpcs_avgpool2_bwd_add')
        return dx, None


def avgpool2_skip(x, premask=None):
    """-> (avgpool2(x), x') where x' aliases x and must be used by x's remaining consumers."""
    return _AvgPool2Skip.apply(x, premask)


class _Detour(torch.autograd.Function):
    """Identity with a node of its own in the autograd graph, no launch in either direction.  The split backward pass of the
    two-bucket exchange (DLWP.keras.Model) stops at the skip tensors; they are the SECOND output of the pooling node, and
    torch.autograd.grad(..., inputs=[that output]) would run every node that reaches the pooling node through its FIRST output
    as well (needed-ness is per node, not per edge) -- the whole encoder.  Behind a detour the capture point is a node only the
    decoder reaches."""
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g


def detour(x):
    return _Detour.apply(x)


class _Upsample2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, N, C = _bnc(x, 'upsample2')
        x = _c(x)
        y = torch.empty((B, 6, 2 * N, 2 * N, C), dtype=x.dtype, device=x.device)
        check(lib().dlwpcs_upsample2_fwd(ptr(x), ptr(y), B, N, C, nat.dtype_tag(x), stream_ptr()),
              'dlwpcs_upsample2_fwd')
        ctx.shape = (B, N, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, N, C = ctx.shape
        dy = _c(dy)
        dx = torch.empty((B, 6, N, N, C), dtype=dy.dtype, device=dy.device)
        check(lib().dlwpcs_upsample2_bwd(ptr(dy), ptr(dx), B, N, C, nat.dtype_tag(dy), stream_ptr()),
              'dlwpcs_upsample2_bwd')
        return dx


def avgpool2(x, premask=None):
    return _AvgPool2.apply(x, premask)


def upsample2(x):
    return _Upsample2.apply(x)


class _Concat2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        require_device(a, 'concat2')
        require_device(b, 'concat2')
        if a.shape[:-1] != b.shape[:-1]:
            raise ValueError('concat2: leading shapes differ: %s vs %s' % (tuple(a.shape), tuple(b.shape)))
        if a.dtype != b.dtype:
            raise TypeError('concat2: dtypes differ: %s vs %s' % (a.dtype, b.dtype))
        a, b = _c(a), _c(b)
        Ca, Cb = a.shape[-1], b.shape[-1]
        rows = a.numel() // Ca
        y = torch.empty(a.shape[:-1] + (Ca + Cb,), dtype=a.dtype, device=a.device)
        check(lib().dlwpcs_concat2(ptr(a), ptr(b), ptr(y), rows, Ca, Cb, nat.dtype_tag(a), stream_ptr()),
              'dlwpcs_concat2')
        ctx.c = (Ca, Cb, rows, a.shape, b.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        Ca, Cb, rows, sa, sb = ctx.c
        dy = _c(dy)
        da = torch.empty(sa, dtype=dy.dtype, device=dy.device) if ctx.needs_input_grad[0] else None
        db = torch.empty(sb, dtype=dy.dtype, device=dy.device) if ctx.needs_input_grad[1] else None
        if da is not None or db is not None:
            check(lib().dlwpcs_split2(ptr(dy), ptr(da), ptr(db), rows, Ca, Cb, nat.dtype_tag(dy), stream_ptr()),
                  'dlwpcs_split2')
        return da, db


def concat_channels(tensors):
    out = tensors[0]
    for t in tensors[1:]:
        out = _Concat2.apply(out, t)
    return out


def state_repack(state, extra, n_time):
    """Next main input of a forecast step: `state` (B, *space, T*V) with `extra` (B, T, *space, E) appended as the last E
    channels of each of the T time steps -> (B, *space, T*(V+E)).  One launch (dlwpcs_state_repack); inference only."""
    require_device(state, 'state_repack')
    require_device(extra, 'state_repack')
    if state.dtype != extra.dtype:
        raise TypeError('state_repack: state is %s but extra is %s' % (state.dtype, extra.dtype))
    state, extra = _c(state), _c(extra)
    B, T = state.shape[0], int(n_time)
    space = tuple(state.shape[1:-1])
    if state.shape[-1] % T or tuple(extra.shape[:2]) != (B, T) or tuple(extra.shape[2:-1]) != space:
        raise ValueError('state_repack: state %s / extra %s do not match %d time steps'
                         % (tuple(state.shape), tuple(extra.shape), T))
    V, E = state.shape[-1] // T, extra.shape[-1]
    S = 1
    for v in space:
        S *= int(v)
    out = torch.empty((B,) + space + (T * (V + E),), dtype=state.dtype, device=state.device)
    check(lib().dlwpcs_state_repack(ptr(state), ptr(extra), ptr(out), B, S, T, V, E, nat.dtype_tag(state), stream_ptr()),
          'dlwpcs_state_repack')
    return out


class _Transpose(torch.autograd.Function):
    """(B, C, S...) <-> (B, S..., C) layout conversion for data_format='channels_first' callers."""

    @staticmethod
    def forward(ctx, x, to_last):
        require_device(x, 'layout')
        x = _c(x)
        B = x.shape[0]
        if to_last:
            C, spatial = x.shape[1], tuple(x.shape[2:])
            S = x.numel() // (B * C) if B * C else 0
            y = torch.empty((B,) + spatial + (C,), dtype=x.dtype, device=x.device)
            check(lib().dlwpcs_cf_to_cl(ptr(x), ptr(y), B, C, S, nat.dtype_tag(x), stream_ptr()), 'dlwpcs_cf_to_cl')
        else:
            C, spatial = x.shape[-1], tuple(x.shape[1:-1])
            S = x.numel() // (B * C) if B * C else 0
            y = torch.empty((B, C) + spatial, dtype=x.dtype, device=x.device)
            check(lib().dlwpcs_cl_to_cf(ptr(x), ptr(y), B, C, S, nat.dtype_tag(x), stream_ptr()), 'dlwpcs_cl_to_cf')
        ctx.to_last = to_last
        return y

    @staticmethod
    def backward(ctx, dy):
        return _Transpose.apply(dy, not ctx.to_last), None


def channels_first_to_last(x):
    return _Transpose.apply(x, True)


def channels_last_to_first(x):
    return _Transpose.apply(x, False)


# ------------------------------------------------------------------------------------------------------------------ #
# Loss and optimizer (Azure/train_cs.py:424-430)
# ------------------------------------------------------------------------------------------------------------------ #

_mse_scratch = {}
_unit_seeds = {}


def unit_seed(device):
    """The cached ones(2) tensor DLWP.keras.Model seeds the backward of every loss node with: _MSE.backward recognises it
    by address and returns the gradient the forward kernel already wrote; any other upstream gradient is applied."""
    key = str(device)
    t = _unit_seeds.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('first training step must run eagerly (graph capture allocates nothing)')
        t = torch.ones(2, dtype=torch.float32, device=device)
        _unit_seeds[key] = t
    return t


class _MSE(torch.autograd.Function):
    """returns a (2,) tensor: [weight * mse, mae]; gradient flows through element 0 only."""

    @staticmethod
    def forward(ctx, y, t, weight):
        require_device(y, 'mse')
        require_device(t, 'mse')
        if y.shape != t.shape:
            raise ValueError('mse: shapes differ: %s vs %s' % (tuple(y.shape), tuple(t.shape)))
        tag = nat.dtype_tag(y)
        if y.dtype != t.dtype:
            if t.dtype != torch.float32:
                raise TypeError('mse: prediction is %s but target is %s' % (y.dtype, t.dtype))
            tag |= nat.MSE_TARGET_F32           # bf16 prediction scored against the fp32 target
        y, t = _c(y), _c(t)
        key = str(y.device)
        scratch = _mse_scratch.get(key)
        if scratch is None:
            scratch = torch.empty(lib().dlwpcs_mse_scratch_bytes(), dtype=torch.uint8, device=y.device)
            _mse_scratch[key] = scratch
        out = torch.empty(2, dtype=torch.float32, device=y.device)
        dy = torch.empty_like(y) if ctx.needs_input_grad[0] else None
        tag |= nat.MSE_OVERWRITE                # out = ..., no zero-fill launch
        check(lib().dlwpcs_mse_fwd_bwd(ptr(y), ptr(t), ptr(dy), ptr(out), y.numel(), weight, tag, ptr(scratch),
                                       stream_ptr()), 'dlwpcs_mse_fwd_bwd')
        ctx.save_for_backward(dy)
        return out

    @staticmethod
    def backward(ctx, dout):
        (dy,) = ctx.saved_tensors
        # The forward kernel already wrote dy = weight * 2 (y - t) / n.  DLWP.keras.Model seeds the backward with
        # unit_seed() (upstream gradient of out[0] exactly 1): no extra pass.  Any other upstream gradient (a scaled or
        # combined loss built on this op) is applied here; out[1] (mae) carries no gradient.
        seed = _unit_seeds.get(str(dout.device))
        if seed is not None and dout.data_ptr() == seed.data_ptr():
            return dy, None, None
        return (dy.float() * dout[0]).to(dy.dtype), None, None


def mse_mae(y, t, weight=1.0):
    return _MSE.apply(y, t, float(weight))


# ---- the other training losses (DLWP.keras.losses / DLWP.custom: 'mae', latitude-weighted, anomaly correlation) ----------
_KINDS = {'mse': nat.LOSS_MSE, 'mae': nat.LOSS_MAE, 'acc': nat.LOSS_ACC}
_REGS = {None: nat.REG_NONE, 'mse': nat.REG_MSE, 'mae': nat.REG_MAE, 'global': nat.REG_GLOBAL}
_NORMS = {'all': nat.NORM_ALL, 'valid': nat.NORM_VALID}


def _loss_field(a, sample_shape, channels_first, what):
    """A weight / climatology field as dlwpcs_loss_desc takes it: broadcast to ONE sample of the model's output, moved to the
    loss's channels_last layout (the engine forms the loss channels_last), stored per cell when it is constant along the
    channels -> (flat fp32 array, div, period)."""
    a = np.asarray(a, dtype=np.float32)
    while a.ndim > len(sample_shape) and a.shape[0] == 1:
        a = a[0]
    try:
        full = np.broadcast_to(a, tuple(sample_shape))
    except ValueError:
        raise ValueError('%s of shape %s does not broadcast to the model output %s' % (what, a.shape, tuple(sample_shape)))
    if channels_first and full.ndim == 4:
        full = np.moveaxis(full, 0, -1)
    c = full.shape[-1] if full.ndim else 1
    if c > 1 and np.array_equal(full, np.broadcast_to(full[..., :1], full.shape)):
        return np.array(full[..., 0]).ravel(), c, full.size // c
    return np.array(full).ravel(), 1, full.size


class DeviceLoss(object):
    """A DLWP.keras.losses.LossSpec made ready for the kernels of one model output: fp32 weight / climatology fields uploaded
    to the model's device ONCE (Model.compile), in the channels_last layout the loss is formed in."""

    def __init__(self, spec, sample_shape, channels_first, device):
        if spec.kind not in _KINDS:
            raise NotImplementedError('loss kind %r' % (spec.kind,))
        if spec.regularize not in _REGS:
            raise NotImplementedError("anomaly-correlation regularize_mean=%r: the DLWP-CS engine builds None / 'mse' / 'mae' / "
                                      "'global' ('spatial' averages over the layout's last two axes per sample: reference "
                                      "DLWP/custom.py:1604-1606,1657-1659)" % (spec.regularize,))
        masked = getattr(spec, 'masked', None)
        if masked is not None and masked not in _NORMS:
            raise ValueError("masked loss: normalize must be 'all' or 'valid', got %r" % (masked,))
        if masked is not None and spec.kind == 'acc':
            raise NotImplementedError('a masked anomaly-correlation loss is not built')
        self.spec = spec
        self.masked = masked            # None, 'all' or 'valid': NaN targets are holes (dlwpcs_loss_masked_fwd_bwd)
        self.kind, self.reg, self.reverse = _KINDS[spec.kind], _REGS[spec.regularize], bool(spec.reverse)
        self.w = self.c = None
        self.wdiv = self.wper = self.cdiv = self.cper = 0
        if spec.weights is not None:
            f, self.wdiv, self.wper = _loss_field(spec.weights, sample_shape, channels_first, 'latitude weight field')
            self.w = torch.as_tensor(f, device=device)
        if spec.clim is not None and spec.kind == 'acc':
            f, self.cdiv, self.cper = _loss_field(spec.clim, sample_shape, channels_first, 'climatology')
            self.c = torch.as_tensor(f, device=device)

    def desc(self, loss_weight, overwrite):
        L = nat.LossDesc()
        L.kind, L.loss_weight, L.regularize, L.reverse, L.overwrite = self.kind, float(loss_weight), self.reg, int(self.reverse), overwrite
        if self.w is not None:
            L.weight, L.weight_div, L.weight_period = ptr(self.w), self.wdiv, self.wper
        if self.c is not None:
            L.clim, L.clim_div, L.clim_period = ptr(self.c), self.cdiv, self.cper
        return L

    def fused_ok(self, cout, cells):
        """Does the fused head (dlwpcs_head_loss_step) serve it: 'mse' / 'mae' with no weight or a per-cell one, not masked
        (a masked loss runs as pw_fwd -> dlwpcs_loss_masked_fwd_bwd -> pw_dgrad, like the anomaly correlation)."""
        return (self.masked is None and self.kind in (nat.LOSS_MSE, nat.LOSS_MAE) and self.c is None
                and (self.w is None or (self.wdiv == cout and self.wper == cells)))


_loss_scratch = {}


class _Loss(torch.autograd.Function):
    """returns a (2,) tensor: [loss_weight * loss, mae] (dlwpcs_loss_fwd_bwd, or dlwpcs_loss_masked_fwd_bwd for a masked
    DeviceLoss); gradient flows through element 0 only."""

    @staticmethod
    def forward(ctx, y, t, dl, weight):
        require_device(y, 'loss')
        require_device(t, 'loss')
        if y.shape != t.shape:
            raise ValueError('loss: shapes differ: %s vs %s' % (tuple(y.shape), tuple(t.shape)))
        tag = nat.dtype_tag(y)
        if y.dtype != t.dtype:
            if t.dtype != torch.float32:
                raise TypeError('loss: prediction is %s but target is %s' % (y.dtype, t.dtype))
            tag |= nat.MSE_TARGET_F32
        for f in (dl.w, dl.c):
            if f is not None and f.device != y.device:
                raise ValueError('loss: the loss fields live on %s, the prediction on %s' % (f.device, y.device))
        per = y[0].numel() if y.dim() > 0 else 1
        for f, div, period in ((dl.w, dl.wdiv, dl.wper), (dl.c, dl.cdiv, dl.cper)):
            if f is not None and div * period != per:
                raise ValueError('loss: field of %d x %d elements for samples of %d' % (period, div, per))
        y, t = _c(y), _c(t)
        key = str(y.device)
        scratch = _loss_scratch.get(key)
        if scratch is None:
            scratch = torch.empty(lib().dlwpcs_loss_scratch_bytes(), dtype=torch.uint8, device=y.device)
            _loss_scratch[key] = scratch
        out = torch.empty(2, dtype=torch.float32, device=y.device)
        dy = torch.empty_like(y) if ctx.needs_input_grad[0] else None
        L = dl.desc(weight, 1)
        if dl.masked is not None:
            check(lib().dlwpcs_loss_masked_fwd_bwd(ctypes.byref(L), ptr(y), ptr(t), _NORMS[dl.masked], ptr(dy), ptr(out), None,
                                                   y.numel(), tag, ptr(scratch), stream_ptr()), 'dlwpcs_loss_masked_fwd_bwd')
        else:
            check(lib().dlwpcs_loss_fwd_bwd(ctypes.byref(L), ptr(y), ptr(t), ptr(dy), ptr(out), y.numel(), tag, ptr(scratch),
                                            stream_ptr()), 'dlwpcs_loss_fwd_bwd')
        ctx.save_for_backward(dy)
        return out

    @staticmethod
    def backward(ctx, dout):
        (dy,) = ctx.saved_tensors
        seed = _unit_seeds.get(str(dout.device))          # (as _MSE.backward)
        if seed is not None and dout.data_ptr() == seed.data_ptr():
            return dy, None, None, None
        return (dy.float() * dout[0]).to(dy.dtype), None, None, None


def loss_stats(y, t, spec, weight=1.0):
    """ops.mse_mae for the loss `spec` (a DeviceLoss): the (2,) stats [weight * loss, mae], gradient through entry 0."""
    return _Loss.apply(y, t, spec, float(weight))


_head_scratch = {}


def head_mse_applicable(x, w_eq, ksize, act, target, loss=None):
    """True when the fused training tail (dlwpcs_head_mse_step) serves this output layer + loss: bf16 activations, pointwise
    kernel on 32 input channels, even C_out in 8..32, no activation, fp32 target, weights packed by the model's pack launch.
    loss: a DeviceLoss (None: 'mse') -- 'mse' / 'mae', unweighted or with a per-cell weight (dlwpcs_head_loss_step)."""
    if loss is not None and not (x.dim() == 5 and loss.fused_ok(w_eq.shape[3], 6 * x.shape[2] * x.shape[3])):
        return False
    if not (DIRECT_PARAM_GRADS and x.is_cuda and x.dtype == torch.bfloat16 and ksize == 1 and act == nat.ACT_NONE):
        return False
    packed = PREPACKED.get(id(w_eq))
    cout = w_eq.shape[3]
    return (packed is not None and packed[0] == nat.BF16 and x.dim() == 5 and x.shape[1] == 6 and x.shape[4] == 32
            and w_eq.shape[2] == 32 and cout % 2 == 0 and 8 <= cout <= 32 and (x.shape[2] * x.shape[3]) % 16 == 0
            and target.dtype == torch.float32 and tuple(target.shape) == tuple(x.shape[:4]) + (cout,)
            and x.numel() < (1 << 31) and x.requires_grad)


class _HeadMSE(torch.autograd.Function):
    """stats = [weight * mse, mae] of the pointwise output layer applied to x, against `target`; the forward launch also
    leaves dy and dx behind (dlwpcs_head_mse_step), the backward only runs the layer's weight gradient."""

    @staticmethod
    def forward(ctx, x, target, w_eq, w_pol, b_eq, b_pol, weight, flip, premask=None, loss=None):
        x, target = _c(x), _c(target)
        B, _, N, _, C0 = x.shape
        Cout = w_eq.shape[3]
        d = _make_desc(B, N, C0, 0, Cout, 1, False, False, flip, nat.ACT_NONE, 0.0, 0.0, nat.BF16)
        packed = PREPACKED[id(w_eq)]
        d.flags |= nat.CONV_PREPACKED
        key = str(x.device)
        scratch = _head_scratch.get(key)
        if scratch is None:
            scratch = torch.empty(lib().dlwpcs_head_mse_scratch_bytes(), dtype=torch.uint8, device=x.device)
            _head_scratch[key] = scratch
        out = torch.empty(2, dtype=torch.float32, device=x.device)
        dy = torch.empty((B, 6, N, N, Cout), dtype=x.dtype, device=x.device)
        dx = torch.empty_like(x)
        defer = DEFER_LOSS_TAIL and not _pending_tail          # (one scratch buffer per device: one deferred tail at a time)
        ow = 1 | (nat.HEAD_DEFER_STAGE2 if defer else 0)
        if loss is not None:
            L = loss.desc(weight, ow)
            check(lib().dlwpcs_head_loss_step(ctypes.byref(d), ctypes.byref(L), ptr(x), ptr(packed[1]),
                                              ptr(packed[2]) if b_eq is not None else 0, ptr(packed[3]), ptr(target), ptr(dy),
                                              ptr(dx), ptr(out), ptr(scratch), int(premask is not None),
                                              float(premask[0]) if premask is not None else 0.0,
                                              float(premask[1]) if premask is not None else 0.0, stream_ptr()),
                  'dlwpcs_head_loss_step')
        elif premask is not None:
            check(lib().dlwpcs_head_mse_step_masked(ctypes.byref(d), ptr(x), ptr(packed[1]),
                                                    ptr(packed[2]) if b_eq is not None else 0, ptr(packed[3]), ptr(target),
                                                    float(weight), ptr(dy), ptr(dx), ptr(out), ow, ptr(scratch),
                                                    float(premask[0]), float(premask[1]), stream_ptr()),
                  'dlwpcs_head_mse_step_masked')
        else:
            check(lib().dlwpcs_head_mse_step(ctypes.byref(d), ptr(x), ptr(packed[1]), ptr(packed[2]) if b_eq is not None else 0,
                                             ptr(packed[3]), ptr(target), float(weight), ptr(dy), ptr(dx), ptr(out), ow,
                                             ptr(scratch), stream_ptr()), 'dlwpcs_head_mse_step')
        if defer:
            tail = nat.LossTail()
            check(lib().dlwpcs_head_mse_tail(ctypes.byref(d), float(weight), 1, ptr(scratch), ptr(out), ctypes.byref(tail)),
                  'dlwpcs_head_mse_tail')
            _pending_tail.append((tail, (scratch, out)))
        ctx.desc = d
        ctx.params = (w_eq, w_pol, None, b_eq, b_pol, None)
        ctx.save_for_backward(x, dy, dx)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, dy, dx = ctx.saved_tensors
        seed = _unit_seeds.get(str(dout.device))
        if seed is None or dout.data_ptr() != seed.data_ptr():
            raise RuntimeError('the fused head + loss step is seeded by DLWP.keras.Model only (upstream gradient 1)')
        d = ctx.desc
        dev = dy.device
        nbytes = lib().dlwpcs_conv_workspace_bytes(ctypes.byref(d))
        need = ctx.needs_input_grad
        direct = DIRECT_PARAM_GRADS and all(p is None or (p.is_leaf and p.grad is not None and p.grad.is_contiguous())
                                            for p in ctx.params)
        if not direct:
            raise RuntimeError('the fused head + loss step accumulates straight into the model\'s flat gradient buffer')
        batching = WGRAD_BATCH and not WGRAD_SIDE_STREAM and wgrad_batch_supported(d)
        defer = DEFER_WGRAD_REDUCE and not WGRAD_SIDE_STREAM and not batching
        ws = _workspace(nbytes, dev, 'defer%d' % len(_deferred)) if defer else _workspace(nbytes, dev)
        _weight_gradients(d, x, None, dy, None, ctx.params, None, ws, nbytes, True, defer, need[2:6],
                          False, ctx.params[3] is not None, False)
        return (dx if need[0] else None), None, None, None, None, None, None, None, None, None


def head_mse(x, target, w_eq, w_pol, b_eq, b_pol, weight=1.0, flip_north_pole=True, premask=None, loss=None):
    """loss: a DeviceLoss the fused head serves (head_mse_applicable), None: 'mse'."""
    return _HeadMSE.apply(x, target, w_eq, w_pol, b_eq, b_pol, float(weight), bool(flip_north_pole), premask, loss)


def adam_step(p, g, m, v, step_dev, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, zero_grads=False):
    """In-place TF2.1-keras Adam on flat fp32 device buffers.  `step_dev`: int32 device tensor; with two elements
    {t-1, ticket = 0} the update and the step increment are ONE launch (dlwpcs_adam_step_fused; zero_grads clears g
    once it has been consumed), with one element the two-launch dlwpcs_adam_step."""
    for t in (p, g, m, v):
        require_device(t, 'adam_step')
        _f32_param(t, 'adam_step')
    if step_dev.numel() >= 2:
        check(lib().dlwpcs_adam_step_fused(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(step_dev), lr, beta1, beta2,
                                           eps, grad_scale, nat.ADAM_ZERO_GRAD if zero_grads else 0, stream_ptr()),
              'dlwpcs_adam_step_fused')
        return
    check(lib().dlwpcs_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(step_dev), lr, beta1, beta2, eps,
                                 grad_scale, stream_ptr()), 'dlwpcs_adam_step')
    if zero_grads:
        g.zero_()


def adam_step_dev(p, g, m, v, state_dev, hyper_dev, zero_grads=False):
    """dlwpcs_adam_step_dev: the fused Adam launch with {lr, beta1, beta2, eps, grad_scale} read from the 5-float device
    tensor `hyper_dev` -- the form a captured hipGraph needs to honour learning-rate changes between replays."""
    for t in (p, g, m, v, hyper_dev):
        require_device(t, 'adam_step_dev')
        _f32_param(t, 'adam_step_dev')
    if hyper_dev.numel() < 5 or state_dev.numel() < 2:
        raise ValueError('adam_step_dev: hyper_dev needs 5 floats, state_dev 2 int32')
    check(lib().dlwpcs_adam_step_dev(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(state_dev), ptr(hyper_dev),
                                     nat.ADAM_ZERO_GRAD if zero_grads else 0, stream_ptr()), 'dlwpcs_adam_step_dev')


def add(a, b):
    require_device(a, 'add')
    require_device(b, 'add')
    a, b = _c(a), _c(b)
    y = torch.empty_like(a)
    check(lib().dlwpcs_add(ptr(a), ptr(b), ptr(y), a.numel(), nat.dtype_tag(a), stream_ptr()), 'dlwpcs_add')
    return y


# ------------------------------------------------------------------------------------------------------------------ #
# Batch feed (reference DLWP/model/generators.py:872-984): gather a batch window out of the HBM-resident data array
# ------------------------------------------------------------------------------------------------------------------ #

def batch_gather(array, samples, var_idx, out, n_steps, t_off, t_stride, c_off, c_stride, channels_last=True):
    """
    array (T, V, *space) fp32 device tensor; samples (B,) / var_idx (nv,) int32 device tensors; out (B, *space, Ctot) or
    (B, Ctot, *space), float32 or bfloat16, written in place: channel c_off + n*c_stride + j <- array[samples + t_off +
    n*t_stride, var_idx[j]].  `array` may also be a packed device source -- an object with `q` (T, V, *space) int16, `scale`
    and `offset` (V,) float32 device tensors, such as a device-resident DLWP.model.PackedSeries: the same gather out of the
    codes, decoded on the way (dlwpcs_batch_gather_i16).
    """
    if not isinstance(array, torch.Tensor) and hasattr(array, 'q'):
        return _batch_gather_i16(array, samples, var_idx, out, n_steps, t_off, t_stride, c_off, c_stride, channels_last)
    for t in (array, out):
        require_device(t, 'batch_gather')
    if array.dtype != torch.float32 or not array.is_contiguous() or not out.is_contiguous():
        raise TypeError('batch_gather: array must be contiguous float32, out contiguous')
    T, V = int(array.shape[0]), int(array.shape[1])
    S = int(array[0, 0].numel())
    B = int(samples.numel())
    Ctot = int(out.shape[-1] if channels_last else out.shape[1])
    if out.numel() != B * S * Ctot:
        raise ValueError('batch_gather: out shape %s does not match batch %d, space %d' % (tuple(out.shape), B, S))
    check(lib().dlwpcs_batch_gather(ptr(array), T, V, S, ptr(samples), B, ptr(var_idx), int(var_idx.numel()),
                                    int(n_steps), int(t_off), int(t_stride), ptr(out), Ctot, int(c_off), int(c_stride),
                                    1 if channels_last else 0, nat.dtype_tag(out), stream_ptr()), 'dlwpcs_batch_gather')
    return out


# ------------------------------------------------------------------------------------------------------------------ #
# The resident series as int16 codes (DLWP/model/packing.py): x = q * scale[v] + offset[v], -32768 = NaN; include/dlwpcs.h
# ------------------------------------------------------------------------------------------------------------------ #

def _packed_tables(scale, offset, V, dev, what):
    for t, name in ((scale, 'scale'), (offset, 'offset')):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or \
                t.numel() != V:
            raise TypeError('%s: %s must be a contiguous float32 tensor of %d entries on %s' % (what, name, V, dev))


def _tvs(x, what):
    if x.dim() < 2:
        raise ValueError('%s: expected (time, variable, *space), got shape %s' % (what, tuple(x.shape)))
    T, V = int(x.shape[0]), int(x.shape[1])
    return T, V, (x.numel() // (T * V) if T * V else 0)


def _batch_gather_i16(src, samples, var_idx, out, n_steps, t_off, t_stride, c_off, c_stride, channels_last):
    q = src.q
    require_device(out, 'batch_gather')
    if not isinstance(q, torch.Tensor) or q.dtype != torch.int16 or q.device != out.device:
        raise nat.NativeError('batch_gather: a packed source holds its int16 codes on the device of `out` (no CPU fallback)')
    if not q.is_contiguous() or not out.is_contiguous():
        raise TypeError('batch_gather: codes and out must be contiguous')
    T, V, S = _tvs(q, 'batch_gather')
    _packed_tables(src.scale, src.offset, V, q.device, 'batch_gather')
    B = int(samples.numel())
    Ctot = int(out.shape[-1] if channels_last else out.shape[1])
    if out.numel() != B * S * Ctot:
        raise ValueError('batch_gather: out shape %s does not match batch %d, space %d' % (tuple(out.shape), B, S))
    check(lib().dlwpcs_batch_gather_i16(ptr(q), T, V, S, ptr(src.scale), ptr(src.offset), ptr(samples), B, ptr(var_idx),
                                        int(var_idx.numel()), int(n_steps), int(t_off), int(t_stride), ptr(out), Ctot, int(c_off),
                                        int(c_stride), 1 if channels_last else 0, nat.dtype_tag(out), stream_ptr()),
          'dlwpcs_batch_gather_i16')
    return out


def channel_range(x):
    """
    (range, nonfinite) of the contiguous fp32 device tensor x (T, V, *space): range (V, 2) float32 = {min, max} over the finite
    elements of every variable ({+inf, -inf} when there are none), nonfinite (V,) int64 = the count of NaN / inf elements.
    Device tensors; two launches on the current stream, no host synchronisation.
    """
    require_device(x, 'channel_range')
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError('channel_range: x must be contiguous float32')
    T, V, S = _tvs(x, 'channel_range')
    dev = x.device
    with torch.cuda.device(dev):
        rng = torch.empty((V, 2), dtype=torch.float32, device=dev)
        bad = torch.empty((V,), dtype=torch.int64, device=dev)
        nbytes = int(lib().dlwpcs_channel_range_scratch_bytes(T, V, S))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        check(lib().dlwpcs_channel_range(ptr(x), T, V, S, ptr(rng), ptr(bad), ptr(scratch), nbytes, stream_ptr()),
              'dlwpcs_channel_range')
    return rng, bad


def pack_i16(x, scale, offset, out=None):
    """
    int16 codes of the contiguous fp32 device tensor x (T, V, *space): clamp(rint((x - offset[v]) / scale[v]), -32767, 32767),
    -32768 for NaN / inf.  scale, offset: (V,) float32 device tensors.  One launch.
    """
    require_device(x, 'pack_i16')
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError('pack_i16: x must be contiguous float32')
    T, V, S = _tvs(x, 'pack_i16')
    _packed_tables(scale, offset, V, x.device, 'pack_i16')
    if out is None:
        out = torch.empty(x.shape, dtype=torch.int16, device=x.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.int16 or out.device != x.device or out.shape != x.shape or \
            not out.is_contiguous():
        raise ValueError('pack_i16: out must be a contiguous int16 tensor of shape %s on %s' % (tuple(x.shape), x.device))
    with torch.cuda.device(x.device):
        check(lib().dlwpcs_pack_i16(ptr(x), T, V, S, ptr(scale), ptr(offset), ptr(out), stream_ptr()), 'dlwpcs_pack_i16')
    return out


def unpack_i16(q, scale, offset, out=None):
    """
    fp32 values of the contiguous int16 device tensor q (T, V, *space): float(q) * scale[v] + offset[v] as two rounded fp32
    operations, NaN for -32768.  scale, offset: (V,) float32 device tensors.  One launch.
    """
    if not isinstance(q, torch.Tensor) or not q.is_cuda:
        raise nat.NativeError('unpack_i16: the codes must be a tensor on a HIP device (no CPU fallback)')
    if q.dtype != torch.int16 or not q.is_contiguous():
        raise TypeError('unpack_i16: q must be contiguous int16')
    T, V, S = _tvs(q, 'unpack_i16')
    _packed_tables(scale, offset, V, q.device, 'unpack_i16')
    if out is None:
        out = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != q.device or out.shape != q.shape or \
            not out.is_contiguous():
        raise ValueError('unpack_i16: out must be a contiguous float32 tensor of shape %s on %s' % (tuple(q.shape), q.device))
    with torch.cuda.device(q.device):
        check(lib().dlwpcs_unpack_i16(ptr(q), T, V, S, ptr(scale), ptr(offset), ptr(out), stream_ptr()), 'dlwpcs_unpack_i16')
    return out


def missing_counts_host(array):
    """
    numpy twin of `missing_counts`: (T, V) int32, the number of NaN elements of every (time, variable) plane of a float array
    (T, V, *space) -- any payload, either sign; +-inf is data -- or of -32768 codes of an int16 array.
    """
    a = np.asarray(array)
    if a.ndim < 2:
        raise ValueError('missing_counts: expected (time, variable, *space), got shape %s' % (tuple(a.shape),))
    if a.dtype == np.int16:
        bad = a == -32768
    elif np.issubdtype(a.dtype, np.floating):
        bad = np.isnan(a)
    else:
        raise TypeError('missing_counts: float data or int16 codes, got %s' % a.dtype)
    return bad.reshape(a.shape[0], a.shape[1], -1).sum(axis=2, dtype=np.int64).astype(np.int32)


def missing_counts(array):
    """
    (T, V) int32 device tensor: the number of missing elements of every (time, variable) plane of `array`, a contiguous fp32
    device tensor (T, V, *space) (missing = NaN) or a packed device source with int16 codes `.q` (missing = the code -32768).
    One dlwpcs_missing_count launch on the current stream, no host synchronisation; numpy twin: `missing_counts_host`.
    """
    q = getattr(array, 'q', array)
    if not isinstance(q, torch.Tensor) or not q.is_cuda:
        raise nat.NativeError('missing_counts: the data must be a tensor on a HIP device (no CPU fallback; missing_counts_host is '
                              'the numpy twin)')
    if q.dtype not in (torch.float32, torch.int16) or not q.is_contiguous():
        raise TypeError('missing_counts: contiguous float32 data or int16 codes, got %s' % q.dtype)
    T, V, S = _tvs(q, 'missing_counts')
    count = torch.empty((T, V), dtype=torch.int32, device=q.device)
    with torch.cuda.device(q.device):
        check(lib().dlwpcs_missing_count(ptr(q), nat.I16 if q.dtype == torch.int16 else nat.F32, T * V, S, ptr(count), stream_ptr()),
              'dlwpcs_missing_count')
    return count


def fill_missing(x, fill, channels_last=True):
    """
    Replace the NaNs of the batch x in place (dlwpcs_fill_missing; one launch on the current stream, no host synchronisation) and
    return x: a contiguous float32 or bfloat16 device tensor (n, ..., C) (channels_last) or (n, C, ...).  fill: one value, or one
    per channel -- a sequence, or a float32 device tensor of C values (made once by a caller that fills every batch); a bfloat16
    element receives the value rounded to nearest even.  Every element that is not NaN keeps its bits.
    """
    require_device(x, 'fill_missing')
    if x.dtype not in (torch.float32, torch.bfloat16) or not x.is_contiguous() or x.dim() < 2:
        raise TypeError('fill_missing: a contiguous float32 / bfloat16 batch (n, ..., C) or (n, C, ...), got %s %s'
                        % (x.dtype, tuple(x.shape)))
    C = int(x.shape[-1] if channels_last else x.shape[1])
    if isinstance(fill, torch.Tensor):
        if fill.dtype != torch.float32 or fill.device != x.device or not fill.is_contiguous():
            raise TypeError('fill_missing: the fill table must be a contiguous float32 tensor on %s' % (x.device,))
        f = fill.reshape(-1)
    else:
        f = torch.as_tensor(np.asarray(fill, dtype=np.float32).reshape(-1), device=x.device)
    if f.numel() == 1:
        div, period = 1, 1
    elif f.numel() == C:
        # channels_last: the channel is the fastest index; channels_first: one channel spans the sample's space
        div, period = (1, C) if channels_last else (int(x[0, 0].numel()), C)
    else:
        raise ValueError('fill_missing: %d fill values for %d channels' % (f.numel(), C))
    if x.numel():
        with torch.cuda.device(x.device):
            check(lib().dlwpcs_fill_missing(ptr(x), nat.dtype_tag(x), x.numel(), ptr(f), div, period, stream_ptr()),
                  'dlwpcs_fill_missing')
    return x


def solar_fill(row_tab, cell_tab, samples, out, n_steps, t_off, t_stride, c_off, c_stride, channels_last=True):
    """
    The computing twin of `batch_gather(insolation[:, None], samples, [0], out, ...)`: channel c_off + n*c_stride of `out`
    <- the insolation of row samples + t_off + n*t_stride, computed from the tables of a DLWP.util.SolarForcing (row_tab (T, 4),
    cell_tab (S, 3), float64 device tensors) instead of read from a dense array.  out (B, *space, Ctot) or (B, Ctot, *space),
    float32 or bfloat16, written in place.  The rows are trusted: the caller checks 0 <= row < T.
    """
    require_device(out, 'solar_fill')
    for t in (row_tab, cell_tab, samples):
        if not isinstance(t, torch.Tensor) or t.device != out.device:
            raise nat.NativeError('solar_fill: tables and samples must be tensors on the device of `out` (no CPU fallback)')
    if row_tab.dtype != torch.float64 or cell_tab.dtype != torch.float64 or not row_tab.is_contiguous() or \
            not cell_tab.is_contiguous() or not out.is_contiguous():
        raise TypeError('solar_fill: tables must be contiguous float64, out contiguous')
    if row_tab.dim() != 2 or row_tab.shape[1] != 4 or cell_tab.dim() != 2 or cell_tab.shape[1] != 3:
        raise ValueError('solar_fill: row table (T, 4) and cell table (S, 3), got %s and %s'
                         % (tuple(row_tab.shape), tuple(cell_tab.shape)))
    if samples.dtype != torch.int32 or not samples.is_contiguous():
        raise TypeError('solar_fill: samples must be a contiguous int32 device tensor')
    T, S = int(row_tab.shape[0]), int(cell_tab.shape[0])
    B = int(samples.numel())
    Ctot = int(out.shape[-1] if channels_last else out.shape[1])
    if out.numel() != B * S * Ctot:
        raise ValueError('solar_fill: out shape %s does not match batch %d, space %d' % (tuple(out.shape), B, S))
    check(lib().dlwpcs_solar_fill(ptr(row_tab), T, ptr(cell_tab), S, ptr(samples), B, int(n_steps), int(t_off), int(t_stride),
                                  ptr(out), Ctot, int(c_off), int(c_stride), 1 if channels_last else 0, nat.dtype_tag(out),
                                  stream_ptr()), 'dlwpcs_solar_fill')
    return out


# ------------------------------------------------------------------------------------------------------------------ #
# Forecast verification (DLWP/verify.py): one strided reduction, include/dlwpcs.h dlwpcs_score
# ------------------------------------------------------------------------------------------------------------------ #

SCORE_METHODS = {'mse': nat.SCORE_MSE, 'rmse': nat.SCORE_RMSE, 'mae': nat.SCORE_MAE, 'acc': nat.SCORE_ACC,
                 'cos': nat.SCORE_COS, 'mean': nat.SCORE_MEAN}


def score_reduce(method, operands, shape, reduced, lagged=None, out_f32=False, indexed=None):
    """
    Reduce fp32 device operands [a (forecast), b (verification), c (climatology), w (weights)] -- each None or
    (tensor, strides in elements over the logical `shape`, 0 = broadcast) -- over the logical dims in `reduced`.
    lagged=None: every dim is ordinary.  lagged=(t_cap, t_slope): dim 0 is the lead f (kept) and dim 1 the time axis
    (reduced), of which only the first n_f = min(shape[1], t_cap - t_slope * f) entries take part.
    indexed=(rows, table_row_stride), lagged form only: the climatology operand -- c of 'acc' / 'cos', a of 'mse' / 'rmse' /
    'mae' -- is a table; `rows` is an int32 device tensor of shape[0] * shape[1] entries, the table row of every (lead, time), and
    the operand's strides over dims 0 and 1 are 0 (dlwpcs_score_indexed: bitwise the result of the materialised operand).
    Returns a device tensor (float64, or float32 with out_f32) shaped like the kept dims, enqueued on the current stream
    with no host synchronisation.
    """
    m = SCORE_METHODS[method]
    if indexed is not None:
        if lagged is None or method == 'mean':
            raise ValueError('score: the indexed form is the lagged form of a two-operand score')
        rows, table_stride = indexed
        if rows.dtype != torch.int32 or not rows.is_cuda or not rows.is_contiguous() or \
                rows.numel() != int(shape[0]) * int(shape[1]):
            raise ValueError('score: the row table is a contiguous int32 device tensor of leads x times entries')
    shape = tuple(int(s) for s in shape)
    reduced = set(int(r) for r in reduced)
    strides, ptrs, dev = [], [], None
    for op in operands:
        if op is None:
            strides.append((0,) * len(shape))
            ptrs.append(0)
            continue
        t, st = op
        require_device(t, 'score')
        if t.dtype != torch.float32:
            raise TypeError('score: operands must be float32, got %s' % t.dtype)
        dev = t.device if dev is None else dev
        if t.device != dev:
            raise ValueError('score: operands on %s and %s' % (dev, t.device))
        strides.append(tuple(int(s) for s in st))
        ptrs.append(t.data_ptr())
    if ptrs[1] == 0:
        raise ValueError('score: the verification operand is required')
    d = nat.ScoreDesc()
    d.method = m
    if lagged is None:
        first = 0
        d.n_lead, d.t_len, d.t_cap, d.t_slope = 1, 1, 1, 0
        out_shape = []
    else:
        if 1 not in reduced or 0 in reduced:
            raise ValueError('score: the lagged form keeps the lead and reduces the time axis')
        first = 2
        d.n_lead, d.t_len, d.t_cap, d.t_slope = shape[0], shape[1], int(lagged[0]), int(lagged[1])
        for k in range(4):
            d.lead_stride[k], d.t_stride[k] = strides[k][0], strides[k][1]
        out_shape = [shape[0]]
    rest = range(first, len(shape))
    kept = [i for i in rest if i not in reduced]
    out_shape += [shape[i] for i in kept]
    if any(shape[i] == 0 for i in kept) or d.n_lead == 0:
        return torch.empty(out_shape, dtype=torch.float32 if out_f32 else torch.float64, device=dev)
    kept = [i for i in kept if shape[i] != 1]
    red = [i for i in rest if i in reduced and shape[i] != 1]
    kc = 1
    if kept and red and shape[kept[-1]] in (2, 4) and kept[-1] > red[-1] and \
            (strides[0][kept[-1]] == 1 or strides[1][kept[-1]] == 1):
        kc = shape[kept[-1]]
        for k in range(4):
            d.kc_stride[k] = strides[k][kept[-1]]
        kept = kept[:-1]
    d.kc = kc
    keep_c, red_c = ([(e, s) for e, s, _ in merge_dims((shape[i], [st[i] for st in strides], None) for i in dims)]
                     for dims in (kept, red))
    if len(keep_c) > nat.SCORE_MAX_DIMS or len(red_c) > nat.SCORE_MAX_DIMS:
        raise NotImplementedError('score: more than %d kept or reduced dims after merging' % nat.SCORE_MAX_DIMS)
    d.n_keep, d.n_red = len(keep_c), len(red_c)
    for i, (e, s) in enumerate(keep_c):
        d.keep_ext[i] = e
        for k in range(4):
            d.keep_stride[k][i] = s[k]
    for i, (e, s) in enumerate(red_c):
        d.red_ext[i] = e
        for k in range(4):
            d.red_stride[k][i] = s[k]
    out = torch.empty(out_shape, dtype=torch.float32 if out_f32 else torch.float64, device=dev)
    nbytes = int(lib().dlwpcs_score_scratch_bytes(ctypes.byref(d)))
    scratch = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        if indexed is not None:
            check(lib().dlwpcs_score_indexed(ctypes.byref(d), ptrs[0] or None, ptrs[1], ptrs[2] or None, ptrs[3] or None,
                                             rows.data_ptr(), int(table_stride), out.data_ptr(), 1 if out_f32 else 0,
                                             ptr(scratch), nbytes, stream_ptr()), 'dlwpcs_score_indexed')
        else:
            check(lib().dlwpcs_score(ctypes.byref(d), ptrs[0] or None, ptrs[1], ptrs[2] or None, ptrs[3] or None,
                                     out.data_ptr(), 1 if out_f32 else 0, ptr(scratch), nbytes, stream_ptr()), 'dlwpcs_score')
    return out


# ------------------------------------------------------------------------------------------------------------------ #
# Zonal spectra (DLWP/verify.py zonal_spectrum / zonal_cross_spectrum / zonal_coherence), include/dlwpcs.h dlwpcs_zonal_spectrum
# ------------------------------------------------------------------------------------------------------------------ #

SPECTRUM_MAX_L = 1728
_twiddles = {}              # (L, device) -> (L, 2) float32 device tensor {cos, -sin}(2 pi m / L)


def spectrum_twiddle_host(L):
    """(L, 2) float32: cos and -sin of 2 pi m / L for m < L, evaluated in float64 and rounded once"""
    ang = 2.0 * np.pi * np.arange(int(L), dtype=np.float64) / float(L)
    return np.stack([np.cos(ang), -np.sin(ang)], axis=1).astype(np.float32)


def spectrum_twiddle(L, device):
    """the twiddle table of dlwpcs_zonal_spectrum for rows of L longitudes on `device`, made once and kept"""
    key = (int(L), str(torch.device(device)))
    hit = _twiddles.get(key)
    if hit is None:
        if torch.cuda.is_current_stream_capturing():
            raise nat.NativeError('zonal_spectrum: first use of L = %d inside a graph capture (run it once eagerly first)' % L)
        hit = torch.from_numpy(spectrum_twiddle_host(L)).to(device)
        _twiddles[key] = hit
    return hit


def spectrum_dims(shape, strides, reduced):
    """
    The leading dims of dlwpcs_zonal_spectrum_desc: [(extent, (stride per operand), kept)] for the logical leading `shape`,
    per-operand `strides` in elements (0 = broadcast) and the set `reduced` of averaged axes.  Unit axes are dropped; neighbours
    with the same flag are merged where every operand allows it (outer stride == inner stride * inner extent).  Pure Python.
    """
    shape = tuple(int(e) for e in shape)
    reduced = set(int(r) % len(shape) for r in reduced) if shape else set()
    return merge_dims((e, [s[i] for s in strides], i not in reduced) for i, e in enumerate(shape))


def spectrum_desc(L, dims, n_wave=None, remove_mean=False):
    """nat.ZonalSpectrumDesc of rows of L longitudes with the leading `dims` of spectrum_dims"""
    if len(dims) > nat.SCORE_MAX_DIMS:
        raise NotImplementedError('zonal_spectrum: more than %d leading dims after merging' % nat.SCORE_MAX_DIMS)
    d = nat.ZonalSpectrumDesc()
    d.L, d.n_wave, d.n_dims, d.remove_mean = int(L), int(n_wave or 0), len(dims), 1 if remove_mean else 0
    for i, (e, st, kept) in enumerate(dims):
        d.ext[i], d.kept[i] = e, 1 if kept else 0
        for k in range(3):
            d.stride[k][i] = st[k]
    return d


def spectrum_launch(d, a, b, w, out, skipped=None):
    """dlwpcs_zonal_spectrum on the current stream: device tensors a, b (None: single form), w (None: unit weights) addressed
    by the descriptor, into the float32 tensor `out` and the int32 tensor `skipped` (None: not wanted)"""
    dev = a.device
    tw = spectrum_twiddle(d.L, dev)
    nbytes = int(lib().dlwpcs_zonal_spectrum_scratch_bytes(ctypes.byref(d)))
    scratch = _workspace(nbytes, dev, 'spectrum') if nbytes else None
    with torch.cuda.device(dev):
        check(lib().dlwpcs_zonal_spectrum(ctypes.byref(d), ptr(a), ptr(b) or None, ptr(w) or None, ptr(tw), ptr(scratch) or None,
                                          ptr(out), ptr(skipped) or None, stream_ptr()), 'dlwpcs_zonal_spectrum')
    return out


def _lon_last(t, lon_axis):
    """t with its longitude axis last and unit-stride: a view where that is possible, else one copy"""
    t = t.movedim(lon_axis, -1)
    if t.shape[-1] > 1 and t.stride(-1) != 1:
        t = t.contiguous()
    return t


def zonal_spectrum(a, b=None, lon_axis=-1, reduced=(), weights=None, n_wave=None, remove_mean=False, counts=False):
    """
    One-sided zonal power spectrum of the float32 device tensor `a` along `lon_axis`, P_k = c_k |X_k|^2 / L^2 (c_k = 1 for k = 0
    and the Nyquist wavenumber of an even L, else 2), as the weighted mean over the axes `reduced` (axes of `a`, the longitude
    axis not among them) of the rows whose values are all finite.  weights: a float32 device tensor that broadcasts against the
    leading shape (a's shape without the longitude axis) by numpy's trailing-axis rule.  n_wave: the first n_wave wavenumbers
    only (default: all L // 2 + 1).  remove_mean: subtract every row's mean first and report P_0 as that mean squared.
    Returns a float32 device tensor (kept axes..., K); with b (same shape as a), the pair form: (4, kept axes..., K) = P_aa, P_bb,
    co-spectrum and quadrature spectrum.  counts=True: also the int32 tensor (kept axes...) of rows that did not count.
    At most two launches on the current stream, no host synchronisation (the twiddle table of an L is uploaded at its first use).
    """
    require_device(a, 'zonal_spectrum')
    ops = [a] if b is None else [a, b]
    for t in ops:
        require_device(t, 'zonal_spectrum')
        if t.dtype != torch.float32:
            raise TypeError('zonal_spectrum: operands must be float32, got %s' % t.dtype)
        if t.device != a.device or t.shape != a.shape:
            raise ValueError('zonal_spectrum: the two operands must have one shape and one device')
    if a.dim() < 1:
        raise ValueError('zonal_spectrum: the input needs a longitude axis')
    ops = [_lon_last(t, lon_axis) for t in ops]
    L = int(ops[0].shape[-1])
    if L < 2:
        raise ValueError('zonal_spectrum: %d longitudes (at least 2)' % L)
    if L > SPECTRUM_MAX_L:
        raise NotImplementedError('zonal_spectrum: %d longitudes, the kernel serves 2 .. %d' % (L, SPECTRUM_MAX_L))
    K = L // 2 + 1
    if n_wave is not None:
        if not 1 <= int(n_wave) <= K:
            raise ValueError('zonal_spectrum: n_wave = %s outside 1 .. L // 2 + 1 = %d' % (n_wave, K))
        K = int(n_wave)
    lead = tuple(int(e) for e in ops[0].shape[:-1])
    nd = len(lead)
    lon = int(lon_axis) % a.dim()
    red = set()
    for r in reduced:
        r = int(r)
        if r < -a.dim() or r >= a.dim() or r % a.dim() == lon:
            raise ValueError('zonal_spectrum: reduced axis %d is out of range or the longitude axis' % r)
        r %= a.dim()
        red.add(r if r < lon else r - 1)                # its place among the leading axes
    strides = [tuple(int(s) for s in t.stride()[:-1]) for t in ops]
    if b is None:
        strides.append((0,) * nd)
    w = None
    if weights is not None:
        require_device(weights, 'zonal_spectrum')
        if weights.dtype != torch.float32 or weights.device != a.device:
            raise TypeError('zonal_spectrum: the weights must be a float32 tensor on the device of the data')
        w = weights
        if w.dim() > nd or any(int(e) not in (1, lead[nd - w.dim() + i]) for i, e in enumerate(w.shape)):
            raise ValueError('zonal_spectrum: weights %s do not broadcast against the leading shape %s' % (tuple(w.shape), lead))
        strides.append((0,) * (nd - w.dim()) + tuple(int(w.stride(i)) if int(w.shape[i]) != 1 else 0 for i in range(w.dim())))
    else:
        strides.append((0,) * nd)
    kept_shape = [lead[i] for i in range(nd) if i not in red]
    out = torch.empty(([] if b is None else [4]) + kept_shape + [K], dtype=torch.float32, device=a.device)
    cnt = torch.empty(kept_shape, dtype=torch.int32, device=a.device) if counts else None
    if out.numel():
        d = spectrum_desc(L, spectrum_dims(lead, strides, red), n_wave, remove_mean)
        spectrum_launch(d, ops[0], ops[1] if b is not None else None, w, out, cnt)
    return (out, cnt) if counts else out


# ------------------------------------------------------------------------------------------------------------------ #
# Spherical-harmonic spectra (DLWP/verify.py spherical_spectrum / spherical_cross_spectrum / spherical_correlation),
# include/dlwpcs.h dlwpcs_sht_spectrum; the tables come from DLWP/remap/spharm.py SphericalTransform
# ------------------------------------------------------------------------------------------------------------------ #

_sht_groups = {}            # (leading shape, reduced axes, device) -> (group_start, row_index) int32 device tensors


def sht_desc(nlat, L, T, dims, lat_strides):
    """nat.ShtSpectrumDesc of fields of nlat x L points analysed up to degree T: `dims` the leading dims of spectrum_dims (all
    kept: they index the fields), lat_strides the element stride of the latitude axis in a and in b"""
    if len(dims) > nat.SCORE_MAX_DIMS:
        raise NotImplementedError('spherical_spectrum: more than %d leading dims after merging' % nat.SCORE_MAX_DIMS)
    d = nat.ShtSpectrumDesc()
    d.nlat, d.L, d.T, d.n_dims = int(nlat), int(L), int(T), len(dims)
    d.lat_stride[0], d.lat_stride[1] = int(lat_strides[0]), int(lat_strides[1])
    for i, (e, st, _) in enumerate(dims):
        d.ext[i] = e
        for k in range(2):
            d.stride[k][i] = st[k]
    return d


def sht_launch(d, a, b, twiddle, table, out, skipped=None):
    """dlwpcs_sht_spectrum on the current stream: device tensors a, b (None: single form) addressed by the descriptor, into the
    float32 tensor `out` ((3,) fields, T + 1) and the int32 tensor `skipped` (fields; None: not wanted)"""
    dev = a.device
    nbytes = int(lib().dlwpcs_sht_spectrum_scratch_bytes(ctypes.byref(d)))
    scratch = _workspace(nbytes, dev, 'sht') if nbytes else None
    with torch.cuda.device(dev):
        check(lib().dlwpcs_sht_spectrum(ctypes.byref(d), ptr(a), ptr(b) or None, ptr(twiddle), ptr(table), ptr(scratch) or None,
                                        ptr(out), ptr(skipped) or None, stream_ptr()), 'dlwpcs_sht_spectrum')
    return out


def sht_groups_host(lead, red):
    """(group_start, row_index) of dlwpcs_group_mean for fields numbered row-major over the leading shape `lead`: a group per
    index of the kept axes (row-major), its members the fields over the averaged axes `red` in row-major order.  numpy only."""
    lead = tuple(int(e) for e in lead)
    kept = [i for i in range(len(lead)) if i not in red]
    idx = np.arange(int(np.prod(lead, dtype=np.int64)), dtype=np.int64).reshape(lead)
    n_groups = int(np.prod([lead[i] for i in kept], dtype=np.int64))
    idx = idx.transpose(kept + sorted(red)).reshape(n_groups, -1)
    return np.arange(n_groups + 1, dtype=np.int64) * idx.shape[1], idx.reshape(-1)


def _sht_group_tables(lead, red, dev):
    key = (tuple(lead), tuple(sorted(red)), str(dev))
    hit = _sht_groups.get(key)
    if hit is None:
        if torch.cuda.is_current_stream_capturing():
            raise nat.NativeError('spherical_spectrum: first use of this averaging inside a graph capture (run it once eagerly first)')
        gs, ri = sht_groups_host(lead, red)
        if ri.size >= 1 << 31:
            raise NotImplementedError('spherical_spectrum: too many fields')
        hit = (torch.from_numpy(gs.astype(np.int32)).to(dev), torch.from_numpy(ri.astype(np.int32)).to(dev))
        _sht_groups[key] = hit
    return hit


def spherical_spectrum(a, b=None, transform=None, lat_axis=-2, lon_axis=-1, reduced=(), counts=False):
    """
    Spherical-harmonic power spectrum S_n = sum_{m<=n} c_m |a_n^m|^2 (n = 0 .. T) of the float32 device tensor `a`, whose
    `lat_axis` and `lon_axis` hold the grid of `transform` (a DLWP.remap.spharm.SphericalTransform: it states the definitions,
    fixes T and holds the tables), as the mean over the axes `reduced` (axes of `a`, neither of the two grid axes) of the fields
    whose values are all finite.  The area weighting is part of the transform.
    Returns a float32 device tensor (kept axes..., T + 1); with b (same shape as a), the pair form: (3, kept axes..., T + 1) = S_aa,
    S_bb and the co-spectrum sum_m c_m Re(a_n^m conj b_n^m); a field counts only when it is finite in both.  A result without a
    counted field is NaN.  counts=True: also the int32 tensor (kept axes...) of fields that did not count.
    Two launches of dlwpcs_sht_spectrum and, when something is averaged, dlwpcs_group_mean (fp64, fixed order) on the current
    stream, no host synchronisation (the tables of a transform and of an averaging are uploaded at their first use).
    """
    if transform is None:
        raise TypeError('spherical_spectrum: a SphericalTransform is required')
    require_device(a, 'spherical_spectrum')
    ops = [a] if b is None else [a, b]
    for t in ops:
        require_device(t, 'spherical_spectrum')
        if t.dtype != torch.float32:
            raise TypeError('spherical_spectrum: operands must be float32, got %s' % t.dtype)
        if t.device != a.device or t.shape != a.shape:
            raise ValueError('spherical_spectrum: the two operands must have one shape and one device')
    nd = a.dim()
    if nd < 2:
        raise ValueError('spherical_spectrum: the input needs a latitude and a longitude axis')
    lat, lon = int(lat_axis), int(lon_axis)
    if not (-nd <= lat < nd and -nd <= lon < nd) or lat % nd == lon % nd:
        raise ValueError('spherical_spectrum: lat_axis %d and lon_axis %d must be two axes of the %d' % (lat, lon, nd))
    lat, lon = lat % nd, lon % nd
    nlat, L, T = int(a.shape[lat]), int(a.shape[lon]), int(transform.truncation)
    if (nlat, L) != (transform.nlat, transform.n_lon):
        raise ValueError('spherical_spectrum: the grid axes hold %d x %d points, the transform is for %d x %d'
                         % (nlat, L, transform.nlat, transform.n_lon))
    if L > SPECTRUM_MAX_L:
        raise NotImplementedError('spherical_spectrum: %d longitudes, the kernel serves 2 .. %d' % (L, SPECTRUM_MAX_L))
    if nlat > nat.SHT_MAX_NLAT:
        raise NotImplementedError('spherical_spectrum: %d latitudes, the kernel serves 2 .. %d' % (nlat, nat.SHT_MAX_NLAT))
    lead_axes = [i for i in range(nd) if i not in (lat, lon)]
    red = set()
    for r in reduced:
        r = int(r)
        if r < -nd or r >= nd or r % nd in (lat, lon):
            raise ValueError('spherical_spectrum: reduced axis %d is out of range or a grid axis' % r)
        red.add(lead_axes.index(r % nd))                # its place among the leading axes
    # longitude last and unit-stride: a view where that is possible, else one copy (the latitude axis keeps its own stride)
    ops = [t.permute(lead_axes + [lat, lon]) for t in ops]
    ops = [t.contiguous() if t.stride(-1) != 1 else t for t in ops]
    lead = tuple(int(e) for e in ops[0].shape[:-2])
    strides = [tuple(int(s) for s in t.stride()[:-2]) for t in ops]
    lat_strides = [int(t.stride(-2)) for t in ops]
    if b is None:
        strides.append((0,) * len(lead))
        lat_strides.append(0)
    kept_shape = [lead[i] for i in range(len(lead)) if i not in red]
    nq = [] if b is None else [3]
    K = T + 1
    dev = a.device
    fields = int(np.prod(lead, dtype=np.int64))
    out = torch.empty(nq + kept_shape + [K], dtype=torch.float32, device=dev)
    cnt = torch.empty(kept_shape, dtype=torch.int32, device=dev) if counts else None
    if fields == 0 or out.numel() == 0:
        if out.numel():
            out.fill_(float('nan'))
        if cnt is not None:
            cnt.zero_()
        return (out, cnt) if counts else out
    twiddle, table = transform.device_tables(dev)
    averaged = any(lead[i] != 1 for i in red)
    rows = out.view(nq + [fields, K]) if not averaged else torch.empty(nq + [fields, K], dtype=torch.float32, device=dev)
    flags = torch.empty((fields,), dtype=torch.int32, device=dev) if counts else None
    d = sht_desc(nlat, L, T, spectrum_dims(lead, strides, ()), lat_strides)
    sht_launch(d, ops[0], ops[1] if b is not None else None, twiddle, table, rows, flags)
    if averaged:
        gs_d, ri_d = _sht_group_tables(lead, red, dev)
        n_groups, longest = int(gs_d.numel()) - 1, fields // max(int(gs_d.numel()) - 1, 1)
        row_axis = len(nq)
        rd, mean = _rows_desc(rows, row_axis, None, n_groups)
        with torch.cuda.device(dev):
            nbytes = int(lib().dlwpcs_group_mean_scratch_bytes(ctypes.byref(rd), n_groups, longest, -1))
            scratch = _workspace(nbytes, dev, 'sht_mean') if nbytes else None
            check(lib().dlwpcs_group_mean(ctypes.byref(rd), rows.data_ptr(), gs_d.data_ptr(), ri_d.data_ptr(), n_groups, longest, -1,
                                          mean.data_ptr(), None, ptr(scratch), nbytes, stream_ptr()), 'dlwpcs_group_mean')
        out = mean.view(nq + kept_shape + [K])
    if counts:
        full = flags.view(lead)
        cnt = full.sum(dim=tuple(sorted(red)), dtype=torch.int32) if red else full
    return (out, cnt) if counts else out


def _sht_grid_axes(a, transform, lat_axis, lon_axis, who):
    """(lat, lon) as non-negative axes of the device tensor `a` after the checks spherical_spectrum makes"""
    nd = a.dim()
    if nd < 2:
        raise ValueError('%s: the input needs a latitude and a longitude axis' % who)
    lat, lon = int(lat_axis), int(lon_axis)
    if not (-nd <= lat < nd and -nd <= lon < nd) or lat % nd == lon % nd:
        raise ValueError('%s: lat_axis %d and lon_axis %d must be two axes of the %d' % (who, lat, lon, nd))
    lat, lon = lat % nd, lon % nd
    nlat, L = int(a.shape[lat]), int(a.shape[lon])
    if (nlat, L) != (transform.nlat, transform.n_lon):
        raise ValueError('%s: the grid axes hold %d x %d points, the transform is for %d x %d'
                         % (who, nlat, L, transform.nlat, transform.n_lon))
    if L > SPECTRUM_MAX_L:
        raise NotImplementedError('%s: %d longitudes, the kernel serves 2 .. %d' % (who, L, SPECTRUM_MAX_L))
    if nlat > nat.SHT_MAX_NLAT:
        raise NotImplementedError('%s: %d latitudes, the kernel serves 2 .. %d' % (who, nlat, nat.SHT_MAX_NLAT))
    return lat, lon


def sht_analysis_launch(d, a, twiddle, table, coef, skipped=None):
    """dlwpcs_sht_analysis on the current stream: the device tensor a addressed by the descriptor (operand 0), into the float32
    tensor `coef` (fields, rows, 2) and the int32 tensor `skipped` (fields; None: not wanted)"""
    dev = a.device
    nbytes = int(lib().dlwpcs_sht_analysis_scratch_bytes(ctypes.byref(d)))
    scratch = _workspace(nbytes, dev, 'sht') if nbytes else None
    with torch.cuda.device(dev):
        check(lib().dlwpcs_sht_analysis(ctypes.byref(d), ptr(a), ptr(twiddle), ptr(table), ptr(scratch) or None, ptr(coef),
                                        ptr(skipped) or None, stream_ptr()), 'dlwpcs_sht_analysis')
    return coef


def sht_synthesis_desc(nlat, L, T, dims, lat_stride):
    """nat.ShtSynthesisDesc of output fields of nlat x L points: `dims` the leading dims of spectrum_dims over the output's
    strides, lat_stride the element stride of its latitude axis"""
    if len(dims) > nat.SCORE_MAX_DIMS:
        raise NotImplementedError('spherical_synthesis: more than %d leading dims after merging' % nat.SCORE_MAX_DIMS)
    d = nat.ShtSynthesisDesc()
    d.nlat, d.L, d.T, d.n_dims, d.lat_stride = int(nlat), int(L), int(T), len(dims), int(lat_stride)
    for i, (e, st, _) in enumerate(dims):
        d.ext[i], d.stride[i] = e, st[0]
    return d


def sht_synthesis_launch(d, coef, response, twiddle, table, out):
    """dlwpcs_sht_synthesis on the current stream: the float32 tensor `coef` (fields, rows, 2), `response` (T + 1 floats or None)
    and the unweighted table, into the device tensor `out` addressed by the descriptor"""
    dev = out.device
    nbytes = int(lib().dlwpcs_sht_synthesis_scratch_bytes(ctypes.byref(d)))
    scratch = _workspace(nbytes, dev, 'sht_synth') if nbytes else None
    with torch.cuda.device(dev):
        check(lib().dlwpcs_sht_synthesis(ctypes.byref(d), ptr(coef), ptr(response) or None, ptr(twiddle), ptr(table),
                                         ptr(scratch) or None, ptr(out), stream_ptr()), 'dlwpcs_sht_synthesis')
    return out


def spherical_analysis(a, transform, lat_axis=-2, lon_axis=-1, counts=False):
    """
    The spherical-harmonic coefficients a_n^m (0 <= m <= n <= T) of the float32 device tensor `a`, whose `lat_axis` and `lon_axis`
    hold the grid of `transform` (a DLWP.remap.spharm.SphericalTransform: it states the definitions and the packing): a complex64
    device tensor (leading axes..., (T + 1)(T + 2) / 2), row spharm.packed_row(m, n, T).  The grid axes may sit anywhere; no copy
    is made while longitude is unit-stride.  A field that holds a NaN or an infinity gets NaN coefficients; counts=True: also the
    int32 tensor (leading axes...) that holds 1 for such a field.  Two launches of dlwpcs_sht_analysis on the current stream.
    """
    if transform is None:
        raise TypeError('spherical_analysis: a SphericalTransform is required')
    require_device(a, 'spherical_analysis')
    if a.dtype != torch.float32:
        raise TypeError('spherical_analysis: the operand must be float32, got %s' % a.dtype)
    lat, lon = _sht_grid_axes(a, transform, lat_axis, lon_axis, 'spherical_analysis')
    nlat, L, T = transform.nlat, transform.n_lon, int(transform.truncation)
    lead_axes = [i for i in range(a.dim()) if i not in (lat, lon)]
    t = a.permute(lead_axes + [lat, lon])
    if t.stride(-1) != 1:
        t = t.contiguous()
    lead = tuple(int(e) for e in t.shape[:-2])
    fields = int(np.prod(lead, dtype=np.int64))
    rows = (T + 1) * (T + 2) // 2
    dev = a.device
    coef = torch.empty(lead + (rows, 2), dtype=torch.float32, device=dev)
    flags = torch.empty(lead, dtype=torch.int32, device=dev) if counts else None
    if fields:
        twiddle, table = transform.device_tables(dev)
        strides = [tuple(int(s) for s in t.stride()[:-2]), (0,) * len(lead)]
        d = sht_desc(nlat, L, T, spectrum_dims(lead, strides, ()), (int(t.stride(-2)), 0))
        sht_analysis_launch(d, t, twiddle, table, coef, flags)
    out = torch.view_as_complex(coef)
    return (out, flags) if counts else out


def _sht_response(response, T, dev, who):
    """the response as a float32 device tensor of T + 1 factors (None stays None); a host array is uploaded, so pass a device
    tensor where the call must be captured"""
    if response is None:
        return None
    if not torch.is_tensor(response):
        if torch.cuda.is_current_stream_capturing():
            raise nat.NativeError('%s: a host response inside a graph capture (pass a device tensor)' % who)
        response = torch.from_numpy(np.ascontiguousarray(np.asarray(response, dtype=np.float64).reshape(-1).astype(np.float32))).to(dev)
    require_device(response, who)
    if response.dtype != torch.float32 or response.device != dev or response.dim() != 1 or not response.is_contiguous():
        raise TypeError('%s: the response must be a contiguous float32 vector on the device of the coefficients' % who)
    if int(response.numel()) != T + 1:
        raise ValueError('%s: a response of %d factors, truncation %d needs %d' % (who, int(response.numel()), T, T + 1))
    return response


def spherical_synthesis(coef, transform, response=None, out=None):
    """
    The fields x[i, j] = sum_m c_m Re(e^{2 pi i j m / L} sum_n r_n a_n^m Pbar_n^m(mu_i)) of the complex64 device tensor `coef`
    (leading axes..., (T + 1)(T + 2) / 2) on the grid of `transform`: a float32 device tensor (leading axes..., nlat, L).
    response: T + 1 real factors r_n per degree (float32 device vector or host array; None: ones, with the same bits).
    out: a float32 device tensor of that shape to write into; any strides with longitude at unit stride.
    Two launches of dlwpcs_sht_synthesis on the current stream, no host synchronisation (the unweighted table of a transform is
    uploaded at its first use).
    """
    if transform is None:
        raise TypeError('spherical_synthesis: a SphericalTransform is required')
    if not isinstance(coef, torch.Tensor) or coef.dtype != torch.complex64:
        raise TypeError('spherical_synthesis: the coefficients must be a complex64 tensor, got %s'
                        % (coef.dtype if isinstance(coef, torch.Tensor) else type(coef)))
    require_device(torch.view_as_real(coef), 'spherical_synthesis')
    nlat, L, T = transform.nlat, transform.n_lon, int(transform.truncation)
    rows = (T + 1) * (T + 2) // 2
    if coef.dim() < 1 or int(coef.shape[-1]) != rows:
        raise ValueError('spherical_synthesis: %s coefficients, truncation %d has %d per field' % (tuple(coef.shape), T, rows))
    if L > SPECTRUM_MAX_L:
        raise NotImplementedError('spherical_synthesis: %d longitudes, the kernel serves 2 .. %d' % (L, SPECTRUM_MAX_L))
    if nlat > nat.SHT_MAX_NLAT:
        raise NotImplementedError('spherical_synthesis: %d latitudes, the kernel serves 2 .. %d' % (nlat, nat.SHT_MAX_NLAT))
    dev = coef.device
    lead = tuple(int(e) for e in coef.shape[:-1])
    if out is None:
        out = torch.empty(lead + (nlat, L), dtype=torch.float32, device=dev)
    else:
        require_device(out, 'spherical_synthesis')
        if out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != lead + (nlat, L):
            raise ValueError('spherical_synthesis: out must be a float32 tensor of shape %s on the device of the coefficients'
                             % (lead + (nlat, L),))
        if out.stride(-1) != 1:
            raise ValueError('spherical_synthesis: out needs unit stride along longitude')
    resp = _sht_response(response, T, dev, 'spherical_synthesis')
    if int(np.prod(lead, dtype=np.int64)):
        flat = torch.view_as_real(coef.contiguous())
        twiddle, table = transform.device_synthesis_tables(dev)
        strides = [tuple(int(s) for s in out.stride()[:-2])]
        d = sht_synthesis_desc(nlat, L, T, spectrum_dims(lead, strides, ()), int(out.stride(-2)))
        sht_synthesis_launch(d, flat, resp, twiddle, table, out)
    return out


# ------------------------------------------------------------------------------------------------------------------ #
# Vector spherical harmonics (DLWP/verify.py spherical_uv / spherical_vrtdiv / spherical_gradient, DLWP/barotropic),
# include/dlwpcs.h dlwpcs_sht_vector_synthesis / dlwpcs_sht_vector_analysis; the tables come from SphericalTransform
# ------------------------------------------------------------------------------------------------------------------ #

VECTOR_OUTPUTS = ('vrt', 'div')


def sht_vector_synthesis_launch(d, coef_a, coef_b, rpsi, rchi, tables, out_u, out_v):
    """dlwpcs_sht_vector_synthesis on the current stream: float32 tensors coef_a, coef_b (fields, rows, 2; either None), the
    responses (T + 1 floats or None) and `tables` = SphericalTransform.device_vector_tables, into out_u (operand 0 of the
    descriptor) and out_v (operand 1)"""
    dev = out_u.device
    nbytes = int(lib().dlwpcs_sht_vector_synthesis_scratch_bytes(ctypes.byref(d)))
    scratch = _workspace(nbytes, dev, 'sht_synth') if nbytes else None
    with torch.cuda.device(dev):
        check(lib().dlwpcs_sht_vector_synthesis(ctypes.byref(d), ptr(coef_a) or None, ptr(coef_b) or None, ptr(rpsi) or None,
                                                ptr(rchi) or None, ptr(tables[0]), ptr(tables[1]), ptr(tables[2]),
                                                ptr(scratch) or None, ptr(out_u), ptr(out_v), stream_ptr()),
              'dlwpcs_sht_vector_synthesis')


def sht_vector_analysis_launch(d, u, v, response, tables, vrt, div, skipped=None):
    """dlwpcs_sht_vector_analysis on the current stream: the device tensors u, v addressed by the descriptor, into the float32
    tensors vrt, div (fields, rows, 2; either None) and the int32 tensor `skipped` (fields; None: not wanted)"""
    dev = u.device
    nbytes = int(lib().dlwpcs_sht_vector_analysis_scratch_bytes(ctypes.byref(d)))
    scratch = _workspace(nbytes, dev, 'sht') if nbytes else None
    with torch.cuda.device(dev):
        check(lib().dlwpcs_sht_vector_analysis(ctypes.byref(d), ptr(u), ptr(v), ptr(response) or None, ptr(tables[0]), ptr(tables[3]),
                                               ptr(tables[4]), ptr(scratch) or None, ptr(vrt) or None, ptr(div) or None,
                                               ptr(skipped) or None, stream_ptr()), 'dlwpcs_sht_vector_analysis')


def _view_span(t, period):
    """(ok, span): span = the elements covered by one block of the dims of `t` with a stride below `period`; ok when every other
    stride is a multiple of `period`, so that the view lies in the blocks [k period, k period + span)"""
    span, ok = 1, True
    for n, st in zip(t.shape, t.stride()):
        if n <= 1:
            continue
        if st < period:
            span += (int(n) - 1) * int(st)
        elif st % period:
            ok = False
    return ok, span


def _may_overlap(a, b):
    """False when the float32 views a and b provably share no element: their address ranges are apart, or both lie in periodic
    blocks of one period (a stride of either) that never meet, as two slices of one interleaved buffer do.  True otherwise."""
    if not a.numel() or not b.numel():
        return False
    lo_a, lo_b = a.data_ptr() // 4, b.data_ptr() // 4
    ext = lambda t: 1 + sum((int(n) - 1) * int(st) for n, st in zip(t.shape, t.stride()))      # noqa: E731
    if any(st < 0 for t in (a, b) for st in t.stride()):
        return True
    if lo_a + ext(a) <= lo_b or lo_b + ext(b) <= lo_a:
        return False
    if lo_a > lo_b:
        a, b, lo_a, lo_b = b, a, lo_b, lo_a
    for period in sorted({int(st) for t in (a, b) for n, st in zip(t.shape, t.stride()) if n > 1 and st > 1}):
        (ok_a, span_a), (ok_b, span_b) = _view_span(a, period), _view_span(b, period)
        r = (lo_b - lo_a) % period
        if ok_a and ok_b and span_a <= r and r + span_b <= period:
            return False
    return True


def _sht_coef_operand(c, rows, who):
    if not isinstance(c, torch.Tensor) or c.dtype != torch.complex64:
        raise TypeError('%s: the coefficients must be a complex64 tensor, got %s' % (who, c.dtype if isinstance(c, torch.Tensor) else type(c)))
    if c.dim() < 1 or int(c.shape[-1]) != rows:
        raise ValueError('%s: %s coefficients, the truncation has %d per field' % (who, tuple(c.shape), rows))
    require_device(torch.view_as_real(c), who)
    return c


def spherical_vector_synthesis(A, B, transform, rpsi=None, rchi=None, out_u=None, out_v=None):
    """
    The wind (u, v) of the potentials psi_n^m = rpsi_n A_n^m and chi_n^m = rchi_n B_n^m on the grid of `transform`:
        u = -dpsi/dphi + (1/cos) dchi/dlambda,   v = (1/cos) dpsi/dlambda + dchi/dphi
    (the factor 1 / radius belongs in the responses).  A, B: complex64 device tensors (leading axes..., (T + 1)(T + 2) / 2) of one
    shape; either may be None (it then costs nothing), not both.  rpsi, rchi: T + 1 real factors per degree (float32 device vector
    or host array; None: ones, with the same bits).  out_u, out_v: float32 device tensors (leading axes..., nlat, L) to write into,
    any strides with longitude at unit stride, the two apart (two slices of one interleaved buffer are).  Returns (u, v).  Three launches of dlwpcs_sht_vector_synthesis on the current
    stream, no host synchronisation (the tables of a transform are uploaded at their first use).
    """
    who = 'spherical_vector_synthesis'
    if transform is None:
        raise TypeError('%s: a SphericalTransform is required' % who)
    if A is None and B is None:
        raise ValueError('%s: both potentials are absent' % who)
    nlat, L, T = transform.nlat, transform.n_lon, int(transform.truncation)
    rows = (T + 1) * (T + 2) // 2
    pots = [None if c is None else _sht_coef_operand(c, rows, who) for c in (A, B)]
    first = pots[0] if pots[0] is not None else pots[1]
    if pots[0] is not None and pots[1] is not None and (pots[0].shape != pots[1].shape or pots[0].device != pots[1].device):
        raise ValueError('%s: the two potentials must have one shape and one device' % who)
    if L > SPECTRUM_MAX_L:
        raise NotImplementedError('%s: %d longitudes, the kernel serves 2 .. %d' % (who, L, SPECTRUM_MAX_L))
    if nlat > nat.SHT_MAX_NLAT:
        raise NotImplementedError('%s: %d latitudes, the kernel serves 2 .. %d' % (who, nlat, nat.SHT_MAX_NLAT))
    dev = first.device
    lead = tuple(int(e) for e in first.shape[:-1])
    outs = []
    for o in (out_u, out_v):
        if o is None:
            o = torch.empty(lead + (nlat, L), dtype=torch.float32, device=dev)
        else:
            require_device(o, who)
            if o.dtype != torch.float32 or o.device != dev or tuple(o.shape) != lead + (nlat, L):
                raise ValueError('%s: an output must be a float32 tensor of shape %s on the device of the coefficients'
                                 % (who, lead + (nlat, L)))
            if o.stride(-1) != 1:
                raise ValueError('%s: an output needs unit stride along longitude' % who)
        outs.append(o)
    if _may_overlap(outs[0], outs[1]):
        raise ValueError('%s: out_u and out_v overlap (or cannot be shown to be apart)' % who)
    rp = _sht_response(rpsi, T, dev, who) if pots[0] is not None else None
    rc = _sht_response(rchi, T, dev, who) if pots[1] is not None else None
    if int(np.prod(lead, dtype=np.int64)):
        flat = [None if c is None else torch.view_as_real(c.contiguous()) for c in pots]
        tables = transform.device_vector_tables(dev)
        strides = [tuple(int(s) for s in o.stride()[:-2]) for o in outs]
        d = sht_desc(nlat, L, T, spectrum_dims(lead, strides, ()), [int(o.stride(-2)) for o in outs])
        sht_vector_synthesis_launch(d, flat[0], flat[1], rp, rc, tables, outs[0], outs[1])
    return outs[0], outs[1]


def spherical_vector_analysis(u, v, transform, response=None, want=VECTOR_OUTPUTS, lat_axis=-2, lon_axis=-1, counts=False):
    """
    The vorticity-like and divergence-like coefficients of the float32 device tensors u, v (one shape, the grid of `transform` on
    `lat_axis` and `lon_axis`):  vrt_n^m = r_n sum_i (w_i / 2) [i Q V_m + D U_m] / L,  div_n^m = r_n sum_i (w_i / 2) [i Q U_m - D V_m] / L.
    response: T + 1 real factors r_n (1 / radius for vorticity and divergence; None: ones).  want: which of 'vrt', 'div', a tuple;
    the result is a tuple of complex64 device tensors (leading axes..., (T + 1)(T + 2) / 2) in that order, and an output that is
    not wanted costs nothing.  A field with a NaN or an infinity in u or in v has NaN coefficients in every output; counts=True:
    also the int32 tensor (leading axes...) that holds 1 for such a field.  Two launches of dlwpcs_sht_vector_analysis.
    """
    who = 'spherical_vector_analysis'
    if transform is None:
        raise TypeError('%s: a SphericalTransform is required' % who)
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in VECTOR_OUTPUTS for w in want) or len(set(want)) != len(want):
        raise ValueError('%s: want %s, a non-empty choice of %s' % (who, want, VECTOR_OUTPUTS))
    for t in (u, v):
        require_device(t, who)
        if t.dtype != torch.float32:
            raise TypeError('%s: operands must be float32, got %s' % (who, t.dtype))
    if u.shape != v.shape or u.device != v.device:
        raise ValueError('%s: u and v must have one shape and one device' % who)
    lat, lon = _sht_grid_axes(u, transform, lat_axis, lon_axis, who)
    nlat, L, T = transform.nlat, transform.n_lon, int(transform.truncation)
    lead_axes = [i for i in range(u.dim()) if i not in (lat, lon)]
    ts = [t.permute(lead_axes + [lat, lon]) for t in (u, v)]
    ts = [t.contiguous() if t.stride(-1) != 1 else t for t in ts]
    lead = tuple(int(e) for e in ts[0].shape[:-2])
    rows = (T + 1) * (T + 2) // 2
    dev = u.device
    out = {w: torch.empty(lead + (rows, 2), dtype=torch.float32, device=dev) for w in want}
    flags = torch.empty(lead, dtype=torch.int32, device=dev) if counts else None
    resp = _sht_response(response, T, dev, who)
    if int(np.prod(lead, dtype=np.int64)):
        tables = transform.device_vector_tables(dev)
        strides = [tuple(int(s) for s in t.stride()[:-2]) for t in ts]
        d = sht_desc(nlat, L, T, spectrum_dims(lead, strides, ()), [int(t.stride(-2)) for t in ts])
        sht_vector_analysis_launch(d, ts[0], ts[1], resp, tables, out.get('vrt'), out.get('div'), flags)
    res = tuple(torch.view_as_complex(out[w]) for w in want)
    return res + (flags,) if counts else res


def barotropic_flux(zeta, u, v, coriolis, out_f=None, out_g=None):
    """((f_i + zeta) u, (f_i + zeta) v) of the contiguous float32 device tensors zeta, u, v (..., nlat, L) and the float32 device
    vector `coriolis` of nlat values; out_f, out_g: contiguous tensors of that shape to write into.  One launch."""
    who = 'barotropic_flux'
    for t in (zeta, u, v, coriolis):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != zeta.device:
            raise TypeError('%s: operands must be contiguous float32 tensors on one device' % who)
        require_device(t, who)
    if zeta.dim() < 2 or u.shape != zeta.shape or v.shape != zeta.shape:
        raise ValueError('%s: zeta, u and v must have one shape (..., nlat, L)' % who)
    nlat, L = int(zeta.shape[-2]), int(zeta.shape[-1])
    if coriolis.dim() != 1 or int(coriolis.numel()) != nlat:
        raise ValueError('%s: %d Coriolis values for %d latitudes' % (who, int(coriolis.numel()), nlat))
    outs = []
    for o in (out_f, out_g):
        if o is None:
            o = torch.empty_like(zeta)
        else:
            require_device(o, who)
            if o.dtype != torch.float32 or o.shape != zeta.shape or not o.is_contiguous() or o.device != zeta.device:
                raise ValueError('%s: an output must be a contiguous float32 tensor of the shape of zeta' % who)
        outs.append(o)
    if _may_overlap(outs[0], outs[1]) or any(_may_overlap(o, t) for o in outs for t in (zeta, u, v)):
        raise ValueError('%s: an output overlaps the other output or an input' % who)
    fields = int(zeta.numel()) // (nlat * L) if nlat * L else 0
    if fields:
        with torch.cuda.device(zeta.device):
            check(lib().dlwpcs_barotropic_flux(fields, nlat, L, ptr(coriolis), ptr(zeta), ptr(u), ptr(v), ptr(outs[0]), ptr(outs[1]),
                                               stream_ptr()), 'dlwpcs_barotropic_flux')
    return outs[0], outs[1]


def barotropic_update(tend, zeta, zeta_prev, damp, dt, robert, first_step):
    """One time step of the barotropic model in place on the contiguous complex64 device tensors zeta, zeta_prev (..., rows), given
    the tendency `tend` of that shape (a third buffer) and the float32 device vector `damp` of rows damping rates (include/dlwpcs.h
    dlwpcs_barotropic_update states the scheme).  One launch.  Returns (zeta, zeta_prev)."""
    who = 'barotropic_update'
    for t in (tend, zeta, zeta_prev):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.complex64:
            raise TypeError('%s: tend, zeta and zeta_prev must be complex64 tensors' % who)
        require_device(torch.view_as_real(t), who)
        if not t.is_contiguous() or t.shape != zeta.shape or t.device != zeta.device:
            raise ValueError('%s: tend, zeta and zeta_prev must be contiguous, of one shape and on one device' % who)
    require_device(damp, who)
    if zeta.dim() < 1:
        raise ValueError('%s: the coefficients need an axis' % who)
    rows = int(zeta.shape[-1])
    if damp.dtype != torch.float32 or damp.dim() != 1 or int(damp.numel()) != rows or not damp.is_contiguous() or damp.device != zeta.device:
        raise ValueError('%s: damp must be a contiguous float32 vector of %d rates on the device of zeta' % (who, rows))
    parts = [torch.view_as_real(t) for t in (tend, zeta, zeta_prev)]
    if _may_overlap(parts[1], parts[2]):
        raise ValueError('%s: zeta and zeta_prev must be two buffers' % who)
    if _may_overlap(parts[0], parts[1]) or _may_overlap(parts[0], parts[2]):
        raise ValueError('%s: tend overlaps a state' % who)
    fields = int(zeta.numel()) // rows if rows else 0
    if fields:
        with torch.cuda.device(zeta.device):
            check(lib().dlwpcs_barotropic_update(fields, rows, ptr(damp), float(dt), float(robert), int(bool(first_step)),
                                                 ptr(torch.view_as_real(tend)), ptr(torch.view_as_real(zeta)),
                                                 ptr(torch.view_as_real(zeta_prev)), stream_ptr()), 'dlwpcs_barotropic_update')
    return zeta, zeta_prev


# ------------------------------------------------------------------------------------------------------------------ #
# Ensemble scores (DLWP/verify.py ensemble_* / rank_histogram), include/dlwpcs.h dlwpcs_ensemble_stats
# ------------------------------------------------------------------------------------------------------------------ #

ENSEMBLE_MAX_M = nat.ENSEMBLE_MAX_M
ENSEMBLE_OUTPUTS = ('mean', 'spread', 'crps', 'rank')


def ensemble_layout(shape, strides, member_axis=0, valid_shape=None, valid_strides=None):
    """
    How dlwpcs_ensemble_stats walks an ensemble of logical `shape` and element `strides` whose members lie along `member_axis`,
    and a verification of `valid_shape` / `valid_strides` (the ensemble's dims without the member axis, extents of 1 broadcast):
    (M, member stride, element shape, order, merged dims).  `order` lists the element dims of extent > 1 from the largest stride
    of the ensemble to the smallest, so that the lanes run along the dim that is contiguous in memory whatever view the caller
    holds; the outputs are laid out in that order and handed back as views of the element shape.  Merged dims as
    layout.merge_dims makes them: [(extent, (ensemble stride, verification stride))].
    """
    return element_layout(shape, strides, member_axis, [(valid_shape, valid_strides)], 'ensemble_stats', 2, nat.SCORE_MAX_DIMS)


def ensemble_desc(M, member_stride, merged, fair=False, ddof=1, variance=False):
    """nat.EnsembleDesc of M members `member_stride` elements apart over the merged dims of ensemble_layout"""
    if int(ddof) not in (0, 1):
        raise ValueError('ensemble_stats: ddof = %s (0 or 1)' % (ddof,))
    d = nat.EnsembleDesc()
    d.M, d.n_dims, d.fair, d.ddof, d.variance = int(M), len(merged), int(bool(fair)), int(ddof), int(bool(variance))
    d.member_stride = int(member_stride)
    for i, (e, s) in enumerate(merged):
        d.ext[i] = e
        d.stride[0][i], d.stride[1][i] = s
    return d


def ensemble_plan(shape, strides, member_axis=0, valid_shape=None, valid_strides=None, ens_ptr=1 << 20, valid_ptr=None,
                  fair=False, ddof=1, variance=False):
    """
    Which code ensemble_stats would run for an ensemble of this shape, these element strides and this address (host only: no
    device is touched, the addresses are looked at for alignment): dict(m_class = member slots of the instantiation, vec = 16-byte
    loads of the ensemble, valid = -1 absent / 0 element by element / 1 16-byte loads, lds = members in LDS, grid, threads).
    valid_ptr defaults to an aligned address when a verification shape is given.  Raises what ensemble_stats would raise.
    """
    M, ms, _, _, merged = ensemble_layout(shape, strides, member_axis, valid_shape, valid_strides)
    d = ensemble_desc(M, ms, merged, fair, ddof, variance)
    if valid_ptr is None and valid_shape is not None:
        valid_ptr = 1 << 21
    info = (ctypes.c_int32 * 8)()
    check(lib().dlwpcs_ensemble_plan_info(ctypes.byref(d), int(ens_ptr), valid_ptr or None, info), 'dlwpcs_ensemble_plan_info')
    return dict(m_class=info[0], vec=bool(info[1]), valid=info[2], lds=bool(info[3]), grid=(info[4], info[5]), threads=info[6])


def _ordered_outputs(names, int_names, per_q, Q, eshape, order, device):
    """
    The outputs of a kernel that writes flat in `order` (layout.element_layout): ({name: flat buffer}, {name: view of it with the
    element shape}); the names in `per_q` carry a leading dim of Q.  float32, int32 for `int_names`.
    """
    n = 1
    for e in eshape:
        n *= e
    perm = [order.index(i) for i in sorted(order)]
    flat, res = {}, {}
    for name in names:
        lead = [Q] if name in per_q else []
        flat[name] = torch.empty(lead + [n], dtype=torch.int32 if name in int_names else torch.float32, device=device)
        if n:
            t = flat[name].view(lead + [eshape[i] for i in order]).permute(list(range(len(lead))) + [len(lead) + q for q in perm])
            for i, e in enumerate(eshape):
                if e == 1:
                    t = t.unsqueeze(len(lead) + i)
            res[name] = t
        else:
            res[name] = flat[name].view(lead + list(eshape))
    return n, flat, res


def ensemble_stats(ens, valid=None, member_axis=0, want=ENSEMBLE_OUTPUTS, fair=False, ddof=1, variance=False):
    """
    Collapse the member axis of the float32 device tensor `ens` element by element: dict of device tensors shaped like `ens`
    without that axis, 'mean', 'spread' (standard deviation with `ddof`; variance=True: the variance), 'crps' (against `valid`;
    fair=True: the pair term over M (M - 1)) -- float32 -- and 'rank' (int32: members strictly below `valid`, 0..M), those named
    in `want`.  `valid`: a float32 device tensor with the dims of `ens` without the member axis, extents of 1 broadcast; 'crps'
    and 'rank' need it.  An element with a NaN or infinite member is NaN / -1 everywhere, a NaN or infinite verification in
    'crps' / 'rank'.  Views are read through their strides (no copy); the results may come back as permuted views.  One launch
    on the current stream, no host synchronisation, no allocation besides the outputs.
    """
    want = tuple(want)
    if not want or any(w not in ENSEMBLE_OUTPUTS for w in want):
        raise ValueError('ensemble_stats: want %s, a non-empty choice of %s' % (want, ENSEMBLE_OUTPUTS))
    require_device(ens, 'ensemble_stats')
    if ens.dtype != torch.float32:
        raise TypeError('ensemble_stats: operands must be float32, got %s' % ens.dtype)
    if valid is not None:
        require_device(valid, 'ensemble_stats')
        if valid.dtype != torch.float32 or valid.device != ens.device:
            raise TypeError('ensemble_stats: the verification must be a float32 tensor on the device of the ensemble')
    elif 'crps' in want or 'rank' in want:
        raise ValueError("ensemble_stats: 'crps' and 'rank' need a verification")
    M, ms, eshape, order, merged = ensemble_layout(ens.shape, ens.stride(), member_axis,
                                                   None if valid is None else valid.shape,
                                                   None if valid is None else valid.stride())
    if M > ENSEMBLE_MAX_M:
        raise NotImplementedError('ensemble_stats: %d members, the kernel serves 2 .. %d' % (M, ENSEMBLE_MAX_M))
    d = ensemble_desc(M, ms, merged, fair, ddof, variance)
    n, flat, res = _ordered_outputs([w for w in ENSEMBLE_OUTPUTS if w in want], ('rank',), (), 0, eshape, order, ens.device)
    if n:
        with torch.cuda.device(ens.device):
            check(lib().dlwpcs_ensemble_stats(ctypes.byref(d), ptr(ens), ptr(valid) or None, ptr(flat.get('mean')) or None,
                                              ptr(flat.get('spread')) or None, ptr(flat.get('crps')) or None,
                                              ptr(flat.get('rank')) or None, stream_ptr()), 'dlwpcs_ensemble_stats')
    return res


# ------------------------------------------------------------------------------------------------------------------ #
# Category scores of an ensemble (DLWP/verify.py brier_score and friends), include/dlwpcs.h dlwpcs_ensemble_category
# ------------------------------------------------------------------------------------------------------------------ #

CATEGORY_MAX_M, CATEGORY_MAX_Q = nat.CATEGORY_MAX_M, nat.CATEGORY_MAX_Q
CATEGORY_OUTPUTS = ('prob', 'brier', 'rps', 'rps_ref', 'code')
_CATEGORY_PER_THRESHOLD = ('prob', 'brier', 'code')


def category_layout(shape, strides, thr_shape, thr_strides, member_axis=0, threshold_axis=0, valid_shape=None, valid_strides=None):
    """
    How dlwpcs_ensemble_category walks an ensemble (as ensemble_layout reads it), its verification and the thresholds:
    (M, member stride, Q, threshold stride, element shape, order, merged dims [(extent, (ens, valid, thr strides))]).  The
    thresholds carry the element dims of the ensemble (extents of 1 broadcast) with the threshold axis at `threshold_axis`; a
    bare (Q,) vector serves every element.
    """
    _, _, eshape, _ = member_split(shape, strides, member_axis, 'ensemble_category', 1)
    tshape = tuple(int(s) for s in thr_shape)
    tstr = tuple(int(s) for s in thr_strides)
    if len(tshape) == 1:
        Q, qs, ts = tshape[0], tstr[0], (0,) * len(eshape)
    else:
        if len(tshape) != len(eshape) + 1 or not -len(tshape) <= int(threshold_axis) < len(tshape):
            raise ValueError('ensemble_category: the thresholds %s must carry the dims of the ensemble without the member axis '
                             '%s and a threshold axis' % (tshape, eshape))
        ta = int(threshold_axis) % len(tshape)
        Q, qs = tshape[ta], tstr[ta]
        rest, rstr = tshape[:ta] + tshape[ta + 1:], tstr[:ta] + tstr[ta + 1:]
        if any(t not in (1, e) for t, e in zip(rest, eshape)):
            raise ValueError('ensemble_category: the thresholds %s without their threshold axis do not match the element dims '
                             '%s (extents of 1 broadcast)' % (tshape, eshape))
        ts = tuple(0 if t == 1 else s for t, s in zip(rest, rstr))
    if Q < 1:
        raise ValueError('ensemble_category: %d thresholds (at least 1)' % Q)
    M, ms, eshape, order, merged = element_layout(shape, strides, member_axis, [(valid_shape, valid_strides), (None, ts)],
                                                  'ensemble_category', 1, nat.SCORE_MAX_DIMS)
    return M, ms, Q, qs, eshape, order, merged


def category_desc(M, member_stride, Q, thr_stride, merged, fair=False, ref_prob=None):
    """nat.CategoryDesc of M members and Q thresholds over the merged dims of category_layout"""
    d = nat.CategoryDesc()
    d.M, d.Q, d.n_dims, d.fair = int(M), int(Q), len(merged), int(bool(fair))
    d.member_stride, d.thr_stride = int(member_stride), int(thr_stride)
    for i, (e, s) in enumerate(merged):
        d.ext[i] = e
        d.stride[0][i], d.stride[1][i], d.stride[2][i] = s
    if ref_prob is not None:
        rp = np.asarray(ref_prob, dtype=np.float32).reshape(-1)
        if rp.size != Q:
            raise ValueError('ensemble_category: %d reference probabilities for %d thresholds' % (rp.size, Q))
        for j in range(min(Q, CATEGORY_MAX_Q)):
            d.ref_prob[j] = float(rp[j])
    return d


def ensemble_category_plan(shape, strides, thr_shape, thr_strides, member_axis=0, threshold_axis=0, valid_shape=None,
                           valid_strides=None, ens_ptr=1 << 20, valid_ptr=None, thr_ptr=1 << 22, fair=False):
    """
    Which code ensemble_category would run (host only: no device is touched, the addresses are looked at for alignment):
    dict(q_class = threshold slots of the instantiation, vec = 16-byte loads of the ensemble, valid = -1 absent / 0 element by
    element / 1 16-byte loads, thr = 0 element by element / 1 16-byte loads / 2 one vector for every element, grid, threads).
    Raises what ensemble_category would raise: NotImplementedError beyond 1024 members or 16 thresholds.
    """
    M, ms, Q, qs, _, _, merged = category_layout(shape, strides, thr_shape, thr_strides, member_axis, threshold_axis, valid_shape,
                                                 valid_strides)
    d = category_desc(M, ms, Q, qs, merged, fair)
    if valid_ptr is None and valid_shape is not None:
        valid_ptr = 1 << 21
    info = (ctypes.c_int32 * 8)()
    check(lib().dlwpcs_ensemble_category_plan_info(ctypes.byref(d), int(ens_ptr), valid_ptr or None, int(thr_ptr), info),
          'dlwpcs_ensemble_category_plan_info')
    return dict(q_class=info[0], vec=bool(info[1]), valid=info[2], thr=info[3], grid=(info[4], info[5]), threads=info[6])


def ensemble_category(ens, valid, thresholds, member_axis=0, threshold_axis=0, want=None, fair=False, ref_prob=None):
    """
    Category scores of the float32 device ensemble `ens` against Q thresholds, element by element, with k_j the members at or
    below threshold j and o_j = 1{valid <= threshold j}: dict of device tensors, those named in `want` --
    'prob' (Q, ...) k_j / M;  'brier' (Q, ...) ((k_j - o_j M) / M)^2;  'rps' (...) the sum of the Brier scores over the
    thresholds (fair=True: minus sum_j k_j (M - k_j) / (M^2 (M - 1)));  'rps_ref' (...) sum_j (ref_prob[j] - o_j)^2, the score
    of the reference forecast `ref_prob`;  'code' (Q, ...) int32 2 k_j + o_j.  (...) is the shape of `ens` without the member
    axis.  want=None: every output the operands allow.  `thresholds`: a float32 device tensor with the element dims of `ens`
    (extents of 1 broadcast) and the threshold axis at `threshold_axis`, or a bare (Q,) vector; `valid` as in ensemble_stats,
    None when only 'prob' is wanted.  Missing values: NaN / -1 (include/dlwpcs.h).  Views are read through their strides; the
    results may come back as permuted views.  One launch on the current stream, no host synchronisation.
    """
    if want is None:
        want = ('prob',) if valid is None else tuple(w for w in CATEGORY_OUTPUTS if w != 'rps_ref' or ref_prob is not None)
    want = tuple(want)
    if not want or any(w not in CATEGORY_OUTPUTS for w in want):
        raise ValueError('ensemble_category: want %s, a non-empty choice of %s' % (want, CATEGORY_OUTPUTS))
    require_device(ens, 'ensemble_category')
    require_device(thresholds, 'ensemble_category')
    if ens.dtype != torch.float32 or thresholds.dtype != torch.float32 or thresholds.device != ens.device:
        raise TypeError('ensemble_category: the ensemble and the thresholds must be float32 tensors on one device')
    if valid is not None:
        require_device(valid, 'ensemble_category')
        if valid.dtype != torch.float32 or valid.device != ens.device:
            raise TypeError('ensemble_category: the verification must be a float32 tensor on the device of the ensemble')
    elif want != ('prob',):
        raise ValueError("ensemble_category: only 'prob' can be had without a verification")
    if 'rps_ref' in want and ref_prob is None:
        raise ValueError("ensemble_category: 'rps_ref' needs the reference probabilities ref_prob")
    M, ms, Q, qs, eshape, order, merged = category_layout(ens.shape, ens.stride(), thresholds.shape, thresholds.stride(),
                                                          member_axis, threshold_axis,
                                                          None if valid is None else valid.shape,
                                                          None if valid is None else valid.stride())
    if M > CATEGORY_MAX_M:
        raise NotImplementedError('ensemble_category: %d members, the kernel serves 1 .. %d' % (M, CATEGORY_MAX_M))
    if Q > CATEGORY_MAX_Q:
        raise NotImplementedError('ensemble_category: %d thresholds, the kernel serves 1 .. %d' % (Q, CATEGORY_MAX_Q))
    if fair and M < 2:
        raise ValueError('ensemble_category: the fair score needs at least 2 members')
    d = category_desc(M, ms, Q, qs, merged, fair, ref_prob)
    n, flat, res = _ordered_outputs([w for w in CATEGORY_OUTPUTS if w in want], ('code',), _CATEGORY_PER_THRESHOLD, Q, eshape, order,
                                    ens.device)
    if n:
        with torch.cuda.device(ens.device):
            check(lib().dlwpcs_ensemble_category(ctypes.byref(d), ptr(ens), ptr(valid) or None, ptr(thresholds),
                                                 ptr(flat.get('prob')) or None, ptr(flat.get('brier')) or None,
                                                 ptr(flat.get('rps')) or None, ptr(flat.get('rps_ref')) or None,
                                                 ptr(flat.get('code')) or None, stream_ptr()), 'dlwpcs_ensemble_category')
    return res


# ------------------------------------------------------------------------------------------------------------------ #
# Climatologies (DLWP/verify.py): grouped mean over rows and indexed row gather, include/dlwpcs.h dlwpcs_rows_desc
# ------------------------------------------------------------------------------------------------------------------ #

def _rows_desc(src, row_axis, out_perm, n_out):
    """(descriptor, output tensor) for rows of `src` along `row_axis`: the output has src's dims in the order `out_perm` (default:
    as they are) with the row axis n_out long, contiguous.  Unit dims are dropped, neighbours merged where both sides allow it,
    and the dim that is contiguous in the source goes last (lanes run along it)."""
    require_device(src, 'rows')
    if src.dtype != torch.float32:
        raise TypeError('rows: the source must be float32, got %s' % src.dtype)
    d, oshape = rows_layout(src.shape, src.stride(), row_axis, out_perm, n_out)
    return d, torch.empty(oshape, dtype=torch.float32, device=src.device)


def rows_layout(shape, strides, row_axis, out_perm, n_out):
    """_rows_desc on a shape and element strides alone (host only): (descriptor, shape of the contiguous output)"""
    shape = tuple(int(s) for s in shape)
    strides = tuple(int(s) for s in strides)
    nd = len(shape)
    row_axis = row_axis % nd
    perm = tuple(range(nd)) if out_perm is None else tuple(int(a) % nd for a in out_perm)
    if sorted(perm) != list(range(nd)):
        raise ValueError('rows: out_perm %s is not a permutation of %d dims' % (out_perm, nd))
    oshape = [n_out if a == row_axis else shape[a] for a in perm]
    ostride, run = [0] * nd, 1
    for pos in range(nd - 1, -1, -1):
        ostride[pos] = run
        run *= max(oshape[pos], 1)                              # (torch's strides of a contiguous tensor)
    at = perm.index(row_axis)
    out_row = ostride[at]
    # (the tag: the row axis separates what may merge)
    dims = [(e, ss, os_) for e, (ss, os_), _ in
            merge_dims((shape[a], (strides[a], ostride[pos]), pos > at) for pos, a in enumerate(perm) if a != row_axis)]
    unit = [i for i, x in enumerate(dims) if x[1] == 1]
    if unit:
        dims.append(dims.pop(unit[-1]))
    if len(dims) > nat.SCORE_MAX_DIMS:
        raise NotImplementedError('rows: more than %d inner dims after merging' % nat.SCORE_MAX_DIMS)
    d = nat.RowsDesc()
    d.n_inner = len(dims)
    d.src_row_stride, d.out_row_stride = strides[row_axis], out_row
    for i, (e, ss, os_) in enumerate(dims):
        d.inner_ext[i], d.src_stride[i], d.out_stride[i] = e, ss, os_
    return d, oshape


def _int32_dev(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).pin_memory().to(dev, non_blocking=True)


def group_mean(src, group_start, row_index, row_axis=0, out_perm=None, split=None, counts=False):
    """
    Per-element mean over groups of rows of the fp32 device tensor `src` (any strides): group k holds the rows
    row_index[group_start[k]:group_start[k + 1]] of `row_axis` (numpy int arrays in CSR form, checked here and uploaded).  NaN
    entries are skipped per element; an element with no member left is NaN.  fp64 sums in a fixed order, rounded to fp32 once.
    The result has src's dims in the order `out_perm` (default: unchanged) with the row axis K long, contiguous: a channels-first
    array is reduced straight into a channels-last result.  split: None = the library chooses between one launch and the
    two-launch slab form, True / False forces it (same bits either way).  counts=True also returns the int32 member counts.
    At most two launches on the current stream, no host synchronisation.
    """
    gs = np.asarray(group_start, dtype=np.int64).reshape(-1)
    ri = np.asarray(row_index, dtype=np.int64).reshape(-1)
    if gs.size < 1 or gs[0] != 0 or np.any(np.diff(gs) < 0) or gs[-1] != ri.size:
        raise ValueError('group_mean: group_start must rise from 0 to len(row_index)')
    n_rows = int(src.shape[row_axis])
    if ri.size and (ri.min() < 0 or ri.max() >= n_rows):
        raise IndexError('group_mean: row index out of range of the %d source rows' % n_rows)
    K = gs.size - 1
    d, out = _rows_desc(src, row_axis, out_perm, K)
    cnt = torch.empty(out.shape, dtype=torch.int32, device=src.device) if counts else None
    if K == 0 or out.numel() == 0:
        return (out, cnt) if counts else out
    longest = int(np.diff(gs).max())
    flag = -1 if split is None else int(bool(split))
    dev = src.device
    with torch.cuda.device(dev):
        gs_d, ri_d = _int32_dev(gs, dev), _int32_dev(ri if ri.size else np.zeros(1), dev)
        nbytes = int(lib().dlwpcs_group_mean_scratch_bytes(ctypes.byref(d), K, longest, flag))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        check(lib().dlwpcs_group_mean(ctypes.byref(d), src.data_ptr(), gs_d.data_ptr(), ri_d.data_ptr(), K, longest, flag,
                                      out.data_ptr(), ptr(cnt), ptr(scratch), nbytes, stream_ptr()), 'dlwpcs_group_mean')
    return (out, cnt) if counts else out


def rows_gather(src, index, row_axis=0, out_perm=None):
    """
    out[i] = row index[i] of `row_axis` of the fp32 device tensor `src` (any strides); a negative index gives a NaN row.
    `index`: numpy ints (checked and uploaded) or an int32 device tensor (trusted).  The result has src's dims in the order
    `out_perm` with the row axis len(index) long, contiguous.  One launch on the current stream.
    """
    n_rows = int(src.shape[row_axis])
    dev = src.device
    if isinstance(index, torch.Tensor):
        if index.dtype != torch.int32 or index.device != dev or not index.is_contiguous():
            raise TypeError('rows_gather: a device index must be contiguous int32 on the device of the source')
        idx = index.reshape(-1)
    else:
        ih = np.asarray(index, dtype=np.int64).reshape(-1)
        if ih.size and ih.max() >= n_rows:
            raise IndexError('rows_gather: row index out of range of the %d source rows' % n_rows)
        idx = None
    n = int(idx.numel()) if idx is not None else int(ih.size)
    d, out = _rows_desc(src, row_axis, out_perm, n)
    if n == 0 or out.numel() == 0:
        return out
    with torch.cuda.device(dev):
        if idx is None:
            idx = _int32_dev(ih, dev)
        check(lib().dlwpcs_rows_gather(ctypes.byref(d), src.data_ptr(), idx.data_ptr(), n, out.data_ptr(), stream_ptr()),
              'dlwpcs_rows_gather')
    return out


TIME_FILTER_MAX_TAPS = nat.TIME_FILTER_MAX_TAPS
_FILTER_MODES = {'sum': 0, 'mean': 1}
_FILTER_FORMS = {None: -1, 'streaming': 0, 'gather': 1}


def _filter_args(n_rows, n_taps, step, origin, n_out, mode, form, slab_rows):
    if mode not in _FILTER_MODES:
        raise ValueError("time_filter: mode must be 'sum' or 'mean', got %r" % (mode,))
    if form not in _FILTER_FORMS:
        raise ValueError("time_filter: form must be None, 'streaming' or 'gather', got %r" % (form,))
    step, origin = int(step), int(origin)
    if not 1 <= n_taps <= TIME_FILTER_MAX_TAPS:
        raise ValueError('time_filter: %d taps (1 .. %d)' % (n_taps, TIME_FILTER_MAX_TAPS))
    if step < 1:
        raise ValueError('time_filter: step %d' % step)
    if not 0 <= origin < n_taps:
        raise ValueError('time_filter: origin %d outside the %d taps' % (origin, n_taps))
    if n_out is None:
        n_out = max(0, (n_rows - n_taps) // step + 1)
    n_out = int(n_out)
    if n_out < 0:
        raise ValueError('time_filter: n_out %d' % n_out)
    slab = 0 if slab_rows is None else int(slab_rows)
    if slab < 0 or (slab_rows is not None and slab == 0):
        raise ValueError('time_filter: slab_rows %r' % (slab_rows,))
    return step, origin, n_out, _FILTER_MODES[mode], _FILTER_FORMS[form], slab


def time_filter_plan(shape, strides, n_taps, row_axis=0, step=1, n_out=None, mode='sum', out_perm=None, form=None, slab_rows=None,
                     aligned=True):
    """
    Which code time_filter would run for a source of this shape and these element strides (host only, no device is touched):
    dict(form = 'streaming' / 'gather', a_class = accumulators per element (gather: 0), vec = 16-byte chunks, slab_rows = output
    rows per time slab, grid).  aligned=False: as for pointers that are not on 16 bytes.  Raises what time_filter would raise.
    """
    n_rows = int(shape[row_axis])
    step, _, n_out, m, f, slab = _filter_args(n_rows, int(n_taps), step, 0, n_out, mode, form, slab_rows)
    d, _ = rows_layout(shape, strides, row_axis, out_perm, n_out)
    info = (ctypes.c_int32 * 8)()
    p = (1 << 20) if aligned else (1 << 20) + 4
    check(lib().dlwpcs_time_filter_plan_info(ctypes.byref(d), p, p, n_rows, int(n_taps), step, n_out, m, f, slab, info),
          'dlwpcs_time_filter_plan_info')
    return dict(form='gather' if info[0] else 'streaming', a_class=info[1], vec=bool(info[2]), slab_rows=info[3],
                grid=(info[4], info[5]), lds_bytes=info[6])


def time_filter(src, taps, row_axis=0, step=1, origin=0, n_out=None, mode='sum', min_weight=0., out_perm=None, form=None,
                slab_rows=None, counts=False):
    """
    A finite-impulse-response filter along `row_axis` of the fp32 device tensor `src` (any strides), in fp32 and in tap order
    (include/dlwpcs.h states the operations): output row j is the sum over k of taps[k] * src[j * step + k - origin].  A row outside
    the source and a NaN entry are missing.  mode='sum': an output with a missing entry is NaN.  mode='mean': the weighted mean of
    the entries present, NaN where their weight is below `min_weight` or none is present.  `taps`: a numpy array (checked, uploaded)
    or an fp32 device tensor (trusted: finite).  n_out: output rows, by default the windows that lie inside the source at origin 0.
    The result has src's dims in the order `out_perm` (default: unchanged) with the row axis n_out long, contiguous.  form: None =
    the library chooses, 'streaming' / 'gather' forces it; slab_rows: output rows per time slab (None = chosen): the same bits
    whatever they are.  counts=True also returns the int32 number of entries present.  One launch on the current stream, no host
    synchronisation, nothing allocated but the results.
    """
    require_device(src, 'time_filter')
    dev = src.device
    if isinstance(taps, torch.Tensor):
        if taps.dtype != torch.float32 or taps.device != dev or taps.dim() != 1 or not taps.is_contiguous():
            raise TypeError('time_filter: device taps must be a contiguous 1-d float32 tensor on the device of the source')
        h = taps
    else:
        hh = np.asarray(taps, dtype=np.float64).reshape(-1)
        h32 = np.ascontiguousarray(hh, dtype=np.float32)
        if not np.all(np.isfinite(h32)):
            raise ValueError('time_filter: the taps must be finite in float32')
        if mode == 'mean' and hh.size and not (np.all(h32 >= 0.) and float(h32.sum(dtype=np.float64)) > 0.):
            raise ValueError("time_filter: mode 'mean' needs taps >= 0 with a positive sum")
        h = None
    n_taps = int(h.numel()) if h is not None else int(hh.size)
    n_rows = int(src.shape[row_axis])
    step, origin, n_out, m, f, slab = _filter_args(n_rows, n_taps, step, origin, n_out, mode, form, slab_rows)
    d, out = _rows_desc(src, row_axis, out_perm, n_out)
    cnt = torch.empty(out.shape, dtype=torch.int32, device=dev) if counts else None
    if out.numel() == 0:
        return (out, cnt) if counts else out
    with torch.cuda.device(dev):
        if h is None:
            h = torch.from_numpy(h32).pin_memory().to(dev, non_blocking=True)
        check(lib().dlwpcs_time_filter(ctypes.byref(d), src.data_ptr(), n_rows, h.data_ptr(), n_taps, step, origin, n_out, m,
                                       float(min_weight), f, slab, out.data_ptr(), ptr(cnt), stream_ptr()), 'dlwpcs_time_filter')
    return (out, cnt) if counts else out


TIME_SPECTRUM_MAX_M = nat.TIME_SPECTRUM_MAX_M
TIME_SPECTRUM_SLAB_SEGMENTS = nat.TIME_SPECTRUM_SLAB_SEGMENTS
_windows = {}               # (window bytes, device) -> float32 device vector


def _spectrum_args(n_rows, n_segment, hop, n_freq, min_count, split, who):
    M = int(n_segment)
    if M < 2:
        raise ValueError('%s: segments of %d rows (at least 2)' % (who, M))
    if M > TIME_SPECTRUM_MAX_M:
        raise NotImplementedError('%s: segments of %d rows, the device serves 2 .. %d' % (who, M, TIME_SPECTRUM_MAX_M))
    hop = max(1, M // 2) if hop is None else int(hop)
    if hop < 1:
        raise ValueError('%s: hop %d' % (who, hop))
    K = M // 2 + 1 if n_freq is None else int(n_freq)
    if not 1 <= K <= M // 2 + 1:
        raise ValueError('%s: n_freq = %s outside 1 .. M // 2 + 1 = %d' % (who, n_freq, M // 2 + 1))
    if int(min_count) < 1:
        raise ValueError('%s: min_count %d (at least 1)' % (who, min_count))
    if split not in (None, False, True):
        raise ValueError('%s: split must be None, False or True' % who)
    n_seg = (n_rows - M) // hop + 1 if n_rows >= M else 0
    return M, hop, K, int(min_count), -1 if split is None else int(bool(split)), n_seg


def spectrum_window_host(window, M):
    """(M float32 weights, their sum of squares in float64) of a window given as None (ones) or M host values: evaluated in
    float64 by the caller, rounded to float32 once here"""
    if window is None:
        w32 = np.ones(int(M), dtype=np.float32)
    else:
        w32 = np.ascontiguousarray(np.asarray(window, dtype=np.float64).reshape(-1), dtype=np.float32)
    if w32.size != int(M):
        raise ValueError('time_spectrum: the window has %d weights, the segment %d rows' % (w32.size, M))
    sw = float((w32.astype(np.float64) ** 2).sum())
    if not np.all(np.isfinite(w32)) or not sw > 0.:
        raise ValueError('time_spectrum: the window must be finite in float32 with a positive sum of squares')
    return w32, sw


def _spectrum_window(window, M, dev):
    w32, sw = spectrum_window_host(window, M)
    key = (w32.tobytes(), str(torch.device(dev)))
    hit = _windows.get(key)
    if hit is None:
        if torch.cuda.is_current_stream_capturing():
            raise nat.NativeError('time_spectrum: first use of a window inside a graph capture (run it once eagerly first)')
        if len(_windows) >= 64:
            _windows.clear()
        hit = torch.from_numpy(w32).to(dev)
        _windows[key] = hit
    return hit, sw


def time_spectrum_plan(shape, strides, n_segment, hop=None, row_axis=0, n_freq=None, pair=False, coefficients=False, out_perm=None,
                       split=None, aligned=True):
    """
    Which launch time_spectrum (coefficients=True: time_fourier) would make for a source of this shape and these element strides
    (host only, no device is touched): dict(n_seg, col_tiles, freq_tiles, slabs, tiles = tiles of the launch, grid = persistent
    workgroups, split, vec = 16-byte loads, lds_bytes).  aligned=False: as for pointers that are not on 16 bytes.  Raises what
    the call would raise.
    """
    n_rows = int(shape[row_axis])
    M, hop, K, _, sp, n_seg = _spectrum_args(n_rows, n_segment, hop, n_freq, 1, split, 'time_spectrum')
    d, _ = rows_layout(shape, strides, row_axis, out_perm, 2 * K if coefficients else K)
    info = (ctypes.c_int64 * 8)()
    p = (1 << 20) if aligned else (1 << 20) + 4
    check(lib().dlwpcs_time_spectrum_plan_info(ctypes.byref(d), p, p if pair else None, n_rows, M, hop, K, 1 if coefficients else 0,
                                               sp, info), 'dlwpcs_time_spectrum_plan_info')
    return dict(n_seg=n_seg, col_tiles=info[0], freq_tiles=info[1], slabs=info[2], tiles=info[3], grid=info[4], split=bool(info[5]),
                vec=bool(info[6]), lds_bytes=info[7])


def time_spectrum(src, b=None, n_segment=None, hop=None, window=None, row_axis=0, detrend=False, n_freq=None, min_count=1,
                  out_perm=None, split=None, counts=False):
    """
    Welch's power spectrum along `row_axis` of the fp32 device tensor `src` (any strides): the mean over the segments of
    `n_segment` rows, `hop` rows apart (None: n_segment // 2), of P_f = c_f |X_f|^2 / (M S_w) for the first `n_freq` frequencies
    (None: all M // 2 + 1), X_f the transform of w_t (x_t - mean) (include/dlwpcs.h states the operations).  window: None (ones)
    or M host values; detrend: subtract the segment's mean per column.  A segment counts where all its values are finite; the
    result is NaN where fewer than `min_count` count.  With `b` (same shape) the pair form: a leading axis of four holds P_aa,
    P_bb, the co-spectrum and the quadrature spectrum, and a segment counts where it is finite in both.  The result has src's dims
    in the order `out_perm` (default: unchanged) with the frequencies where the row axis stood, contiguous.  split: None = the
    library chooses, True / False forces slabs of segments to have workgroups of their own (the same bits).  counts=True also
    returns the int32 number of segments that counted, without the row axis.  At most two launches on the current stream, no host
    synchronisation.
    """
    require_device(src, 'time_spectrum')
    if src.dtype != torch.float32:
        raise TypeError('time_spectrum: the source must be float32, got %s' % src.dtype)
    dev = src.device
    if b is not None:
        require_device(b, 'time_spectrum')
        if b.dtype != torch.float32 or b.device != dev or tuple(b.shape) != tuple(src.shape):
            raise TypeError('time_spectrum: the second operand must be float32 of the same shape on the same device')
        if b.stride() != src.stride():
            src, b = src.contiguous(), b.contiguous()
    n_rows = int(src.shape[row_axis])
    M, hop, K, mc, sp, n_seg = _spectrum_args(n_rows, n_rows if n_segment is None else n_segment, hop, n_freq, min_count, split,
                                              'time_spectrum')
    d, oshape = rows_layout(src.shape, src.stride(), row_axis, out_perm, K)
    nd = src.dim()
    at = (tuple(range(nd)) if out_perm is None else tuple(int(a) % nd for a in out_perm)).index(row_axis % nd)
    outer = int(np.prod(oshape))
    out = torch.empty(([4] if b is not None else []) + list(oshape), dtype=torch.float32, device=dev)
    # the counts have the layout of one frequency row: frequency 0 of an array of the result's shape
    cnt = torch.empty(oshape, dtype=torch.int32, device=dev) if counts else None
    if out.numel():
        with torch.cuda.device(dev):
            w, sw = _spectrum_window(window, M, dev)
            tw = spectrum_twiddle(M, dev)
            nbytes = int(lib().dlwpcs_time_spectrum_scratch_bytes(ctypes.byref(d), n_rows, M, hop, K, 1 if b is not None else 0, sp))
            scratch = _workspace(nbytes, dev, 'spectrum') if nbytes else None
            check(lib().dlwpcs_time_spectrum(ctypes.byref(d), src.data_ptr(), ptr(b) or None, n_rows, M, hop, w.data_ptr(),
                                             tw.data_ptr(), sw, 1 if detrend else 0, K, mc, 0, sp, outer, 0, out.data_ptr(),
                                             ptr(cnt) or None, ptr(scratch) or None, nbytes, stream_ptr()), 'dlwpcs_time_spectrum')
    return (out, cnt.select(at, 0)) if counts else out


def time_fourier(src, n_segment=None, hop=None, window=None, row_axis=0, detrend=False, n_freq=None, out_perm=None):
    """
    The transform of time_spectrum without the averaging: X_f = sum_t w_t (x_t - mean) exp(-2 pi i f t / M) per segment, unscaled.
    The result is float32 with a leading segment axis, then src's dims in the order `out_perm` with the row axis replaced by
    (frequency, 2 = Re | Im), contiguous; a segment that holds a value that is not finite is NaN in its column.  n_segment=None:
    one segment over the whole axis.  One launch on the current stream.
    """
    require_device(src, 'time_fourier')
    if src.dtype != torch.float32:
        raise TypeError('time_fourier: the source must be float32, got %s' % src.dtype)
    dev = src.device
    n_rows = int(src.shape[row_axis])
    M, hop, K, _, _, n_seg = _spectrum_args(n_rows, n_rows if n_segment is None else n_segment, hop, n_freq, 1, None, 'time_fourier')
    d, oshape = rows_layout(src.shape, src.stride(), row_axis, out_perm, 2 * K)
    nd = src.dim()
    at = (tuple(range(nd)) if out_perm is None else tuple(int(a) % nd for a in out_perm)).index(row_axis % nd)
    outer = int(np.prod(oshape))
    part = int(d.out_row_stride)
    d.out_row_stride = 2 * part
    out = torch.empty([n_seg] + list(oshape), dtype=torch.float32, device=dev)
    if out.numel():
        with torch.cuda.device(dev):
            w, sw = _spectrum_window(window, M, dev)
            tw = spectrum_twiddle(M, dev)
            check(lib().dlwpcs_time_spectrum(ctypes.byref(d), src.data_ptr(), None, n_rows, M, hop, w.data_ptr(), tw.data_ptr(), sw,
                                             1 if detrend else 0, K, 1, 1, -1, outer, part, out.data_ptr(), None, None, 0,
                                             stream_ptr()), 'dlwpcs_time_spectrum')
    return out.view([n_seg] + list(oshape[:at]) + [K, 2] + list(oshape[at + 1:]))


TIME_LAG_MAX_LAGS = nat.TIME_LAG_MAX_LAGS
TIME_LAG_SLAB_ROWS = nat.TIME_LAG_SLAB_ROWS
_LAG_FORMS = {'auto': nat.LAG_AUTO, 'pair': nat.LAG_PAIR, 'index': nat.LAG_INDEX}
_LAG_MODES = {'skip': 0, 'propagate': 1}
_LAG_MAX_BLOCK = 16


def lag_progression(lags, who='time_lag'):
    """(lag0, lag_step, n_lags) of an int sequence that is an ascending arithmetic progression; anything else: ValueError"""
    lg = np.asarray(lags)
    if lg.ndim != 1 or lg.size < 1 or lg.dtype.kind not in 'iu':
        raise ValueError('%s: lags must be a non-empty sequence of ints, got %r' % (who, lags))
    lg = lg.astype(np.int64)
    if lg.size > TIME_LAG_MAX_LAGS:
        raise ValueError('%s: %d lags (1 .. %d)' % (who, lg.size, TIME_LAG_MAX_LAGS))
    step = int(lg[1] - lg[0]) if lg.size > 1 else 1
    if step < 1 or np.any(np.diff(lg) != step):
        raise ValueError('%s: lags must be an ascending arithmetic progression, got %r' % (who, lags))
    return int(lg[0]), step, int(lg.size)


def _lag_plan_args(split, lag_block, who='time_lag'):
    if split not in (None, False, True):
        raise ValueError('%s: split must be None, False or True' % who)
    lb = 0 if lag_block is None else int(lag_block)
    if lag_block is not None and not 1 <= lb <= _LAG_MAX_BLOCK:
        raise ValueError('%s: lag_block %r outside 1 .. %d' % (who, lag_block, _LAG_MAX_BLOCK))
    return -1 if split is None else int(bool(split)), lb


def time_lag_plan(shape, strides, n_lags, lag_step=1, row_axis=0, form='auto', out_perm=None, split=None, lag_block=None, aligned=True):
    """
    Which launch time_lag would make for a source of this shape and these element strides (host only, no device is touched):
    dict(lag_block = lags per pass, passes, vec = 16-byte chunks, slabs, split, tiles = tiles of the launch, grid = persistent
    workgroups, scratch_bytes).  form: 'auto', 'pair' or 'index'.  aligned=False: as for pointers that are not on 16 bytes.
    Raises what the call would raise.
    """
    if form not in _LAG_FORMS:
        raise ValueError("time_lag: form must be 'auto', 'pair' or 'index', got %r" % (form,))
    n_lags, lag_step = int(n_lags), int(lag_step)
    if not 1 <= n_lags <= TIME_LAG_MAX_LAGS:
        raise ValueError('time_lag: %d lags (1 .. %d)' % (n_lags, TIME_LAG_MAX_LAGS))
    if lag_step < 1:
        raise ValueError('time_lag: lag_step %d' % lag_step)
    sp, lb = _lag_plan_args(split, lag_block)
    d, _ = rows_layout(shape, strides, row_axis, out_perm, n_lags)
    info = (ctypes.c_int64 * 8)()
    p = (1 << 20) if aligned else (1 << 20) + 4
    check(lib().dlwpcs_time_lag_plan_info(ctypes.byref(d), p, None if form == 'auto' else p, _LAG_FORMS[form], int(shape[row_axis]),
                                          lag_step, n_lags, sp, lb, info), 'dlwpcs_time_lag_plan_info')
    return dict(lag_block=info[0], passes=info[1], vec=info[2] == 4, slabs=info[3], split=bool(info[4]), tiles=info[5], grid=info[6],
                scratch_bytes=info[7])


def _lag_center(center, cshape, dev, what):
    if center is None:
        return None
    if not isinstance(center, torch.Tensor) or center.dtype != torch.float32 or center.device != dev or tuple(center.shape) != tuple(cshape):
        raise TypeError('time_lag: %s must be a float32 tensor of shape %s on the device of the data' % (what, tuple(cshape)))
    return center


def time_lag(a, b=None, lags=(0,), center_a=None, center_b=None, row_axis=0, missing='skip', min_count=1, out_perm=None, split=None,
             lag_block=None, counts=False):
    """
    Lagged covariances along `row_axis` of the fp32 device tensor `a` (any strides), per column and lag l: the mean over the pairs
    present of (a[t] - center_a) * (b[t + l] - center_b), a positive lag meaning that a leads (include/dlwpcs.h states the
    operations: fp32 deviations, exact fp64 products added in row order inside slabs of 512 rows, one division, one rounding).
    b: None (the auto form, b = a), a tensor of a's shape (the pair form; both are made contiguous where their strides differ) or a
    1-d tensor of T values shared by every column (the index form).  lags: ints in an ascending arithmetic progression, at most
    1024; they may be negative, and a lag beyond the series has no pairs.  center_a / center_b: None (subtract nothing) or the fp32
    one-row result of group_mean with one group and the same `out_perm`; in the index form center_b is one value; in the auto form
    center_b = None means center_a.  A NaN entry is missing.  missing='skip': NaN where fewer than max(min_count, 1) pairs are
    present; 'propagate': NaN where any pair in range has a missing entry.  The result has a's dims in the order `out_perm`
    (default: unchanged) with the lags where the row axis stood, contiguous; counts=True also returns the int32 pair counts of
    the same shape.  split: None = the library chooses, True / False forces the slabs to have workgroups of their own;
    lag_block: the lags per pass (None = chosen, at most 16): the same bits whatever they are.  At most two launches on the
    current stream, no host synchronisation.
    """
    require_device(a, 'time_lag')
    if a.dtype != torch.float32:
        raise TypeError('time_lag: the source must be float32, got %s' % a.dtype)
    if missing not in _LAG_MODES:
        raise ValueError("time_lag: missing must be 'skip' or 'propagate', got %r" % (missing,))
    if int(min_count) < 0:
        raise ValueError('time_lag: min_count %d' % min_count)
    lag0, lag_step, n_lags = lag_progression(lags)
    sp, lb = _lag_plan_args(split, lag_block)
    dev = a.device
    nd = a.dim()
    if nd < 1:
        raise ValueError('time_lag: the source has no row axis')
    row_axis = row_axis % nd
    T = int(a.shape[row_axis])
    form = 'auto'
    if b is not None:
        require_device(b, 'time_lag')
        if b.dtype != torch.float32 or b.device != dev:
            raise TypeError('time_lag: the second operand must be float32 on the device of the first')
        if tuple(b.shape) == tuple(a.shape):
            form = 'pair'
            if b.stride() != a.stride():
                a, b = a.contiguous(), b.contiguous()
        elif b.dim() == 1 and int(b.shape[0]) == T:
            form = 'index'
            b = b.contiguous()
        else:
            raise ValueError('time_lag: b %s must have the shape of a %s or be a vector of its %d rows' % (tuple(b.shape), tuple(a.shape), T))
    perm = tuple(range(nd)) if out_perm is None else tuple(int(x) % nd for x in out_perm)
    if sorted(perm) != list(range(nd)):
        raise ValueError('time_lag: out_perm %s is not a permutation of %d dims' % (out_perm, nd))
    cshape = [1 if ax == row_axis else int(a.shape[ax]) for ax in perm]
    center_a = _lag_center(center_a, cshape, dev, 'center_a')
    if form == 'index':
        if center_b is not None:
            if not isinstance(center_b, torch.Tensor):
                center_b = torch.tensor([float(center_b)], dtype=torch.float32).to(dev)
            if center_b.dtype != torch.float32 or center_b.device != dev or center_b.numel() != 1:
                raise TypeError('time_lag: in the index form center_b is one float32 value')
    else:
        center_b = _lag_center(center_b, cshape, dev, 'center_b')
        if center_a is not None and center_b is not None and center_a.stride() != center_b.stride():
            center_a, center_b = center_a.contiguous(), center_b.contiguous()
    one = center_a if center_a is not None else (center_b if form != 'index' else None)
    cstr = [0] * nd
    if one is not None:
        for pos, ax in enumerate(perm):
            cstr[ax] = int(one.stride(pos))
    d, cst, oshape = _apply_layout(tuple(a.shape), tuple(a.stride()), cstr, row_axis, out_perm, n_lags, True)
    out = torch.empty(oshape, dtype=torch.float32, device=dev)
    cnt = torch.empty(oshape, dtype=torch.int32, device=dev) if counts else None
    if out.numel():
        cs = (ctypes.c_int64 * nat.SCORE_MAX_DIMS)(*cst)
        with torch.cuda.device(dev):
            nbytes = int(lib().dlwpcs_time_lag_scratch_bytes(ctypes.byref(d), _LAG_FORMS[form], T, lag_step, n_lags, sp, lb))
            scratch = _workspace(nbytes, dev, 'time_lag') if nbytes else None
            check(lib().dlwpcs_time_lag(ctypes.byref(d), a.data_ptr() or None, ptr(b) or None, _LAG_FORMS[form], T, lag0, lag_step,
                                        n_lags, ptr(center_a) or None, ptr(center_b) or None, cs, _LAG_MODES[missing], int(min_count),
                                        sp, lb, out.data_ptr(), ptr(cnt) or None, ptr(scratch) or None, nbytes, stream_ptr()),
                  'dlwpcs_time_lag')
    return (out, cnt) if counts else out


RESAMPLE_STAGED_ROWS = nat.RESAMPLE_STAGED_ROWS
_RESAMPLE_FORMS = {None: nat.RESAMPLE_CHOOSE, 'staged': nat.RESAMPLE_STAGED, 'direct': nat.RESAMPLE_DIRECT}
_RESAMPLE_MODES = {'skip': 0, 'propagate': 1}


def _resample_args(form, splits):
    if form not in _RESAMPLE_FORMS:
        raise ValueError("row_resample: form must be None, 'staged' or 'direct', got %r" % (form,))
    sp = 0 if splits is None else int(splits)
    if splits is not None and sp < 1:
        raise ValueError('row_resample: splits %r (None or at least 1)' % (splits,))
    return _RESAMPLE_FORMS[form], sp


def _resample_counts(n_rows, block_length, n_draw):
    """(L, n_draw, nb) checked against the T rows"""
    T, L = int(n_rows), int(block_length)
    nd = T if n_draw is None else int(n_draw)
    if not 1 <= L <= max(T, 1) or T < 1:
        raise ValueError('row_resample: block_length %d of %d rows (1 .. rows)' % (L, T))
    if nd < 1:
        raise ValueError('row_resample: n_draw %d' % nd)
    return L, nd, -(-nd // L)


def row_resample_plan(shape, strides, n_resamples, n_blocks, block_length, row_axis=0, out_perm=None, form=None, aligned=True,
                      splits=None):
    """
    Which launch row_resample would make for a source of this shape and these element strides, drawing n_blocks blocks of
    block_length rows (the last one cut so that as many rows are drawn as the source has, where that fits n_blocks; else all
    blocks are whole) per resample (host only, no device is touched): dict(form = 'staged' / 'direct', tile_cols, staged_rows =
    the row cap of the staged form, grid = persistent workgroups, lds_bytes, table = block-sum table used, vec = 16-byte staging
    chunks, splits = resample ranges per column tile).  aligned=False: as for a pointer that is not on 16 bytes.  Raises what
    the call would raise.
    """
    fm, sp = _resample_args(form, splits)
    T, L, nb = int(shape[row_axis]), int(block_length), int(n_blocks)
    n_draw = T if -(-T // max(L, 1)) == nb else nb * L
    d, _ = rows_layout(shape, strides, row_axis, out_perm, int(n_resamples))
    info = (ctypes.c_int64 * 8)()
    p = (1 << 20) if aligned else (1 << 20) + 4
    check(lib().dlwpcs_row_resample_plan_info(ctypes.byref(d), p, T, int(n_resamples), nb, L, n_draw, fm, sp, info),
          'dlwpcs_row_resample_plan_info')
    return dict(form='direct' if info[0] else 'staged', tile_cols=info[1], staged_rows=info[2], grid=info[3], lds_bytes=info[4],
                table=bool(info[5]), vec=info[6] == 4, splits=info[7])


def row_resample(src, starts, block_length=1, n_draw=None, row_axis=0, missing='skip', min_count=1, out_perm=None, form=None,
                 counts=False, splits=None):
    """
    Block-bootstrap means along `row_axis` of the fp32 device tensor `src` (any strides) with T rows: resample b is the mean per
    element over the rows (starts[b, j] + i) mod T, i < block_length, block j = 0 .. nb-1 in this order, the last block cut so
    that n_draw rows (default T) are drawn; nb = ceil(n_draw / block_length) (include/dlwpcs.h states the operations: a block
    summed in row order in fp64 from zero, the block sums added in draw order, one division, one rounding).  starts: (B, nb)
    numpy ints (checked against 0 .. T-1 here and uploaded) or a contiguous int32 device tensor (trusted).  A NaN entry is
    missing.  missing='skip': NaN where fewer than max(min_count, 1) entries are present; 'propagate': NaN where any drawn entry
    is missing.  The result has src's dims in the order `out_perm` (default: unchanged) with the row axis B long, contiguous;
    counts=True also returns the int32 counts of the same shape.  form: None = the library chooses, 'staged' (the series tile by
    tile in LDS, at most RESAMPLE_STAGED_ROWS rows) or 'direct' (rows read from memory); splits: None = chosen, else the number
    of resample ranges a column tile is cut into: the same bits whatever they are.  One launch on the current stream, no host
    synchronisation.
    """
    require_device(src, 'row_resample')
    if src.dtype != torch.float32:
        raise TypeError('row_resample: the source must be float32, got %s' % src.dtype)
    if missing not in _RESAMPLE_MODES:
        raise ValueError("row_resample: missing must be 'skip' or 'propagate', got %r" % (missing,))
    if int(min_count) < 1:
        raise ValueError('row_resample: min_count %d (at least 1)' % min_count)
    fm, sp = _resample_args(form, splits)
    dev = src.device
    if src.dim() < 1:
        raise ValueError('row_resample: the source has no row axis')
    row_axis = row_axis % src.dim()
    T = int(src.shape[row_axis])
    if isinstance(starts, torch.Tensor):
        if starts.dtype != torch.int32 or starts.device != dev or not starts.is_contiguous() or starts.dim() != 2:
            raise TypeError('row_resample: device starts must be a contiguous (B, nb) int32 tensor on the device of the source')
        st_d, B, nb_given = starts, int(starts.shape[0]), int(starts.shape[1])
    else:
        sh = np.asarray(starts)
        if sh.ndim != 2 or (sh.size and sh.dtype.kind not in 'iu'):
            raise ValueError('row_resample: starts must be a (B, nb) array of ints, got shape %s %s' % (sh.shape, sh.dtype))
        if sh.size and (sh.min() < 0 or sh.max() >= T):
            raise IndexError('row_resample: block start out of range of the %d source rows' % T)
        st_d, B, nb_given = None, int(sh.shape[0]), int(sh.shape[1])
    d, oshape = rows_layout(src.shape, src.stride(), row_axis, out_perm, B)
    out = torch.empty(oshape, dtype=torch.float32, device=dev)
    cnt = torch.empty(oshape, dtype=torch.int32, device=dev) if counts else None
    if out.numel() == 0:
        return (out, cnt) if counts else out
    L, nd, nb = _resample_counts(T, block_length, n_draw)
    if nb_given != nb:
        raise ValueError('row_resample: starts has %d blocks per resample, %d draws in blocks of %d need %d' % (nb_given, nd, L, nb))
    with torch.cuda.device(dev):
        if st_d is None:
            st_d = _int32_dev(sh, dev)
        check(lib().dlwpcs_row_resample(ctypes.byref(d), src.data_ptr(), st_d.data_ptr(), T, B, nb, L, nd, _RESAMPLE_MODES[missing],
                                        int(min_count), fm, sp, out.data_ptr(), ptr(cnt) or None, stream_ptr()), 'dlwpcs_row_resample')
    return (out, cnt) if counts else out


SPELL_STATISTICS = ('n_valid', 'n_true', 'n_spells', 'spell_rows', 'longest', 'longest_start')
SPELL_SLAB_CLASSES = (32, 64, 128, 256, 512, 1024)
_SPELL_OPS = {'>': nat.SPELL_GT, '>=': nat.SPELL_GE, '<': nat.SPELL_LT, '<=': nat.SPELL_LE}
_SPELL_MODES = {'break': nat.SPELL_BREAK, 'propagate': nat.SPELL_PROPAGATE}
_SPELL_FORMS = ('statistics', 'statistics_slabs', 'rows', 'rows_slabs')


def _spell_slab(slab_rows, per_row):
    if slab_rows is None:
        return 0
    sr = int(slab_rows)
    if per_row and sr not in SPELL_SLAB_CLASSES:
        raise ValueError('time_spell: slab_rows %r with per-row outputs (None or one of %s)' % (slab_rows, SPELL_SLAB_CLASSES))
    if sr < 32 or sr % 32:
        raise ValueError('time_spell: slab_rows %r (None or a positive multiple of 32)' % (slab_rows,))
    return sr


def time_spell_plan(shape, strides, row_axis=0, out_perm=None, slab_rows=None, per_row=False, aligned=True):
    """
    Which launches time_spell would make for a source of this shape and these element strides (host only, no device is touched):
    dict(form = 'statistics' / 'statistics_slabs' / 'rows' / 'rows_slabs', slab_rows, slabs, reg_class = words of 32 rows a lane
    holds (statistics only: 0), vec = 16-byte chunks, grid = persistent workgroups, launches, scratch_bytes).  per_row: position
    or length is asked for.  The four-column chunk holds at most class 8: a larger slab is served with vec = False.
    aligned=False: as for a pointer that is not on 16 bytes.  Raises what the call would raise.
    """
    sr = _spell_slab(slab_rows, per_row)
    d, _ = rows_layout(shape, strides, row_axis, out_perm, int(shape[row_axis % len(shape)]))
    info = (ctypes.c_int64 * 8)()
    p = (1 << 20) if aligned else (1 << 20) + 4
    check(lib().dlwpcs_time_spell_plan_info(ctypes.byref(d), p, int(shape[row_axis % len(shape)]), sr, int(bool(per_row)), info),
          'dlwpcs_time_spell_plan_info')
    return dict(form=_SPELL_FORMS[info[0]], slab_rows=info[1], slabs=info[2], reg_class=info[3], vec=info[4] == 4, grid=info[5],
                launches=info[6], scratch_bytes=info[7])


def _spell_threshold(threshold, threshold_index, src, row_axis):
    """(fp32 device table, its stride per axis of src with 0 where it broadcasts, K, the int32 device index or None)"""
    dev, nd, T = src.device, src.dim(), int(src.shape[row_axis])
    if isinstance(threshold, torch.Tensor):
        if threshold.dtype != torch.float32 or threshold.device != dev:
            raise TypeError('time_spell: a tensor threshold must be float32 on the device of the source')
        th = threshold
    elif isinstance(threshold, (bool, np.bool_)) or not isinstance(threshold, (int, float, np.integer, np.floating)):
        raise TypeError('time_spell: the threshold must be a number or a float32 device tensor, got %r' % type(threshold))
    else:
        th = torch.tensor([float(threshold)], dtype=torch.float32).to(dev)
    if th.dim() > nd:
        raise ValueError('time_spell: threshold %s has more dims than the source %s' % (tuple(th.shape), tuple(src.shape)))
    th = th.reshape((1,) * (nd - th.dim()) + tuple(th.shape))
    tstr = [0] * nd
    for ax in range(nd):
        e = int(th.shape[ax])
        if ax != row_axis and e != 1 and e != int(src.shape[ax]):
            raise ValueError('time_spell: threshold %s does not broadcast against the source %s' % (tuple(th.shape), tuple(src.shape)))
        tstr[ax] = int(th.stride(ax)) if e != 1 else 0
    K = int(th.shape[row_axis])
    if K < 1:
        raise ValueError('time_spell: the threshold table has no rows')
    if threshold_index is None:
        if K != 1:
            raise ValueError('time_spell: a threshold of %d rows needs a threshold_index' % K)
        return th, tstr, K, None
    if isinstance(threshold_index, torch.Tensor):
        ti = threshold_index
        if ti.dtype != torch.int32 or ti.device != dev or not ti.is_contiguous() or tuple(ti.shape) != (T,):
            raise TypeError('time_spell: a device threshold_index must be a contiguous int32 tensor of the %d rows on the device of '
                            'the source' % T)
        return th, tstr, K, ti
    ih = np.asarray(threshold_index)
    if ih.shape != (T,) or (ih.size and ih.dtype.kind not in 'iu'):
        raise ValueError('time_spell: threshold_index must hold one int per row (%d), got shape %s %s' % (T, ih.shape, ih.dtype))
    if ih.size and (ih.min() < 0 or ih.max() >= K):
        raise IndexError('time_spell: threshold row out of range of the %d table rows' % K)
    return th, tstr, K, (_int32_dev(ih, dev) if ih.size else None)


def time_spell(src, threshold, threshold_index=None, op='>', min_length=1, row_axis=0, missing='break', out_perm=None, slab_rows=None,
               position=False, length=False, statistics=True):
    """
    Spells along `row_axis` of the fp32 device tensor `src` (any strides): per column the maximal runs of rows on which
    `src op threshold` holds (include/dlwpcs.h states the definition).  threshold: a number, or a float32 device tensor that
    broadcasts against src with K rows on the row axis; threshold_index (numpy ints, checked against 0 .. K-1 and uploaded, or a
    contiguous int32 device tensor, trusted) names the table row of every source row and may be left out for K = 1.  op: '>',
    '>=', '<' or '<='; a comparison with a NaN on either side is false and marks the entry missing.  A spell qualifies when it
    has at least `min_length` rows.  missing='break': a missing row is a false row; 'propagate': a column with any missing row
    has -1 everywhere but in n_valid.

    Returns, in this order, those asked for (one alone: not in a tuple), all int32 and contiguous in the dim order `out_perm`
    (default: src's): position (src's shape; the 1-based place inside the qualifying spell, else 0), length (src's shape; the
    length of the qualifying spell, else 0), statistics (a leading axis of the six SPELL_STATISTICS, then src's shape with the
    row axis one long).  slab_rows: None = the library chooses, else the rows of a time slab (per-row outputs: one of
    SPELL_SLAB_CLASSES; statistics only: a multiple of 32): the same integers whatever it is.  At most three launches on the
    current stream (statistics asked for together with per-row outputs behind an outer dim: one call more), no host
    synchronisation.
    """
    require_device(src, 'time_spell')
    if src.dtype != torch.float32:
        raise TypeError('time_spell: the source must be float32, got %s' % src.dtype)
    if op not in _SPELL_OPS:
        raise ValueError("time_spell: op must be '>', '>=', '<' or '<=', got %r" % (op,))
    if missing not in _SPELL_MODES:
        raise ValueError("time_spell: missing must be 'break' or 'propagate', got %r" % (missing,))
    if isinstance(min_length, bool) or not isinstance(min_length, (int, np.integer)) or int(min_length) < 1:
        raise ValueError('time_spell: min_length %r (an int of at least 1)' % (min_length,))
    per_row = bool(position or length)
    if not (per_row or statistics):
        raise ValueError('time_spell: nothing is asked for')
    sr = _spell_slab(slab_rows, per_row)
    dev = src.device
    nd = src.dim()
    if nd < 1:
        raise ValueError('time_spell: the source has no row axis')
    row_axis = row_axis % nd
    T = int(src.shape[row_axis])
    if T > nat.SPELL_MAX_ROWS:
        raise NotImplementedError('time_spell: %d rows (at most 2^31 - 1)' % T)
    th, tstr, K, ti = _spell_threshold(threshold, threshold_index, src, row_axis)
    shape, sstr = tuple(src.shape), tuple(src.stride())
    d_rows, cst_rows, oshape = _apply_layout(shape, sstr, tstr, row_axis, out_perm, T, True)
    d_stat, cst_stat, sshape = _apply_layout(shape, sstr, tstr, row_axis, out_perm, 1, True)
    perm = tuple(range(nd)) if out_perm is None else tuple(int(a) % nd for a in out_perm)
    pos = torch.empty(oshape, dtype=torch.int32, device=dev) if position else None
    ln = torch.empty(oshape, dtype=torch.int32, device=dev) if length else None
    stats = torch.empty([nat.SPELL_STATS] + sshape, dtype=torch.int32, device=dev) if statistics else None
    n_col = int(np.prod(sshape, dtype=np.int64))
    if T == 0 or n_col == 0:
        if stats is not None:
            stats.zero_()
            stats[5].fill_(-1)
    else:
        def run(d, cst, p, l, s):
            want = int(p is not None or l is not None)
            slab = sr if want or not per_row else 0         # (a class forced for the rows says nothing about the statistics' own call)
            nbytes = int(lib().dlwpcs_time_spell_scratch_bytes(ctypes.byref(d), src.data_ptr(), T, slab, want))
            scratch = _workspace(nbytes, dev, 'time_spell') if nbytes else None
            cs = (ctypes.c_int64 * nat.SCORE_MAX_DIMS)(*cst)
            check(lib().dlwpcs_time_spell(ctypes.byref(d), src.data_ptr(), T, th.data_ptr(), tstr[row_axis], cs, ptr(ti) or None,
                                          _SPELL_OPS[op], int(min_length), _SPELL_MODES[missing], slab, ptr(p) or None, ptr(l) or None, ptr(s) or None, n_col,
                                          ptr(scratch) or None, nbytes, stream_ptr()), 'dlwpcs_time_spell')
        with torch.cuda.device(dev):
            if not per_row:
                run(d_stat, cst_stat, None, None, stats)
            elif stats is None or perm[0] == row_axis:
                run(d_rows, cst_rows, pos, ln, stats)       # (the row axis outermost: one output row has the strides of T of them)
            else:
                run(d_rows, cst_rows, pos, ln, None)
                run(d_stat, cst_stat, None, None, stats)
    res = tuple(r for r in (pos, ln, stats) if r is not None)
    return res[0] if len(res) == 1 else res


RANK_STATISTICS = ('n_valid', 'concordant', 'discordant', 'tie_a', 'tie_b', 'tie_both', 'tie3_a', 'tie3_b')
RANK_MAX_ROWS = nat.RANK_MAX_ROWS
# the row caps of the staged tiles, smallest first (the pair form holds two tiles: half of each)
RANK_STAGE_ROWS = (nat.RANK_STAGE_ROWS_SMALL, nat.RANK_STAGE_ROWS_64, nat.RANK_STAGE_ROWS_32, nat.RANK_STAGE_ROWS_16)
_RANK_FORMS = {None: 0, 'staged': 1, 'direct': 2}
_RANK_KINDS = {'trend': nat.RANK_TREND, 'pair': nat.RANK_PAIR, 'index': nat.RANK_INDEX}
_RANK_MODES = {'skip': nat.RANK_SKIP, 'propagate': nat.RANK_PROPAGATE}


def _rank_args(form, splits):
    if form not in _RANK_FORMS:
        raise ValueError("time_rank: form must be None, 'staged' or 'direct', got %r" % (form,))
    sp = 0 if splits is None else int(splits)
    if splits is not None and sp < 1:
        raise ValueError('time_rank: splits %r (None or at least 1)' % (splits,))
    return _RANK_FORMS[form], sp


def time_rank_plan(shape, strides, kind='trend', row_axis=0, out_perm=None, per_row=False, form=None, splits=None, aligned=True):
    """
    Which launch time_rank would make for a source of this shape and these element strides (host only, no device is touched):
    dict(form = 'staged' / 'direct', tile_cols, tile_rows = the row cap of the staged tile (direct: 0), vec = 16-byte staging
    chunks, splits = workgroups that share a column tile, grid = workgroups, launches, scratch_bytes).  kind: 'trend', 'pair' or
    'index'; per_row: the launch of the ranks, else that of the statistics.  aligned=False: as for pointers that are not on 16
    bytes.  Raises what the call would raise.
    """
    if kind not in _RANK_KINDS:
        raise ValueError("time_rank: kind must be 'trend', 'pair' or 'index', got %r" % (kind,))
    fm, sp = _rank_args(form, splits)
    T = int(shape[row_axis % len(shape)])
    d, _ = rows_layout(shape, strides, row_axis, out_perm, T if per_row else 1)
    info = (ctypes.c_int64 * 8)()
    p = (1 << 20) if aligned else (1 << 20) + 4
    check(lib().dlwpcs_time_rank_plan_info(ctypes.byref(d), p, None if kind == 'trend' else p, _RANK_KINDS[kind], T, int(bool(per_row)),
                                           fm, sp, info), 'dlwpcs_time_rank_plan_info')
    return dict(form={0: None, 1: 'staged', 2: 'direct'}[info[0]], tile_cols=info[1], tile_rows=info[2], vec=info[3] == 4,
                splits=info[4], grid=info[5], launches=info[6], scratch_bytes=info[7])


def time_rank(a, b=None, row_axis=0, missing='skip', ranks=False, stats=True, out_perm=None, form=None, splits=None):
    """
    Rank statistics along `row_axis` of the fp32 device tensor `a` (any strides; include/dlwpcs.h states the definition).  b: None
    (the trend form: the partner of a row is its number), a tensor of a's shape (the pair form; both are made contiguous where their
    strides differ) or a 1-d tensor of T values shared by every column (the index form).  A row is present when a, and b where
    there is one, is not NaN; missing='skip' counts over the present rows, 'propagate' gives a column with any missing row NaN
    ranks and -1 in every statistic but n_valid.

    Returns, in this order, those asked for (one alone: not in a tuple), contiguous in the dim order `out_perm` (default: a's):
    rank_a (ranks=True; fp32 mid-ranks, a's shape), rank_b (ranks=True with a b), stats (stats=True; int64, a leading axis of the
    eight RANK_STATISTICS, then a's shape with the row axis one long).  form: None = the library chooses, 'staged' (the column
    tile in LDS, up to RANK_STAGE_ROWS[-1] rows, half of that in the pair form) or 'direct'; splits: None = chosen, else the
    workgroups that share a column tile: the same integers whatever they are.  At most three launches on the current stream (ranks
    together with statistics behind an outer dim: one call more), no host synchronisation.
    """
    require_device(a, 'time_rank')
    if a.dtype != torch.float32:
        raise TypeError('time_rank: the source must be float32, got %s' % a.dtype)
    if missing not in _RANK_MODES:
        raise ValueError("time_rank: missing must be 'skip' or 'propagate', got %r" % (missing,))
    if not (ranks or stats):
        raise ValueError('time_rank: nothing is asked for')
    fm, sp = _rank_args(form, splits)
    dev, nd = a.device, a.dim()
    if nd < 1:
        raise ValueError('time_rank: the source has no row axis')
    row_axis = row_axis % nd
    T = int(a.shape[row_axis])
    if T > RANK_MAX_ROWS:
        raise NotImplementedError('time_rank: %d rows (at most %d)' % (T, RANK_MAX_ROWS))
    kind = 'trend'
    if b is not None:
        require_device(b, 'time_rank')
        if b.dtype != torch.float32 or b.device != dev:
            raise TypeError('time_rank: the second operand must be float32 on the device of the first')
        if tuple(b.shape) == tuple(a.shape):
            kind = 'pair'
            if b.stride() != a.stride():
                a, b = a.contiguous(), b.contiguous()
        elif b.dim() == 1 and int(b.shape[0]) == T:
            kind = 'index'
            b = b.contiguous()
        else:
            raise ValueError('time_rank: b %s must have the shape of a %s or be a vector of its %d rows' % (tuple(b.shape), tuple(a.shape), T))
    perm = tuple(range(nd)) if out_perm is None else tuple(int(x) % nd for x in out_perm)
    d_rows, oshape = rows_layout(a.shape, a.stride(), row_axis, out_perm, T)
    d_stat, sshape = rows_layout(a.shape, a.stride(), row_axis, out_perm, 1)
    ra = torch.empty(oshape, dtype=torch.float32, device=dev) if ranks else None
    rb = torch.empty(oshape, dtype=torch.float32, device=dev) if ranks and kind != 'trend' else None
    st = torch.empty([nat.RANK_STATS] + sshape, dtype=torch.int64, device=dev) if stats else None
    n_col = int(np.prod(sshape, dtype=np.int64))
    if T == 0 or n_col == 0:
        if st is not None:
            st.zero_()
    else:
        def run(d, pa, pb, s):
            nbytes = 0
            if s is not None:
                nbytes = int(lib().dlwpcs_time_rank_scratch_bytes(ctypes.byref(d), a.data_ptr(), ptr(b) or None, _RANK_KINDS[kind], T, 0,
                                                                  fm, sp))
            scratch = _workspace(nbytes, dev, 'time_rank') if nbytes else None
            check(lib().dlwpcs_time_rank(ctypes.byref(d), a.data_ptr(), ptr(b) or None, _RANK_KINDS[kind], T, _RANK_MODES[missing], fm, sp,
                                         ptr(pa) or None, ptr(pb) or None, ptr(s) or None, n_col, ptr(scratch) or None, nbytes,
                                         stream_ptr()), 'dlwpcs_time_rank')
        with torch.cuda.device(dev):
            if not ranks:
                run(d_stat, None, None, st)
            elif st is None or perm[0] == row_axis:
                run(d_rows, ra, rb, st)                     # (the row axis outermost: one output row has the strides of T of them)
            else:
                run(d_rows, ra, rb, None)
                run(d_stat, None, None, st)
    res = tuple(r for r in (ra, rb, st) if r is not None)
    return res[0] if len(res) == 1 else res


ROW_GRAM_SLAB_COLS = nat.ROW_GRAM_SLAB_COLS
ROW_GRAM_GROUP_SLABS = nat.ROW_GRAM_GROUP_SLABS


def _gram_split(split):
    if split not in (None, False, True):
        raise ValueError('row_gram: split must be None, False or True')
    return -1 if split is None else int(bool(split))


def _gram_same_columns(da, db):
    n = da.n_inner
    return db.n_inner == n and all(da.inner_ext[i] == db.inner_ext[i] and da.out_stride[i] == db.out_stride[i] for i in range(n))


def row_gram_plan(shape, strides, n_rows_b=None, row_axis=0, split=None, aligned=True):
    """
    Which launch row_gram would make for a source of this shape and these element strides (host only, no device is touched);
    n_rows_b: the cross form against that many rows laid out like the source.  dict(row_tiles_a, row_tiles_b, tile_pairs, slabs,
    groups, split, vec = 16-byte loads, grid = workgroups of the product launch).  aligned=False: as for pointers that are not
    on 16 bytes.  Raises what the call would raise.
    """
    sp = _gram_split(split)
    d, _ = rows_layout(shape, strides, row_axis, None, 1)
    info = (ctypes.c_int64 * 8)()
    p = (1 << 20) if aligned else (1 << 20) + 4
    cross = n_rows_b is not None
    check(lib().dlwpcs_row_gram_plan_info(ctypes.byref(d), p, int(shape[row_axis]), ctypes.byref(d) if cross else None,
                                          p if cross else None, int(n_rows_b) if cross else 0, sp, info), 'dlwpcs_row_gram_plan_info')
    return dict(row_tiles_a=info[0], row_tiles_b=info[1], tile_pairs=info[2], slabs=info[3], groups=info[4], split=bool(info[5]),
                vec=bool(info[6]), grid=info[7])


def _gram_center(center, cshape, dev, who):
    """(mode, given mean or None) of a centring argument: False, True or an fp32 device tensor that broadcasts to the columns"""
    if center is False or center is None:
        return 0, None
    if center is True:
        return 1, None
    if not isinstance(center, torch.Tensor) or center.dtype != torch.float32 or center.device != dev:
        raise TypeError('%s: a given mean must be a float32 tensor on the device of the data' % who)
    return 2, center.expand(cshape).contiguous()


def row_gram(a, b=None, weight_root=None, row_axis=0, center=True, center_b=None, split=None, counts=False, mean=False):
    """
    The Gram matrix between the rows along `row_axis` of the fp32 device tensor `a` (any strides) and those of `b` (None: of `a`
    itself, the symmetric form): out[s, t] = sum over the columns of y_a[s] y_b[t], y = r (x - mean), as a (Ta, Tb) float64
    device tensor (include/dlwpcs.h states the operations and the summation order).  `b` has a's shape but for the row axis and
    a's order of dims in memory.  weight_root: None (ones) or an fp32 device tensor that broadcasts to a's shape without the row
    axis: the root of the weights, it goes on both operands.  center / center_b (None: as center): True = the operand's own mean
    over its rows, False = none, or a tensor = that mean.  A column with a value that is not finite in either operand or in the
    weight root, or a NaN in a given mean, is excluded.  split: None = the library chooses, True / False forces the groups of
    columns to have workgroups of their own (the same bits).  counts=True also returns the number of columns kept (an int64 device
    scalar), mean=True the fp32 mean subtracted from `a` per column (NaN at an excluded column).  At most three launches on the
    current stream, no host synchronisation.
    """
    require_device(a, 'row_gram')
    if a.dtype != torch.float32:
        raise TypeError('row_gram: the source must be float32, got %s' % a.dtype)
    dev = a.device
    nd = a.dim()
    if nd < 1:
        raise ValueError('row_gram: the source has no row axis')
    row_axis = row_axis % nd
    sp = _gram_split(split)
    cshape = tuple(a.shape[:row_axis]) + tuple(a.shape[row_axis + 1:])
    Ta = int(a.shape[row_axis])
    da, _ = rows_layout(a.shape, a.stride(), row_axis, None, 1)
    db, Tb = None, Ta
    if b is not None:
        require_device(b, 'row_gram')
        if b.dtype != torch.float32 or b.device != dev or b.dim() != nd or \
                tuple(b.shape[:row_axis]) + tuple(b.shape[row_axis + 1:]) != cshape:
            raise ValueError('row_gram: b %s must be float32 on the device of a with the shape of a %s but for axis %d'
                             % (tuple(b.shape), tuple(a.shape), row_axis))
        Tb = int(b.shape[row_axis])
        db, _ = rows_layout(b.shape, b.stride(), row_axis, None, 1)
        if not _gram_same_columns(da, db):
            raise ValueError('row_gram: a and b walk their columns differently (strides %s and %s): lay b out in memory like a'
                             % (tuple(a.stride()), tuple(b.stride())))
    ca, ga = _gram_center(center, cshape, dev, 'row_gram')
    cb, gb = (ca, ga) if center_b is None else _gram_center(center_b, cshape, dev, 'row_gram')
    if weight_root is not None:
        if not isinstance(weight_root, torch.Tensor) or weight_root.dtype != torch.float32 or weight_root.device != dev:
            raise TypeError('row_gram: weight_root must be a float32 tensor on the device of the data')
        weight_root = weight_root.expand(cshape).contiguous()
    out = torch.empty((Ta, Tb), dtype=torch.float64, device=dev)
    nv = torch.zeros((), dtype=torch.int64, device=dev) if counts else None
    mu = torch.full(cshape, float('nan'), dtype=torch.float32, device=dev) if mean else None
    if out.numel():
        with torch.cuda.device(dev):
            nbytes = int(lib().dlwpcs_row_gram_scratch_bytes(ctypes.byref(da), Ta, ctypes.byref(db) if db is not None else None, Tb, sp))
            scratch = _workspace(nbytes, dev, 'row_gram')
            # (b == NULL means the symmetric form: a b without columns, whose pointer torch leaves null, still reads as the cross form)
            check(lib().dlwpcs_row_gram(ctypes.byref(da), a.data_ptr() or None, Ta, ctypes.byref(db) if db is not None else None,
                                        None if b is None else (b.data_ptr() or 4), Tb, ptr(weight_root) or None, ca, ptr(ga) or None,
                                        cb, ptr(gb) or None, sp, out.data_ptr(), Tb, ptr(mu) or None, ptr(nv) or None,
                                        scratch.data_ptr(), nbytes, stream_ptr()), 'dlwpcs_row_gram')
    res = (out,) + ((nv,) if counts else ()) + ((mu,) if mean else ())
    return res if len(res) > 1 else out


REGRESSION_MAX_TERMS = nat.REGRESSION_MAX_TERMS
_FIT_MODES ={'skip': 0, 'propagate': 1}
_FIT_FORMS = {None: -1, False: 0, True: 1}


def _fit_basis(basis, n_rows, dev, who):
    """(device tensor or None, float32 host array or None, K) of a (T, K) basis: numpy values are checked and rounded to float32,
    a device tensor is trusted"""
    if isinstance(basis, torch.Tensor):
        if basis.dtype != torch.float32 or basis.device != dev or basis.dim() != 2 or not basis.is_contiguous():
            raise TypeError('%s: a device basis must be a contiguous (T, K) float32 tensor on the device of the data' % who)
        b, b32, shape = basis, None, tuple(basis.shape)
    else:
        bh = np.asarray(basis, dtype=np.float64)
        if bh.ndim != 2:
            raise ValueError('%s: the basis must be (T, K), got %d dims' % (who, bh.ndim))
        with np.errstate(over='ignore'):
            b32 = np.ascontiguousarray(bh, dtype=np.float32)
        if not np.all(np.isfinite(b32)):
            raise ValueError('%s: the basis must be finite in float32' % who)
        b, shape = None, b32.shape
    if not 1 <= shape[1] <= REGRESSION_MAX_TERMS:
        raise ValueError('%s: %d terms (1 .. %d)' % (who, shape[1], REGRESSION_MAX_TERMS))
    if shape[0] != n_rows:
        raise ValueError('%s: the basis has %d rows, the data %d' % (who, shape[0], n_rows))
    return b, b32, int(shape[1])


def _fit_args(n_terms, missing, min_count, pivot_tol, slab_rows, split, gram):
    if missing not in _FIT_MODES:
        raise ValueError("time_regression: missing must be 'skip' or 'propagate', got %r" % (missing,))
    if split not in _FIT_FORMS or gram not in _FIT_FORMS:
        raise ValueError('time_regression: split and gram must be None, False or True')
    mc = n_terms if min_count is None else int(min_count)
    if mc < n_terms:
        raise ValueError('time_regression: min_count %d below the %d terms' % (mc, n_terms))
    tol = 0. if pivot_tol is None else float(pivot_tol)
    if not 0. <= tol < 1.:
        raise ValueError('time_regression: pivot_tol %r outside [0, 1)' % (pivot_tol,))
    slab = 0 if slab_rows is None else int(slab_rows)
    if slab < 0 or (slab_rows is not None and slab == 0):
        raise ValueError('time_regression: slab_rows %r' % (slab_rows,))
    return _FIT_MODES[missing], mc, tol, slab, _FIT_FORMS[split], _FIT_FORMS[gram]


def time_regression_plan(shape, strides, n_terms, row_axis=0, out_perm=None, slab_rows=None, split=None, gram=None, aligned=True):
    """
    Which code time_regression would run for a source of this shape and these element strides (host only, no device is touched):
    dict(split, gram = every column its own G, k_class = the term class, chunk = elements per lane, grid, lds_bytes, slab_rows).
    aligned=False: as for pointers that are not on 16 bytes.  Raises what time_regression would raise.
    """
    n_terms = int(n_terms)
    if not 1 <= n_terms <= REGRESSION_MAX_TERMS:
        raise ValueError('time_regression: %d terms (1 .. %d)' % (n_terms, REGRESSION_MAX_TERMS))
    m, mc, _, slab, sp, gr = _fit_args(n_terms, 'skip', None, None, slab_rows, split, gram)
    d, _ = rows_layout(shape, strides, row_axis, out_perm, n_terms)
    info = (ctypes.c_int32 * 8)()
    p = (1 << 20) if aligned else (1 << 20) + 4
    check(lib().dlwpcs_time_regression_plan_info(ctypes.byref(d), p, p, int(shape[row_axis]), n_terms, m, mc, slab, sp, gr,
                                                 d.out_row_stride, info), 'dlwpcs_time_regression_plan_info')
    return dict(split=bool(info[0]), gram=bool(info[1]), k_class=info[2], chunk=info[3], grid=(info[4], info[5]), lds_bytes=info[6],
                slab_rows=info[7])


def time_regression(src, basis, row_axis=0, missing='skip', min_count=None, pivot_tol=None, out_perm=None, slab_rows=None, split=None,
                    gram=None, counts=False):
    """
    The least-squares coefficients of the (T, K) `basis` along `row_axis` of the fp32 device tensor `src` (any strides), per
    element, over the rows that are not NaN: fp64 normal equations in a fixed order, factorised without a square root
    (include/dlwpcs.h states the operations).  missing='skip': fitted to the rows present; 'propagate': an element with a missing
    row is NaN.  An element with fewer than `min_count` rows present (None: K), a singular system (a pivot below `pivot_tol` times
    its diagonal entry, None: 2^-40) or a coefficient that is not finite is NaN in all K terms.  `basis`: a numpy array (checked,
    rounded to float32 once: the coefficients belong to the rounded basis) or an fp32 device tensor (trusted: finite).  The result
    has src's dims in the order `out_perm` (default: unchanged) with K terms where the row axis stood, contiguous.  split / gram:
    None = the library chooses, True / False forces the two-launch slab form / an own normal matrix for every column;
    slab_rows: rows per slab of the summation order (None: 512, part of the definition).  The same bits whatever split and gram
    are.  counts=True also returns the int32 number of rows present, without the row axis.  Four launches on the current stream
    (two of them one small workgroup or one per slab), no host synchronisation.
    """
    require_device(src, 'time_regression')
    dev = src.device
    n_rows = int(src.shape[row_axis])
    b, b32, K = _fit_basis(basis, n_rows, dev, 'time_regression')
    m, mc, tol, slab, sp, gr = _fit_args(K, missing, min_count, pivot_tol, slab_rows, split, gram)
    d, out = _rows_desc(src, row_axis, out_perm, K)
    at = (tuple(range(src.dim())) if out_perm is None else tuple(int(a) % src.dim() for a in out_perm)).index(row_axis % src.dim())
    # the counts have the layout of one term: term 0 of an array of the coefficients' shape
    cnt = torch.empty(out.shape, dtype=torch.int32, device=dev) if counts else None
    if out.numel():
        with torch.cuda.device(dev):
            if b is None:
                b = torch.from_numpy(b32).pin_memory().to(dev, non_blocking=True)
            nbytes = int(lib().dlwpcs_time_regression_scratch_bytes(ctypes.byref(d), n_rows, K, slab, sp))
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            check(lib().dlwpcs_time_regression(ctypes.byref(d), src.data_ptr(), n_rows, b.data_ptr(), K, m, mc, tol, slab, sp, gr,
                                               out.data_ptr(), d.out_row_stride, ptr(cnt), ptr(scratch), nbytes, stream_ptr()),
                  'dlwpcs_time_regression')
    return (out, cnt.select(at, 0)) if counts else out


def time_regression_apply(coef, basis, src=None, term_axis=0, row_axis=None, out_perm=None):
    """
    The fitted values sum_k basis[r, k] * coef[k] for every row r of the (R, K) `basis` (src=None), or the residuals src - fitted,
    in fp64 rounded to fp32 once.  `coef`: an fp32 device tensor with K terms along `term_axis` (any strides); `src`: an fp32 device
    tensor with R rows along `row_axis` (None: term_axis) and coef's other dims in coef's order.  NaN where a coefficient of the
    element or the source is NaN.  R need not be the length of the fit.  The result has the dims of `src` (of coef, with R rows
    where the terms stood) in the order `out_perm`, contiguous.  One launch on the current stream.
    """
    require_device(coef, 'time_regression_apply')
    if coef.dtype != torch.float32:
        raise TypeError('time_regression_apply: the coefficients must be float32, got %s' % coef.dtype)
    dev = coef.device
    nd = coef.dim()
    term_axis = term_axis % nd
    row_axis = term_axis if row_axis is None else row_axis % nd
    n_rows = int(src.shape[row_axis]) if src is not None else int(np.shape(basis)[0])
    b, b32, K = _fit_basis(basis, n_rows, dev, 'time_regression_apply')
    if int(coef.shape[term_axis]) != K:
        raise ValueError('time_regression_apply: %d coefficients along axis %d, the basis has %d terms' % (coef.shape[term_axis], term_axis, K))
    crest = [a for a in range(nd) if a != term_axis]
    if src is not None:
        require_device(src, 'time_regression_apply')
        if src.dtype != torch.float32 or src.device != dev:
            raise TypeError('time_regression_apply: the source must be float32 on the device of the coefficients')
        srest = [a for a in range(nd) if a != row_axis]
        if src.dim() != nd or [src.shape[a] for a in srest] != [coef.shape[a] for a in crest] or int(src.shape[row_axis]) != n_rows:
            raise ValueError('time_regression_apply: the source %s does not match the coefficients %s' % (tuple(src.shape), tuple(coef.shape)))
        shape, sstr = tuple(src.shape), tuple(src.stride())
    else:
        srest = crest
        row_axis = term_axis
        shape = tuple(n_rows if a == term_axis else int(coef.shape[a]) for a in range(nd))
        sstr = (0,) * nd
    cstr = [0] * nd
    for sa, ca in zip(srest, crest):
        cstr[sa] = int(coef.stride(ca))
    d, cst, oshape = _apply_layout(shape, sstr, cstr, row_axis, out_perm, n_rows, src is not None)
    out = torch.empty(oshape, dtype=torch.float32, device=dev)
    if out.numel():
        cs = (ctypes.c_int64 * nat.SCORE_MAX_DIMS)(*cst)
        with torch.cuda.device(dev):
            if b is None:
                b = torch.from_numpy(b32).pin_memory().to(dev, non_blocking=True)
            check(lib().dlwpcs_time_regression_apply(ctypes.byref(d), ptr(src), n_rows, b.data_ptr(), K, coef.data_ptr(),
                                                     int(coef.stride(term_axis)), cs, 0 if src is None else 1, out.data_ptr(), stream_ptr()),
                  'dlwpcs_time_regression_apply')
    return out


def _apply_layout(shape, sstr, cstr, row_axis, out_perm, n_out, has_src):
    """rows_layout with a third operand: (descriptor of source and output, the coefficients' stride per inner dim, output shape).
    Neighbours merge where source, coefficients and output all allow it; the dim that is contiguous in the source (without one:
    in the output) goes last."""
    nd = len(shape)
    perm = tuple(range(nd)) if out_perm is None else tuple(int(a) % nd for a in out_perm)
    if sorted(perm) != list(range(nd)):
        raise ValueError('rows: out_perm %s is not a permutation of %d dims' % (out_perm, nd))
    oshape = [n_out if a == row_axis else int(shape[a]) for a in perm]
    ostride, run = [0] * nd, 1
    for pos in range(nd - 1, -1, -1):
        ostride[pos] = run
        run *= max(oshape[pos], 1)
    at = perm.index(row_axis)
    dims = [(e, st) for e, st, _ in
            merge_dims((int(shape[a]), (int(sstr[a]), int(cstr[a]), ostride[pos]), pos > at) for pos, a in enumerate(perm) if a != row_axis)]
    unit = [i for i, x in enumerate(dims) if x[1][0 if has_src else 2] == 1]
    if unit:
        dims.append(dims.pop(unit[-1]))
    if len(dims) > nat.SCORE_MAX_DIMS:
        raise NotImplementedError('rows: more than %d inner dims after merging' % nat.SCORE_MAX_DIMS)
    d = nat.RowsDesc()
    d.n_inner = len(dims)
    d.src_row_stride, d.out_row_stride = int(sstr[row_axis]), ostride[at]
    cst = [0] * nat.SCORE_MAX_DIMS
    for i, (e, st) in enumerate(dims):
        d.inner_ext[i], d.src_stride[i], cst[i], d.out_stride[i] = e, st[0], st[1], st[2]
    return d, cst, oshape


QUANTILE_MAX_PROBS = nat.QUANTILE_MAX_PROBS


def _probs(probs, who):
    p = np.ascontiguousarray(np.asarray(probs, dtype=np.float64).reshape(-1))
    if not 1 <= p.size <= QUANTILE_MAX_PROBS:
        raise ValueError('%s: %d probabilities (1 .. %d)' % (who, p.size, QUANTILE_MAX_PROBS))
    if not np.all((p >= 0.) & (p <= 1.)):
        raise ValueError('%s: probabilities %s outside [0, 1]' % (who, p[~((p >= 0.) & (p <= 1.))]))
    return p


def group_quantile_plan(shape, strides, n_groups, max_group_rows, n_probs, row_axis=0, out_perm=None):
    """
    Which code group_quantile would run for a source of this shape and these element strides (host only, no device is touched):
    dict(form = 'staged' / 'long', rows, lanes = the class (long: 0 rows, the threads of a workgroup), p_class = probability
    slots of the instantiation, grid, lds_bytes).  Raises what group_quantile would raise for these counts.
    """
    d, _ = rows_layout(shape, strides, row_axis, out_perm, n_groups)
    info = (ctypes.c_int32 * 8)()
    check(lib().dlwpcs_group_quantile_plan_info(ctypes.byref(d), 1 << 20, int(n_groups), int(max_group_rows), int(n_probs), info),
          'dlwpcs_group_quantile_plan_info')
    return dict(form='long' if info[0] else 'staged', rows=info[1], lanes=info[2], p_class=info[3], grid=(info[4], info[5]),
                lds_bytes=info[6])


def group_quantile(src, group_start, row_index, probs, row_axis=0, out_perm=None, counts=False):
    """
    Per-element quantiles over groups of rows of the fp32 device tensor `src` (any strides): group k holds the rows
    row_index[group_start[k]:group_start[k + 1]] of `row_axis` (numpy int arrays in CSR form, checked here and uploaded), `probs`
    up to 16 probabilities in [0, 1].  NaN entries are no members; an element with no member left is NaN.  numpy's default
    ('linear') quantile, interpolated in fp64 and rounded to fp32 once (include/dlwpcs.h states the operations).  The result has
    a leading dim len(probs), then src's dims in the order `out_perm` (default: unchanged) with the row axis K long, contiguous.
    counts=True also returns the int32 member counts (one slice).  One launch on the current stream, no host synchronisation.
    """
    p = _probs(probs, 'group_quantile')
    gs = np.asarray(group_start, dtype=np.int64).reshape(-1)
    ri = np.asarray(row_index, dtype=np.int64).reshape(-1)
    if gs.size < 1 or gs[0] != 0 or np.any(np.diff(gs) < 0) or gs[-1] != ri.size:
        raise ValueError('group_quantile: group_start must rise from 0 to len(row_index)')
    n_rows = int(src.shape[row_axis])
    if ri.size and (ri.min() < 0 or ri.max() >= n_rows):
        raise IndexError('group_quantile: row index out of range of the %d source rows' % n_rows)
    K = gs.size - 1
    require_device(src, 'group_quantile')
    if src.dtype != torch.float32:
        raise TypeError('group_quantile: the source must be float32, got %s' % src.dtype)
    d, oshape = rows_layout(src.shape, src.stride(), row_axis, out_perm, K)
    out = torch.empty([p.size] + oshape, dtype=torch.float32, device=src.device)
    cnt = torch.empty(oshape, dtype=torch.int32, device=src.device) if counts else None
    if K == 0 or out.numel() == 0:
        return (out, cnt) if counts else out
    longest = int(np.diff(gs).max())
    dev = src.device
    with torch.cuda.device(dev):
        gs_d, ri_d = _int32_dev(gs, dev), _int32_dev(ri if ri.size else np.zeros(1), dev)
        check(lib().dlwpcs_group_quantile(ctypes.byref(d), src.data_ptr(), gs_d.data_ptr(), ri_d.data_ptr(), K, longest,
                                          p.ctypes.data, p.size, out.data_ptr(), int(out.stride(0)), ptr(cnt), stream_ptr()),
              'dlwpcs_group_quantile')
    return (out, cnt) if counts else out


# ------------------------------------------------------------------------------------------------------------------ #
# Offline-map remapping (DLWP/remap): one sparse matrix over a strided stack of fields, include/dlwpcs.h dlwpcs_sparse_map_apply
# ------------------------------------------------------------------------------------------------------------------ #

def _space_stride(shape, strides):
    """the one stride of the consecutive space dims, or None when they are not one evenly strided run"""
    run = [(int(e), int(s)) for e, s in zip(shape, strides) if int(e) != 1]
    for (e0, s0), (e1, s1) in zip(run[:-1], run[1:]):
        if s0 != s1 * e1:
            return None
    return run[-1][1] if run else 1


def sparse_map_apply(m, x, space_axes, out=None, skipna=False, min_valid=0.5, renormalize=True, frac_out=None):
    """
    y = m applied to the source grid in the consecutive `space_axes` of the fp32 / bf16 device tensor x (DLWP.remap.OfflineMap;
    the axes hold m.src_shape, or one axis of m.n_a cells), which the result replaces with m.dst_shape.  One launch on the
    current stream, no host synchronisation.  `out`: a float32 tensor or view of the result's shape to write into (e.g. a
    permuted channels_last buffer); otherwise a new contiguous fp32 tensor is returned.

    skipna=True (dlwpcs_sparse_map_apply_masked; the other keywords need it): a NaN in x is a missing value and is left out of
    its rows' sums.  An output with holes among its entries is NaN when the weight of its present entries is below `min_valid`
    (in [0, 1]; 0.5: the majority of the row) of the row's weight, when none is present, or when min_valid is 1; otherwise it
    is the sum over the present entries, scaled by (row weight / present weight) with `renormalize`.  Where nothing is missing
    the result has the bits of the plain launch.  `frac_out`: a float32 tensor or view of the result's shape that receives
    the present share of every output's weight (1 where nothing is missing, 0 for a row without entries), or True to allocate
    it; with it the return value is (y, frac).  The map must hold no negative weight.

    Views are read and written in place through their strides: after merging, the dim of smallest output stride is the inner
    dim of the descriptor (lanes span it) when x is also denser along it than along the space axis, and the other dims are up
    to three outer dims.  Only a layout that cannot be described so -- space axes that are not one evenly strided run, or more
    than three outer dims -- is copied: x with .contiguous(), and the result through a contiguous temporary that is copied
    into `out`.
    """
    require_device(x, 'sparse_map_apply')
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError('sparse_map_apply: x must be float32 or bfloat16, got %s' % x.dtype)
    if not skipna and frac_out is not None and frac_out is not False:
        raise ValueError('sparse_map_apply: frac_out needs skipna=True')
    if skipna:
        m.check_skipna(min_valid)
    a0, a1 = m._space(tuple(x.shape), space_axes)
    dev = x.device
    row_ptr, col, val = m.to(dev)
    shape = tuple(x.shape[:a0]) + tuple(m.dst_shape) + tuple(x.shape[a1:])
    b1 = a0 + len(m.dst_shape)

    def result(t, name):
        if t is None or t is True:
            return torch.empty(shape, dtype=torch.float32, device=dev)
        require_device(t, 'sparse_map_apply')
        if t.dtype != torch.float32 or tuple(t.shape) != shape or t.device != dev:
            raise ValueError('sparse_map_apply: %s must be a float32 tensor of shape %s on %s, got %s %s on %s'
                             % (name, shape, dev, t.dtype, tuple(t.shape), t.device))
        return t
    out = result(out, 'out')
    frac = result(frac_out, 'frac_out') if skipna and frac_out is not None and frac_out is not False else None
    if frac is not None and frac.stride() != out.stride():
        # the kernel writes both through one set of strides: a fraction of another layout goes through a twin of `out`
        frac_user, frac = frac, torch.empty_strided(shape, out.stride(), dtype=torch.float32, device=dev)
    else:
        frac_user = frac
    if out.numel() == 0:
        return out if frac is None else (out, frac_user)

    def describe(xv, yv):
        xs = _space_stride(xv.shape[a0:a1], xv.stride()[a0:a1])
        ys = _space_stride(yv.shape[a0:b1], yv.stride()[a0:b1])
        if xs is None or ys is None:
            return None
        # (the tag: the dims before and after the space axes do not merge with each other)
        rest = [(e, sx, sy) for e, (sx, sy), _ in
                merge_dims([(xv.shape[i], (xv.stride(i), yv.stride(i)), 0) for i in range(a0)] +
                           [(xv.shape[i], (xv.stride(i), yv.stride(i - a1 + b1)), 1) for i in range(a1, xv.dim())])]
        # inner (lanes span it): the dim of smallest output stride, if x is also denser along it than along the space axis;
        # otherwise it becomes the fastest outer dim, whose consecutive slices a lane handles together
        inner = min(range(len(rest)), key=lambda i: (abs(rest[i][2]), -i)) if rest else None
        if inner is not None and abs(rest[inner][1]) >= abs(xs):
            inner = None
        # outer dims slowest first by x stride: the slices of one lane lie as close together as the layout allows
        outer = sorted((d for i, d in enumerate(rest) if i != inner), key=lambda d: (abs(d[1]), abs(d[2])), reverse=True)
        if len(outer) > 3:
            return None
        d = nat.SparseMapDesc()
        d.n_a, d.n_b, d.nnz = m.n_a, m.n_b, m.nnz
        d.x_dtype = nat.dtype_tag(xv)
        d.n_outer = len(outer)
        for i, (e, sx, sy) in enumerate(outer):
            d.outer_ext[i], d.x_outer_stride[i], d.y_outer_stride[i] = e, sx, sy
        d.x_space_stride, d.y_space_stride = xs, ys
        d.inner_ext, d.x_inner_stride, d.y_inner_stride = (rest[inner] if inner is not None else (1, 0, 0))
        return d

    y, f = out, frac
    d = describe(x, y)
    if d is None:                       # the documented fallback: contiguous operands
        x = x.contiguous()
        y = out if out.is_contiguous() else torch.empty(shape, dtype=torch.float32, device=dev)
        if frac is not None:
            f = frac if y is out else torch.empty(shape, dtype=torch.float32, device=dev)
        d = describe(x, y)
    with torch.cuda.device(dev):
        if skipna:
            check(lib().dlwpcs_sparse_map_apply_masked(ctypes.byref(d), row_ptr.data_ptr(), ptr(col), ptr(val), x.data_ptr(),
                                                       y.data_ptr(), ptr(f), float(min_valid),
                                                       nat.MAP_RENORMALIZE if renormalize else 0, stream_ptr()),
                  'dlwpcs_sparse_map_apply_masked')
        else:
            check(lib().dlwpcs_sparse_map_apply(ctypes.byref(d), row_ptr.data_ptr(), ptr(col), ptr(val), x.data_ptr(),
                                                y.data_ptr(), stream_ptr()), 'dlwpcs_sparse_map_apply')
        if y is not out:
            out.copy_(y)
        if f is not frac_user:
            frac_user.copy_(f)
    return out if frac is None else (out, frac_user)


# ------------------------------------------------------------------------------------------------------------------ #
# Conservative map generation (DLWP/remap/overlap.py): overlap areas of lat-lon and cube cells, include/dlwpcs.h dlwpcs_overlap_desc
# ------------------------------------------------------------------------------------------------------------------ #

def overlap_csr(cube, ll, dust, device):
    """
    The overlap areas of the cells of a DLWP.remap LatLonGrid and CubeSphereGrid as device tensors (row_ptr int64
    [n_lat * n_lon + 1], col int32, area float64): dlwpcs_overlap_count, an exclusive scan, dlwpcs_overlap_fill, on the current
    stream of `device`.  The number of entries is read back between the two launches (one host synchronisation).
    """
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise nat.NativeError('overlap_csr: %s is not a HIP device (device=None runs the host twin)' % dev)
    d = nat.OverlapDesc()
    d.N, d.n_lat, d.n_lon, d.dust = int(cube.N), int(ll.n_lat), int(ll.n_lon), float(dust)
    fr = np.ascontiguousarray(cube.frames, dtype=np.float64)
    ctypes.memmove(ctypes.addressof(d.frames), fr.ctypes.data, fr.nbytes)
    n = int(ll.n_lat) * int(ll.n_lon)
    with torch.cuda.device(dev):
        sl = torch.from_numpy(np.ascontiguousarray(ll.sin_lat_edges, dtype=np.float64)).to(dev)
        lo = torch.from_numpy(np.ascontiguousarray(ll.lon_edges_rad, dtype=np.float64)).to(dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        check(lib().dlwpcs_overlap_count(ctypes.byref(d), ptr(sl), ptr(lo), ptr(counts), stream_ptr()), 'dlwpcs_overlap_count')
        row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, dtype=torch.int64, out=row_ptr[1:])
        nnz = int(row_ptr[-1].item())
        col = torch.empty(nnz, dtype=torch.int32, device=dev)
        area = torch.empty(nnz, dtype=torch.float64, device=dev)
        check(lib().dlwpcs_overlap_fill(ctypes.byref(d), ptr(sl), ptr(lo), ptr(row_ptr), ptr(col), ptr(area), nnz, stream_ptr()),
              'dlwpcs_overlap_fill')
    return row_ptr, col, area


def overlap_areas(cube, ll, dust, device):
    """overlap_csr brought back to the host: (row_ptr int64, col int32, area float64) numpy arrays"""
    return tuple(t.cpu().numpy() for t in overlap_csr(cube, ll, dust, device))


# ------------------------------------------------------------------------------------------------------------------ #
# Bilinear sampling of the cube at points (DLWP/remap/bilinear.py): include/dlwpcs.h dlwpcs_cube_bilinear_desc
# ------------------------------------------------------------------------------------------------------------------ #

def cube_bilinear(cube, lat, lon, device):
    """
    The cells and weights that sample a field on a DLWP.remap CubeSphereGrid at the points (lat, lon) in degrees, as device
    tensors (col int32 (n, 4), w float64 (n, 4)): one dlwpcs_cube_bilinear launch on the current stream of `device`.  lat / lon
    that are tensors on that device are read where they lie; anything else is checked on the host and uploaded.  ValueError
    for non-finite input or |lat| > 90, before the launch (tensors on the device are checked there: one read-back).
    """
    from .remap.bilinear import _checked_points, cube_edges
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise nat.NativeError('cube_bilinear: %s is not a HIP device (device=None runs the host twin)' % dev)
    with torch.cuda.device(dev):
        dev = torch.device('cuda', torch.cuda.current_device())
        if all(isinstance(x, torch.Tensor) and x.device == dev for x in (lat, lon)):
            if lat.shape != lon.shape:
                raise ValueError('lat and lon must have one shape, got %s and %s' % (tuple(lat.shape), tuple(lon.shape)))
            la, lo = (x.detach().to(torch.float64).reshape(-1).contiguous() for x in (lat, lon))
            if la.numel():
                ok = torch.stack([torch.isfinite(la).all() & torch.isfinite(lo).all(), (la.abs() <= 90.).all()]).tolist()
                if not ok[0]:
                    raise ValueError('lat and lon must be finite')
                if not ok[1]:
                    raise ValueError('latitudes must lie within [-90, 90]')
        else:
            la, lo = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (lat, lon))
            la, lo = (torch.from_numpy(np.array(x, dtype=np.float64)).to(dev) for x in _checked_points(la, lo))
        n = int(la.numel())
        d = nat.CubeBilinearDesc()
        d.N, d.n_points = int(cube.N), n
        fr = np.ascontiguousarray(cube.frames, dtype=np.float64)
        ctypes.memmove(ctypes.addressof(d.frames), fr.ctypes.data, fr.nbytes)
        ed = np.ascontiguousarray(cube_edges(), dtype=np.int32)
        ctypes.memmove(ctypes.addressof(d.edge), ed.ctypes.data, ed.nbytes)
        col = torch.empty((n, 4), dtype=torch.int32, device=dev)
        w = torch.empty((n, 4), dtype=torch.float64, device=dev)
        check(lib().dlwpcs_cube_bilinear(ctypes.byref(d), ptr(la), ptr(lo), ptr(col), ptr(w), stream_ptr()), 'dlwpcs_cube_bilinear')
    return col, w


# ------------------------------------------------------------------------------------------------------------------ #
# Per-variable scaling (DLWP/model/preprocessing.py): channel moments and the channel affine, include/dlwpcs.h dlwpcs_chan_desc
# ------------------------------------------------------------------------------------------------------------------ #

def _chan_desc(x, axis, y=None, row0=False):
    """dlwpcs_chan_desc of the dims of x (and of y, same shape, its own strides) around the channel dim `axis`: the leading k dims
    are the rows, every other dim the inner extent, and each group has to merge into one strided dim on every operand.  k = 1
    (rows = dim 0) is tried first, then 0, then 2 .. axis; row0=True (a row list indexes dim 0) allows k = 1 only.  None when no
    split can be described."""
    nd = x.dim()
    y = x if y is None else y
    dims = [(int(x.shape[i]), int(x.stride(i)), int(y.stride(i))) for i in range(nd)]
    if row0:
        ks = [1] if axis >= 1 else []
    else:
        ks = [k for k in [1, 0] + list(range(2, axis + 1)) if k <= axis]
    for k in ks:
        rows, inner = ([(e,) + st for e, st, _ in merge_dims((e, (sx, sy), None) for e, sx, sy in group)]
                       for group in (dims[:k], dims[k:axis] + dims[axis + 1:]))
        if len(rows) > 1 or len(inner) > 1:
            continue
        r, s = (rows or [(1, 0, 0)])[0], (inner or [(1, 0, 0)])[0]
        if min(r[1:] + s[1:] + dims[axis][1:]) < 0:
            continue
        d = nat.ChanDesc()
        d.R, d.row_stride, d.dst_row_stride = r
        d.S, d.inner_stride, d.dst_inner_stride = s
        d.C, d.chan_stride, d.dst_chan_stride = dims[axis]
        return d
    return None


def channel_moments(x, axis=1, rows=None, center=None, skipna=False, as_numpy=False):
    """
    {count, sum (x - center[c]), sum (x - center[c])^2} of every channel c along `axis` of the fp32 device tensor x, over the rows
    (entries of dim 0) in `rows` -- numpy ints, checked and uploaded, or an int32 device tensor, trusted; duplicates count as
    given; None = all -- and over every other dim.  center: None (0) or C float64 values (numpy or a device tensor).  skipna:
    leave NaN elements out of all three (else they propagate into the sums).  fp64 sums in an order fixed by the shape: the
    same call gives the same bits.  Views are read through their strides where dim 0, the channel dim and the merged rest
    describe them (channels-first and channels-last arrays and their channel / row slices do), otherwise copied with
    .contiguous().  Returns a (C, 3) float64 device tensor; two launches on the current stream, no host synchronisation.
    as_numpy=True downloads it (one synchronisation).
    """
    require_device(x, 'channel_moments')
    if x.dtype != torch.float32:
        raise TypeError('channel_moments: x must be float32, got %s' % x.dtype)
    axis = axis % x.dim()
    dev = x.device
    n_rows, rows_d = 0, None
    if rows is not None:
        if axis == 0:
            raise ValueError('channel_moments: a row list selects entries of dim 0, which is the channel dim here')
        if isinstance(rows, torch.Tensor):
            if rows.dtype != torch.int32 or rows.device != dev or not rows.is_contiguous():
                raise TypeError('channel_moments: a device row list must be contiguous int32 on the device of x')
            rows_d = rows.reshape(-1)
        else:
            rh = np.asarray(rows, dtype=np.int64).reshape(-1)
            if rh.size and (rh.min() < 0 or rh.max() >= int(x.shape[0])):
                raise IndexError('channel_moments: row index out of range of the %d rows' % int(x.shape[0]))
            rows_d = rh
        n_rows = int(rows_d.numel() if isinstance(rows_d, torch.Tensor) else rows_d.size)
    d = _chan_desc(x, axis, row0=rows is not None)
    if d is None:
        x = x.contiguous()
        d = _chan_desc(x, axis, row0=rows is not None)
    C = int(d.C)
    with torch.cuda.device(dev):
        out = torch.empty((C, 3), dtype=torch.float64, device=dev)
        if C == 0:
            return out.cpu().numpy() if as_numpy else out
        if rows is not None and n_rows == 0:
            out.zero_()
            return out.cpu().numpy() if as_numpy else out
        if rows_d is not None and not isinstance(rows_d, torch.Tensor):
            rows_d = _int32_dev(rows_d, dev)
        ctr = None
        if center is not None:
            if isinstance(center, torch.Tensor):
                ctr = center.to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
            else:
                ctr = torch.from_numpy(np.ascontiguousarray(np.asarray(center, dtype=np.float64).reshape(-1))).to(dev)
            if ctr.numel() != C:
                raise ValueError('channel_moments: center has %d entries, the array %d channels' % (ctr.numel(), C))
        nbytes = int(lib().dlwpcs_channel_moments_scratch_bytes(ctypes.byref(d), n_rows))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        check(lib().dlwpcs_channel_moments(ctypes.byref(d), x.data_ptr(), ptr(rows_d), n_rows, ptr(ctr), 1 if skipna else 0,
                                           out.data_ptr(), ptr(scratch), nbytes, stream_ptr()), 'dlwpcs_channel_moments')
    return out.cpu().numpy() if as_numpy else out


def channel_affine(x, a, b, mode, axis=1, out=None):
    """
    out = x * a[c] + b[c] (mode nat.AFFINE_MUL_ADD) or (x - b[c]) / a[c] (nat.AFFINE_SUB_DIV) with c the index along `axis`:
    fp32 device tensors, a and b of C entries, two separately rounded fp32 operations per element.  `out`: a float32 tensor or
    view of x's shape with any layout (a permuted buffer changes the layout in the same pass; `out is x` works in place);
    default a new contiguous tensor.  Views are read and written through their strides where leading dims, the channel dim
    and the merged rest describe both sides; otherwise x is copied with .contiguous() and the result goes through a contiguous
    temporary.  One launch on the current stream, no host synchronisation.  A descriptor the library does not serve raises
    NotImplementedError.
    """
    require_device(x, 'channel_affine')
    dev = x.device
    axis = axis % x.dim()
    for t, what in ((x, 'x'), (a, 'a'), (b, 'b')):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev:
            raise TypeError('channel_affine: %s must be a float32 tensor on %s' % (what, dev))
    C = int(x.shape[axis])
    a, b = a.reshape(-1).contiguous(), b.reshape(-1).contiguous()
    if a.numel() != C or b.numel() != C:
        raise ValueError('channel_affine: tables of %d and %d entries, the array has %d channels' % (a.numel(), b.numel(), C))
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=dev)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != dev or out.shape != x.shape:
        raise ValueError('channel_affine: out must be a float32 tensor of shape %s on %s' % (tuple(x.shape), dev))
    if out.numel() == 0:
        return out
    y = out
    d = _chan_desc(x, axis, y)
    if d is None:                           # the documented fallback: contiguous operands
        x = x.contiguous()
        y = out if out.is_contiguous() else torch.empty(x.shape, dtype=torch.float32, device=dev)
        d = _chan_desc(x, axis, y)
    with torch.cuda.device(dev):
        check(lib().dlwpcs_channel_affine(ctypes.byref(d), x.data_ptr(), a.data_ptr(), b.data_ptr(), int(mode), y.data_ptr(),
                                          stream_ptr()), 'dlwpcs_channel_affine')
        if y is not out:
            out.copy_(y)
    return out
