"""
How the analysis kernels see a strided view: the dims a descriptor lists.  Pure Python on shapes and element strides (no torch, no
ctypes); DLWP/ops.py turns the results into descriptors.  The device side of the same layer is csrc/strided.h; a new analysis
family starts from the two ("Shared addressing").
"""


def merge_dims(dims):
    """
    `dims`: (extent, strides -- one per operand, in elements, 0 = broadcast --, tag) in walking order.  Unit extents are dropped;
    neighbours with equal tags merge where every operand allows it (outer stride == inner stride * inner extent), so that a walk
    over the result reaches the same offsets in the same order.  Returns [(extent, strides tuple, tag)].
    """
    out = []
    for e, st, tag in dims:
        e, st = int(e), tuple(int(s) for s in st)
        if e == 1:
            continue
        if out and out[-1][2] == tag and all(ps == cs * e for ps, cs in zip(out[-1][1], st)):
            out[-1] = (out[-1][0] * e, st, tag)
        else:
            out.append((e, st, tag))
    return out


def member_split(shape, strides, member_axis, who, min_members=2):
    """(M, member stride, element shape, element strides) of an ensemble whose members lie along `member_axis`"""
    shape = tuple(int(s) for s in shape)
    strides = tuple(int(s) for s in strides)
    nd = len(shape)
    if nd < 1 or not -nd <= int(member_axis) < nd:
        raise ValueError('%s: member axis %s out of range of %d axes' % (who, member_axis, nd))
    ax = int(member_axis) % nd
    if shape[ax] < min_members:
        raise ValueError('%s: %d members (at least %d)' % (who, shape[ax], min_members))
    return shape[ax], strides[ax], shape[:ax] + shape[ax + 1:], strides[:ax] + strides[ax + 1:]


def element_layout(shape, strides, member_axis, others, who, min_members=2, max_dims=None):
    """
    How a kernel with one lane per element walks an ensemble of logical `shape` and element `strides` whose members lie along
    `member_axis`: (M, member stride, element shape, order, merged dims).  `others`: further operands over the element dims, each
    (shape, strides) -- a verification: the element dims, extents of 1 broadcast -- or (None, strides) with the broadcast strides
    already 0.  `order` lists the element dims of extent > 1 from the largest stride of the ensemble to the smallest, so that the
    lanes run along the dim that is contiguous in memory whatever view the caller holds.  Merged dims: those dims in that order
    through merge_dims, [(extent, (ensemble stride, stride of each other operand))].
    """
    M, ms, eshape, es = member_split(shape, strides, member_axis, who, min_members)
    ops = [es]
    for oshape, ostrides in others:
        if oshape is None:
            ops.append(tuple(ostrides) if ostrides is not None else (0,) * len(eshape))
            continue
        oshape = tuple(int(s) for s in oshape)
        if len(oshape) != len(eshape) or any(v not in (1, e) for v, e in zip(oshape, eshape)):
            raise ValueError('%s: the verification %s must carry the dims of the ensemble without the member axis %s '
                             '(extents of 1 broadcast)' % (who, oshape, eshape))
        ops.append(tuple(0 if v == 1 else int(s) for v, s in zip(oshape, ostrides)))
    order = sorted((i for i in range(len(eshape)) if eshape[i] != 1), key=lambda i: -abs(es[i]))
    merged = [(e, s) for e, s, _ in merge_dims((eshape[i], [o[i] for o in ops], None) for i in order)]
    if max_dims is not None and len(merged) > max_dims:
        raise NotImplementedError('%s: more than %d element dims after merging' % (who, max_dims))
    return M, ms, eshape, order, merged

