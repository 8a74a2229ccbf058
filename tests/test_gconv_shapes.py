"""
The shape arithmetic in front of the generic convolution (DLWP/ops.py: _same_pads, _valid_len, the empty-output refusal of
cs_gconv), without a device: three statements of one rule must agree on every small axis --

* ops._same_pads / ops._valid_len: what the kernels are launched with (leading pad, output length);
* oracle.cs_oracle._same_pads: what the fp64 reference of tests/test_gpu_gconv.py pads with (leading, trailing);
* custom._conv_output_length: what CubeSphereConv2D.compute_output_shape promises.

n in 1..13, k in 1..5, s in 1..3, d in 1..3: every parity of face and kernel, windows wider than the axis, strides beyond
the kernel.
"""
import itertools

import pytest
import torch

from oracle import cs_oracle as orc

AXES = list(itertools.product(range(1, 14), range(1, 6), range(1, 4), range(1, 4)))      # (n, k, s, d)


def test_same_pads_agree():
    from DLWP import custom, ops
    for n, k, s, d in AXES:
        lead, out = ops._same_pads(n, k, s, d)
        o_lead, o_trail = orc._same_pads(n, k, s, d)
        assert lead == o_lead, (n, k, s, d)
        assert o_trail - o_lead in (0, 1), (n, k, s, d)                                 # the extra row goes after
        # the oracle's padded axis, convolved 'valid', has as many outputs as the kernels are launched for
        padded = n + o_lead + o_trail
        assert (padded - (k - 1) * d - 1) // s + 1 == out, (n, k, s, d)
        assert out == custom._conv_output_length(n, k, padding='same', stride=s, dilation=d), (n, k, s, d)
        assert out >= 1


def test_valid_length_agrees():
    from DLWP import custom, ops
    n_empty = 0
    for n, k, s, d in AXES:
        out = ops._valid_len(n, k, s, d)
        assert out == custom._conv_output_length(n, k, padding='valid', stride=s, dilation=d), (n, k, s, d)
        fits = (k - 1) * d + 1 <= n
        assert (out >= 1) == fits, (n, k, s, d)
        if fits:                                                                          # last window ends inside the axis,
            assert (out - 1) * s + (k - 1) * d + 1 <= n < out * s + (k - 1) * d + 1, (n, k, s, d)       # the next one does not
        n_empty += not fits
    assert n_empty > 0                                                                    # the sweep reaches the refusal


@pytest.mark.parametrize('H,W,kh,kw,sh,sw,dh,dw', [
    (2, 5, 3, 3, 1, 1, 1, 1),       # window taller than the face
    (5, 2, 3, 3, 1, 1, 1, 1),       # ... wider
    (4, 4, 3, 3, 2, 2, 2, 2),       # only the dilated window (5) does not fit
    (1, 1, 2, 1, 3, 3, 1, 1),       # the smallest face
    (5, 4, 1, 3, 1, 1, 1, 2),       # one axis fits, the other is short by one
])
def test_cs_gconv_refuses_an_empty_output(monkeypatch, H, W, kh, kw, sh, sw, dh, dw):
    """the refusal comes from the shape arithmetic, before any launch: reached here with the device check taken out"""
    from DLWP import ops
    assert ops._valid_len(H, kh, sh, dh) < 1 or ops._valid_len(W, kw, sw, dw) < 1
    monkeypatch.setattr(ops, 'require_device', lambda t, what: None)
    x = torch.zeros((1, 6, H, W, 2))
    w = torch.zeros((kh, kw, 2, 3))
    with pytest.raises(ValueError, match='empty output'):
        ops.cs_gconv(x, w, w, strides=(sh, sw), padding='valid', dilation=(dh, dw))


def test_cs_gconv_refuses_an_unknown_padding(monkeypatch):
    from DLWP import ops
    monkeypatch.setattr(ops, 'require_device', lambda t, what: None)
    x = torch.zeros((1, 6, 4, 4, 2))
    w = torch.zeros((3, 3, 2, 3))
    with pytest.raises(ValueError, match='padding'):
        ops.cs_gconv(x, w, w, padding='full')
