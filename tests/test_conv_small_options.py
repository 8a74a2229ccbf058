"""CPU side of the small-face convolution path: the engine option that routes to it and its two entry points in the ctypes table."""
import os

import pytest


def test_small_conv_option_defaults_on_and_parses(monkeypatch):
    from DLWP.options import DEFAULTS, option, snapshot
    monkeypatch.delenv('DLWPCS_OPTIONS', raising=False)
    assert DEFAULTS['small_conv'] is True and option('small_conv') is True
    monkeypatch.setenv('DLWPCS_OPTIONS', 'small_conv=0')
    assert option('small_conv') is False and snapshot()['small_conv'] is False
    assert option('dgrad_gather') is True                   # (the other options keep their defaults)
    monkeypatch.setenv('DLWPCS_OPTIONS', 'small_conv=1,graphs=0')
    assert option('small_conv') is True and option('graphs') is False


def test_small_entry_points_share_the_general_ones_prototypes():
    from DLWP import _native as nat
    P = nat.PROTOTYPES
    assert P['dlwpcs_conv_small_fwd'] == P['dlwpcs_conv_fwd']
    assert P['dlwpcs_conv_small_bwd_data'] == P['dlwpcs_conv_bwd_data_masked']
    assert nat.E_UNSUPPORTED == -2
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dlwpcs.h')).read()
    assert '#define DLWPCS_E_UNSUPPORTED -2' in header
    for name in ('dlwpcs_conv_small_fwd', 'dlwpcs_conv_small_bwd_data'):
        assert ('int %s(' % name) in header


def test_engine_offers_only_layers_the_kernel_can_serve():
    from DLWP import _native as nat, ops

    def d(**kw):
        base = dict(B=2, N=12, C0=64, C1=0, Cout=128, ksize=3, halo=1, up0=0, flip_north_pole=1, act=0, alpha=0., vmax=0.,
                    dtype=nat.BF16, flags=0, c0_valid=0)
        base.update(kw)
        return nat.ConvDesc(**base)
    assert ops._small_conv_ok(d())
    assert ops._small_conv_ok(d(N=16)) and not ops._small_conv_ok(d(N=24))
    for kw in (dict(dtype=nat.F32), dict(ksize=1, halo=0), dict(C1=32), dict(up0=1), dict(C0=14), dict(Cout=48), dict(halo=0), dict(B=0)):
        assert not ops._small_conv_ok(d(**kw)), kw


def test_unsupported_request_is_refused_without_a_device():
    """validation comes before any device work: a shape outside the kernel's conditions answers E_UNSUPPORTED with null pointers"""
    import ctypes
    from DLWP import _native as nat
    lib = nat.lib()
    d = nat.ConvDesc(B=1, N=24, C0=64, C1=0, Cout=64, ksize=3, halo=1, up0=0, flip_north_pole=1, act=0, alpha=0., vmax=0.,
                     dtype=nat.BF16, flags=0, c0_valid=0)
    assert lib.dlwpcs_conv_small_fwd(ctypes.byref(d), None, None, None, None, None, None, None, None, None, None, None, 0, None) == nat.E_UNSUPPORTED
    assert lib.dlwpcs_conv_small_bwd_data(ctypes.byref(d), None, None, None, None, None, None, None, None, 0., 0., None, None, 0, None) == nat.E_UNSUPPORTED
    assert b'320' in lib.dlwpcs_last_error()
