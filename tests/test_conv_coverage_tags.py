"""
CPU check of the case table in test_gpu_conv_coverage.py against the library's registered kernel tags
(dlwpcs_prof_known_tag): every instantiation the dispatch can launch is declared by some case, and every tag the table leaves
out is listed in its UNREACHABLE dict with a reason.  No device work.
"""
import ctypes
import os

import pytest

import test_gpu_conv_coverage as cov

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def native():
    from DLWP import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location('dlwpcs_build', os.path.join(ROOT, 'dlwp-cs_amd', 'build.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    return nat


def _registered(nat):
    lib = nat.lib()
    buf = ctypes.create_string_buffer(200)
    out = set()
    for i in range(lib.dlwpcs_prof_known_tags()):
        nat.check(lib.dlwpcs_prof_known_tag(i, buf, 200), 'dlwpcs_prof_known_tag')
        out.add(buf.value.decode())
    return out


def test_declared_tags_cover_every_registered_tag(native):
    reg = _registered(native)
    declared = set().union(*(c.tags for c in cov.CASES)) | set().union(*(c.tags for c in cov.TUNE_CASES + cov.NOSTRIP_CASES))
    assert declared - reg == set(), 'declared tags the library does not register'
    assert sorted(reg - set(cov.UNREACHABLE)) == sorted(declared), 'registered tags neither declared by a case nor UNREACHABLE'


def test_unreachable_entries_are_registered_and_explained(native):
    reg = _registered(native)
    for tag, why in cov.UNREACHABLE.items():
        assert tag in reg, tag
        assert isinstance(why, str) and len(why) > 20, tag
    declared = set().union(*(c.tags for c in cov.CASES)) | set().union(*(c.tags for c in cov.TUNE_CASES + cov.NOSTRIP_CASES))
    assert not declared & set(cov.UNREACHABLE), 'a tag is both declared and UNREACHABLE'
