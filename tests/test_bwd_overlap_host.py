"""STGCN_FEATURE_BWD_OVERLAP without a GPU: the export, the feature bit and the
process-wide switch stgcn_bwd_overlap (1 = the folded backward's small kernels on
the library's side stream, the default; 0 = serial; negative = query)."""
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.hip_lib.load_library()


def test_export_header_and_feature_bit(pkg, lib):
    hl = pkg.hip_lib
    assert "stgcn_bwd_overlap" in hl.EXPORTED
    assert hasattr(lib, "stgcn_bwd_overlap")
    header = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    assert re.search(r"^int stgcn_bwd_overlap\(int enable\);", header, flags=re.M)
    assert re.search(r"^#define STGCN_FEATURE_BWD_OVERLAP 128\b", header, flags=re.M)
    assert lib.stgcn_features() & 128 == hl.FEATURE_BWD_OVERLAP == 128
    assert lib.stgcn_features() & 127 == 127  # (the earlier bits stay)
    assert lib.stgcn_abi_version() == hl.ABI_VERSION == 11


def test_switch_defaults_to_on_and_round_trips(lib):
    assert lib.stgcn_bwd_overlap(-1) == 1       # the default
    try:
        assert lib.stgcn_bwd_overlap(0) == 1    # returns the previous mode
        assert lib.stgcn_bwd_overlap(-1) == 0
        assert lib.stgcn_bwd_overlap(-7) == 0   # any negative value only queries
        assert lib.stgcn_bwd_overlap(1) == 0
        assert lib.stgcn_bwd_overlap(-1) == 1
        assert lib.stgcn_bwd_overlap(5) == 1    # non-zero: on
        assert lib.stgcn_bwd_overlap(-1) == 1
    finally:
        lib.stgcn_bwd_overlap(1)
