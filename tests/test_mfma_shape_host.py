"""CPU suite: the mfma_shape option of the 256-query filter tile: documented, validated, routed (tavb_plan_filter_shape, the rule the
launcher and the option setter use), and both MFMA shapes of the tile ship in libtavb.so."""

import os

from typeagent_py_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_documents_the_shape_option_and_its_getter():
    text = open(os.path.join(ROOT, "include", "tavb.h")).read()
    assert '"mfma_shape"' in text and '"last_mfma_shape"' in text


def test_both_shapes_of_the_filter_tile_are_in_the_library():
    lib = open(_native.library_path(), "rb").read()
    # mfma_scan_kernel<0, 4, 8, 6, 4, SPLIT, BD, M16>: the shipping 16x16x32 form, its 32x32x16 twin, and the 16x16x32 ablations that
    # tools/ceiling.py (mfma_ablate = 258) and the profiles (256) select
    for abl, m16 in (("0", "1"), ("0", "0"), ("256", "1"), ("258", "1")):
        name = f"_ZN4tavb12_GLOBAL__N_116mfma_scan_kernelILi{abl}ELi4ELi8ELi6ELi4ELb0ELb0ELb{m16}EEEvNS0_16MfmaDeviceParamsE"
        assert name.encode() in lib, name


def test_filter_shape_routing():
    plan = _native.plan_filter_shape
    assert plan(16) == 16 and plan(32) == 32
    # the 128-query tile, the SPLIT exact form, the direct query operand and the staging schedules stay on 32x32x16
    assert plan(16, query_tile=128) == 32
    assert plan(16, split=True) == 32
    assert plan(16, bdirect=True) == 32
    assert plan(16, sched=1) == 32 and plan(16, sched=3) == 32
    # the like-for-like ablations exist for both shapes; the others are 32x32x16 only
    assert plan(16, ablate=256) == 16 and plan(16, ablate=258) == 16
    assert plan(32, ablate=258) == 32 and plan(16, ablate=264) == 32 and plan(16, ablate=1) == 32
    assert plan(16, bdirect=True, ablate=258) == 16  # (an ablation ignores mfma_bdirect, as the launcher does)


def test_filter_shape_validation():
    import pytest

    for bad in (0, 8, 31, 64, -16):
        with pytest.raises(ValueError, match="mfma_shape"):
            _native.plan_filter_shape(bad)
    with pytest.raises(ValueError, match="query_tile"):
        _native.plan_filter_shape(16, query_tile=64)
