"""CPU guards on the resources of the stripe-bundle kernels (frieda_amd/csrc/stripe_bundles.hip).

The tests compile `stripe_bundles.hip`, `bundles.hip` and `cells.hip` for gfx950 (device only, no GPU needed) and read the kernels'
METADATA — registers, scratch, static LDS — nothing else; no instruction is looked at.

The yardstick is the one of tests/test_bundles_registers.py: gfx950 has 512 VGPRs per SIMD lane allocated in blocks of 8 and at most 8
waves per SIMD; the single-blob bundle kernels and the block cells kernels all sit at that top step, which 64 VGPRs still keep.  When
they were written, with the flags of the Makefile:

    kernel                                     VGPRs    waves per SIMD
    stripe_bundle_open_witness_kernel             48                 8    (117 before the wave's number was declared uniform)
    stripe_bundle_walk_kernel<true>, <false>  48, 48                 8    (dynamic LDS only: 36 bytes per stripe of the largest bundle)

None had scratch or spills.  bundles.hip and cells.hip must still compile to the kernel sets their own tests list.
"""
import pytest

import test_bundles_registers as BR
import test_cells_registers as CR

# mangled-name part -> most VGPRs that keep 8 waves per SIMD
KERNELS = {
    "stripe_bundle_open_witness_kernel": 64,
    "stripe_bundle_walk_kernelILb1E": 64,
    "stripe_bundle_walk_kernelILb0E": 64,
}
WALKS = ("stripe_bundle_walk_kernelILb1E", "stripe_bundle_walk_kernelILb0E")


@pytest.fixture(scope="module")
def stripe_metadata(tmp_path_factory):
    return BR.metadata(tmp_path_factory.mktemp("isa"), "stripe_bundles")


def test_every_kernel_is_a_stripe_bundle_kernel_and_is_listed(stripe_metadata):
    assert all("stripe_bundle_" in n for n in stripe_metadata), sorted(stripe_metadata)
    for part in KERNELS:
        assert len(BR.select(stripe_metadata, part)) == 1, part
    assert len(stripe_metadata) == len(KERNELS), sorted(stripe_metadata)


@pytest.mark.parametrize("part", sorted(KERNELS))
def test_no_scratch_no_spills(stripe_metadata, part):
    for name, m in BR.select(stripe_metadata, part).items():
        assert m["private_segment_fixed_size"] == 0, f"{name}: {m['private_segment_fixed_size']} B of scratch per lane: something spilled"
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, name


@pytest.mark.parametrize("part", sorted(KERNELS))
def test_vgprs_keep_the_occupancy_step(stripe_metadata, part):
    for name, m in BR.select(stripe_metadata, part).items():
        assert m["vgpr_count"] <= KERNELS[part], f"{name}: {m['vgpr_count']} VGPRs = {BR.waves_per_simd(m['vgpr_count'])} waves per SIMD, 8 asked"
        assert BR.waves_per_simd(m["vgpr_count"]) == 8


def test_the_walk_has_no_static_lds(stripe_metadata):
    for part in WALKS:
        for name, m in BR.select(stripe_metadata, part).items():
            assert m["group_segment_fixed_size"] == 0, name


def test_bundles_and_cells_keep_their_kernel_sets(tmp_path):
    bundles = BR.metadata(tmp_path, "bundles")
    assert len(bundles) == len(BR.KERNELS) and all(len(BR.select(bundles, part)) == 1 for part in BR.KERNELS), sorted(bundles)
    cells = BR.metadata(tmp_path, "cells")
    for part, (count, _) in CR.KERNELS.items():
        assert len(BR.select(cells, part)) == count, part
    assert not [n for n in cells if "bundle_" in n], "no bundle kernel lives in cells.hip"
    (name, m), = BR.select(cells, "cells_roots_kernel").items()
    assert m["group_segment_fixed_size"] == BR.ROOTS_LDS, name
