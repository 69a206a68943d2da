"""CPU guards on the resources of the kernels a frieda_prove_seeds_blobs call launches (frieda_amd/csrc/tree.hip, decommit.hip).

The tests compile the two files for gfx950 (device only, no GPU needed) and read the kernels' METADATA — registers, scratch, static
LDS — nothing else; no instruction is looked at.

The block form is a uniform branch in kernels that exist: job y's first layer comes from its blob's row of a table instead of from the
one shared source.  The yardstick is what each of those kernels held at the parent commit b3c4133 ("Encoded handles for a block in one
call and straight from a rebuild"), compiled with the flags of the Makefile; gfx950 has 512 VGPRs per SIMD lane allocated in blocks of
8 and at most 8 waves per SIMD:

    kernel                                      VGPRs parent -> now     waves per SIMD (both)
    top_kernel (seeds_first_alpha)                    106 -> 108                 4
    tree5_kernel<FOLD_CIRCLE> TP, plain           36, 35 -> 36, 35               8
    tree9_kernel<FOLD_CIRCLE> TP, plain           58, 58 -> 58, 58               8
    tree5r_kernel<FOLD_CIRCLE, reg-only> TP, plain 55, 52 -> 56, 52              8
    tree5r_kernel<FOLD_CIRCLE, LDS> TP, plain     57, 54 -> 58, 54               8
    tree5rs_fold_circle_kernel TP, plain        102, 103 -> 102, 103             4
    tail_kernel                                       170 -> 170                 2
    decommit_kernel                                   106 -> 111                 4

Every other kernel of tree.hip (leaf, node and line-fold instantiations, the grind, the fused small first tree) compiles to the
registers it had: the lookup is instantiated for the circle fold alone.  None has scratch or spills, before or after.
"""
import pytest

import test_bundles_registers as BR

# mangled-name part -> (most VGPRs that keep the parent's waves per SIMD, those waves)
TOUCHED = {
    "10top_kernelE": (128, 4),
    "tree5_kernelILi2ELj256ELb1EE": (64, 8),
    "tree5_kernelILi2ELj256ELb0EE": (64, 8),
    "tree9_kernelILi2ELb1EE": (64, 8),
    "tree9_kernelILi2ELb0EE": (64, 8),
    "tree5r_kernelILi2ELb1ELb1EE": (64, 8),
    "tree5r_kernelILi2ELb1ELb0EE": (64, 8),
    "tree5r_kernelILi2ELb0ELb1EE": (64, 8),
    "tree5r_kernelILi2ELb0ELb0EE": (64, 8),
    "tree5rs_fold_circle_kernelILb1EE": (128, 4),
    "tree5rs_fold_circle_kernelILb0EE": (128, 4),
    "11tail_kernelE": (256, 2),
    "decommit_kernel": (128, 4),
}
# launched by the call, not touched by it: the parent's VGPR count itself
UNTOUCHED = {
    "tree7q_kernel": 59,
    "grind_dev_kernel": 51,
    "tree5_kernelILi1ELj256ELb1EE": 36,
    "tree5_kernelILi1ELj256ELb0EE": 35,
    "tree5_kernelILi3ELj256ELb1EE": 36,
    "tree5_kernelILi3ELj256ELb0EE": 35,
    "tree9_kernelILi3ELb1EE": 58,
    "tree9_kernelILi3ELb0EE": 58,
    "tree5r_kernelILi3ELb1ELb1EE": 58,
    "tree5r_kernelILi3ELb1ELb0EE": 52,
    "tree5r_kernelILi3ELb0ELb1EE": 60,
    "tree5r_kernelILi3ELb0ELb0EE": 54,
    "tree5r_kernelILi1ELb0ELb1EE": 56,
    "tree5r_kernelILi1ELb0ELb0EE": 65,
}
STATIC_LDS = {"10top_kernelE": 67936, "11tail_kernelE": 117104, "decommit_kernel": 54064, "tree5rs_fold_circle_kernelILb1EE": 12544,
              "tree5rs_fold_circle_kernelILb0EE": 12544}


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isa")
    m = dict(BR.metadata(tmp, "tree"))
    m.update(BR.metadata(tmp, "decommit"))
    return m


def _one(meta, part):
    found = BR.select(meta, part)
    assert len(found) == 1, (part, sorted(found))
    return next(iter(found.items()))


@pytest.mark.parametrize("part", sorted(TOUCHED) + sorted(UNTOUCHED))
def test_no_scratch_no_spills(meta, part):
    name, m = _one(meta, part)
    assert m["private_segment_fixed_size"] == 0, f"{name}: {m['private_segment_fixed_size']} B of scratch per lane: something spilled"
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, name


@pytest.mark.parametrize("part", sorted(TOUCHED))
def test_touched_kernels_keep_their_occupancy_step(meta, part):
    name, m = _one(meta, part)
    most, waves = TOUCHED[part]
    assert m["vgpr_count"] <= most, f"{name}: {m['vgpr_count']} VGPRs = {BR.waves_per_simd(m['vgpr_count'])} waves per SIMD, {waves} at the parent commit"
    assert BR.waves_per_simd(m["vgpr_count"]) == waves, name


@pytest.mark.parametrize("part", sorted(UNTOUCHED))
def test_untouched_kernels_keep_their_registers(meta, part):
    name, m = _one(meta, part)
    assert m["vgpr_count"] == UNTOUCHED[part], f"{name}: {m['vgpr_count']} VGPRs, {UNTOUCHED[part]} at the parent commit"


@pytest.mark.parametrize("part", sorted(STATIC_LDS))
def test_static_lds_is_the_parents(meta, part):
    name, m = _one(meta, part)
    assert m["group_segment_fixed_size"] == STATIC_LDS[part], name
