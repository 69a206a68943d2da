"""CPU guards on the resources of the split verify route (frieda_amd/csrc/verify_split.hip) and on verify.hip beside it.

The tests compile `verify_split.hip` and `verify.hip` for gfx950 (device only, no GPU needed) and read the kernels' METADATA —
registers, scratch, static LDS — nothing else; no instruction is looked at.

What the kernels held when they were written, on top of commit bea51ef ("frieda_prove_jobs: any list of (handle, seed) jobs, cut into
passes"), compiled with the flags of the Makefile:

    kernel                                   VGPRs    SGPRs    waves per SIMD    static LDS    scratch    spills (VGPR, SGPR)
    verify_walk_kernel                          48       54                 8             0          0                   0, 0    (dynamic LDS: 36 bytes per entry of q_cap)
    verify_chain_kernel<false>, <true>    143, 143  98, 100                 3           644          0                   0, 0    (dynamic LDS: 24 bytes per entry of q_cap)
    verify_many_kernel<false>, <true>     144, 145      104                 3           644          0    0; 58, 68 SGPRs    (the parent commit: the same figures)

The limits are the issue's: the walk kernel at 8 waves per SIMD (<= 64 VGPRs; bundle_walk_kernel runs the same walk step at 49) without
scratch or static LDS; the chain kernels without scratch or spills and with at least the 3 waves per SIMD of verify_many_kernel (<= 168
VGPRs); verify_many_kernel, which now takes its point helpers and the last-layer evaluation from verify_dev.h, with no more VGPRs than
at the parent commit and still without scratch.  gfx950: 512 VGPRs per SIMD lane allocated in blocks of 8, at most 8 waves per SIMD.

"No spills" is what the project's other register tests hold: vgpr_spill_count and sgpr_spill_count both zero, for all three kernels of
the new file.  The chain kernels run qdev::generate_queries, the query code they share with verify_many_kernel and the prover's
decommit.hip.  Fully unrolled, its 64-lane rank holds all 64 broadcast values in SGPRs at once; beside the uniform values a chain wave
keeps across the call that is more than the register file has, and the compiler parked 67 / 71 SGPRs in lanes of a VGPR (as it does in
verify_many_kernel, 58 / 68, at the parent commit and now).  The chain kernels therefore ask for the rank loop in steps of 8
(generate_queries<64, 8>; the default stays the full unroll, so verify.hip and decommit.hip compile as before): no spill of either kind.
"""
import pytest

from test_bundles_registers import metadata, select, waves_per_simd

# mangled-name part -> most VGPRs
SPLIT_KERNELS = {
    "verify_walk_kernel": 64,
    "verify_chain_kernelILb0E": 168,
    "verify_chain_kernelILb1E": 168,
}
# verify_many_kernel<false>, <true> at the parent commit
PARENT_VGPRS = {"verify_many_kernelILb0E": 144, "verify_many_kernelILb1E": 145}


@pytest.fixture(scope="module")
def split_metadata(tmp_path_factory):
    return metadata(tmp_path_factory.mktemp("isa"), "verify_split")


@pytest.fixture(scope="module")
def verify_metadata(tmp_path_factory):
    return metadata(tmp_path_factory.mktemp("isa"), "verify")


def test_every_kernel_of_the_new_file_is_listed(split_metadata):
    for part in SPLIT_KERNELS:
        assert len(select(split_metadata, part)) == 1, part
    assert len(split_metadata) == len(SPLIT_KERNELS), sorted(split_metadata)


@pytest.mark.parametrize("part", sorted(SPLIT_KERNELS))
def test_no_scratch_no_spills(split_metadata, part):
    for name, m in select(split_metadata, part).items():
        assert m["private_segment_fixed_size"] == 0, f"{name}: {m['private_segment_fixed_size']} B of scratch per lane: something spilled"
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, name


@pytest.mark.parametrize("part", sorted(SPLIT_KERNELS))
def test_vgprs_keep_the_occupancy_step(split_metadata, part):
    for name, m in select(split_metadata, part).items():
        print(name, m)
        assert m["vgpr_count"] <= SPLIT_KERNELS[part], f"{name}: {m['vgpr_count']} VGPRs = {waves_per_simd(m['vgpr_count'])} waves per SIMD"
    assert waves_per_simd(SPLIT_KERNELS["verify_walk_kernel"]) == 8 and waves_per_simd(168) == 3


def test_the_walk_has_no_static_lds(split_metadata):
    for name, m in select(split_metadata, "verify_walk_kernel").items():
        assert m["group_segment_fixed_size"] == 0, name


@pytest.mark.parametrize("part", sorted(PARENT_VGPRS))
def test_verify_many_kernel_gained_nothing_from_the_shared_header(verify_metadata, part):
    (name, m), = select(verify_metadata, part).items()
    print(name, m)
    assert m["vgpr_count"] <= PARENT_VGPRS[part], f"{name}: {m['vgpr_count']} VGPRs, {PARENT_VGPRS[part]} at the parent commit"
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, name
