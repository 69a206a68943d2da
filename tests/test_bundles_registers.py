"""CPU guards on the resources of the bundle kernels (frieda_amd/csrc/bundles.hip).

The tests compile `bundles.hip` and `cells.hip` for gfx950 (device only, no GPU needed) and read the kernels' METADATA — registers,
scratch, static LDS — nothing else; no instruction is looked at.

The yardstick is what the kernels held when they were written, on top of commit 8203df5 ("Sampling client: one cell pass driver, one
rebuild tail, owned buffers"), compiled with the flags of the Makefile:

    kernel                               VGPRs    waves per SIMD
    bundle_open_witness_kernel              58                 8
    bundle_walk_kernel<true>, <false>   49, 49                 8    (dynamic LDS only: 36 bytes per cell of the largest bundle)

None had scratch or spills.  gfx950: 512 VGPRs per SIMD lane allocated in blocks of 8, at most 8 waves per SIMD: all of them sit at the
top step, which 64 VGPRs still keep.  cells_roots_kernel, which the bundle verifier launches unchanged, keeps its static LDS.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frieda_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# mangled-name part -> most VGPRs that keep the waves per SIMD measured above
KERNELS = {
    "bundle_open_witness_kernel": 64,
    "bundle_walk_kernelILb1E": 64,
    "bundle_walk_kernelILb0E": 64,
}
ROOTS_LDS = 17536  # 8 * (512 + 4) + 256 words: tests/test_cells_registers.py


def waves_per_simd(vgprs):
    return min(8, 512 // (8 * ((vgprs + 7) // 8)))


def metadata(tmp, name):
    """{kernel name: {field: int}} from the code object metadata of csrc/<name>.hip"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp / (name + ".s")
    # the flags of frieda_amd/csrc/Makefile
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-x", "hip", "--cuda-device-only", "-S",
           "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, name + ".hip"), "-o", str(out)]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    text = out.read_text()
    text = text[text.index("amdhsa.kernels:"):]
    meta = {}
    for block in re.split(r"^  - \.agpr_count:", text, flags=re.M)[1:]:
        kname = re.search(r"^    \.name:\s+(\S+)", block, re.M).group(1)
        meta[kname] = {k: int(v) for k, v in re.findall(r"^    \.(vgpr_count|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", block, re.M)}
    return meta


@pytest.fixture(scope="module")
def bundles_metadata(tmp_path_factory):
    return metadata(tmp_path_factory.mktemp("isa"), "bundles")


def select(meta, part):
    found = {n: m for n, m in meta.items() if part in n}
    assert found, (part, sorted(meta))
    return found


def test_every_kernel_is_a_bundle_kernel_and_is_listed(bundles_metadata):
    assert all("bundle_" in n for n in bundles_metadata), sorted(bundles_metadata)
    for part in KERNELS:
        assert len(select(bundles_metadata, part)) == 1, part
    assert len(bundles_metadata) == len(KERNELS), sorted(bundles_metadata)


@pytest.mark.parametrize("part", sorted(KERNELS))
def test_no_scratch_no_spills(bundles_metadata, part):
    for name, m in select(bundles_metadata, part).items():
        assert m["private_segment_fixed_size"] == 0, f"{name}: {m['private_segment_fixed_size']} B of scratch per lane: something spilled"
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, name


@pytest.mark.parametrize("part", sorted(KERNELS))
def test_vgprs_keep_the_occupancy_step(bundles_metadata, part):
    for name, m in select(bundles_metadata, part).items():
        assert m["vgpr_count"] <= KERNELS[part], f"{name}: {m['vgpr_count']} VGPRs = {waves_per_simd(m['vgpr_count'])} waves per SIMD, 8 when it was written"


def test_the_walk_has_no_static_lds(bundles_metadata):
    for part in ("bundle_walk_kernelILb1E", "bundle_walk_kernelILb0E"):
        for name, m in select(bundles_metadata, part).items():
            assert m["group_segment_fixed_size"] == 0, name


def test_roots_kernel_static_lds_is_unchanged(tmp_path):
    (name, m), = select(metadata(tmp_path, "cells"), "cells_roots_kernel").items()
    assert m["group_segment_fixed_size"] == ROOTS_LDS, name
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0
