"""CPU guards on the resources of the encode's hot transform kernels (frieda_amd/csrc/ntt.hip).

ntt_tile12_rep_kernel keeps its source tiles in registers in its first stage's layout and, in its packed-source form, unpacks them from
the blob with sixty-four loads in flight per thread; the other three kernels were tried in the same form (profiles/r13_encode_stage0.txt)
and went back.  Such changes are only worth having while they cost no resident wave: these tests compile `ntt.hip` for gfx950 (device
only, no GPU needed) and read the kernels' METADATA — registers, scratch, static LDS — nothing else; no instruction is looked at.

The yardstick is the occupancy step each kernel held before that work, measured by compiling commit 9ce9b74 ("Tests: same bytes on a
poisoned workspace and on a caller's stream") with the same flags:

    kernel                          VGPRs at 9ce9b74    waves per SIMD    step (most VGPRs that keep them)
    ntt_tile12_kernel<3, 0>         112                 4                 128
    ntt_tile12_kernel<2, 4>          92                 5                  96
    ntt_tile12_kernel<1, 8>          78                 6                  80
    ntt_tile12_rep_kernel<2>        101                 4                 128

(profiles/r06_ntt_occupancy.txt has the first two.)  gfx950: 512 VGPRs per SIMD lane allocated in blocks of 8, at most 8 waves per SIMD,
160 KiB of LDS per CU; a 256-thread workgroup is one wave on each of the CU's four SIMDs, so workgroups per CU by registers = waves per SIMD.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frieda_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
LDS_PER_CU = 160 << 10

# mangled-name part -> most VGPRs that keep the waves per SIMD the kernel had at 9ce9b74
KERNELS = {
    "ntt_tile12_kernelILi3ELi0EE": 128,
    "ntt_tile12_kernelILi2ELi4EE": 96,
    "ntt_tile12_kernelILi1ELi8EE": 80,
    "ntt_tile12_rep_kernelILi2E": 128,  # (every instantiation over two columns: plain and packed source)
}


def waves_per_simd(vgprs):
    return min(8, 512 // (8 * ((vgprs + 7) // 8)))


@pytest.fixture(scope="module")
def ntt_metadata(tmp_path_factory):
    """{kernel name: {field: int}} from the code object metadata of ntt.hip"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "ntt.s"
    # the flags of frieda_amd/csrc/Makefile
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-x", "hip", "--cuda-device-only", "-S",
           "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "ntt.hip"), "-o", str(out)]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    text = out.read_text()
    text = text[text.index("amdhsa.kernels:"):]
    meta = {}
    for block in re.split(r"^  - \.agpr_count:", text, flags=re.M)[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", block, re.M).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"^    \.(vgpr_count|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", block, re.M)}
    return meta


def select(meta, part):
    found = {n: m for n, m in meta.items() if part in n}
    assert found, (part, sorted(meta))
    return found


def test_the_four_kernels_are_there(ntt_metadata):
    for part in KERNELS:
        select(ntt_metadata, part)
    assert len(select(ntt_metadata, "ntt_tile12_rep_kernelILi2E")) == 2, "the rep kernel has a plain and a packed-source instantiation"


@pytest.mark.parametrize("part", sorted(KERNELS))
def test_no_scratch(ntt_metadata, part):
    for name, m in select(ntt_metadata, part).items():
        assert m["private_segment_fixed_size"] == 0, f"{name}: {m['private_segment_fixed_size']} B of scratch per lane: something spilled"
        assert m["vgpr_spill_count"] == 0, name


@pytest.mark.parametrize("part", sorted(KERNELS))
def test_vgprs_keep_the_occupancy_step(ntt_metadata, part):
    for name, m in select(ntt_metadata, part).items():
        assert m["vgpr_count"] <= KERNELS[part], (
            f"{name}: {m['vgpr_count']} VGPRs = {waves_per_simd(m['vgpr_count'])} waves per SIMD, had {waves_per_simd(KERNELS[part])} at 9ce9b74")


@pytest.mark.parametrize("part", sorted(KERNELS))
def test_static_lds_does_not_cost_a_workgroup(ntt_metadata, part):
    for name, m in select(ntt_metadata, part).items():
        by_regs = waves_per_simd(m["vgpr_count"])
        by_lds = LDS_PER_CU // m["group_segment_fixed_size"]
        assert by_lds >= by_regs, f"{name}: {m['group_segment_fixed_size']} B of LDS allow {by_lds} workgroups per CU, the registers {by_regs}"
