"""CPU guards on the resources of the cells kernels (frieda_amd/csrc/cells.hip).

The open-values, open-paths and walk kernels are templates: over the blob a cell is opened from (the one of the call, or the row of a
per-blob table) and over where the walk takes a cell's commitment from (the kernel arguments, or a table in device memory).  The
single-blob instantiations must stay what the separate single-blob kernels were, and the table forms what their copies were.  These
tests compile `cells.hip` for gfx950 (device only, no GPU needed) and read the kernels' METADATA — registers, scratch, static LDS —
nothing else; no instruction is looked at.

The yardstick is what the separate kernels held at commit 9fe6748 ("Encode: rep kernel starts from registers and unpacks the blob
itself"), measured by compiling that commit's cells.hip with the same flags:

    kernel at 9fe6748                           VGPRs    waves per SIMD    instantiation now
    cells_open_values_kernel<4>, <1>              8, 8                 8    cells_open_values_kernel<VEC, CellsOpenArgs>
    cells_open_blobs_values_kernel<4>, <1>      11, 11                 8    cells_open_values_kernel<VEC, CellsOpenBlobsArgs>
    cells_open_paths_kernel                         45                 8    cells_open_paths_kernel<CellsOpenArgs>
    cells_open_blobs_paths_kernel                   51                 8    cells_open_paths_kernel<CellsOpenBlobsArgs>
    cells_walk_kernel<true>, <false>            41, 38                 8    cells_walk_kernel<LEAF, false>
    cells_walk_blobs_kernel<true>, <false>      41, 38                 8    cells_walk_kernel<LEAF, true>
    cells_roots_kernel                              47                 8    (not a template; 17536 B of static LDS)

None had scratch or spills.  gfx950: 512 VGPRs per SIMD lane allocated in blocks of 8, at most 8 waves per SIMD: all of them sat at
the top step, which 64 VGPRs still keep.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frieda_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# mangled-name part -> (instantiations, most VGPRs that keep the waves per SIMD their twins had at 9fe6748)
KERNELS = {
    "cells_open_values_kernelILi4ENS0_13CellsOpenArgsE": (1, 64),
    "cells_open_values_kernelILi1ENS0_13CellsOpenArgsE": (1, 64),
    "cells_open_values_kernelILi4ENS0_18CellsOpenBlobsArgsE": (1, 64),
    "cells_open_values_kernelILi1ENS0_18CellsOpenBlobsArgsE": (1, 64),
    "cells_open_paths_kernelINS0_13CellsOpenArgsE": (1, 64),
    "cells_open_paths_kernelINS0_18CellsOpenBlobsArgsE": (1, 64),
    "cells_walk_kernelILb1ELb0E": (1, 64),
    "cells_walk_kernelILb0ELb0E": (1, 64),
    "cells_walk_kernelILb1ELb1E": (1, 64),
    "cells_walk_kernelILb0ELb1E": (1, 64),
}
ROOTS_LDS = 17536  # 8 * (512 + 4) + 256 words


def waves_per_simd(vgprs):
    return min(8, 512 // (8 * ((vgprs + 7) // 8)))


@pytest.fixture(scope="module")
def cells_metadata(tmp_path_factory):
    """{kernel name: {field: int}} from the code object metadata of cells.hip"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "cells.s"
    # the flags of frieda_amd/csrc/Makefile
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-x", "hip", "--cuda-device-only", "-S",
           "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "cells.hip"), "-o", str(out)]
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


def test_every_instantiation_is_there_and_no_other(cells_metadata):
    for part, (count, _) in KERNELS.items():
        assert len(select(cells_metadata, part)) == count, part
    templated = [n for n in cells_metadata if re.search(r"cells_(open_values|open_paths|walk)_kernel", n)]
    assert len(templated) == len(KERNELS), sorted(templated)
    assert not [n for n in cells_metadata if "_blobs_" in n], "the table forms are instantiations, not kernels of their own"


@pytest.mark.parametrize("part", sorted(KERNELS))
def test_no_scratch(cells_metadata, part):
    for name, m in select(cells_metadata, part).items():
        assert m["private_segment_fixed_size"] == 0, f"{name}: {m['private_segment_fixed_size']} B of scratch per lane: something spilled"
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, name


@pytest.mark.parametrize("part", sorted(KERNELS))
def test_vgprs_keep_the_occupancy_step(cells_metadata, part):
    for name, m in select(cells_metadata, part).items():
        assert m["vgpr_count"] <= KERNELS[part][1], (
            f"{name}: {m['vgpr_count']} VGPRs = {waves_per_simd(m['vgpr_count'])} waves per SIMD, its twin had {waves_per_simd(KERNELS[part][1])} at 9fe6748")


def test_roots_kernel_static_lds_is_unchanged(cells_metadata):
    (name, m), = select(cells_metadata, "cells_roots_kernel").items()
    assert m["group_segment_fixed_size"] == ROOTS_LDS, name
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0
