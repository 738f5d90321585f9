"""The build writes a per-kernel resource table (registers, scratch, occupancy) next to each object; the hot kernels
must stay inside the budgets their launch geometry assumes -- a few extra live registers silently halve the
workgroups per CU (measured: igemm_bf16_ws_kernel<128, 2> at 151 VGPRs ran the training step 6 % slower)."""
import glob
import os
import re

import pytest

OBJ = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "centroids-reid_amd", "lib", "obj")


def _table():
    rows = {}
    for path in glob.glob(os.path.join(OBJ, "*.res")):
        for line in open(path):
            kv = dict(t.split("=", 1) for t in line.split() if "=" in t)
            if "name" in kv:
                rows[kv["name"]] = kv
    return rows


def _demangled(name):
    # _Z20igemm_bf16_ws_kernelILi128ELi2EEv... -> ("igemm_bf16_ws_kernel", [128, 2])
    m = re.match(r"_Z\d+([A-Za-z0-9_]+?)(I.*)?$", name)
    base = m.group(1) if m else name
    args = [int(a) for a in re.findall(r"Li(\d+)E", name.split("Ev")[0])]
    return base, args


def test_hot_kernels_keep_their_occupancy_budget():
    rows = _table()
    if not rows:
        pytest.skip("no resource tables (library not built here)")
    seen = two_per_cu = 0
    for name, kv in rows.items():
        base, args = _demangled(name)
        if base in ("igemm_bf16_ws_kernel", "igemm_bf16_dma_kernel", "wgrad_bf16_dma_kernel", "sqdist_f32_kernel",
                    "sqdist_count_f32_kernel", "sqdist_stream_h16_kernel", "igemm1x1_stream_kernel"):
            assert int(kv.get("scratch", 0)) == 0, (name, kv)
            assert int(kv.get("vgpr_spill", 0)) == 0, (name, kv)
            seen += 1
        if base == "igemm_bf16_ws_kernel":
            # 512 threads = 2 waves per SIMD per workgroup; two workgroups per CU need 4 waves per SIMD = 128 VGPRs.
            # The 256-row variant (third template argument) runs one workgroup per CU: 256 registers, no spills.
            limit = 256 if (len(args) == 3 and args[2] == 256) else 128
            if args[:2] == [64, 2] and (len(args) < 3 or args[2] == 128):
                limit = 80                                   # the 128 x 64 two-stage tile runs THREE workgroups per CU (6 waves / SIMD)
            assert int(kv["vgprs"]) + int(kv.get("agprs", 0)) <= limit, (name, kv)
        if base == "sqdist_stream_h16_kernel" or (base == "sqdist_count_f32_kernel" and "Lb1E" in name.split("Ev")[0]):
            # __launch_bounds__(256, 2): every 16-bit streamed kernel and the FULLK (second template argument true) fp32 ones
            # run two workgroups per CU = 2 waves per SIMD, so 256 registers per lane and not one more.
            assert int(kv["vgprs"]) + int(kv.get("agprs", 0)) <= 256, (name, kv)
            assert int(kv["occupancy"]) >= 2, (name, kv)
            two_per_cu += 1
    assert seen >= 10
    assert two_per_cu >= 6                                       # 2 dtypes x 2 epilogues, and the FULLK fp32 count and top-k


def test_no_shipped_kernel_spills():
    """Every kernel of libcreid_hip.so -- not only the hot ones a default plan selects -- compiles without scratch memory and
    without vector-register spills (igemm_bf16_kernel<128>, igemm_bf16_pp_kernel<256, 256, 4, 1, 2, 1> and
    rank_rows_lds_kernel used to spill; the first now runs one workgroup per SIMD pair, the second combination is routed to the
    ping-pong form and no longer instantiated, the third re-derives its thread index per row instead of keeping hoisted
    addresses live across the whole row loop)."""
    rows = _table()
    if not rows:
        pytest.skip("no resource tables (library not built here)")
    bad = {n: (kv.get("scratch"), kv.get("vgpr_spill")) for n, kv in rows.items()
           if int(kv.get("scratch", 0)) != 0 or int(kv.get("vgpr_spill", 0)) != 0}
    assert not bad, bad
    assert len(rows) > 150                                      # the whole library was looked at
