"""The tap-fused weight-gradient kernel (csrc/conv_wgrad.hip wgrad_bf16_taps_kernel), without a GPU: a Python mirror of its coverage
rule, split rule, halo slot map and LDS swizzle, checked against the convolution's own source pixels and against the library's
workspace sizes.

The mirror, the shapes, the small-integer operands and the fp64 reference here are shared with tests/test_wgrad_taps_gpu.py."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

TPK = 128                                        # pixels per k-step
CHANNELS = [(64, 64), (64, 192), (128, 64), (256, 256), (512, 128)]      # C_in -> C_out: a swap of the two indices shows
SIZES = [(16, 8), (8, 16), (4, 32)]              # OW = 8, 16, 32
BATCHES = [1, 3, 5]                              # odd: the last split is short
PRODUCTION = [(64, 64, 64, 64, 32), (64, 128, 128, 32, 16), (64, 256, 256, 16, 8), (64, 512, 512, 16, 8)]   # (B, cin, cout, H, W)


# ------------------------------------------------------------------------------------ mirror of the kernel's geometry
def covers(cin, cout, k, stride, pad, oh, ow, sh, sw, M, is16=True):
    """wgrad_taps_covers (conv_wgrad.hip)"""
    if not is16 or k != 3 or stride != 1 or pad != 1 or cin not in (64, 128, 256, 512):
        return False
    if cout <= 0 or cout % 64 != 0 or (sh, sw) != (oh, ow) or ow not in (8, 16, 32):
        return False
    return (oh * ow) % TPK == 0 and M > 0 and M % (oh * ow) == 0


def taps_splits(M, cin, cout, target=None):
    """plan_wgrad_route: (splits, pixels per split); target = CREID_WGRAD_TAPS_WGS, None: the built-in workgroup target"""
    tiles = (cout // 64) * (cin // 64)
    target = target or (192 if tiles <= 4 else 256)
    steps = M // TPK
    splits = max(1, min(steps, (target + tiles // 2) // tiles))
    per = (steps + splits - 1) // splits
    return (steps + per - 1) // per, per * TPK


def halo_dims(ow):
    rows, hp = TPK // ow, ow + 2
    return rows, hp, (rows + 2) * hp


def slice_slot(kk, ow):
    return kk * 16 + 2 * ((kk * 16) // ow)


def lane_rows(lane):
    """transposing-read lane map: this lane's pixel row within a 16-pixel slice (low half; the high half is + 4) and channel"""
    li = lane & 15
    return 8 * (lane >> 5) + (li >> 2), 16 * ((lane >> 4) & 1) + 4 * (li & 3)


def read_byte_address(lane, kk, tap, hi, wn, ow):
    """byte address, relative to the halo patch of a stage, that `lane` presents for slice kk under `tap`: exactly the kernel's
    (fb[tap] ^ FLIP) + immediate offset"""
    _, hp, _ = halo_dims(ow)
    t_row, t_col = lane_rows(lane)
    col = wn * 32 + t_col
    slot = t_row + 2 * (t_row // ow) + (tap // 3) * hp + tap % 3
    fb = 2 * (slot * 64 + (((col >> 5) ^ ((slot >> 1) & 1)) << 5) + (col & 31))
    s = slice_slot(kk, ow)
    return (fb ^ (((s >> 1) & 1) * 64)) + (s + (4 if hi else 0)) * 128


def fill_source(slot, oy0, oh, ow):
    """source pixel (iy, ix) the DMA copies into `slot` of a k-step that starts at image row oy0; None: the zero page"""
    _, hp, nslot = halo_dims(ow)
    hr, hx = divmod(slot, hp)
    iy, ix = oy0 - 1 + hr, hx - 1
    if slot >= nslot or not (1 <= hx <= ow) or not (0 <= iy < oh):
        return None
    return iy, ix


def conv_source(oy, ox, r, s, oh, ow):
    iy, ix = oy + r - 1, ox + s - 1
    return (iy, ix) if (0 <= iy < oh and 0 <= ix < ow) else None


GEOMS = sorted({(h, w) for h, w in SIZES} | {(p[3], p[4]) for p in PRODUCTION})


@pytest.mark.parametrize("oh,ow", GEOMS)
def test_every_pixel_tap_pair_maps_to_one_halo_slot_or_the_zero_page(oh, ow):
    """The address a lane presents for (slice, tap, half) decodes -- swizzle undone -- to the slot (p / OW + r, p % OW + s) of its
    pixel p, and that slot was filled with exactly the convolution's source pixel, or with zeros where that lies outside the image:
    for every k-step of an image."""
    rows, hp, nslot = halo_dims(ow)
    for oy0 in range(0, oh, rows):
        for kk in range(TPK // 16):
            for lane in range(64):
                t_row, t_col = lane_rows(lane)
                for hi in (0, 1):
                    p = kk * 16 + t_row + 4 * hi
                    for tap in range(9):
                        for wn in (0, 1):
                            a = read_byte_address(lane, kk, tap, hi, wn, ow)
                            slot, within = divmod(a, 128)
                            assert 0 <= slot < nslot
                            assert slot == (p // ow + tap // 3) * hp + p % ow + tap % 3
                            col = (((within >> 6) ^ ((slot >> 1) & 1)) << 5) + ((within & 63) >> 1)     # undo the DMA's swizzle
                            assert col == wn * 32 + t_col
                            assert fill_source(slot, oy0, oh, ow) == conv_source(oy0 + p // ow, p % ow, tap // 3, tap % 3, oh, ow)


@pytest.mark.parametrize("ow", [8, 16, 32])
def test_fragment_reads_are_conflict_free_per_16_lane_group(ow):
    """A ds_read_b64_tr_b16 serves 16 lanes x 8 bytes per pass: the 16 addresses of a lane group (4 consecutive slots x 4 chunks of
    8 bytes) must fall on 32 different banks of the 64 -- the standard wgrad_bf16_dma_kernel's comments claim for its 128-byte
    rows -- for each of the nine taps, whatever its one-slot shifts; the dY tile's rows likewise."""
    for kk in range(TPK // 16):
        for hi in (0, 1):
            for wn in (0, 1):
                for grp in range(4):
                    lanes = range(16 * grp, 16 * grp + 16)
                    for tap in range(9):
                        banks = set()
                        for lane in lanes:
                            a = read_byte_address(lane, kk, tap, hi, wn, ow)
                            banks |= {(a >> 2) & 63, ((a + 4) >> 2) & 63}
                        assert len(banks) == 32, (ow, kk, tap, grp)
                    banks = set()
                    for lane in lanes:                                                       # the dY tile (wm = wn here)
                        t_row, t_col = lane_rows(lane)
                        col, row = wn * 32 + t_col, kk * 16 + t_row + 4 * hi
                        a = 2 * (row * 64 + (((col >> 5) ^ ((row >> 1) & 1)) << 5) + (col & 31))
                        banks |= {(a >> 2) & 63, ((a + 4) >> 2) & 63}
                    assert len(banks) == 32


def test_coverage_predicate():
    for cin, cout in CHANNELS:
        for h, w in SIZES:
            for B in BATCHES:
                assert covers(cin, cout, 3, 1, 1, h, w, h, w, B * h * w)
    for B, cin, cout, h, w in PRODUCTION:
        assert covers(cin, cout, 3, 1, 1, h, w, h, w, B * h * w)
    assert not covers(128, 128, 3, 2, 1, 8, 8, 16, 16, 2 * 64)                 # stride 2
    assert not covers(64, 256, 1, 1, 0, 16, 8, 16, 8, 128)                     # 1 x 1
    assert not covers(192, 64, 3, 1, 1, 16, 8, 16, 8, 128)                     # C_in not a power of two
    assert not covers(1024, 64, 3, 1, 1, 16, 8, 16, 8, 128)                    # C_in beyond the table
    assert not covers(64, 64, 3, 1, 1, 16, 8, 16, 8, 128, is16=False)          # fp32
    assert not covers(64, 96, 3, 1, 1, 16, 8, 16, 8, 128)                      # C_out % 64
    assert not covers(64, 64, 3, 1, 1, 12, 16, 12, 16, 192)                    # OH * OW % 128
    assert not covers(64, 64, 3, 1, 1, 8, 4, 8, 4, 128)                        # OW = 4
    # the LDS ring: three stages of (dY tile + halo patch rounded up to whole DMA instructions) fit 160 KB
    for ow in (8, 16, 32):
        _, _, nslot = halo_dims(ow)
        assert 3 * (TPK * 64 + (nslot + 63) // 64 * 64 * 64) * 2 <= 160 * 1024                 # (8 waves x 8 slots per DMA pass)
        assert (slice_slot(7, ow) + 4) * 128 < 65536                           # the reads' immediate offsets


def test_split_rule():
    for B, cin, cout, h, w in PRODUCTION:
        splits, per = taps_splits(B * h * w, cin, cout)
        assert per % 64 == 0 and (splits - 1) * per < B * h * w <= splits * per
        assert 160 <= splits * (cin // 64) * (cout // 64) <= 256               # at most one workgroup per CU
    assert taps_splits(5 * 128, 64, 64, 2) == (2, 384)                         # (3, 2) k-steps: the last split is short
    assert taps_splits(5 * 128, 64, 64, 1) == (1, 640)


# ------------------------------------------------------------------------------------ the library's own answer
def _lib():
    from centroids_reid_amd import _lib as L
    return L, L.lib()


def _ws_bytes(L, lib, B, h, w, cin, cout, k, s, dtype):
    p = k // 2
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    d = L.ConvDesc(B, h, w, cin, oh, ow, cout, k, k, s, p)
    return int(lib.creid_conv2d_wgrad_workspace_bytes(C.byref(d), L._DT[dtype]))


def tile_splits(M, cout, K):
    """plan_wgrad's built-in rule for a 16-bit shape without a measured plan (defaults of its environment knobs)"""
    tm = 128 if cout % 128 == 0 else 64
    tn = 128 if K % 128 == 0 else 64
    tiles = (cout // tm) * (K // tn)
    splits = (512 + tiles - 1) // tiles
    if splits >= 8:
        splits = (splits + 4) // 8 * 8
    splits = max(1, min(splits, (M + 255) // 256))
    per = ((M + splits - 1) // splits + 63) // 64 * 64
    return (M + per - 1) // per


def test_workspace_bytes_follow_the_route(monkeypatch):
    """creid_conv2d_wgrad_workspace_bytes = splits * NCO * K * 4 with the split count of the route actually taken: the tap-fused
    rule with the switch on (the default), the tile kernels' built-in rule with CREID_WGRAD_TAPS=0 (measured plans cleared, so
    that the rule is the one mirrored here); shapes the route does not cover do not see the switch."""
    L, lib = _lib()
    monkeypatch.setenv("CREID_DEBUG_KNOBS", "1")
    for v in ("CREID_WGRAD_TAPS_WGS", "CREID_WGRAD_TARGET_WGS", "CREID_WGRAD_MAX_SPLITS", "CREID_WGRAD_XCD"):
        monkeypatch.delenv(v, raising=False)
    shapes = PRODUCTION + [(b, ci, co, hh, ww) for ci, co in CHANNELS for hh, ww in SIZES for b in BATCHES]
    try:
        lib.creid_tune_clear()
        for dtype in (torch.bfloat16, torch.float16):
            for B, cin, cout, h, w in shapes:
                M, K = B * h * w, 9 * cin
                monkeypatch.setenv("CREID_WGRAD_TAPS", "1")
                on = _ws_bytes(L, lib, B, h, w, cin, cout, 3, 1, dtype)
                assert on == taps_splits(M, cin, cout)[0] * cout * K * 4, (B, cin, cout, h, w)
                monkeypatch.setenv("CREID_WGRAD_TAPS", "0")
                assert _ws_bytes(L, lib, B, h, w, cin, cout, 3, 1, dtype) == tile_splits(M, cout, K) * cout * K * 4, (B, cin, cout, h, w)
                monkeypatch.delenv("CREID_WGRAD_TAPS")
                assert _ws_bytes(L, lib, B, h, w, cin, cout, 3, 1, dtype) == on              # on by default
        monkeypatch.setenv("CREID_WGRAD_TAPS_WGS", "2")
        assert _ws_bytes(L, lib, 5, 16, 8, 64, 64, 3, 1, torch.bfloat16) == 2 * 64 * 576 * 4
        monkeypatch.delenv("CREID_WGRAD_TAPS_WGS")
        # not covered: stride 2, 1 x 1, fp32, OW = 4
        for B, h, w, cin, cout, k, s, dtype in [(2, 16, 16, 128, 128, 3, 2, torch.bfloat16), (2, 16, 8, 64, 256, 1, 1, torch.bfloat16),
                                                (2, 16, 8, 64, 64, 3, 1, torch.float32), (2, 8, 4, 64, 64, 3, 1, torch.bfloat16)]:
            monkeypatch.setenv("CREID_WGRAD_TAPS", "1")
            on = _ws_bytes(L, lib, B, h, w, cin, cout, k, s, dtype)
            monkeypatch.setenv("CREID_WGRAD_TAPS", "0")
            assert _ws_bytes(L, lib, B, h, w, cin, cout, k, s, dtype) == on
            if dtype != torch.float32:
                oh, ow = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
                assert on == tile_splits(B * oh * ow, cout, k * k * cin) * cout * k * k * cin * 4
    finally:
        lib.creid_tune_clear()
        L.load_tuned_plans()


# ------------------------------------------------------------------------------------ operands and fp64 reference
def pm12(shape, gen, device="cpu"):
    """operands from {-2, -1, 1, 2}: every product an integer, every partial sum <= 4 * 5 * 128 < 2^24 -> exact in fp32 in ANY
    summation order, and exact in bf16 / f16 storage"""
    v = torch.randint(0, 4, shape, generator=gen, device=device)
    return torch.tensor([-2.0, -1.0, 1.0, 2.0], device=device)[v]


def ref_wgrad(x, dy):
    """stride-1 pad-1 3x3 weight gradient, OIHW fp64, tap by tap over GEMM rows (x [B,H,W,cin], dy [B,H,W,cout])"""
    B, H, W, cin = x.shape
    cout = dy.shape[3]
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    g = dy.double().reshape(-1, cout).t()
    dw = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, device=x.device)
    for r in range(3):
        for s in range(3):
            dw[:, :, r, s] = g @ xp[:, r:r + H, s:s + W, :].reshape(-1, cin)
    return dw


def test_reference_matches_torch_and_sees_index_swaps():
    gen = torch.Generator().manual_seed(5)
    x, dy = pm12((2, 4, 8, 8), gen), pm12((2, 4, 8, 16), gen)
    ref = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2).double(), (16, 8, 3, 3), dy.permute(0, 3, 1, 2).double(), padding=1)
    got = ref_wgrad(x, dy)
    assert torch.equal(got, ref)
    assert not torch.equal(got, got.flip(2)) and not torch.equal(got, got.flip(3))       # a mirrored tap order would show
    assert float(got.abs().max()) < 2.0 ** 24


# ------------------------------------------------------------------------------------ resource table
def test_taps_kernel_resource_budget():
    """Every instantiation (3 widths x 2 dtypes, all launched): no scratch, no spills, the LDS ring of its width, and at most 256
    registers -- 512 threads are two waves per SIMD."""
    import glob
    import os
    import re
    obj = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "centroids-reid_amd", "lib", "obj")
    rows = []
    for path in glob.glob(os.path.join(obj, "*.res")):
        for line in open(path):
            kv = dict(t.split("=", 1) for t in line.split() if "=" in t)
            if "wgrad_bf16_taps_kernel" in kv.get("name", ""):
                rows.append(kv)
    assert len(rows) == 6, "resource tables of the built library (centroids-reid_amd/build.py writes them)"
    for kv in rows:
        ow = int(re.search(r"taps_kernelILi(\d+)E", kv["name"]).group(1))
        _, _, nslot = halo_dims(ow)
        assert int(kv["scratch"]) == 0 and int(kv["vgpr_spill"]) == 0 and int(kv["sgpr_spill"]) == 0, kv
        assert int(kv["lds"]) == 3 * (TPK * 64 + (nslot + 63) // 64 * 64 * 64) * 2, kv
        assert int(kv["vgprs"]) + int(kv.get("agprs", 0)) <= 256, kv
