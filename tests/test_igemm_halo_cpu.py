"""The resident-halo form of the producer/consumer convolution kernel (csrc/conv_igemm.hip igemm_bf16_halo_kernel), without a GPU:
a Python mirror of its eligibility rule, halo slot map and LDS swizzle checked against the convolution's own source pixels; the
condition that makes the exact GPU test (tests/test_igemm_halo_gpu.py) sensitive to a wrong halo border, shown on the reference
alone; and the kernel's rows of the build's resource table.

The mirror, the small-integer operands and the fp64 reference here are shared with the GPU test."""
import glob
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "centroids-reid_amd", "lib", "obj")

# (channels, B, H, W, N tile, ring depth): the smallest shapes that reach every border case -- two tiles per image (zero row above
# the first and below the second, the image boundary inside M), one tile per image (all four borders), OW = 64 / 32 / 16 / 8
CASES = [(64, 2, 8, 32, 64, 3), (64, 1, 4, 64, 64, 2), (128, 2, 16, 16, 64, 3), (128, 2, 16, 16, 128, 3),
         (256, 3, 16, 8, 64, 3), (256, 3, 16, 8, 128, 2)]
# the training step of the benchmark (B = 64, 256 x 128): layer1 / layer2 / layer3 conv2
PRODUCTION = [(64, 64, 64, 32), (128, 64, 32, 16), (256, 64, 16, 8)]


# ------------------------------------------------------------------------------------ mirror of the kernel's geometry
def halo_pw(c):
    """DMA pieces (8 slots) per producer wave per 64-channel plane"""
    return 9 if c == 64 else 6


def halo_lds_bytes(c, bn, ns):
    return ((c // 64) * 4 * halo_pw(c) * 512 + ns * bn * 64) * 2


def halo_covers(c, k, stride, pad, oh, ow, sh, sw, M, bn, ns, is16=True):
    """igemm_halo_covers (conv_igemm.hip), forward and transposed alike"""
    if not is16 or k != 3 or stride != 1 or pad != 1 or c not in (64, 128, 256):
        return False
    if (sh, sw) != (oh, ow) or ow not in (8, 16, 32, 64):
        return False
    if (oh * ow) % 128 != 0 or M % (oh * ow) != 0:
        return False
    if (128 // ow + 2) * (ow + 2) > 32 * halo_pw(c):
        return False
    if ns not in (2, 3, 4) or bn not in (64, 128):
        return False
    return halo_lds_bytes(c, bn, ns) < 160 * 1024


def swizzle_key(hr, hc, ow):
    return ((hc >> 1) + (4 * hr if ow == 8 else 0)) & 7


def read_slot(r, tr, ts, ow, transposed):
    """halo (row, column) that tile row r reads under tap (tr, ts)"""
    dr, dc = (2 - tr, 2 - ts) if transposed else (tr, ts)
    return r // ow + dr, r % ow + dc


def fill_source(slot, y0, oh, ow):
    """source pixel (iy, ix) the prologue copies into `slot` of a tile that starts at image row y0; None: the zero page"""
    nslot = (128 // ow + 2) * (ow + 2)
    hr, hc = divmod(slot, ow + 2)
    iy, ix = y0 - 1 + hr, hc - 1
    if slot >= nslot or not (0 <= iy < oh and 0 <= ix < ow):
        return None
    return iy, ix


def conv_source(oy, ox, tr, ts, oh, ow, transposed):
    """igemm_src_pixel at stride 1, pad 1"""
    iy, ix = (oy + 1 - tr, ox + 1 - ts) if transposed else (oy + tr - 1, ox + ts - 1)
    return (iy, ix) if (0 <= iy < oh and 0 <= ix < ow) else None


B128_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
               [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]     # ds_read_b128 lane groups of one k half


@pytest.mark.parametrize("oh,ow", sorted({(c[2], c[3]) for c in CASES} | {(p[2], p[3]) for p in PRODUCTION}))
@pytest.mark.parametrize("transposed", [0, 1])
def test_slot_map_reads_the_convolutions_source_pixels(oh, ow, transposed):
    """Every (tile row, tap) reads a slot inside the halo image whose filled content is exactly the source pixel of the
    convolution (or zero where that pixel lies outside the image), for every tile of an image."""
    nslot = (128 // ow + 2) * (ow + 2)
    for y0 in range(0, oh, 128 // ow):
        for r in range(128):
            oy, ox = y0 + r // ow, r % ow
            for tr in range(3):
                for ts in range(3):
                    hr, hc = read_slot(r, tr, ts, ow, transposed)
                    assert 0 <= hr < 128 // ow + 2 and 0 <= hc < ow + 2
                    slot = hr * (ow + 2) + hc
                    assert slot < nslot
                    assert fill_source(slot, y0, oh, ow) == conv_source(oy, ox, tr, ts, oh, ow, transposed)


@pytest.mark.parametrize("ow", [8, 16, 32, 64])
def test_swizzle_key_is_conflict_free_for_every_tap(ow):
    """A ds_read_b128 serves fixed groups of 16 lanes per LDS cycle, 16 bytes each over 64 banks: the 16 lanes must hit 16
    different 16-byte bank groups = (slot parity, swizzled chunk).  All lanes of a k half read the same logical chunk."""
    for wm in range(2):
        for i in range(2):
            for tr in range(3):
                for ts in range(3):
                    for ch in range(8):
                        for grp in B128_GROUPS:
                            banks = set()
                            for l31 in grp:
                                hr, hc = read_slot(wm * 64 + i * 32 + l31, tr, ts, ow, 0)
                                slot = hr * (ow + 2) + hc
                                banks.add(((slot & 1) << 3) | (ch ^ swizzle_key(hr, hc, ow)))
                            assert len(banks) == 16, (ow, wm, i, tr, ts, ch)


def test_eligibility_rule():
    for c, B, H, W, bn, ns in CASES:
        assert halo_covers(c, 3, 1, 1, H, W, H, W, B * H * W, bn, ns), (c, B, H, W)
    for c, B, H, W in PRODUCTION:
        for bn in (64, 128):
            assert halo_covers(c, 3, 1, 1, H, W, H, W, B * H * W, bn, 3), (c, B, H, W)
        assert (128 // W + 2) * (W + 2) * 128 * (c // 64) <= (c // 64) * 4 * halo_pw(c) * 1024      # the image fits its planes
    # two workgroups per CU where the issue's LDS budget says so: layer1 (C = 64) at either N tile, layer2 (C = 128) at BN = 64
    assert halo_lds_bytes(64, 64, 3) <= 80 * 1024 and halo_lds_bytes(64, 128, 2) <= 80 * 1024 and halo_lds_bytes(128, 64, 3) <= 80 * 1024
    assert not halo_covers(128, 3, 2, 1, 8, 8, 16, 16, 2 * 64, 64, 3)          # stride 2
    assert not halo_covers(512, 3, 1, 1, 16, 8, 16, 8, 128, 64, 3)             # C = 512: the halo would need 184 KB
    assert not halo_covers(64, 3, 1, 1, 80, 80, 80, 80, 6400, 64, 2)           # 80 x 80: rows do not tile 128
    assert not halo_covers(64, 1, 1, 0, 16, 8, 16, 8, 128, 64, 2)              # 1 x 1
    assert not halo_covers(64, 3, 1, 1, 16, 8, 16, 8, 128, 64, 2, is16=False)  # fp32
    assert not halo_covers(256, 3, 1, 1, 16, 8, 16, 8, 128, 128, 4)            # 96 KB halo + 64 KB ring: no room
    assert not halo_covers(128, 3, 1, 1, 32, 32, 32, 32, 1024, 64, 3)          # 204 slots > the 192 of a 24 KB plane
    assert not halo_covers(64, 3, 1, 1, 12, 16, 12, 16, 192, 64, 2)            # OH * OW % 128 != 0


# ------------------------------------------------------------------------------------ operands and fp64 reference
def pm12(shape, gen):
    """operands drawn from {-2, -1, 1, 2} (fp32): every product an integer, every sum < 4 * 2304 < 2^24 -> exact in fp32"""
    v = torch.randint(0, 4, shape, generator=gen)
    return torch.tensor([-2.0, -1.0, 1.0, 2.0])[v]


def ref_conv3x3(src, w_oihw, transposed, border="zero"):
    """Stride-1 pad-1 3x3 convolution (transposed: its data gradient, src = dY) of an NHWC tensor, fp64, tap by tap over GEMM rows.
    border = "zero": out-of-image taps contribute nothing.  "rows" / "cols": what a halo without bounds logic would read instead --
    the tensor's neighbouring rows (the next / previous image's, wrapping at the ends) for taps above / below the image, or the
    neighbouring pixel in memory (the end of the previous row) for taps left / right of it; the other direction stays zero-padded."""
    B, H, W, C = src.shape
    s = src.double().reshape(-1, C)
    wd = w_oihw.double()
    b, y, x = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing="ij")
    out = torch.zeros(B * H * W, wd.shape[1] if transposed else wd.shape[0], dtype=torch.float64)
    for r in range(3):
        for c in range(3):
            iy, ix = (y + 1 - r, x + 1 - c) if transposed else (y + r - 1, x + c - 1)
            oky, okx = (iy >= 0) & (iy < H), (ix >= 0) & (ix < W)
            ok = {"zero": oky & okx, "rows": okx, "cols": oky}[border]
            flat = (((b * H + iy) * W + ix) % (B * H * W)).reshape(-1)
            a = s[flat] * ok.reshape(-1, 1).double()
            out += a @ (wd[:, :, r, c] if transposed else wd[:, :, r, c].t())
    return out.view(B, H, W, -1)


@pytest.mark.parametrize("case", CASES[:2] + CASES[2:6:2], ids=lambda c: f"c{c[0]}_B{c[1]}_{c[2]}x{c[3]}")
@pytest.mark.parametrize("transposed", [0, 1])
def test_exact_operands_see_a_wrong_border(case, transposed):
    """With operands from {+-1, +-2}, padding with the neighbouring image's rows (or the neighbouring row's columns) instead of
    zeros changes at least 90 % of the outputs of the border rows (columns): the exact comparison of the GPU test cannot pass with
    a halo that skips its bounds logic."""
    c, B, H, W, _, _ = case
    gen = torch.Generator().manual_seed(c + B + H + W + transposed)
    src, w = pm12((B, H, W, c), gen), pm12((c, c, 3, 3), gen)
    ref = ref_conv3x3(src, w, transposed)
    rows = ref_conv3x3(src, w, transposed, "rows")
    cols = ref_conv3x3(src, w, transposed, "cols")
    brow = torch.cat([(rows != ref)[:, 0], (rows != ref)[:, -1]]).double().mean()
    bcol = torch.cat([(cols != ref)[:, :, 0], (cols != ref)[:, :, -1]]).double().mean()
    assert float(brow) >= 0.9 and float(bcol) >= 0.9, (float(brow), float(bcol))
    assert torch.equal(rows[:, 1:-1], ref[:, 1:-1]) and torch.equal(cols[:, :, 1:-1], ref[:, :, 1:-1])   # interior untouched
    assert float(ref.abs().max()) < 2.0 ** 24


def test_reference_matches_torch_conv():
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(3)
    x, w = pm12((2, 5, 6, 8), gen), pm12((8, 8, 3, 3), gen)
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    y = F.conv2d(xr, w.double(), padding=1)
    dy = pm12(tuple(y.shape), gen).double()
    (y * dy).sum().backward()
    assert torch.equal(ref_conv3x3(x, w, 0), y.detach().permute(0, 2, 3, 1))
    assert torch.equal(ref_conv3x3(dy.permute(0, 2, 3, 1).contiguous(), w, 1), xr.grad.permute(0, 2, 3, 1))


# ------------------------------------------------------------------------------------ resource table
def test_halo_kernel_resource_budget():
    """No scratch, no spills; the instantiations whose LDS lets two workgroups share a CU (<= 80 KB) stay within 128 registers
    (512 threads = 2 waves per SIMD per workgroup)."""
    rows = []
    for path in glob.glob(os.path.join(OBJ, "*.res")):
        for line in open(path):
            kv = dict(t.split("=", 1) for t in line.split() if "=" in t)
            if "igemm_bf16_halo_kernel" in kv.get("name", ""):
                rows.append(kv)
    if not rows:
        pytest.skip("no resource tables (library not built here)")
    assert len(rows) == 34                                       # 3 channel counts x 2 N tiles x 3 ring depths x 2 dtypes - 2
    two = 0
    for kv in rows:
        c, bn, ns = (int(a) for a in re.findall(r"Li(\d+)E", kv["name"].split("Ev")[0])[:3])
        assert int(kv["scratch"]) == 0 and int(kv["vgpr_spill"]) == 0 and int(kv["sgpr_spill"]) == 0, kv
        assert int(kv["lds"]) == halo_lds_bytes(c, bn, ns), kv
        regs = int(kv["vgprs"]) + int(kv.get("agprs", 0))
        if halo_lds_bytes(c, bn, ns) <= 80 * 1024:
            assert regs <= 128, kv
            two += 1
        else:
            assert regs <= 256, kv
    assert two >= 12
