"""The stem convolution (7 x 7, stride 2, pad 3, 3 -> 64 channels on the pre-padded NHWC4 image; stem_geom of csrc/conv_common.hpp:
32-element taps, pitch 4, K = 256 of which 147 are real, no bounds check) checked EXACTLY against fp64 at ragged, tiny and
odd-width shapes -- tests/stem_exact.py: operands in {-2..2}, every result an exact integer, 16-bit outputs the one correctly
rounded value, every output and the weight gradient's workspace pre-filled with NaN.  fp32 runs igemm_f32_kernel and
wgrad_f32_kernel, bf16 and f16 run igemm_bf16_dma_kernel<64, 2> and wgrad_bf16_dma_kernel<64, 128> on its stem route; all three
run image_pad_kernel and stem_weight_prep_kernel.

  A  shapes chosen for a branch that can break (table below); per shape the layout pass, the weight pass, the training forward
     with and without statistics, the folded-affine forward with and without ReLU, the weight gradient plain and accumulating;
  B  the one-launch stem (creid_stem_conv_pool_fwd_affine, conv_stem.hip) against fp64 conv -> affine -> (ReLU) -> one rounding
     -> max-pool -- its first check that does not go through the tile kernel -- in its three forms, and its three refusals;
  C  the operand the input transforms write (DeviceTransform(..., layout="stem"), what bench.py feeds): the stem forward on it
     is bit-identical to the forward on creid_image_to_nhwc4_pad of the NCHW result (the one case with real-valued operands).

Every comparison is an equality.  Counts, split counts and the measured run time: profiles/stem_exact_sweep.md."""
import random

import numpy as np
import pytest
import torch

import conv_exact as ce
import stem_exact as se

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

# ------------------------------------------------------------------------------------ A: shapes
WHY_A = {
    (1, 2, 2): "M = 1; 40 of the 49 taps fall on padding",
    (3, 2, 2): "M = 3: three images in one tile row block",
    (1, 2, 6): "OW = 3: inc_ok false in the weight gradient; W % 4 != 0 takes the generic path of image_pad_kernel",
    (2, 6, 2): "OW = 1: one-column maps",
    (1, 4, 4): "M = 4, W % 4 == 0: the vector path of image_pad_kernel with G = 3",
    (2, 10, 6): "odd output extent 5 x 3; image borders inside a tile",
    (3, 14, 10): "odd output extent 7 x 5",
    (1, 4, 128): "OW = 64, OH = 2: inc_ok with dy_rows = 1; M = 128 is exactly one 128-row tile and two 64-pixel k-steps",
    (3, 2, 128): "OW = 64, OH = 1: every k-step is a whole image, the carry into the image index fires on every step",
    (2, 6, 64): "OW = 32, OH = 3: dy_rows = 2 does not divide OH, the carry happens mid-step",
    (1, 2, 64): "OW = 32, OH = 1: 64 / OW > OH, so inc_ok is false although OW divides 64",
    (1, 2, 258): "M = 129: one row past a tile",
    (1, 2, 254): "M = 127: one row short of a tile",
    (5, 6, 10): "M = 75: ragged final 64-pixel k-step",
    (1, 2, 320): "OW = 160: does not divide 64 (the IBN-a width)",
    (9, 16, 8): "M = 288: several weight-gradient splits, the last one ragged",
    (3, 20, 40): "M = 600: three 16-bit splits (256 + 256 + 88) -- the 2-D grid; 1, 2, 4 and 8 splits take the shared-range map",
}
assert list(WHY_A) == se.GROUP_A


def _id(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def _run(shape, dtype, what, min_launches, min_compared):
    B, H, W = shape
    sw = se.run_stem(B, H, W, DT[dtype])
    print(f"{what}| {_id(shape)} {dtype}: {sw.launches} launches, {sw.compared} comparisons, {sw.splits} weight-gradient split(s)")
    assert not sw.failures, f"{what} {_id(shape)} {dtype}: {len(sw.failures)} failure(s):\n" + "\n".join(sw.failures[:40])
    # (none of these shapes brings a 128-pixel sum of squares to 2^24, where conv_exact.SUMSQ_REL would take over)
    assert sw.sumsq_exact, "a statistics sum of squares reaches 2^24: the comparison would no longer be an equality"
    # a silently skipped launch or comparison fails here: layout 1, weights 2, forward 1 + 3 statistics, forward without
    # statistics 1, affine 2, weight gradient 2 (+ 2 for the one-launch stem)
    assert sw.launches >= min_launches and sw.compared >= min_compared
    return sw


@pytest.mark.parametrize("dtype", list(DT), ids=list(DT))
@pytest.mark.parametrize("shape", se.GROUP_A, ids=_id)
def test_stem_is_exact(shape, dtype):
    _run(shape, dtype, "A", 8, 12)


def _plan_splits(M, ks):
    """plan_wgrad (csrc/conv_wgrad.hip) for the stem's 64 x 256 weight-gradient GEMM without a registered plan: two 64 x 128
    tiles, so the 512-workgroup target asks for 256 splits and the cap max_splits = ceil(M / (4 ks)) decides for every M below
    65536; a split is whole k-steps of ks pixels"""
    max_splits = max(1, -(-M // (4 * ks)))
    per = -(-(-(-M // max_splits)) // ks) * ks
    return -(-M // per), per, max_splits


def test_split_kinds_are_covered():
    """For both k-step sizes (64 pixels for the 16-bit kernels, 16 for fp32) group A holds a case with one split, a case with
    several splits of which the last is ragged (shorter than the others and no whole number of k-steps), and a case that
    reaches max_splits; the split counts the library plans (from its workspace size) are the mirrored rule's."""
    from centroids_reid_amd import _lib as L
    L.lib()
    for dtype, ks in (("bf16", 64), ("f16", 64), ("fp32", 16)):
        kinds = set()
        for (B, H, W) in se.GROUP_A:
            M = B * (H // 2) * (W // 2)
            assert not any((kind, M, 64, 256, mode) in ce.PLANS for kind, mode in ((0, 4), (1, 4), (1, 12))), \
                "a group A shape must not meet a shipped plan"
            splits, per, max_splits = _plan_splits(M, ks)
            got = se.wgrad_splits(B, H, W, DT[dtype])
            print(f"splits| {_id((B, H, W))} {dtype}: M = {M}, {got} split(s) of {per} pixels, max_splits {max_splits}")
            assert got == splits
            last = M - (splits - 1) * per
            kinds |= {"one"} if splits == 1 else set()
            kinds |= {"ragged"} if splits > 1 and last < per and last % ks else set()
            kinds |= {"max"} if splits == max_splits and splits > 1 else set()
        assert kinds == {"one", "ragged", "max"}, (dtype, kinds)


# ------------------------------------------------------------------------------------ B: the one-launch stem
# (B, H, W), CREID_STEM_FORM, CREID_STEM_WGS (0: the default grid)
GROUP_B = [
    ((1, 8, 128), 1, 0),          # one four-row step per image: the pool's top and bottom border in the same step
    ((2, 16, 128), 0, 0),         # one eight-row step per image (the eight-wave form)
    ((3, 24, 128), 1, 2),         # nine steps over two workgroups: a run begins inside an image, the row above is recomputed
    ((1, 8, 320), 1, 0),          # the 160-wide form, one step
    ((2, 16, 320), 1, 3),         # ... four steps over three workgroups
]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape,form,wgs", GROUP_B, ids=[f"{_id(s)}_form{f}_wgs{w}" for s, f, w in GROUP_B])
def test_one_launch_stem_is_exact(shape, form, wgs, dtype, monkeypatch):
    assert se.fused_accepts(shape[1], shape[2], DT[dtype])
    monkeypatch.setenv("CREID_STEM_FORM", str(form))
    if wgs:
        monkeypatch.setenv("CREID_STEM_WGS", str(wgs))
    _run(shape, dtype, f"B form {form} wgs {wgs}", 10, 14)


@pytest.mark.parametrize("shape,dtype,code", [((1, 8, 64), "bf16", se.E_SHAPE), ((1, 12, 128), "f16", se.E_SHAPE),
                                              ((1, 8, 128), "fp32", se.E_DTYPE)], ids=["W64", "H12", "fp32"])
def test_one_launch_stem_refuses(shape, dtype, code):
    """one refused shape per rule (W in {128, 320}; H % 8 == 0; 16-bit types): the error code, and the output untouched"""
    from centroids_reid_amd import _lib as L
    lib = L.lib()
    B, H, W = shape
    dt = DT[dtype]
    assert not se.fused_accepts(H, W, dt)
    xpad = torch.zeros((B, H + 8, W + 6, 4), device="cuda", dtype=dt)
    w = torch.zeros((64, 256), device="cuda", dtype=dt)
    ss = torch.ones((2, 64), device="cuda")
    y = torch.full((B, H // 4, W // 4, 64), float("nan"), device="cuda", dtype=dt)
    for relu in (0, 1):
        assert lib.creid_stem_conv_pool_fwd_affine(B, H, W, L.ptr(xpad), L.ptr(w), L.ptr(y), L.ptr(ss), relu, L._DT[dt],
                                                   L.stream()) == code
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


# ------------------------------------------------------------------------------------ C: the transforms' operand
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stem_on_the_transforms_operand(dtype):
    from centroids_reid_amd import _lib as L
    from centroids_reid_amd.transforms import DeviceTransform, StemOperand
    lib, st, dt = L.lib(), L.stream(), DT[dtype]
    B, H, W = 2, 6, 10
    imgs = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
    t = DeviceTransform((H, W), [0.485, 0.456, 0.406], [0.229, 0.224, 0.225], is_train=True, padding=2)
    params = t.draw(B, rnd=random.Random(3), generator=torch.Generator().manual_seed(4))
    params[0, :3] = (1, 0, 0)                                                # flipped, cropped at the black border
    params[0, 3:] = (1, 1, 2, 3, 4)                                          # with an erased block
    x_nchw = t(imgs, params).contiguous()
    op = t(imgs, params, layout="stem", dtype=dt)
    assert isinstance(op, StemOperand) and tuple(op.xpad.shape) == (B, H + 8, W + 6, 4) and op.xpad.dtype == dt
    xpad = torch.full_like(op.xpad, float("nan"))
    L.check(lib.creid_image_to_nhwc4_pad(L.ptr(x_nchw), B, H, W, L._DT[dt], L.ptr(xpad), st), "image_pad")
    gen = torch.Generator(device="cuda").manual_seed(11)
    w8 = torch.randint(-2, 3, (64, 3, 7, 7), generator=gen, device="cuda").float()
    w_stem = torch.full((64, 8, 32), float("nan"), device="cuda", dtype=dt)
    L.check(lib.creid_stem_weight_prep(L.ptr(w8), L._DT[dt], L.ptr(w_stem), st), "stem_weight_prep")
    M = B * (H // 2) * (W // 2)
    outs = []
    for operand in (op.xpad, xpad):
        y = torch.full((M, 64), float("nan"), device="cuda", dtype=dt)
        part = torch.full(((M + 127) // 128, 2, 64), float("nan"), device="cuda")
        L.check(lib.creid_stem_conv_fwd(B, H, W, L.ptr(operand), L.ptr(w_stem), L.ptr(y), L.ptr(part), L._DT[dt], st), "stem_conv_fwd")
        outs.append((y, part))
    torch.cuda.synchronize()
    compared = 0
    for a, b in ((op.xpad, xpad), (outs[0][0], outs[1][0]), (outs[0][1], outs[1][1])):
        assert bool(torch.isfinite(a.float()).all()) and bool(torch.isfinite(b.float()).all())
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
        compared += 1
    assert float(outs[0][0].float().abs().max()) > 0
    print(f"C| {B}x{H}x{W} {dtype}: 4 launches, {compared} comparisons")
    assert compared == 3
