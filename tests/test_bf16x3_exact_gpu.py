"""GPU: the bf16x3 convolutions (igemm_x3_kernel<64 | 128> forward and data gradient, wgrad_x3_kernel<TM, TN>) EXACTLY against the
three-term fp64 reference of tests/x3_exact.py, with all three MFMA passes contributing.

Operands come from the grid a + b 2^-11 (x3_exact.grid_operands): the kernels' split gives an integer hi plane and a busy lo plane
(non-zero in 4/7 of the elements), every term is a multiple of 2^-11 and every fp32 partial sum is exact in any order while
x3_exact.exactness_margin stays below 1 -- asserted for every output before anything is compared.  The result is then one fixed
number, so every comparison is equality of values over the whole tensor (+0 == -0); a lo element staged in the wrong row, chunk
or plane, a missing pass, or a misaddressed weight lo plane changes almost every output (tests/test_bf16x3_exact_cpu.py measures
how many).  The only tolerance is on the sums of squares of the statistics, whose terms are not exact (see test_fwd_stats_exact).
The small-integer tests of tests/test_bf16x3_train_gpu.py, whose lo planes are all zero, see one of the three passes."""
import ctypes as C
import zlib

import pytest
import torch
import torch.nn.functional as F

import x3_exact as xe

pytestmark = pytest.mark.gpu

# B, H, W, cin, cout, k, stride (H x W the convolution's input), each the smallest shape that reaches what its comment names
BASE_CASES = [
    (2, 16, 8, 64, 64, 1, 1),            # baseline; weight-gradient tile 64 x 64 (K = 64)
    (2, 16, 8, 64, 64, 3, 1),            # ... K = 576
    (1, 10, 10, 64, 256, 1, 1),          # M = 100: ragged single tile, one weight-gradient split longer than M; tile 128 x 64
    (2, 16, 8, 256, 64, 1, 1),           # weight-gradient tile 64 x 128
    (4, 16, 8, 128, 128, 3, 2),          # stride-2 3 x 3 (absent taps stage zeros); weight-gradient tile 128 x 128
    (2, 15, 9, 256, 512, 1, 2),          # stride-2 1 x 1 on odd H and W
]
FWD_CASES = BASE_CASES + [
    (2, 8, 4, 512, 512, 3, 1),           # K = 4608, M = 64: half a tile
    (16, 64, 32, 64, 256, 1, 1),         # igemm_x3_kernel<128> exactly at the threshold (256 x 2 workgroups)
    (255, 16, 8, 64, 256, 1, 1),         # 510 workgroups of 128 x 128: <64> at N = 256, one step under the threshold
    (2, 181, 181, 64, 128, 3, 1),        # <128>, 3 x 3, ragged last tile (M = 65 522), odd row length
]
FWD_STATS_CASES = FWD_CASES
FWD_AFFINE_CASES = FWD_CASES
DGRAD_CASES = BASE_CASES + [
    (2, 8, 4, 512, 512, 3, 1),           # K = 4608, M = 64
    (16, 64, 32, 256, 64, 1, 1),         # <128> data gradient (N = cin = 256, M = 32 768)
    (16, 64, 32, 256, 128, 3, 2),        # <128> with the stride-2 3 x 3 gather
    (3, 105, 104, 256, 512, 1, 2),       # <128>, ragged last tile (M = 32 760), stride-2 1 x 1, odd H
]
WGRAD_CASES = BASE_CASES + [
    (1, 75, 75, 64, 64, 1, 1),           # M = 5625: 88 splits of 64 pixels, the last one 57 (not a multiple of the 32-pixel k-step)
    (8, 64, 32, 64, 64, 1, 1),           # M = 16 384: 256 splits (min(512 / tiles, ceil(M / 64))); dense operands near the
                                         # exactness limit (4/9 M / 8192 = 0.89)
    (2, 8, 4, 512, 512, 3, 1),           # one or two splits, K = 4608
]
# operand density per (direction, case), below 1 only where dense operands fail the margin assertion (the largest margin, the
# M = 16 384 weight gradient's, is 0.92 with dense operands)
DENSITY = {}


@pytest.fixture(scope="module")
def cache():
    """operands and fp64 references on the device, computed once per (direction, case) and left unchanged"""
    c = {}
    yield c
    c.clear()
    torch.cuda.empty_cache()


def _gen(case, tag):
    return torch.Generator(device="cuda").manual_seed(zlib.crc32(repr((case, tag)).encode()))


def _check_lo_plane(plane, w, perm):
    """the lo plane the weight preparation wrote is split(w)[1] in the kernel's layout, and is busy"""
    want = xe.split(w)[1].permute(*perm).to(torch.bfloat16)
    assert torch.equal(plane, want), "weight lo plane differs from bf16(w - bf16(w))"
    assert bool((plane != 0).any()), "weight lo plane is all zero"


def _ready(d):
    """the conditions on the inputs: exact in any order, and an fp32 value"""
    assert d["margin"] < 1, f"operands leave the exact range (margin {d['margin']:.3f}): thin this case with DENSITY"
    assert xe.is_fp32(d["ref"])


def _fwd(cache, case):
    if ("fwd", case) not in cache:
        from centroids_reid_amd import layers as ly
        B, H, W, cin, cout, k, s = case
        p = k // 2
        g = _gen(case, "fwd")
        dens = DENSITY.get(("fwd", case), 1.0)
        x, w = xe.grid_operands((B, H, W, cin), g, dens), xe.grid_operands((cout, cin, k, k), g, dens)
        ref = xe.ref_fwd_x3(x, w, s, p).reshape(-1, cout)
        d = {"x": x, "w": w, "w2": ly.weight_prep_x3(w), "ref": ref, "s": s, "p": p, "gen": g,
             "margin": float(xe.exactness_margin(xe.ref_fwd_x3, x, w, s, p).max())}
        print(f"fwd {case}: igemm_x3_kernel<{xe.x3_bn(ref.shape[0], cout)}>, M {ref.shape[0]}, K {cin * k * k}, margin {d['margin']:.3f}")
        cache[("fwd", case)] = d
    return cache[("fwd", case)]


def _assert_equal(failures):
    failures = [f for f in failures if f[1] is not None]
    assert not failures, "\n".join(f"{name}: {msg}" for name, msg in failures)


@pytest.mark.parametrize("case", FWD_STATS_CASES)
def test_fwd_stats_exact(cache, case):
    """conv2d_fwd_x3(..., with_stats=True): the raw output and the column sums of every 128-row tile equal fp64 exactly (the
    sums under the same condition as the output: sum |y| of a tile below 8192, asserted).  Sums of squares: y is a multiple of
    2^-11, so y^2 is not exact in fp32; a column takes at most 34 roundings in the kernel (32 fused multiply-adds per lane, one
    lane-half add, one wave merge), each at most 2^-24 of the running sum, which the project's own derived bound
    test_plan_sweep_gpu.SUMSQ_REL = 130 * 2^-24 relative to the fp64 value covers; that bound is used here unchanged."""
    from centroids_reid_amd import layers as ly
    from test_plan_sweep_gpu import SUMSQ_REL
    d = _fwd(cache, case)
    _ready(d)
    cout, ref = case[4], d["ref"]
    _check_lo_plane(d["w2"][1], d["w"], (0, 2, 3, 1))
    y, part = ly.conv2d_fwd_x3(d["x"], d["w2"], d["s"], d["p"], with_stats=True)
    M = ref.shape[0]
    tiles = F.pad(ref, (0, 0, 0, (-M) % 128)).view(-1, 128, cout)
    assert float(tiles.abs().sum(1).max()) * xe.MARGIN_SCALE < 1
    t1, t2 = tiles.sum(1), (tiles * tiles).sum(1)
    assert xe.is_fp32(t1) and tuple(part.shape) == (tiles.shape[0], 2, cout)
    sq = part[:, 1].double()
    over = (sq - t2).abs() > SUMSQ_REL * t2
    _assert_equal([("output", xe.mismatch(y.view(-1, cout), ref)), ("tile sums", xe.mismatch(part[:, 0], t1)),
                   ("tile sums of squares beyond SUMSQ_REL", xe.mismatch(torch.where(over, sq, t2), t2))])


@pytest.mark.parametrize("case", FWD_AFFINE_CASES)
def test_fwd_affine_exact(cache, case):
    """conv2d_fwd_affine_x3 with per-channel scale in {0.5, 1, 1.5, 2} and shift in multiples of 0.25, (a) plus a grid-tensor
    residual, then ReLU and (b) neither: relu(fma(acc, scale, shift) + residual) in fp64, every stage an fp32 value (asserted),
    so the kernel's two roundings change nothing and the output equals it exactly."""
    from centroids_reid_amd import layers as ly
    d = _fwd(cache, case)
    _ready(d)
    cout, ref = case[4], d["ref"]
    if "ss" not in d:
        g = d["gen"]
        d["ss"] = torch.stack([torch.randint(1, 5, (cout,), generator=g, device="cuda") * 0.5,
                               torch.randint(-8, 9, (cout,), generator=g, device="cuda") * 0.25]).float().contiguous()
        d["res"] = xe.grid_operands(tuple(ref.shape), g)
    ss, res = d["ss"], d["res"]
    v = ref * ss[0].double() + ss[1].double()
    e_res = v + res.double()
    assert xe.is_fp32(v) and xe.is_fp32(e_res)
    _check_lo_plane(d["w2"][1], d["w"], (0, 2, 3, 1))
    oshape = (case[0], *xe.out_hw(case[1], case[2], case[5], d["s"], d["p"]), cout)
    got_res = ly.conv2d_fwd_affine_x3(d["x"], d["w2"], d["s"], d["p"], ss, res.view(oshape), True)
    got_plain = ly.conv2d_fwd_affine_x3(d["x"], d["w2"], d["s"], d["p"], ss, None, False)
    _assert_equal([("residual + ReLU", xe.mismatch(got_res.view(-1, cout), torch.relu(e_res))),
                   ("neither", xe.mismatch(got_plain.view(-1, cout), v))])


@pytest.mark.parametrize("case", DGRAD_CASES)
def test_dgrad_exact(case):
    """conv2d_dgrad_x3 without and with add_src (a grid tensor; ref + add_src is an fp32 value, asserted) equals fp64 exactly."""
    from centroids_reid_amd import layers as ly
    B, H, W, cin, cout, k, s = case
    p = k // 2
    oh, ow = xe.out_hw(H, W, k, s, p)
    g = _gen(case, "dgrad")
    dens = DENSITY.get(("dgrad", case), 1.0)
    dy, w = xe.grid_operands((B, oh, ow, cout), g, dens), xe.grid_operands((cout, cin, k, k), g, dens)
    add = xe.grid_operands((B, H, W, cin), g)
    ref = xe.ref_dgrad_x3(dy, w, s, p, H, W).reshape(-1, cin)
    d = {"ref": ref, "margin": float(xe.exactness_margin(xe.ref_dgrad_x3, dy, w, s, p, H, W).max())}
    print(f"dgrad {case}: igemm_x3_kernel<{xe.x3_bn(B * H * W, cin)}>, M {B * H * W}, K {cout * k * k}, margin {d['margin']:.3f}")
    _ready(d)
    e_add = ref + add.view(-1, cin).double()
    assert xe.is_fp32(e_add)
    krsc, crsk = ly.weight_prep_x3_train(w)
    _check_lo_plane(krsc[1], w, (0, 2, 3, 1))
    _check_lo_plane(crsk[1], w, (1, 2, 3, 0))
    got = ly.conv2d_dgrad_x3(dy, crsk, (H, W), s, p)
    got_add = ly.conv2d_dgrad_x3(dy, crsk, (H, W), s, p, add_src=add)
    _assert_equal([("dgrad", xe.mismatch(got.view(-1, cin), ref)), ("dgrad + add_src", xe.mismatch(got_add.view(-1, cin), e_add))])


@pytest.mark.parametrize("case", WGRAD_CASES)
def test_wgrad_exact(case):
    """The weight gradient in its four forms equals fp64 exactly: conv2d_wgrad_x3; accumulate=True onto a grid tensor (its
    magnitude counted in the margin); the partial tiles summed by creid_conv2d_wgrad_reduce_job(CREID_F32); and by
    creid_conv2d_wgrad_reduce(CREID_F32) -- with exact partials the two summation orders give the same bits.  The partial tiles
    themselves, summed in fp64, are checked too, which tells a wrong kernel from a wrong reduction."""
    from centroids_reid_amd import _lib as L, layers as ly
    B, H, W, cin, cout, k, s = case
    p = k // 2
    oh, ow = xe.out_hw(H, W, k, s, p)
    K = cin * k * k
    g = _gen(case, "wgrad")
    dens = DENSITY.get(("wgrad", case), 1.0)
    x, dy = xe.grid_operands((B, H, W, cin), g, dens), xe.grid_operands((B, oh, ow, cout), g, dens)
    dw0 = xe.grid_operands((cout, cin, k, k), g)
    ref = xe.ref_wgrad_x3(x, dy, k, s, p)
    margin = xe.exactness_margin(xe.ref_wgrad_x3, x, dy, k, s, p) + dw0.abs().double() * xe.MARGIN_SCALE
    d = {"ref": ref, "margin": float(margin.max())}
    lib = L.lib()
    ws, desc = ly.conv2d_wgrad_x3(x, dy, k, s, p, partials_only=True)
    nbytes = lib.creid_conv2d_wgrad_x3_workspace_bytes(C.byref(desc))
    splits = nbytes // (cout * K * 4)
    print(f"wgrad {case}: wgrad_x3_kernel<{', '.join(map(str, xe.wgrad_tile(cout, K)))}>, M {B * oh * ow}, K {K}, {splits} splits, "
          f"margin {d['margin']:.3f}")
    _ready(d)
    e_acc = ref + dw0.double()
    assert xe.is_fp32(e_acc) and splits >= 1 and nbytes == splits * cout * K * 4
    partial_sum = ws[:nbytes].view(torch.float32).view(splits, cout, k, k, cin).double().sum(0).permute(0, 3, 1, 2)
    one = ly.conv2d_wgrad_x3(x, dy, k, s, p)
    acc = ly.conv2d_wgrad_x3(x, dy, k, s, p, dw=dw0.clone(), accumulate=True)
    dw_job, dw_red = torch.zeros_like(one), torch.zeros_like(one)
    L.check(lib.creid_conv2d_wgrad_reduce_job(C.byref(desc), L.ptr(dw_job), 0, L.ptr(ws), nbytes, L.F32, L.stream()), "reduce_job")
    L.check(lib.creid_conv2d_wgrad_reduce(C.byref(desc), L.ptr(dw_red), 0, L.ptr(ws), nbytes, L.F32, L.stream()), "reduce")
    flat = ref.view(cout, -1)
    _assert_equal([("partial tiles summed in fp64", xe.mismatch(partial_sum.reshape(cout, -1), flat)),
                   ("conv2d_wgrad_x3", xe.mismatch(one.view(cout, -1), flat)),
                   ("accumulate", xe.mismatch(acc.view(cout, -1), e_acc.view(cout, -1))),
                   ("partials + reduce_job", xe.mismatch(dw_job.view(cout, -1), flat)),
                   ("partials + reduce", xe.mismatch(dw_red.view(cout, -1), flat))])
