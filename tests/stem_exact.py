"""Exact checks of the stem convolution (7 x 7, stride 2, pad 3, 3 -> 64 channels on the pre-padded NHWC4 image) against the fp64
reference of tests/conv_exact.py (shared by tests/test_stem_exact_gpu.py and tests/test_stem_exact_cpu.py).

Operands are small integers ({-2..2}: image, weights, incoming gradient): every product is an integer, every forward sum is
bounded by 4 * 147 = 588 and every weight-gradient sum by 4 M (M = B * H/2 * W/2 <= 2304 here), both far below 2^24.  The fp32
accumulators are therefore exact in any summation order, tile, k-step or split, the fp64 reference is exact however its GEMM
runs, and the expected 16-bit output is the one correctly rounded value of the exact result (|y| <= 588 < the f16 maximum).  So
outputs are compared bit for bit (as values: +0 == -0), the fp32 output and the whole fp32 weight gradient included; a missing,
extra or misplaced product term changes a result by >= 1.  The folded affine uses conv_exact.run_geometry's choice -- a dyadic
scale k / 2 (here with a random sign) and a shift j / 4 per channel -- so y * scale + shift is a multiple of 1/4 below 2^11:
exactly representable in fp32 (asserted), and the epilogue's single fp32 multiply-add has one possible answer.

The reference is conv_exact.ref_fwd / ref_wgrad with k = 7, s = 2, p = 3 on the NHWC [B, H, W, 3] image -- for even H and W
exactly the stem.  What ties it to the kernels' operands is the LAYOUT CONTRACT, modelled here in fp64 without a GPU
(`ref_xpad`, `ref_w_stem`, `packed_gemm`) and proven equal to F.conv2d by tests/test_stem_exact_cpu.py:

  xpad   [B, H + 8, W + 6, 4]   the image at rows 3 .. H + 2, columns 3 .. W + 2, channels 0 .. 2; zeros elsewhere
  w_stem [64][8][32]            k = r * 32 + s * 4 + c; zero at r == 7, s == 7, c == 3
  GEMM   row m -> (b, oy, ox);  A[m, r * 32 + s * 4 + c] = xpad[b, 2 oy + r, 2 ox + s, c];  y[m, o] = sum_k A[m, k] w_stem[o, k]

`run_stem(B, H, W, dtype)` drives, over the C ABI and with every output pre-filled with NaN (an element no launch writes is a
mismatch): the layout pass, the weight pass, the training forward with and without statistics, the folded-affine forward with
and without ReLU, the weight gradient plain and accumulating (NaN-filled workspace of the size the library asks for) and --
where creid_stem_conv_pool_fwd_affine accepts the shape -- the one-launch stem with its max-pool."""
import zlib

import torch
import torch.nn.functional as F

import conv_exact as ce

E_ARG, E_DTYPE, E_WS, E_SHAPE = -1, -2, -3, -4            # include/creid.h
PAD = 3                                                   # image offset inside xpad (rows and columns)

# (B, H, W): what each shape exercises is tabulated in tests/test_stem_exact_gpu.py and profiles/stem_exact_sweep.md
GROUP_A = [(1, 2, 2), (3, 2, 2), (1, 2, 6), (2, 6, 2), (1, 4, 4), (2, 10, 6), (3, 14, 10), (1, 4, 128), (3, 2, 128), (2, 6, 64),
           (1, 2, 64), (1, 2, 258), (1, 2, 254), (5, 6, 10), (1, 2, 320), (9, 16, 8), (3, 20, 40)]


# ------------------------------------------------------------------------------------ the layout contract (no GPU)
def ref_xpad(x_nchw, dtype=torch.float64):
    """NCHW [B, 3, H, W] -> the stem operand [B, H + 8, W + 6, 4] in `dtype`: F.pad + permute + a zero 4th channel"""
    B, _, H, W = x_nchw.shape
    xp = F.pad(x_nchw.double(), (PAD, W + 6 - PAD - W, PAD, H + 8 - PAD - H))       # (left, right, top, bottom)
    xp = torch.cat([xp, torch.zeros_like(xp[:, :1])], 1).permute(0, 2, 3, 1).contiguous()
    assert tuple(xp.shape) == (B, H + 8, W + 6, 4)
    return xp.to(dtype)


def ref_w_stem(w_oihw, dtype=torch.float64):
    """OIHW [64, 3, 7, 7] -> [64][8][32], k = r * 32 + s * 4 + c, zero at r == 7, s == 7, c == 3"""
    ws = torch.zeros(64, 8, 8, 4, dtype=torch.float64, device=w_oihw.device)
    ws[:, :7, :7, :3] = w_oihw.double().permute(0, 2, 3, 1)
    return ws.view(64, 8, 32).to(dtype)


def packed_gemm(xpad, w_stem, B, H, W):
    """The GEMM the kernels implement on the packed operands, fp64: y [B, H/2, W/2, 64] and the largest (row, column) index of
    xpad it reads"""
    oh, ow = H // 2, W // 2
    rows = 2 * torch.arange(oh)[:, None] + torch.arange(8)[None, :]                  # [oh, 8]: 2 oy + r
    cols = 2 * torch.arange(ow)[:, None] + torch.arange(8)[None, :]                  # [ow, 8]: 2 ox + s
    a = xpad.double()[:, rows[:, :, None, None], cols[None, None, :, :], :]          # [B, oh, 8, ow, 8, 4]
    a = a.permute(0, 1, 3, 2, 4, 5).reshape(B * oh * ow, 256)
    y = a @ w_stem.double().reshape(64, 256).t()
    return y.view(B, oh, ow, 64), int(rows.max()), int(cols.max())


# ------------------------------------------------------------------------------------ the GPU run
def fused_accepts(H, W, dtype):
    """what creid_stem_conv_pool_fwd_affine covers (include/creid.h)"""
    return dtype != torch.float32 and W in (128, 320) and H % 8 == 0


def wgrad_splits(B, H, W, dtype):
    """split count of the stem weight gradient, from the workspace the library asks for ([splits][64][256] fp32)"""
    from centroids_reid_amd import _lib as L
    return max(1, int(L.lib().creid_stem_conv_wgrad_workspace_bytes(B, H, W, L._DT[dtype])) // (64 * 256 * 4))


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def run_stem(B, H, W, dtype):
    """One shape through every stem launch; returns the conv_exact.Sweep that holds the counts and, in `failures`, one line per
    launch that differs (geometry, mismatch count, first differing element)."""
    from centroids_reid_amd import _lib as L
    lib, st, dt = L.lib(), L.stream(), L._DT[dtype]
    sw = ce.Sweep(dtype, False)
    geom = f"stem B={B} {H}x{W} {str(dtype).replace('torch.', '')}"
    oh, ow = H // 2, W // 2
    M = B * oh * ow
    key = (M, 64, 256)
    gen = torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(("stem", B, H, W)).encode()))

    def ints(shape_, lo=-2, hi=2):
        return torch.randint(lo, hi + 1, shape_, generator=gen, device="cuda", dtype=torch.int8)

    x8, w8, dy8 = ints((B, 3, H, W)), ints((64, 3, 7, 7)), ints((B, oh, ow, 64))
    dw0 = ints((64, 3, 7, 7), -3, 3).float()
    sign = torch.randint(0, 2, (64,), generator=gen, device="cuda") * 2 - 1
    ss = torch.stack([torch.randint(1, 5, (64,), generator=gen, device="cuda") * 0.5 * sign,
                      torch.randint(-8, 9, (64,), generator=gen, device="cuda") * 0.25]).float().contiguous()
    x_nchw, w_oihw, dy = x8.float().contiguous(), w8.float().contiguous(), dy8.to(dtype).contiguous()

    def ok(rc, what):
        if rc != 0:
            sw.failures.append(f"{what} {geom}: returned {rc}")
        return rc == 0

    def go(name, fn):
        return sw.launch(key, name, fn, geom)

    # ---- launches (every output NaN-filled first)
    xpad, w_stem = _nan((B, H + 8, W + 6, 4), dtype), _nan((64, 8, 32), dtype)
    ok(go("layout", lambda: lib.creid_image_to_nhwc4_pad(L.ptr(x_nchw), B, H, W, dt, L.ptr(xpad), st)), "layout")
    ok(go("weights", lambda: lib.creid_stem_weight_prep(L.ptr(w_oihw), dt, L.ptr(w_stem), st)), "weights")
    rows = (M + 127) // 128
    y_st, part, y_pl = _nan((M, 64), dtype), _nan((rows, 2, 64), torch.float32), _nan((M, 64), dtype)
    ok(go("fwd", lambda: lib.creid_stem_conv_fwd(B, H, W, L.ptr(xpad), L.ptr(w_stem), L.ptr(y_st), L.ptr(part), dt, st)), "fwd")
    ok(go("fwd_nostats", lambda: lib.creid_stem_conv_fwd(B, H, W, L.ptr(xpad), L.ptr(w_stem), L.ptr(y_pl), None, dt, st)),
       "fwd_nostats")
    y_aff = {}
    for relu in (0, 1):
        y_aff[relu] = _nan((M, 64), dtype)
        ok(go(f"aff_relu{relu}", lambda: lib.creid_stem_conv_fwd_affine(B, H, W, L.ptr(xpad), L.ptr(w_stem), L.ptr(y_aff[relu]),
                                                                         L.ptr(ss), relu, dt, st)), f"aff_relu{relu}")
    nbytes = int(lib.creid_stem_conv_wgrad_workspace_bytes(B, H, W, dt))
    sw.splits = max(1, nbytes // (64 * 256 * 4))
    if nbytes < 64 * 256 * 4 or nbytes % (64 * 256 * 4):
        sw.failures.append(f"wgrad {geom}: workspace of {nbytes} bytes is no whole number of [64][256] fp32 partial tiles")
    ws = _nan((max(nbytes, 16) // 4,), torch.float32)
    dw, dw_acc = _nan((64, 3, 7, 7), torch.float32), dw0.clone()
    ok(go("wgrad", lambda: lib.creid_stem_conv_wgrad(B, H, W, L.ptr(xpad), L.ptr(dy), L.ptr(dw), 0, L.ptr(ws), nbytes, dt, st)),
       "wgrad")
    ws.fill_(float("nan"))
    ok(go("wgrad_acc", lambda: lib.creid_stem_conv_wgrad(B, H, W, L.ptr(xpad), L.ptr(dy), L.ptr(dw_acc), 1, L.ptr(ws), nbytes, dt,
                                                          st)), "wgrad_acc")
    y_pool = {}
    if fused_accepts(H, W, dtype):
        for relu in (0, 1):
            y_pool[relu] = _nan((B * (oh // 2) * (ow // 2), 64), dtype)
            ok(go(f"pool_relu{relu}", lambda: lib.creid_stem_conv_pool_fwd_affine(B, H, W, L.ptr(xpad), L.ptr(w_stem),
                                                                                   L.ptr(y_pool[relu]), L.ptr(ss), relu, dt, st)),
               f"pool_relu{relu}")
    torch.cuda.synchronize()

    # ---- references and comparisons
    state = {}
    rd = (lambda t: ce._rd(t, dtype)) if dtype != torch.float32 else (lambda t: t.float().double())
    sw.compare("layout", geom, key, xpad.view(-1, 4), ref_xpad(x8, dtype).view(-1, 4), 0, state)
    sw.compare("weights", geom, key, w_stem.view(64, 256), ref_w_stem(w8, dtype).view(64, 256), 0, state)
    w4 = w_stem.view(64, 8, 8, 4).double()
    zeros = torch.cat([w4[:, 7].reshape(64, -1), w4[:, :, 7].reshape(64, -1), w4[:, :, :, 3].reshape(64, -1)], 1)
    sw.compare("weights_zero_entries", geom, key, zeros, torch.zeros_like(zeros), 0, state)

    x_nhwc = x8.permute(0, 2, 3, 1).contiguous()
    y = ce.ref_fwd(x_nhwc, w8, 2, PAD, 0, B).reshape(M, 64)
    ypad = F.pad(y, (0, 0, 0, (-M) % 128)).view(-1, 128, 64)               # rows beyond M contribute nothing
    tile = (ypad.sum(1), (ypad * ypad).sum(1), ypad.abs().amax(1))
    sw.sumsq_exact = bool((128 * tile[2] * tile[2] < 2.0 ** 24).all())    # else _check_stats falls back on ce.SUMSQ_REL
    ce._check_stats(sw, "fwd", geom, key, part.double(), tile, 0, state)
    sw.compare("fwd", geom, key, y_st, rd(y), 0, state)
    sw.compare("fwd_nostats", geom, key, y_pl, rd(y), 0, state)
    v = y * ss[0].double() + ss[1].double()
    assert torch.equal(v.float().double(), v), "the affine result must be exactly representable in fp32"
    for relu in (0, 1):
        e = rd(torch.relu(v) if relu else v)
        sw.compare(f"aff_relu{relu}", geom, key, y_aff[relu], e, 0, state)
        if relu in y_pool:
            # conv -> affine -> (ReLU) -> ONE rounding -> 3 x 3 / 2 pad-1 max-pool: rounding is monotone, so the maximum of the
            # rounded values is the exact answer
            pooled = F.max_pool2d(e.view(B, oh, ow, 64).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).reshape(-1, 64)
            sw.compare(f"pool_relu{relu}", geom, key, y_pool[relu], pooled, 0, state)
    dwr = ce.ref_wgrad(x_nhwc, dy8, 7, 2, PAD)
    sw.compare("wgrad", geom, key, dw.view(64, -1), dwr.view(64, -1), 0, state)
    sw.compare("wgrad_acc", geom, key, dw_acc.view(64, -1), (dwr + dw0.double()).view(64, -1), 0, state)
    sw.report(geom, state)
    return sw
