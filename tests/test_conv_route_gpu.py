"""GPU: the route creid_conv_route_describe words is the one that runs.  For each case: describe, launch, and compare with the
observables the library has -- creid_igemm_halo_launches, creid_wgrad_taps_launches and the registry's hit / decline counts --
at the smallest shapes where each branch exists.  Outputs are compared bit for bit where two routes are documented to agree
(halo / producer-consumer, c64 / tile, a declined plan / no plan)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "f16"]
FWD, DGRAD, WGRAD, STEM_FWD, STEM_WGRAD = range(5)
BNRED, JOB = 32, 128


def _L():
    from centroids_reid_amd import _lib as L
    return L


def describe(geom, op, bits, dtype):
    """geom = (B, cin, cout, k, stride, H, W), or (B, H, W) for the stem"""
    from centroids_reid_amd import layers as ly
    L = _L()
    if op >= STEM_FWD:
        d = L.ConvDesc(geom[0], geom[1], geom[2], 3, geom[1] // 2, geom[2] // 2, 64, 7, 7, 2, 3)
    else:
        B, cin, cout, k, s, H, W = geom
        d = ly.conv_desc(B, H, W, cin, cout, k, s, k // 2)[0]
    buf = C.create_string_buffer(512)
    assert L.lib().creid_conv_route_describe(C.byref(d), op, bits, L._DT[dtype], buf, len(buf)) == 0
    return buf.value.decode()


def counters():
    lib = _L().lib()
    return int(lib.creid_igemm_halo_launches()), int(lib.creid_wgrad_taps_launches())


def run_as_described(text, fn):
    """launch; "halo" / "taps" in the description <=> the matching counter advanced by one"""
    h0, t0 = counters()
    out = fn()
    h1, t1 = counters()
    assert h1 - h0 == (1 if "halo" in text else 0), text
    assert t1 - t0 == (1 if "taps" in text else 0), text
    return out


class plan:
    """one registered plan; the shipped plans on exit"""
    def __init__(self, key, word):
        self.key, self.word = key, word

    def __enter__(self):
        lib = _L().lib()
        lib.creid_tune_clear()
        assert lib.creid_tune_set(*self.key, *self.word) == 0
        return self

    def counts(self):
        lib = _L().lib()
        return int(lib.creid_tune_count(*self.key, 0)), int(lib.creid_tune_count(*self.key, 1))

    def __exit__(self, *exc):
        _L().lib().creid_tune_clear()
        _L().load_tuned_plans()


def _operands(dtype, B, cin, cout, k, s, H, W, seed):
    from centroids_reid_amd import layers as ly
    rng = np.random.default_rng(seed)
    t = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32)).to(dtype).cuda()
    oh, ow = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    w = torch.from_numpy((rng.standard_normal((cout, cin, k, k)) / (k * cin ** 0.5)).astype(np.float32)).cuda()
    return t(B, H, W, cin), t(B, oh, ow, cout), w, ly.weight_prep(w, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_c64_forward_and_its_switch(dtype, monkeypatch):
    from centroids_reid_amd import layers as ly
    geom = (1, 64, 64, 3, 1, 4, 32)                                # M = 128: one tile
    x, _, _, (krsc, _) = _operands(dtype, *geom, seed=1)
    a = describe(geom, FWD, 0, dtype)
    assert "conv3x3_c64_kernel<32," in a
    y = run_as_described(a, lambda: ly.conv2d_fwd(x, krsc, 1, 1))
    monkeypatch.setenv("CREID_C64_3X3", "0")
    b = describe(geom, FWD, 0, dtype)
    assert "igemm_bf16_halo_kernel<64," in b
    y0 = run_as_described(b, lambda: ly.conv2d_fwd(x, krsc, 1, 1))
    assert torch.equal(y, y0) and float(y.float().abs().max()) > 0.1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_halo_and_taps_and_their_switches(dtype, monkeypatch):
    from centroids_reid_amd import layers as ly
    geom = (2, 128, 128, 3, 1, 16, 8)
    x, dy, _, (krsc, crsk) = _operands(dtype, *geom, seed=2)
    outs = {}
    for halo in ("1", "0"):
        monkeypatch.setenv("CREID_IGEMM_HALO", halo)
        for op, fn in ((FWD, lambda: ly.conv2d_fwd(x, krsc, 1, 1)), (DGRAD, lambda: ly.conv2d_dgrad(dy, crsk, (16, 8), 1, 1))):
            text = describe(geom, op, 0, dtype)
            assert ("igemm_bf16_halo_kernel<128," if halo == "1" else "igemm_bf16_ws_kernel<") in text, text
            outs[halo, op] = run_as_described(text, fn)
    for op in (FWD, DGRAD):
        assert torch.equal(outs["1", op], outs["0", op])
    dws = {}
    for taps in ("1", "0"):
        monkeypatch.setenv("CREID_WGRAD_TAPS", taps)
        text = describe(geom, WGRAD, 0, dtype)
        assert ("wgrad_bf16_taps_kernel<8," if taps == "1" else "wgrad_bf16_dma_kernel<") in text, text
        dws[taps] = run_as_described(text, lambda: ly.conv2d_wgrad(x, dy, 3, 1, 1))
    # the two routes sum the same 256 exact fp32 products per element in another order: each is within n * 2^-24 * sum|terms|
    bound = 2 * 256 * 2.0 ** -24 * 256 * float(x.float().abs().max()) * float(dy.float().abs().max())
    assert float(dws["0"].abs().max()) > 0.1 and float((dws["1"] - dws["0"]).abs().max()) <= bound


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stride2_data_gradient_runs_parity_rows(dtype):
    from centroids_reid_amd import layers as ly
    geom = (2, 128, 128, 3, 2, 16, 16)                             # M / 4 = 128: one tile per parity class
    _, dy, w, (_, crsk) = _operands(dtype, *geom, seed=3)
    text = describe(geom, DGRAD, 0, dtype)
    assert "igemm_bf16_ws_kernel<" in text and " parity=1" in text
    dx = run_as_described(text, lambda: ly.conv2d_dgrad(dy, crsk, (16, 16), 2, 1))
    _, crsk32 = ly.weight_prep(w, torch.float32)
    ref = ly.conv2d_dgrad(dy.float(), crsk32, (16, 16), 2, 1)
    assert "igemm_f32_kernel<" in describe(geom, DGRAD, 0, torch.float32)
    # 16-bit weights and outputs against the exact-f32 kernel on the same 16-bit dy: two roundings of <= 2^-8 (bf16) per element
    err = float((dx.float() - ref).norm() / ref.norm())
    assert err <= 2.0 ** -7, err


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_planned_and_applied_or_declined(dtype):
    from centroids_reid_amd import layers as ly
    geom = (2, 64, 256, 1, 1, 16, 8)
    x, _, _, (krsc, _) = _operands(dtype, *geom, seed=4)
    key = (1, 256, 256, 64, 2)                                     # kind, M, N, K, transposed | stride << 1
    base_text = describe(geom, FWD, 0, dtype)
    base = run_as_described(base_text, lambda: ly.conv2d_fwd(x, krsc, 1, 0))
    with plan(key, (128, 3, 4)) as p:                              # kind 4: the second streamed kernel; p1 = 3: slabs of <= 128 columns
        text = describe(geom, FWD, 0, dtype)
        assert "igemm1x1_stream2_kernel<128, 1, 2," in text and "plan=hit" in text
        assert p.counts() == (0, 0), "describing must not count"
        y = run_as_described(text, lambda: ly.conv2d_fwd(x, krsc, 1, 0))
        assert p.counts() == (1, 0)
    bad_bn = 1 | (3 << 2) | (2 << 4)                               # kind 5 with 384-column tiles: 256 % 384 != 0
    with plan(key, (bad_bn, 0, 5)) as p:
        text = describe(geom, FWD, 0, dtype)
        assert "plan=declined" in text and text.split(" | ")[0] == base_text.split(" | ")[0]
        y2 = run_as_described(text, lambda: ly.conv2d_fwd(x, krsc, 1, 0))
        assert p.counts() == (1, 1)
    assert torch.equal(y2, base)
    # (the streamed kernel sums the same 64 products per output in fp32: at most the last place of the 16-bit result moves)
    assert float((y.float() - base.float()).norm() / base.float().norm()) <= 2.0 ** -8


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_reduction_carries_the_reduce_job(dtype):
    """1 x 1, 256 -> 64 data gradient with the next BatchNorm backward's reduction fused and the previous weight gradient's split
    reduction riding in the grid: same dx and partials as without the job, same dw as the job launched alone"""
    from centroids_reid_amd import layers as ly
    L = _L()
    lib, dt = L.lib(), L._DT[dtype]
    geom = (2, 256, 64, 1, 1, 16, 8)
    x, dy, _, (_, crsk) = _operands(dtype, *geom, seed=5)
    rng = np.random.default_rng(6)
    mean = torch.from_numpy(rng.standard_normal(256).astype(np.float32)).cuda()
    invstd = torch.from_numpy(rng.uniform(0.5, 2.0, 256).astype(np.float32)).cuda()
    act = torch.relu(x)
    wg = (2, 64, 64, 3, 1, 8, 8)                                   # the carried job: a 3 x 3, 64 -> 64 weight gradient's partials
    wx, wdy, _, _ = _operands(dtype, *wg, seed=7)
    wd = ly.conv_desc(2, 8, 8, 64, 64, 3, 1, 1)[0]
    nbytes = lib.creid_conv2d_wgrad_workspace_bytes(C.byref(wd), dt)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    L.check(lib.creid_conv2d_wgrad_partials(C.byref(wd), L.ptr(wx), L.ptr(wdy), L.ptr(ws), nbytes, dt, L.stream()), "partials")
    dw_alone = torch.zeros((64, 64, 3, 3), dtype=torch.float32, device="cuda")
    L.check(lib.creid_conv2d_wgrad_reduce_job(C.byref(wd), L.ptr(dw_alone), 0, L.ptr(ws), nbytes, dt, L.stream()), "reduce job")
    text = describe(geom, DGRAD, BNRED | JOB | (64 << 16), dtype)
    assert "igemm_bf16_ws_kernel<" in text and " wred=64" in text and "pre=" not in text
    d = ly.conv_desc(2, 16, 8, 256, 64, 1, 1, 0)[0]
    dx = torch.empty((2, 16, 8, 256), dtype=dtype, device="cuda")
    part = torch.empty((lib.creid_bn2d_bwd_rows(256), 2, 256), dtype=torch.float32, device="cuda")
    dw = torch.zeros_like(dw_alone)
    run_as_described(text, lambda: L.check(lib.creid_conv2d_dgrad_fused_nhwc(
        C.byref(d), L.ptr(dy), L.ptr(crsk), L.ptr(dx), None, 1, None, L.ptr(x), L.ptr(act), None, L.ptr(mean), L.ptr(invstd), L.ptr(part),
        0, C.byref(wd), L.ptr(dw), 0, L.ptr(ws), nbytes, dt, L.stream()), "dgrad_fused"))
    dx0, part0 = ly.conv2d_dgrad_bnred(dy, crsk, (16, 8), 1, 0, x, act, mean, invstd)
    assert torch.equal(dx, dx0) and torch.equal(part, part0) and torch.equal(dw, dw_alone)
    assert float(dw.abs().max()) > 0.1 and float(dx.float().abs().max()) > 0.1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stem_runs_its_dma_kernels(dtype):
    from centroids_reid_amd import layers as ly
    B, H, W = 2, 32, 16
    rng = np.random.default_rng(8)
    img = torch.from_numpy(rng.standard_normal((B, 3, H, W)).astype(np.float32)).cuda()
    w = torch.from_numpy((rng.standard_normal((64, 3, 7, 7)) / 12.0).astype(np.float32)).cuda()
    xpad, ws = ly.stem_prepare(img, w, dtype)
    text = describe((B, H, W), STEM_FWD, 0, dtype)
    assert "igemm_bf16_dma_kernel<64, 2," in text
    y = run_as_described(text, lambda: ly.stem_conv_fwd(xpad, ws, B, H, W))
    ref = torch.nn.functional.conv2d(img.to(dtype).float().cpu(), w.to(dtype).float().cpu(), stride=2, padding=3).permute(0, 2, 3, 1)
    assert float((y.float().cpu() - ref).norm() / ref.norm()) <= 2.0 ** -8    # one output rounding (<= 2^-9 relative) on exact operands
    text = describe((B, H, W), STEM_WGRAD, 0, dtype)
    assert "wgrad_bf16_dma_kernel<" in text
    dy = torch.from_numpy(rng.standard_normal((B, H // 2, W // 2, 64)).astype(np.float32)).to(dtype).cuda()
    dw = run_as_described(text, lambda: ly.stem_conv_wgrad(xpad, dy, B, H, W))
    assert bool(torch.isfinite(dw).all()) and float(dw.abs().max()) > 0.1
