"""Every shipped launch plan (centroids-reid_amd/tuned_plans.json) and the built-in rules at the same production shapes, checked
EXACTLY against an fp64 reference of the same convolution.

Operands are small integers ({-2..2}): every product is an integer and every partial sum is bounded by 4 K (forward, data
gradient; K <= 4608) or 4 M (weight gradient; M <= 3.3 M), both below 2^24.  The fp32 accumulators are therefore exact in any
summation order, split or k-grouping, the fp64 reference is exact however its GEMM runs, and the expected 16-bit output is the one
correctly rounded value of the exact result.  So outputs are compared bit for bit (as values: +0 == -0), the weight gradient over
the whole fp32 tensor; a missing, extra or misplaced product term changes a result by >= 1.

Geometries: bench_train.conv_plan_keys over bench_train.PLAN_WORKLOADS (tests/test_plan_keys_cpu.py: every plan is reached).  Per
launch the registry's counters (creid_tune_count) must show the plan under test found and applied; the documented exceptions are
mirrored in `_declines`.

The fp64 tap-by-tap references, the comparison and `run_geometry` live in tests/conv_exact.py, shared with the sweep of odd, tiny
and ragged geometries (tests/test_conv_edge_sweep_gpu.py)."""
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

from centroids_reid_amd.bench_train import PLAN_WORKLOADS, conv_plan_keys
from conv_exact import (CHUNK_ELEMS, PLANS, SUMSQ_REL, Sweep, _check_stats, _count, _declines, _rd,  # noqa: F401
                        assert_clean as _assert_clean, ref_dgrad, ref_fwd, ref_wgrad, run_geometry)

WORKLOADS = [(B, H, W) for (H, W), batches in PLAN_WORKLOADS.items() for B in batches]


def geometries(B, H, W, last_strides=(1, 2)):
    """{(cin, cout, k, stride, h, w): keys} of the workload, each geometry once."""
    out = {}
    for ls in last_strides:
        for shape, keys in conv_plan_keys(B, H, W, ls):
            out[shape] = keys
    return out


@pytest.mark.parametrize("case", [(2, 9, 7, 8, 6, 3, 1), (2, 10, 8, 8, 6, 3, 2), (3, 8, 6, 4, 8, 1, 2), (2, 5, 5, 4, 4, 1, 1),
                                  # degenerate maps (tests/test_conv_edge_sweep_gpu.py): a 1 x 1 image, W = 1, H = 1, stride 2 on 1 x 1
                                  # (3 x 3 and 1 x 1), a 2 x 2 map under the 3 x 3 footprint, stride 2 over odd and even extents
                                  (2, 1, 1, 4, 4, 3, 1), (2, 6, 1, 4, 4, 3, 1), (2, 1, 6, 4, 4, 3, 1), (2, 1, 1, 4, 6, 3, 2),
                                  (2, 1, 1, 4, 6, 1, 2), (3, 2, 2, 4, 4, 3, 1), (3, 7, 5, 4, 6, 3, 2), (2, 8, 6, 4, 6, 3, 2),
                                  (2, 9, 7, 4, 6, 1, 2)])
def test_reference_matches_torch_conv(case):
    """The tap-by-tap reference against torch's own fp64 convolution and its gradients (CPU), odd sizes, stride 2 and one-pixel
    extents included."""
    B, H, W, cin, cout, k, s = case
    p = k // 2
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randint(-2, 3, (B, H, W, cin), generator=g, dtype=torch.int8)
    w = torch.randint(-2, 3, (cout, cin, k, k), generator=g, dtype=torch.int8)
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    y = F.conv2d(xr, wr, stride=s, padding=p)
    dy = torch.randint(-2, 3, tuple(y.shape), generator=g, dtype=torch.int8)
    (y * dy.double()).sum().backward()
    dy = dy.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(ref_fwd(x, w, s, p, 0, B), y.detach().permute(0, 2, 3, 1))
    assert torch.equal(ref_dgrad(dy, w, s, p, H, W, 0, B), xr.grad.permute(0, 2, 3, 1))
    assert torch.equal(ref_wgrad(x, dy, k, s, p), wr.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("B,H,W", WORKLOADS, ids=[f"B{b}_{h}x{w}" for b, h, w in WORKLOADS])
def test_plan_sweep_exact(B, H, W, dtype, monkeypatch):
    """Forward with statistics, folded eval-mode forward (residual + ReLU, and neither), data gradient (with and without
    add_src), weight gradient (and accumulate=True) of every convolution of the workload, with the shipped plans and with the
    registry cleared; every plan of the workload found and applied (or the documented decline) along the way."""
    from centroids_reid_amd import _lib as L
    L.lib()
    assert L.N_PLANS == len(PLANS), "the shipped plan file must be registered"
    sw = Sweep(dtype, True)
    geoms = geometries(B, H, W)
    for shape, keys in geoms.items():
        run_geometry(sw, B, shape, keys, monkeypatch)
    mine = {key for keys in geoms.values() for key in keys.values() if key in PLANS}
    never = sorted(kk for kk in mine - sw.applied if not _declines(kk, PLANS[kk], dtype, "fwd" if kk[4] & 8 == 0 else "aff"))
    if never:
        sw.failures.append(f"plans of this workload never applied: {never[:10]}")
    _assert_clean(sw, f"B={B} {H}x{W} {dtype}")


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", [(64, 256, 128), (56, 320, 320)], ids=["B64_256x128", "B56_320x320"])
def test_plan_sweep_exact_fp32(B, H, W, monkeypatch):
    """The exact-parity mode's kernels (fp32, no plans) on the training geometries: everything exact, the output included."""
    from centroids_reid_amd import _lib as L
    L.lib()
    sw = Sweep(torch.float32, False)
    for shape, keys in geometries(B, H, W, (1,)).items():
        run_geometry(sw, B, shape, keys, monkeypatch)
    _assert_clean(sw, f"B={B} {H}x{W} fp32")


# ------------------------------------------------------------------------------------ precision with continuous operands
def _half_ulp(v, dtype):
    """half an ulp of the 16-bit dtype at |v| (f16: subnormal spacing 2^-24 below 2^-14)"""
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** emin)))
    return torch.exp2(e - mant - 1)


def plan_word_representatives():
    """one geometry per distinct (kind, plan word): the smallest M that runs it -> [(B, shape, key)]"""
    best = {}
    for B, H, W in WORKLOADS:
        for shape, keys in geometries(B, H, W).items():
            for key in keys.values():
                if key in PLANS:
                    word = (key[0], PLANS[key])
                    if word not in best or key[1] < best[word][2][1]:
                        best[word] = (B, shape, key)
    return sorted(best.values(), key=lambda t: t[2])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_plan_words_accumulate_in_fp32(dtype, monkeypatch):
    """Integer operands cannot see accumulation in too little precision (a bf16-rounded partial sum is still exact below 256): per
    distinct plan word, at its smallest geometry, and with the built-in rules at the same shape, normal-distributed operands against
    fp64 of the same rounded operands.  Forward / data gradient: |got - ref| <= 1/2 ulp_dtype(ref) + K 2^-24 (|x| |w|) (fp32
    accumulation in any order, then one rounding; the ulp is taken at |ref| + the accumulation bound).  Weight gradient (fp32):
    |got - ref| <= (pixels per split + splits) 2^-24 (|dy|^T |x|), the split count read back from the workspace size."""
    import ctypes as C
    from centroids_reid_amd import layers as ly, _lib as L
    lib = L.lib()
    u = 2.0 ** -24
    failures = []
    for B, shape, key in plan_word_representatives():
        cin, cout, k, s, h, w = shape
        p = k // 2
        oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        gen = torch.Generator(device="cuda").manual_seed(zlib.crc32(repr((B, shape, "normal")).encode()))
        x = torch.randn((B, h, w, cin), generator=gen, device="cuda").to(dtype)
        wt = (torch.randn((cout, cin, k, k), generator=gen, device="cuda") / (cin * k * k) ** 0.5).to(dtype).float()
        dy = torch.randn((B, oh, ow, cout), generator=gen, device="cuda").to(dtype)
        krsc, crsk = ly.weight_prep(wt, dtype)
        ones = torch.stack([torch.ones(cout, device="cuda"), torch.zeros(cout, device="cuda")]).contiguous()
        geom = f"B={B} {cin}->{cout} k{k} s{s} {h}x{w} key {key} plan {PLANS[key]}"
        launch = "wgrad" if key[0] == 0 else "dgrad" if key[4] & 1 else "aff_plain" if key[4] & 8 else "fwd_noc64"
        if _declines(key, PLANS[key], dtype, launch):
            continue                              # (the f16 stream1x1 word: no f16 kernel, the built-in rule runs -- swept exactly)
        if key[0] == 1 and key[2] == 64 and key[3] == 576 and not key[4] & 1:
            monkeypatch.setenv("CREID_C64_3X3", "0")     # the plan, not the c64 kernel that pre-empts it
        for path in ("plan", "rules"):
            try:
                if path == "rules":
                    lib.creid_tune_clear()
                else:
                    h0, d0 = _count(key, 0), _count(key, 1)
                if key[0] == 0:
                    got = ly.conv2d_wgrad(x, dy, k, s, p)
                    d, _, _ = ly.conv_desc(B, h, w, cin, cout, k, s, p)
                    splits = lib.creid_conv2d_wgrad_workspace_bytes(C.byref(d), L._DT[dtype]) // (cout * cin * k * k * 4)
                elif key[4] & 1:
                    got = ly.conv2d_dgrad(dy, crsk, (h, w), s, p)
                elif key[4] & 8:
                    got = ly.conv2d_fwd_affine(x, krsc, s, p, ones, None, False)
                else:
                    got = ly.conv2d_fwd(x, krsc, s, p)
                if path == "plan" and not (_count(key, 0) > h0 and _count(key, 1) == d0):
                    failures.append(f"{geom}: plan not found and applied")
            finally:
                if path == "rules":
                    lib.creid_tune_clear()
                    L.load_tuned_plans()
            torch.cuda.synchronize()
            if key[0] == 0:
                ref, mag = ref_wgrad(x, dy, k, s, p), ref_wgrad(x.abs(), dy.abs(), k, s, p)
                M = B * oh * ow
                bound = ((M + splits - 1) // splits + 64 + splits) * u * mag       # (+ 64: the split length rounds up to k-steps)
                err = (got.double() - ref).abs()
            else:
                if key[4] & 1:
                    ref, mag = ref_dgrad(dy, wt, s, p, h, w, 0, B), ref_dgrad(dy.abs(), wt.abs(), s, p, h, w, 0, B)
                else:
                    ref, mag = ref_fwd(x, wt, s, p, 0, B), ref_fwd(x.abs(), wt.abs(), s, p, 0, B)
                acc_bound = key[3] * u * mag
                bound = acc_bound + _half_ulp(ref.abs() + acc_bound, dtype)
                err = (got.double() - ref).abs()
            bad = err > bound
            if bool(bad.any()):
                i = int(bad.reshape(-1).nonzero()[0])
                failures.append(f"{path} {geom}: {int(bad.sum())} outside the bound, first flat index {i}: err "
                                f"{float(err.reshape(-1)[i]):.3e} bound {float(bound.reshape(-1)[i]):.3e}")
            del got, ref, mag, err, bound, bad
        monkeypatch.delenv("CREID_C64_3X3", raising=False)
        torch.cuda.empty_cache()
    assert not failures, f"{len(failures)} failure(s):\n" + "\n".join(failures[:40])


# ------------------------------------------------------------------------------------ production dispatch
def _bypassed(B, H, W, mode):
    """plan keys of the workload that the backbone's fused entry points never look up, by design (backbone.py):
      * training: conv3 of the bottlenecks whose width is in CREID_C3_AXF (default 64, 128) runs creid_conv1x1_bnrelu_fwd
        (bn2 + ReLU on the operand path; conv_stream.hip, no plan lookup);
      * training: the data gradient of a stride-2 1 x 1 downsample is computed compact, as a stride-1 1 x 1 GEMM over the output
        grid (key (1, B oh ow, cin, cout, 1)) that the block's conv1 data gradient scatter-adds (backbone.py, add_src_stride=2):
        its stride-2 key is never looked up;
      * eval: in layer1, conv3 of block i and conv1 of block i + 1 run as one creid_bottleneck_c3_c1_fwd_* launch (conv_pair.hip,
        no plan lookup).
    A key some other launch of the workload still looks up is not bypassed."""
    shapes = conv_plan_keys(B, H, W, 1)
    axf = {int(v) for v in os.environ.get("CREID_C3_AXF", "64,128").split(",") if v.strip()}
    fused, plain = set(), set()
    for i, (shape, keys) in enumerate(shapes):
        cin, cout, k, s, h, w = shape
        if mode == "train":
            is_c3 = k == 1 and s == 1 and cout == 4 * cin and i >= 2 and shapes[i - 1][0][2] == 3
            (fused if is_c3 and cin in axf else plain).add(keys["fwd"])
            (fused if k == 1 and s == 2 and h % 2 == 0 and w % 2 == 0 else plain).add(keys["dgrad"])
        else:
            # layer1 (h == H // 4): conv3 (64 -> 256) of blocks 0, 1 and conv1 (256 -> 64) of blocks 1, 2
            in_pair = h == H // 4 and ((cin, cout, k) == (64, 256, 1) and i < 8 and shapes[i - 1][0][2] == 3 or
                                       (cin, cout, k) == (256, 64, 1))
            for kk in (keys["fwd_eval"], keys["fwd"]):
                (fused if in_pair else plain).add(kk)
    return fused - plain


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_production_dispatch_reaches_the_swept_plans(dtype):
    """One eager training forward_backward of the benchmark model (ResNet50, P16 x K4, 256 x 128) and one eval-mode embedding
    forward at B = 128: every plan conv_plan_keys assigns to the workload is looked up by the backbone's real launches (fused
    forms included) except the keys `_bypassed` lists, and none is declined except the documented cases of `_declines`."""
    from centroids_reid_amd import _lib as L
    from centroids_reid_amd.bench_train import make_model, synthetic_batch
    lib = L.lib()
    report = []

    def check(mode, B, H, W, run):
        lib.creid_tune_clear()
        L.load_tuned_plans()                       # fresh counters
        run()
        torch.cuda.synchronize()
        keys = {}
        for shape, kk in conv_plan_keys(B, H, W, 1):
            names = ("fwd", "dgrad", "wgrad") if mode == "train" else ("fwd_eval", "fwd")
            for nm in names:
                if kk[nm] in PLANS:
                    keys[kk[nm]] = nm
        if mode == "eval":                         # a plain forward key serves eval only where it has no eval-mode twin
            keys = {kk: nm for kk, nm in keys.items() if nm == "fwd_eval" or kk[:4] + (kk[4] | 8,) not in PLANS}
        bypass = _bypassed(B, H, W, mode)
        unhit = {kk for kk in keys if _count(kk, 0) == 0}
        declined = {kk for kk in PLANS if _count(kk, 1) > 0}
        allowed = {kk for kk in declined if _declines(kk, PLANS[kk], dtype, "fwd" if mode == "train" else "aff_plain")}
        if unhit != bypass & set(keys):
            report.append(f"{mode}: not looked up {sorted(unhit - bypass)}; listed as bypassed but looked up "
                          f"{sorted((bypass & set(keys)) - unhit)}")
        if declined - allowed:
            report.append(f"{mode}: declined {sorted(declined - allowed)}")

    try:
        model = make_model(dtype=dtype)
        batch = synthetic_batch(16, 4, 256, 128, 0)
        check("train", 64, 256, 128, lambda: model.forward_backward(batch, 0))
        del model
        emb = make_model(dtype=dtype).eval()
        x = torch.randn((128, 3, 256, 128), generator=torch.Generator(device="cuda").manual_seed(5), device="cuda")

        def fwd():
            with torch.no_grad():
                emb.bn(emb.backbone(x)[1])
        check("eval", 128, 256, 128, fwd)
    finally:
        lib.creid_tune_clear()
        L.load_tuned_plans()
    assert not report, "\n".join(report)
