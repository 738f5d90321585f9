"""GPU parity: the eval-mode forward with BatchNorm folded into the convolution epilogue (creid_conv2d_fwd_affine_nhwc,
creid_stem_conv_fwd_affine, creid_bn2d_fold_multi) -- the path of validation_step (modelling/bases.py:169-177) and of
inference/inference_utils.py:104-113.  Layer level against a torch fp64 reference of conv -> eval BatchNorm -> (+residual)
-> ReLU; network level against the three-launch schedule (conv, finalize, apply) it replaces: bit-identical in fp32 parity
mode, and the reference goldens' `eval_feat` are checked by tests/test_backbone_gpu.py through the folded path (default)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CASES = [  # B, H, W, cin, cout, k, stride, residual, relu
    (2, 16, 8, 64, 64, 1, 1, False, True),
    (2, 16, 8, 64, 64, 3, 1, False, True),
    (2, 16, 8, 64, 256, 1, 1, True, True),
    (4, 16, 8, 128, 128, 3, 2, False, True),
    (2, 16, 8, 256, 512, 1, 2, False, False),      # downsample branch: no ReLU
    (1, 10, 10, 64, 256, 1, 1, True, True),        # M = 100: partial tile
    (2, 8, 4, 512, 512, 3, 1, False, True),
    (1, 6, 6, 1024, 2048, 1, 1, True, True),
    (8, 16, 8, 512, 2048, 1, 1, True, True),       # N tile 128, several row tiles
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", CASES)
def test_conv_affine_layer(case, dtype):
    from centroids_reid_amd import layers as ly
    B, H, W, cin, cout, k, stride, with_res, relu = case
    pad = k // 2
    rng = np.random.default_rng(sum(int(c) for c in case))
    x = torch.from_numpy(rng.standard_normal((B, cin, H, W)).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32))
    gamma = torch.from_numpy(rng.uniform(0.5, 1.5, cout).astype(np.float32))
    beta = torch.from_numpy(rng.standard_normal(cout).astype(np.float32) * 0.3)
    rm = torch.from_numpy(rng.standard_normal(cout).astype(np.float32) * 0.2)
    rv = torch.from_numpy(rng.uniform(0.5, 2.0, cout).astype(np.float32))
    y = F.conv2d(x.to(dtype).double(), w.to(dtype).double(), stride=stride, padding=pad)
    y = F.batch_norm(y, rm.double(), rv.double(), gamma.double(), beta.double(), False, 0.0, 1e-5)
    res = None
    if with_res:
        res = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32)).to(dtype)
        y = y + res.double()
    if relu:
        y = y.clamp(min=0)
    krsc, _ = ly.weight_prep(w.cuda(), dtype)
    ss = ly.bn_fold(gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda())
    sc = gamma / torch.sqrt(rv + 1e-5)
    np.testing.assert_allclose(ss[0].cpu().numpy(), sc.numpy(), rtol=2e-6)
    np.testing.assert_allclose(ss[1].cpu().numpy(), (beta - rm * sc).numpy(), rtol=1e-5, atol=1e-6)
    xg = x.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()
    rg = res.permute(0, 2, 3, 1).contiguous().cuda() if res is not None else None
    yg = ly.conv2d_fwd_affine(xg, krsc, stride, pad, ss, rg, relu)
    rt, at = {torch.bfloat16: (3e-2, 3e-2), torch.float16: (4e-3, 4e-3), torch.float32: (1e-4, 1e-4)}[dtype]
    np.testing.assert_allclose(yg.float().cpu().permute(0, 3, 1, 2).numpy(), y.float().numpy(), rtol=rt, atol=at)
    if relu:
        assert float(yg.float().min()) >= 0.0
    # the bounds derived from the kernels' arithmetic (tests/eval_audit.py), on the operands as stored: the tolerances above cannot
    # see a dropped rounding, a wrong eps or a truncated accumulator; these can (tests/test_eval_audit_cpu.py)
    import eval_audit as ea
    import layer_audit as la
    au = la.Audit("layer")
    ea.check_fold(au, "bn", ss, gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda(), 1e-5)
    ea.check_folded_conv(au, "conv", "folded conv", yg.view(-1, cout), xg, krsc.permute(0, 3, 1, 2).double(), stride, pad, ss, relu, rg,
                         dtype)
    assert not au.failures, au.failures


def _eval_feat(arch, dtype, fold, x, sd):
    from centroids_reid_amd import backbone as bb
    os.environ["CREID_EVAL_FOLD"] = "1" if fold else "0"
    try:
        net = (bb.ResNet(last_stride=1) if arch == "resnet50" else bb.resnet50_ibn_a(1)).cuda()
        net.load_state_dict(sd, strict=False)
        eng = bb.BackboneEngine(net, dtype)
        with torch.no_grad():
            base, feat = eng.forward(x, False, True)
        return base, feat, eng
    finally:
        os.environ.pop("CREID_EVAL_FOLD", None)


@pytest.mark.parametrize("arch,H,W", [("resnet50", 64, 32), ("resnet50", 256, 128), ("resnet50_ibn_a", 64, 64)])
def test_folded_eval_forward_equals_three_launch_schedule_fp32(arch, H, W):
    """fp32 parity mode: conv + finalize(eval) + apply and the folded epilogue run the same fmaf / add / max per element."""
    from oracle import backbone_oracle as bo
    sd = {k: v.cuda() for k, v in bo.make_state_dict(arch, 1, seed=11).items()}
    x = bo.synthetic_images(3, H, W, seed=2).cuda()
    b0, f0, _ = _eval_feat(arch, torch.float32, False, x, sd)
    b1, f1, eng = _eval_feat(arch, torch.float32, True, x, sd)
    assert torch.equal(f0, f1), float((f0 - f1).abs().max())
    assert torch.equal(b0, b1)
    # the folded constants follow the running statistics: perturb them and the result must follow, with no dirty flag
    with torch.no_grad():
        eng.net.layer2[0].bn2.running_var.mul_(1.7)
        _, f2 = eng.forward(x, False, False)
    assert not torch.equal(f1, f2)


@pytest.mark.parametrize("arch,H,W", [("resnet50", 256, 128), ("resnet50_ibn_a", 64, 64)])
def test_folded_eval_forward_bf16_close_to_fp32(arch, H, W):
    from oracle import backbone_oracle as bo
    sd = {k: v.cuda() for k, v in bo.make_state_dict(arch, 1, seed=12).items()}
    x = bo.synthetic_images(4, H, W, seed=3).cuda()
    _, f32, _ = _eval_feat(arch, torch.float32, True, x, sd)
    _, fbf, _ = _eval_feat(arch, torch.bfloat16, True, x, sd)
    _, fbu, _ = _eval_feat(arch, torch.bfloat16, False, x, sd)
    cos = F.cosine_similarity(f32, fbf, dim=1)
    cos_u = F.cosine_similarity(f32, fbu, dim=1)
    assert float(cos.min()) > 0.995, cos
    # one rounding per layer instead of two: the folded bf16 forward is no further from fp32 than the unfolded one (+ slack)
    assert float((1 - cos).max()) <= 1.5 * float((1 - cos_u).max()) + 1e-4


@pytest.mark.parametrize("arch,H,W", [("resnet50", 256, 128), ("resnet50_ibn_a", 64, 64)])
def test_folded_eval_forward_f16_closer_to_fp32_than_bf16(arch, H, W):
    """f16 as the compute type of the eval-mode forward (the reference's mixed precision is fp16 autocast, utils/misc.py:111):
    10 explicit mantissa bits against bf16's 7 -- the embeddings must sit several times closer to the fp32 ones, finite, and the
    folded forward must equal the three-launch schedule's arithmetic up to one rounding per layer."""
    from oracle import backbone_oracle as bo
    sd = {k: v.cuda() for k, v in bo.make_state_dict(arch, 1, seed=12).items()}
    x = bo.synthetic_images(4, H, W, seed=3).cuda()
    _, f32, _ = _eval_feat(arch, torch.float32, True, x, sd)
    _, fbf, _ = _eval_feat(arch, torch.bfloat16, True, x, sd)
    _, fh, _ = _eval_feat(arch, torch.float16, True, x, sd)
    assert bool(torch.isfinite(fh).all())
    cos_b = F.cosine_similarity(f32, fbf, dim=1)
    cos_h = F.cosine_similarity(f32, fh, dim=1)
    assert float(cos_h.min()) > 0.9999, cos_h
    assert float((1 - cos_h).max()) < 0.25 * float((1 - cos_b).max()), (cos_h, cos_b)
    rel = float(((fh - f32).norm(dim=1) / f32.norm(dim=1)).max())
    assert rel < 1e-2, rel


def test_f16_training_forward_backward_close_to_fp32():
    """f16 -- the reference's own mixed precision (utils/misc.py:111) -- as a TRAINING compute type (round 5): forward + backward
    of the whole backbone with the head gradient multiplied by a loss scale on the way in.  Whole-network gradients of a
    randomly initialised ResNet50 are chaotic in any 16-bit type (ReLU masks flip, train-mode BatchNorm over a small batch
    amplifies), so the statement is relative: unscaled, every weight gradient sits CLOSER to the fp32 one than bf16's does (and
    the forward features 5 x closer); the kernels themselves are pinned per layer against
    fp64 (test_backbone_gpu.py::test_conv_fwd_dgrad_wgrad[float16]) and the training-level claim by the 20-step trajectory
    (test_f16_train_gpu.py)."""
    from oracle import backbone_oracle as bo
    from centroids_reid_amd import backbone as bb
    from centroids_reid_amd.solver import LossScaler
    sd = bo.make_state_dict("resnet50", 1, seed=5)
    x = bo.synthetic_images(16, 128, 64, seed=4).cuda()
    coef = torch.from_numpy(np.random.default_rng(3).standard_normal((16, 2048)).astype(np.float32)).cuda() / 16.0
    grads, feats = {}, {}
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        net = bb.ResNet(last_stride=1)
        net.load_state_dict(sd)
        net = net.cuda()
        eng = bb.BackboneEngine(net, dt)
        scale = 1.0
        if dt == torch.float16:
            eng.loss_scaler = LossScaler("cuda", init_scale=256.0)
            scale = 256.0
        _, feats[dt] = eng.forward(x, True)
        eng.backward(coef)
        grads[dt] = {n: p.grad.double() / scale for n, p in net.named_parameters() if p.grad is not None}
        assert all(torch.isfinite(g).all() for g in grads[dt].values()), dt

    def rel(dt, name):
        a, r = grads[dt][name], grads[torch.float32][name]
        return float((a - r).norm() / r.norm())
    table = {n: (rel(torch.float16, n), rel(torch.bfloat16, n)) for n in
             ("layer4.2.conv3.weight", "layer4.2.conv2.weight", "layer4.0.downsample.0.weight", "layer3.1.conv2.weight",
              "layer2.0.downsample.0.weight", "layer1.0.conv1.weight", "conv1.weight", "layer3.1.bn2.weight")}
    # measured on this recipe: f16 0.27 (last block) ... 0.70 (stem) of the fp32 gradient's norm, bf16 1.2-1.3 -- a randomly
    # initialised, BatchNorm-perturbed ResNet50 at batch 16 decorrelates its gradients under ANY rounding; f16 is closer everywhere
    for name, (r16, rbf) in table.items():
        assert r16 < rbf, (name, table)
    # training-mode features: batch statistics divide by the spread of a stored (rounded) convolution output whose per-channel
    # mean is several times that spread in a randomly initialised network, which amplifies the storage rounding ~50 x over the
    # eval-mode forward (measured, tests/probes/f16_fwd_check.py: bf16 1.3e-1 / 2.7e-3, f16 2.6e-2 / 3.1e-4 train / eval) -- the same
    # for any 16-bit storage of pre-BatchNorm activations, the reference's autocast included; f16 sits 5 x closer than bf16
    f32 = feats[torch.float32]
    e16 = float(((feats[torch.float16] - f32).norm(dim=1) / f32.norm(dim=1)).max())
    ebf = float(((feats[torch.bfloat16] - f32).norm(dim=1) / f32.norm(dim=1)).max())
    assert e16 < 0.4 * ebf and e16 < 5e-2, (e16, ebf)


def test_eval_forward_after_training_step_uses_fresh_statistics():
    """train -> eval -> train: the folded constants are rebuilt from the running statistics on every eval forward."""
    from oracle import backbone_oracle as bo
    from centroids_reid_amd import backbone as bb
    sd = {k: v.cuda() for k, v in bo.make_state_dict("resnet50", 1, seed=13).items()}
    net = bb.ResNet(last_stride=1).cuda()
    net.load_state_dict(sd, strict=False)
    eng = bb.BackboneEngine(net, torch.float32)
    x = bo.synthetic_images(4, 64, 32, seed=4).cuda()
    with torch.no_grad():
        _, e0 = eng.forward(x, False)
        eng.forward(x, True)                      # updates every running statistic
        eng.saved = None
        _, e1 = eng.forward(x, False)
    os.environ["CREID_EVAL_FOLD"] = "0"
    try:
        eng2 = bb.BackboneEngine(net, torch.float32)
        with torch.no_grad():
            _, e2 = eng2.forward(x, False)
    finally:
        os.environ.pop("CREID_EVAL_FOLD", None)
    assert not torch.equal(e0, e1)
    assert torch.equal(e1, e2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,H,W,relu,wgs,form", [
    (3, 256, 128, 0, 0, 0),       # one run per image part, default grid
    (3, 256, 128, 1, 5, 0),       # 48 steps over 5 workgroups: runs start inside images (the row above is computed first)
    (2, 256, 128, 0, 7, 1),       # four-wave workgroups, four rows per step
    (5, 64, 128, 1, 3, 1),
    (2, 320, 320, 1, 0, 0),       # the IBN-a configuration's image size
    (3, 320, 320, 0, 7, 0),
    (1, 16, 128, 1, 0, 0),        # one step per image
])
def test_stem_conv_pool_one_launch_equals_two_launches(B, H, W, relu, wgs, form, dtype, monkeypatch):
    """creid_stem_conv_pool_fwd_affine (conv_stem.hip: conv1 + folded bn1 (+ ReLU) + 3x3/2 max-pool, the full-resolution tensor
    never written) against creid_stem_conv_fwd_affine + creid_maxpool3x3s2_fwd: identical bits."""
    from centroids_reid_amd import _lib as L
    lib = L.lib()
    dt = L.dtype_code(torch.empty(0, dtype=dtype))
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + H + W + relu)
    img = torch.randn((B, 3, H, W), generator=g, device="cuda", dtype=torch.float32)
    xpad = torch.empty((B, H + 8, W + 6, 4), device="cuda", dtype=dtype)
    st = L.stream()
    L.check(lib.creid_image_to_nhwc4_pad(L.ptr(img), B, H, W, dt, L.ptr(xpad), st), "image_pad")
    w = torch.zeros((64, 8, 8, 4), device="cuda", dtype=torch.float32)
    w[:, :7, :7, :3] = torch.randn((64, 7, 7, 3), generator=g, device="cuda") / 12.0
    w = w.reshape(64, 256).to(dtype).contiguous()
    ss = torch.empty((2, 64), device="cuda", dtype=torch.float32)
    ss[0] = torch.rand(64, generator=g, device="cuda") + 0.5
    ss[1] = torch.randn(64, generator=g, device="cuda") * 0.3
    H1, W1 = H // 2, W // 2
    y0 = torch.empty((B, H1, W1, 64), device="cuda", dtype=dtype)
    ref = torch.empty((B, H1 // 2, W1 // 2, 64), device="cuda", dtype=dtype)
    L.check(lib.creid_stem_conv_fwd_affine(B, H, W, L.ptr(xpad), L.ptr(w), L.ptr(y0), L.ptr(ss), relu, dt, st), "stem")
    L.check(lib.creid_maxpool3x3s2_fwd(L.ptr(y0), B, H1, W1, 64, dt, L.ptr(ref), None, st), "maxpool")
    if wgs:
        monkeypatch.setenv("CREID_STEM_WGS", str(wgs))
    monkeypatch.setenv("CREID_STEM_FORM", str(form))
    got = torch.full_like(ref, float("nan"))
    L.check(lib.creid_stem_conv_pool_fwd_affine(B, H, W, L.ptr(xpad), L.ptr(w), L.ptr(got), L.ptr(ss), relu, dt, st), "stem_pool")
    torch.cuda.synchronize()
    assert torch.isfinite(ref.float()).all()
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), \
        f"max |diff| {(got.float() - ref.float()).abs().max().item()}, differing {(got != ref).sum().item()} of {ref.numel()}"


def test_stem_conv_pool_refuses_other_sizes():
    from centroids_reid_amd import _lib as L
    lib = L.lib()
    x = torch.zeros((1, 64 + 8, 64 + 6, 4), device="cuda", dtype=torch.bfloat16)
    w = torch.zeros((64, 256), device="cuda", dtype=torch.bfloat16)
    ss = torch.zeros((2, 64), device="cuda")
    y = torch.zeros((1, 16, 16, 64), device="cuda", dtype=torch.bfloat16)
    assert lib.creid_stem_conv_pool_fwd_affine(1, 64, 64, L.ptr(x), L.ptr(w), L.ptr(y), L.ptr(ss), 0, L.dtype_code(y),
                                               L.stream()) == -4


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,H,W,wgs", [(2, 16, 8, 0), (3, 10, 10, 0), (8, 64, 32, 0), (5, 64, 32, 7), (1, 3, 5, 0)])
def test_block_boundary_one_launch_equals_two_launches(B, H, W, wgs, dtype, monkeypatch):
    """creid_bottleneck_c3_c1_fwd_affine (conv_pair.hip: conv3 + bn3 + residual + ReLU of a layer1 bottleneck and conv1 + bn1 +
    ReLU of the next one, the block output written once and never read back) against two creid_conv2d_fwd_affine_nhwc calls:
    both outputs bit-identical.  Row counts that are no multiple of the 128-row tile, a workgroup cap (several tiles per workgroup)."""
    from centroids_reid_amd import _lib as L
    from centroids_reid_amd import layers as ly
    lib = L.lib()
    rng = np.random.default_rng(B * 100 + H + W)
    t = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
    a2 = t(rng.standard_normal((B, H, W, 64))).to(dtype)
    res = t(rng.standard_normal((B, H, W, 256))).to(dtype)
    w3 = t(rng.standard_normal((256, 64, 1, 1)) / 8.0)
    w1 = t(rng.standard_normal((64, 256, 1, 1)) / 16.0)
    k3, _ = ly.weight_prep(w3, dtype)
    k1, _ = ly.weight_prep(w1, dtype)
    ss3 = t(np.stack([rng.uniform(0.5, 1.5, 256), rng.standard_normal(256) * 0.3]))
    ss1 = t(np.stack([rng.uniform(0.5, 1.5, 64), rng.standard_normal(64) * 0.3]))
    ref3 = ly.conv2d_fwd_affine(a2, k3, 1, 0, ss3, res, True)
    ref1 = ly.conv2d_fwd_affine(ref3, k1, 1, 0, ss1, None, True)
    if wgs:
        monkeypatch.setenv("CREID_STREAM1X1_WGS", str(wgs))
    M = B * H * W
    out3 = torch.full((B, H, W, 256), float("nan"), device="cuda", dtype=dtype)
    out1 = torch.full((B, H, W, 64), float("nan"), device="cuda", dtype=dtype)
    L.check(lib.creid_bottleneck_c3_c1_fwd_affine(M, 64, 256, 64, L.ptr(a2), L.ptr(k3), L.ptr(ss3), L.ptr(res), L.ptr(out3),
                                                  L.ptr(k1), L.ptr(ss1), L.ptr(out1), L.dtype_code(a2), L.stream()), "pair")
    torch.cuda.synchronize()
    assert torch.equal(out3.view(torch.int16), ref3.view(torch.int16)), f"block output: {(out3 != ref3).sum().item()} of {ref3.numel()} differ"
    assert torch.equal(out1.view(torch.int16), ref1.view(torch.int16)), f"conv1 output: {(out1 != ref1).sum().item()} of {ref1.numel()} differ"
    assert lib.creid_bottleneck_c3_c1_fwd_affine(M, 128, 512, 128, L.ptr(a2), L.ptr(k3), L.ptr(ss3), L.ptr(res), L.ptr(out3),
                                                 L.ptr(k1), L.ptr(ss1), L.ptr(out1), L.dtype_code(a2), L.stream()) == -4


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_block_boundary_statistics_variant(dtype):
    """creid_bottleneck_c3_c1_fwd_stats (the next block's conv1 feeds an IBN layer): the block output and the RAW conv1 output are
    bit-identical to creid_conv2d_fwd_affine_nhwc + creid_conv2d_fwd_nhwc, the per-tile statistics partials equal up to the
    grouping of the fp32 column sums; row counts that are no multiple of 128 are refused."""
    from centroids_reid_amd import _lib as L
    from centroids_reid_amd import layers as ly
    lib = L.lib()
    B, H, W = 6, 16, 16
    rng = np.random.default_rng(17)
    t = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
    a2 = t(rng.standard_normal((B, H, W, 64))).to(dtype)
    res = t(rng.standard_normal((B, H, W, 256))).to(dtype)
    k3, _ = ly.weight_prep(t(rng.standard_normal((256, 64, 1, 1)) / 8.0), dtype)
    k1, _ = ly.weight_prep(t(rng.standard_normal((64, 256, 1, 1)) / 16.0), dtype)
    ss3 = t(np.stack([rng.uniform(0.5, 1.5, 256), rng.standard_normal(256) * 0.3]))
    ref3 = ly.conv2d_fwd_affine(a2, k3, 1, 0, ss3, res, True)
    ref1, refp = ly.conv2d_fwd(ref3, k1, 1, 0, with_stats=True)
    M = B * H * W
    out3 = torch.full_like(ref3, float("nan")); out1 = torch.full_like(ref1, float("nan"))
    part = torch.full((M // 128, 2, 64), float("nan"), device="cuda")
    L.check(lib.creid_bottleneck_c3_c1_fwd_stats(M, 64, 256, 64, L.ptr(a2), L.ptr(k3), L.ptr(ss3), L.ptr(res), L.ptr(out3), L.ptr(k1),
                                                 L.ptr(out1), L.ptr(part), L.dtype_code(a2), L.stream()), "pair_stats")
    torch.cuda.synchronize()
    assert torch.equal(out3.view(torch.int16), ref3.view(torch.int16))
    assert torch.equal(out1.view(torch.int16), ref1.view(torch.int16))
    np.testing.assert_allclose(part.cpu().numpy().reshape(-1), refp.cpu().numpy().reshape(-1), rtol=2e-6, atol=1e-5)
    assert lib.creid_bottleneck_c3_c1_fwd_stats(M - 64, 64, 256, 64, L.ptr(a2), L.ptr(k3), L.ptr(ss3), L.ptr(res), L.ptr(out3), L.ptr(k1),
                                                L.ptr(out1), L.ptr(part), L.dtype_code(a2), L.stream()) == -4
