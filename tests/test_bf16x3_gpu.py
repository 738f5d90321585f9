"""GPU: the bf16x3 eval-mode forward (CREID_BF16X3, csrc/conv_x3.hip) -- fp32 activations, weights split into bf16 (hi, lo)
planes, three bf16 MFMAs per product.  Layer level against torch fp64, network level against the reference's own recordings
and against the product's fp32 mode, batch invariance, tie-aware ranking agreement, and the mixed use (train in bf16, embed in
bf16x3) with its weight-change tracking."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (test_eval_fold_gpu.py CASES) + a 320 x 320 layer-1 3 x 3 and 1 x 1 (M = 6400), and a shape large enough for the 128-wide N tile
CASES = [  # B, H, W, cin, cout, k, stride, residual, relu
    (2, 16, 8, 64, 64, 1, 1, False, True),
    (2, 16, 8, 64, 64, 3, 1, False, True),
    (2, 16, 8, 64, 256, 1, 1, True, True),
    (4, 16, 8, 128, 128, 3, 2, False, True),       # stride-2 3 x 3
    (2, 16, 8, 256, 512, 1, 2, False, False),      # downsample branch: no ReLU
    (1, 10, 10, 64, 256, 1, 1, True, True),        # M = 100: partial tile
    (2, 8, 4, 512, 512, 3, 1, False, True),        # K = 4608
    (1, 6, 6, 1024, 2048, 1, 1, True, True),
    (8, 16, 8, 512, 2048, 1, 1, True, True),
    (1, 80, 80, 64, 64, 3, 1, False, True),        # ResNet50-IBN-a at 320 x 320, layer1 conv2
    (1, 80, 80, 64, 256, 1, 1, True, True),        # ... and its conv3
    (16, 64, 32, 64, 256, 1, 1, True, True),       # 512 workgroups of 128 x 128
]


def _case_tensors(case):
    B, H, W, cin, cout, k, stride, with_res, relu = case
    rng = np.random.default_rng(sum(int(c) for c in case))
    x = torch.from_numpy(rng.standard_normal((B, cin, H, W)).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32))
    gamma = torch.from_numpy(rng.uniform(0.5, 1.5, cout).astype(np.float32))
    beta = torch.from_numpy(rng.standard_normal(cout).astype(np.float32) * 0.3)
    rm = torch.from_numpy(rng.standard_normal(cout).astype(np.float32) * 0.2)
    rv = torch.from_numpy(rng.uniform(0.5, 2.0, cout).astype(np.float32))
    return x, w, gamma, beta, rm, rv, rng


@pytest.mark.parametrize("case", CASES)
def test_conv_affine_layer_x3(case):
    """max|err| against fp64 of the UNROUNDED fp32 operands <= 6e-5 on these unit-scale cases; the bf16 mode's error on the same
    case is more than 10x larger.  Measured on MI355X: 1.5e-5 .. 4.8e-5 (the largest on the 8.4 M outputs of the last case).
    That is the split's own resolution, not an accumulation effect: hi and lo each round to 8 significant bits, so a product
    carries up to ~3 * 2^-16 relative error (lo rounding of either operand, the dropped lo * lo term); over K unit-scale terms
    that is a ~1e-5 standard error, times the folded BatchNorm scale (up to 2.1 here), and the max over 10^5..10^7 outputs
    lands at 3-5e-5.  (An earlier estimate put this bar at 3e-5; the network-level bars below are the ones that matter.)"""
    from centroids_reid_amd import layers as ly
    B, H, W, cin, cout, k, stride, with_res, relu = case
    pad = k // 2
    x, w, gamma, beta, rm, rv, rng = _case_tensors(case)
    y = F.conv2d(x.double(), w.double(), stride=stride, padding=pad)
    y = F.batch_norm(y, rm.double(), rv.double(), gamma.double(), beta.double(), False, 0.0, 1e-5)
    res = None
    if with_res:
        res = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32))
        y = y + res.double()
    if relu:
        y = y.clamp(min=0)
    ref = y.permute(0, 2, 3, 1).numpy()
    ss = ly.bn_fold(gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda())
    xg = x.permute(0, 2, 3, 1).contiguous().cuda()
    rg = res.permute(0, 2, 3, 1).contiguous().cuda() if res is not None else None
    w2 = ly.weight_prep_x3(w.cuda())
    hi = w.to(torch.bfloat16)
    assert torch.equal(w2[0].cpu(), hi.permute(0, 2, 3, 1))
    assert torch.equal(w2[1].cpu(), (w - hi.float()).to(torch.bfloat16).permute(0, 2, 3, 1))
    yg = ly.conv2d_fwd_affine_x3(xg, w2, stride, pad, ss, rg, relu)
    assert yg.dtype == torch.float32
    err = float(np.abs(yg.cpu().numpy().astype(np.float64) - ref).max())
    assert err <= 6e-5, err
    krsc, _ = ly.weight_prep(w.cuda(), torch.bfloat16)
    yb = ly.conv2d_fwd_affine(xg.to(torch.bfloat16), krsc, stride, pad, ss, rg.to(torch.bfloat16) if rg is not None else None, relu)
    err_b = float(np.abs(yb.float().cpu().numpy().astype(np.float64) - ref).max())
    assert err_b > 10 * err, (err_b, err)


@pytest.mark.parametrize("case", [(2, 16, 8, 64, 64, 1, 1), (2, 16, 16, 64, 64, 3, 1), (1, 10, 10, 256, 128, 3, 2),
                                  (2, 8, 4, 512, 512, 3, 1), (1, 80, 80, 64, 64, 1, 1)])
def test_conv_raw_with_stats_x3(case):
    """creid_conv2d_fwd_nhwc in bf16x3 (IBN-a's conv1 in eval): raw output and the per-128-row (sum, sumsq) partials."""
    from centroids_reid_amd import layers as ly
    B, H, W, cin, cout, k, stride = case
    pad = k // 2
    rng = np.random.default_rng(sum(case))
    x = torch.from_numpy(rng.standard_normal((B, cin, H, W)).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32))
    y = F.conv2d(x.double(), w.double(), stride=stride, padding=pad).permute(0, 2, 3, 1).reshape(-1, cout)
    yg, part = ly.conv2d_fwd_x3(x.permute(0, 2, 3, 1).contiguous().cuda(), ly.weight_prep_x3(w.cuda()), stride, pad, True)
    err = float((yg.reshape(-1, cout).cpu().double() - y).abs().max())
    assert err <= 6e-5, err                                  # (measured: <= 3.3e-5; see test_conv_affine_layer_x3)
    M = y.shape[0]
    rows = (M + 127) // 128
    pad_rows = torch.zeros(rows * 128 - M, cout, dtype=torch.float64)
    yt = torch.cat([y, pad_rows]).view(rows, 128, cout)
    np.testing.assert_allclose(part[:, 0].cpu().numpy(), yt.sum(1).numpy(), rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(part[:, 1].cpu().numpy(), (yt * yt).sum(1).numpy(), rtol=1e-5, atol=1e-3)


def _net(arch, sd):
    from centroids_reid_amd import backbone as bb
    net = bb.build_backbone(arch, 1)
    net.load_state_dict(sd, strict=False)
    return net.cuda()


@pytest.mark.parametrize("arch,golden_name,H,W", [("resnet50", "backbone_r50_2x256x128", 256, 128),
                                                  ("resnet50_ibn_a", "backbone_r50ibn_2x64x64", 64, 64),
                                                  ("resnet50_ibn_a", "backbone_r50ibn_2x320x320", 320, 320)])
def test_eval_feat_vs_reference_recordings(golden, arch, golden_name, H, W):
    """The bar the fp32 mode meets in test_backbone_gpu.py: the reference's own eval-mode embeddings within 1e-4."""
    from centroids_reid_amd import backbone as bb
    from oracle import backbone_oracle as bo
    g = golden(golden_name)
    eng = bb.BackboneEngine(_net(arch, bo.make_state_dict(arch, 1)), "bf16x3")
    with torch.no_grad():
        _, feat = eng.forward(bo.synthetic_images(2, H, W, seed=7).cuda(), training=False)
    np.testing.assert_allclose(feat.cpu().numpy(), g["eval_feat"], rtol=0, atol=1e-4)


def _neck(feat, D, seed=3):
    """eval-mode BNNeck (modelling/bases.py:171-173) with fixed non-trivial statistics, in fp64, then L2 normalisation."""
    rng = np.random.default_rng(seed)
    rm = torch.from_numpy(rng.standard_normal(D) * 0.1).cuda()
    rv = torch.from_numpy(rng.uniform(0.5, 2.0, D)).cuda()
    f = F.batch_norm(feat.double(), rm, rv, None, None, False, 0.0, 1e-5)
    return F.normalize(f, dim=1)


@pytest.mark.parametrize("arch,H,W", [("resnet50", 256, 128), ("resnet50_ibn_a", 320, 320)])
def test_embedding_vs_fp32_mode(arch, H, W):
    """B = 32, same weights: relative L2 error of the L2-normalised BNNeck embedding <= 5e-5 per row (emulation: <= 8e-6;
    f16 sits near 6e-4 and bf16 higher, so this separates the modes)."""
    from centroids_reid_amd import backbone as bb
    from oracle import backbone_oracle as bo
    net = _net(arch, bo.make_state_dict(arch, 1, seed=11))
    x = bo.synthetic_images(32, H, W, seed=5).cuda()
    with torch.no_grad():
        f32 = bb.BackboneEngine(net, torch.float32).forward(x, False)[1]
        fx3 = bb.BackboneEngine(net, "bf16x3").forward(x, False)[1]
        fb16 = bb.BackboneEngine(net, torch.bfloat16).forward(x, False)[1]
    e32, ex3, eb = _neck(f32, f32.shape[1]), _neck(fx3, f32.shape[1]), _neck(fb16, f32.shape[1])
    rel = (ex3 - e32).norm(dim=1)
    rel_b = (eb - e32).norm(dim=1)
    assert float(rel.max()) <= 5e-5, float(rel.max())
    assert float(rel_b.max()) > 5e-5                             # (the yardstick does separate the modes)


def test_batch_invariance():
    """A 3-image forward followed by a 125-image forward equals one 128-image forward, bit for bit (run_inference's
    macro-batching promise): the k order of every output element depends on the shape alone."""
    from centroids_reid_amd import backbone as bb
    from oracle import backbone_oracle as bo
    eng = bb.BackboneEngine(_net("resnet50", bo.make_state_dict("resnet50", 1, seed=2)), "bf16x3")
    x = bo.synthetic_images(128, 256, 128, seed=9).cuda()
    with torch.no_grad():
        whole = eng.forward(x, False)[1]
        parts = torch.cat([eng.forward(x[:3].contiguous(), False)[1], eng.forward(x[3:].contiguous(), False)[1]])
    assert torch.equal(whole, parts)


def _clustered_embeddings(n_id=96, n_query=2, n_gallery=6, H=256, W=128, noise=0.6, seed=0):
    """bench_train.map_delta_bf16's clustered-identity recipe: fp32 and bf16x3 embeddings (BNNeck, eval) of one model."""
    from centroids_reid_amd.bench_train import make_model
    torch.manual_seed(seed)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    per = n_query + n_gallery
    base = torch.randn((n_id, 3, H // 16, W // 16), generator=gen, device="cuda")
    base = F.interpolate(base, size=(H, W), mode="bilinear", align_corners=False)
    x = base.repeat_interleave(per, 0) + noise * torch.randn((n_id * per, 3, H, W), generator=gen, device="cuda")
    pid = np.repeat(np.arange(n_id), per)
    slot = np.tile(np.arange(per), n_id)
    q_rows = np.nonzero(slot < n_query)[0]; g_rows = np.nonzero(slot >= n_query)[0]
    order = np.concatenate([q_rows, g_rows])
    cams = np.concatenate([np.zeros(len(q_rows), np.int64), np.ones(len(g_rows), np.int64)])
    model = make_model(dtype=torch.float32)
    model.train()
    with torch.no_grad():
        for s in range(0, 512, 64):                                       # settle the running statistics (fp32)
            _, f = model.backbone(x[s:s + 64])
            model.bn(f)
    model.eval()
    embs = {}
    for mode in (None, "bf16x3"):
        model.backbone.eval_precision = mode
        out = []
        with torch.no_grad():
            for s in range(0, len(x), 128):
                _, f = model.backbone(x[s:s + 128])
                out.append(model.bn(f).float())
        embs[mode] = torch.cat(out)[torch.as_tensor(order, device="cuda")].contiguous()
    return embs[None], embs["bf16x3"], pid[order], cams, len(q_rows)


def test_tie_aware_ranking_and_map():
    """Wherever the fp32 and bf16x3 gallery orders of a query differ, the swapped items' fp32 distances differ by at most 4 eps
    (eps = the measured max L2 error of a normalised embedding); |delta mAP| <= 1e-3 (at 192 queries, delta mAP is rank-flip
    noise between near-tied gallery rows -- not a 1e-4 yardstick)."""
    from centroids_reid_amd import reid_metric as rm
    e32, ex3, pids, cams, nq = _clustered_embeddings()
    n32, nx3 = F.normalize(e32.double(), dim=1), F.normalize(ex3.double(), dim=1)
    eps = float((n32 - nx3).norm(dim=1).max())
    assert eps <= 5e-5, eps

    def dist(n):
        return torch.cdist(n[:nq], n[nq:])

    d32 = dist(n32)
    rank32 = rm.rank_rows((d32 ** 2).float().contiguous())
    rankx3 = rm.rank_rows((dist(nx3) ** 2).float().contiguous())
    assert rank32.shape == rankx3.shape
    # along the bf16x3 order the fp32 distances may only dip by near-ties: running max minus current <= 4 eps (+ the
    # float32 rounding of the squared distances the ranking kernel sorts)
    dx = torch.gather(d32, 1, rankx3)
    dip = float((torch.cummax(dx, dim=1).values - dx).max())
    assert dip <= 4 * eps + 1e-6, (dip, eps)
    _, map32, _ = rm.R1_mAP(num_query=nq).compute(e32, pids, cams)
    _, mapx3, _ = rm.R1_mAP(num_query=nq).compute(ex3, pids, cams)
    print(f"eps {eps:.2e}, max distance dip {dip:.2e}, mAP fp32 {map32:.6f} bf16x3 {mapx3:.6f} (delta {mapx3 - map32:+.2e}), "
          f"{int((rank32 != rankx3).any(dim=1).sum())} of {nq} queries with a reordering")
    assert abs(mapx3 - map32) <= 1e-3


def _ctl(dtype, eval_precision, num_classes=20):
    from centroids_reid_amd.config import get_cfg_defaults
    from centroids_reid_amd.train_ctl_model import CTLModel
    cfg = get_cfg_defaults()
    cfg.MODEL.PRETRAINED = False
    cfg.MODEL.NAME = "resnet50"
    cfg.DATALOADER.NUM_INSTANCE = 4
    cfg.USE_MIXED_PRECISION = dtype != torch.float32
    model = CTLModel(cfg, num_classes=num_classes, num_query=0, compute_dtype=dtype, eval_precision=eval_precision).cuda().train()
    model.configure_optimizers()
    return model


def _eval_emb(model, x):
    model.eval()
    with torch.no_grad():
        _, f = model.backbone(x)
        e = model.bn(f)
    model.train()
    return e


def test_train_bf16_embed_bf16x3():
    """A CTLModel trained in bf16 with eval_precision='bf16x3': after one training step the next eval forward reflects the new
    weights (the ctypes optimiser's writes reach the eval engine) and equals a freshly built bf16x3 model on the same state
    dict, bit for bit."""
    from centroids_reid_amd.bench_train import synthetic_batch
    torch.manual_seed(0)
    model = _ctl(torch.bfloat16, "bf16x3")
    x = synthetic_batch(4, 4, 128, 64, 0, num_classes=20)[0]
    e0 = _eval_emb(model, x)
    assert model.backbone.engine_for(False).x3 and model.backbone.engine.dtype == torch.bfloat16
    model.training_step(synthetic_batch(4, 4, 128, 64, 1, num_classes=20), 0)
    e1 = _eval_emb(model, x)
    assert not torch.equal(e0, e1)
    fresh = _ctl(torch.bfloat16, "bf16x3")
    fresh.load_state_dict(model.state_dict())
    e2 = _eval_emb(fresh, x)
    assert torch.equal(e1, e2)
    with pytest.raises(Exception, match="eval-mode forward only"):
        model.backbone.engine_for(False).forward(x, True)


def test_unsupported_entry_points_return_e_dtype():
    """Only the forward convolutions and the weight preparation take CREID_BF16X3; every other entry point that takes a dtype
    refuses it before launching anything (real, correctly sized buffers all the same)."""
    from centroids_reid_amd import _lib as L
    lib, st = L.lib(), L.stream()
    X3 = L.BF16X3
    B, H, W, Cc = 2, 16, 8, 64
    a = torch.zeros(B * H * W * 256, device="cuda")
    b = torch.zeros(B * H * W * 256, device="cuda")
    ss = torch.ones(2 * 256, device="cuda")
    feat = torch.zeros(B * 256, device="cuda")
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda")
    d = L.ConvDesc(B, H, W, Cc, H, W, Cc, 3, 3, 1, 1)
    rcs = {
        "conv2d_dgrad_nhwc": lib.creid_conv2d_dgrad_nhwc(C.byref(d), L.ptr(a), L.ptr(b), L.ptr(feat), None, X3, st),
        "conv2d_wgrad_nhwc": lib.creid_conv2d_wgrad_nhwc(C.byref(d), L.ptr(a), L.ptr(b), L.ptr(feat), 0, L.ptr(ws), ws.numel(), X3, st),
        "conv1x1_bnrelu_fwd": lib.creid_conv1x1_bnrelu_fwd(L.ptr(a), L.ptr(ss), L.ptr(b), B * H * W, 64, 64, L.ptr(feat), None, None,
                                                           None, X3, st),
        "stem_conv_fwd_affine": lib.creid_stem_conv_fwd_affine(1, 16, 8, L.ptr(a), L.ptr(b), L.ptr(feat), L.ptr(ss), 0, X3, st),
        "stem_conv_pool_fwd_affine": lib.creid_stem_conv_pool_fwd_affine(1, 16, 8, L.ptr(a), L.ptr(b), L.ptr(feat), L.ptr(ss), 0, X3, st),
        "bottleneck_c3_c1_fwd_affine": lib.creid_bottleneck_c3_c1_fwd_affine(128, 64, 256, 64, L.ptr(a), L.ptr(b), L.ptr(ss), L.ptr(a),
                                                                             L.ptr(feat), L.ptr(b), L.ptr(ss), L.ptr(feat), X3, st),
        "bn2d_apply": lib.creid_bn2d_apply(L.ptr(a), L.ptr(ss), None, 1, 128, 64, X3, L.ptr(b), st),
        "maxpool3x3s2_fwd": lib.creid_maxpool3x3s2_fwd(L.ptr(a), 1, 16, 8, 64, X3, L.ptr(b), None, st),
        "gap_fwd": lib.creid_gap_fwd(L.ptr(a), 2, 16, 64, X3, L.ptr(feat), st),
        "nhwc_to_nchw_f32": lib.creid_nhwc_to_nchw_f32(L.ptr(a), 2, 16, 64, X3, L.ptr(b), st),
        "stem_weight_prep": lib.creid_stem_weight_prep(L.ptr(a), X3, L.ptr(b), st),
        "image_to_nhwc4_pad": lib.creid_image_to_nhwc4_pad(L.ptr(a), 1, 16, 8, X3, L.ptr(b), st),
    }
    torch.cuda.synchronize()
    assert all(rc == -2 for rc in rcs.values()), rcs          # CREID_E_DTYPE
