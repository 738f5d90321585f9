"""GPU: bf16x3 training (compute_dtype="bf16x3") -- the data gradient, the weight gradient and the training weight copies of the
split-operand bf16 path (three bf16 MFMAs per product, fp32 activations), layer by layer against fp64 (bit-exact on small-integer
operands, bounded on normal ones), and the whole training step against the fp32 CPU oracle, the reference's recordings, fp64
gradients and the product's fp32 mode; determinism, graph capture, weight-change tracking and checkpoint interchange."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# the distinct ResNet50 convolution shapes (conv input size H x W): 1 x 1 and 3 x 3, stride 1 and 2, 64..2048 channels, a partial
# 128-row tile, IBN-a's 80 x 80 layer-1 shapes
CASES = [  # B, H, W, cin, cout, k, stride
    (2, 16, 8, 64, 64, 1, 1),
    (2, 16, 8, 64, 64, 3, 1),
    (2, 16, 8, 64, 256, 1, 1),
    (2, 16, 8, 256, 64, 1, 1),
    (4, 16, 8, 128, 128, 3, 2),
    (2, 16, 8, 256, 512, 1, 2),
    (2, 16, 8, 512, 1024, 1, 2),
    (1, 10, 10, 64, 256, 1, 1),          # M = 100: partial tile
    (2, 8, 4, 512, 512, 3, 1),
    (2, 8, 4, 2048, 512, 1, 1),
    (1, 6, 6, 1024, 2048, 1, 1),
    (1, 80, 80, 64, 64, 3, 1),
    (1, 80, 80, 64, 256, 1, 1),
]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _operands(case, integer):
    B, H, W, cin, cout, k, stride = case
    pad = k // 2
    oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    rng = np.random.default_rng(sum(int(c) for c in case) + (7 if integer else 0))
    if integer:                          # exact in bf16 (lo = 0) and in every fp32 partial sum
        x = rng.integers(-3, 4, (B, cin, H, W)).astype(np.float32)
        dy = rng.integers(-3, 4, (B, cout, oh, ow)).astype(np.float32)
        w = rng.integers(-3, 4, (cout, cin, k, k)).astype(np.float32)
    else:
        x = rng.standard_normal((B, cin, H, W)).astype(np.float32)
        dy = rng.standard_normal((B, cout, oh, ow)).astype(np.float32)
        w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
    add = rng.integers(-3, 4, (B, cin, H, W)).astype(np.float32) if integer else rng.standard_normal((B, cin, H, W)).astype(np.float32)
    return [torch.from_numpy(a) for a in (x, dy, w, add)] + [pad]


def _ref_dgrad(dy, w, xshape, stride, pad):
    return torch.nn.grad.conv2d_input(xshape, w.double(), dy.double(), stride=stride, padding=pad)


def _ref_wgrad(x, dy, wshape, stride, pad):
    return torch.nn.grad.conv2d_weight(x.double(), wshape, dy.double(), stride=stride, padding=pad)


@pytest.mark.parametrize("case", CASES)
def test_weight_prep_planes_exact(case):
    """hi = bf16(w), lo = bf16(w - hi) (round to nearest even) in both copies; crsk is krsc transposed."""
    from centroids_reid_amd import layers as ly
    _, _, w, _, _ = _operands(case, False)
    w = w * 3.7                                                # (not a power-of-two scale: lo carries real bits)
    krsc, crsk = ly.weight_prep_x3_train(w.cuda())
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    want = torch.stack([hi.permute(0, 2, 3, 1), lo.permute(0, 2, 3, 1)])
    assert torch.equal(krsc.cpu().view(torch.int16), want.contiguous().view(torch.int16))
    assert torch.equal(crsk.cpu(), krsc.cpu().permute(0, 4, 2, 3, 1))
    # the forward-only preparation writes the same krsc planes
    assert torch.equal(ly.weight_prep_x3(w.cuda()).cpu().view(torch.int16), krsc.cpu().view(torch.int16))


@pytest.mark.parametrize("case", CASES)
def test_dgrad_exact_integers(case):
    """Small-integer operands: lo planes are zero and every fp32 sum is exact -- the data gradient, with and without add_src,
    equals fp64 bit for bit."""
    from centroids_reid_amd import layers as ly
    B, H, W, cin, cout, k, stride = case
    x, dy, w, add, pad = _operands(case, True)
    _, crsk = ly.weight_prep_x3_train(w.cuda())
    ref = _ref_dgrad(dy, w, x.shape, stride, pad)
    got = ly.conv2d_dgrad_x3(_nhwc(dy).cuda(), crsk, (H, W), stride, pad)
    assert torch.equal(_nchw(got).cpu().double(), ref)
    got = ly.conv2d_dgrad_x3(_nhwc(dy).cuda(), crsk, (H, W), stride, pad, add_src=_nhwc(add).cuda())
    assert torch.equal(_nchw(got).cpu().double(), ref + add.double())


@pytest.mark.parametrize("case", CASES)
def test_wgrad_exact_integers(case):
    """Small-integer operands: the weight gradient (and accumulate onto an integer tensor) equals fp64 bit for bit."""
    from centroids_reid_amd import layers as ly
    B, H, W, cin, cout, k, stride = case
    x, dy, w, _, pad = _operands(case, True)
    ref = _ref_wgrad(x, dy, w.shape, stride, pad)
    xg, dyg = _nhwc(x).cuda(), _nhwc(dy).cuda()
    got = ly.conv2d_wgrad_x3(xg, dyg, k, stride, pad)
    assert torch.equal(got.cpu().double(), ref)
    acc = w.clone().cuda()
    ly.conv2d_wgrad_x3(xg, dyg, k, stride, pad, dw=acc, accumulate=True)
    assert torch.equal(acc.cpu().double(), ref + w.double())


def _errs(got, ref):
    d = got.double().cpu() - ref
    rms = float(ref.pow(2).mean().sqrt())
    return float(d.norm() / ref.norm()), float(d.abs().max()) / rms


@pytest.mark.parametrize("case", CASES)
def test_dgrad_wgrad_normal_operands(case):
    """Unit-normal operands, weights scaled by 1/sqrt(fan-in), against fp64 of the unrounded fp32 operands: relative L2 <= 2e-5
    and max-abs <= 1e-4 * rms(ref) for both gradients; the bf16 mode's error on the same case is more than 10x larger."""
    from centroids_reid_amd import layers as ly
    B, H, W, cin, cout, k, stride = case
    x, dy, w, _, pad = _operands(case, False)
    _, crsk = ly.weight_prep_x3_train(w.cuda())
    xg, dyg = _nhwc(x).cuda(), _nhwc(dy).cuda()
    ref_d = _ref_dgrad(dy, w, x.shape, stride, pad)
    ref_w = _ref_wgrad(x, dy, w.shape, stride, pad)
    e_d = _errs(_nchw(ly.conv2d_dgrad_x3(dyg, crsk, (H, W), stride, pad)), ref_d)
    e_w = _errs(ly.conv2d_wgrad_x3(xg, dyg, k, stride, pad), ref_w)
    _, crsk16 = ly.weight_prep(w.cuda(), torch.bfloat16)
    b_d = _errs(_nchw(ly.conv2d_dgrad(dyg.bfloat16(), crsk16, (H, W), stride, pad)), ref_d)
    b_w = _errs(ly.conv2d_wgrad(xg.bfloat16(), dyg.bfloat16(), k, stride, pad), ref_w)
    print(f"{case}: dgrad rel {e_d[0]:.2e} max/rms {e_d[1]:.2e} (bf16 {b_d[0]:.2e}); wgrad rel {e_w[0]:.2e} max/rms {e_w[1]:.2e} "
          f"(bf16 {b_w[0]:.2e})")
    for e, b in ((e_d, b_d), (e_w, b_w)):
        assert e[0] <= 2e-5 and e[1] <= 1e-4, e
        assert b[0] > 10 * e[0], (b, e)


@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[6], CASES[11]])
def test_partials_summed_by_the_existing_reduce(case):
    """creid_conv2d_wgrad_x3_partials + creid_conv2d_wgrad_reduce_job(CREID_F32) equals the one-call weight gradient bit for bit
    (and creid_conv2d_wgrad_reduce(CREID_F32), the other summation order, agrees to fp32 rounding)."""
    from centroids_reid_amd import _lib as L, layers as ly
    B, H, W, cin, cout, k, stride = case
    x, dy, w, _, pad = _operands(case, False)
    xg, dyg = _nhwc(x).cuda(), _nhwc(dy).cuda()
    one = ly.conv2d_wgrad_x3(xg, dyg, k, stride, pad)
    ws, d = ly.conv2d_wgrad_x3(xg, dyg, k, stride, pad, partials_only=True)
    nbytes = L.lib().creid_conv2d_wgrad_x3_workspace_bytes(C.byref(d))
    dw = torch.zeros_like(one)
    L.check(L.lib().creid_conv2d_wgrad_reduce_job(C.byref(d), L.ptr(dw), 0, L.ptr(ws), nbytes, L.F32, L.stream()), "reduce_job")
    assert torch.equal(dw, one)
    dw2 = torch.zeros_like(one)
    L.check(L.lib().creid_conv2d_wgrad_reduce(C.byref(d), L.ptr(dw2), 0, L.ptr(ws), nbytes, L.F32, L.stream()), "reduce")
    assert float((dw2 - one).norm() / one.norm()) < 1e-6


def test_engine_weight_copies_match_the_layer_prep():
    """The engine's one-launch preparation of all 52 non-stem convolutions writes exactly the single-convolution planes."""
    from centroids_reid_amd import backbone as bb, layers as ly
    net = bb.build_backbone("resnet50", 1).cuda()
    eng = bb.BackboneEngine(net, "bf16x3", trainable=True)
    eng.prep_weights()
    for u in eng.all_units():
        if u is eng.stem:
            continue
        krsc, crsk = ly.weight_prep_x3_train(u.conv.weight.detach())
        assert torch.equal(u.w_krsc.view(torch.int16), krsc.view(torch.int16))
        assert torch.equal(u.w_crsk.view(torch.int16), crsk.view(torch.int16))


def test_default_engine_still_refuses_to_train():
    from centroids_reid_amd import _lib as L, backbone as bb
    net = bb.build_backbone("resnet50", 1).cuda()
    with pytest.raises(L.CreidError, match="eval-mode forward only"):
        bb.BackboneEngine(net, "bf16x3").forward(torch.zeros(2, 3, 64, 32, device="cuda"), True)


# ----------------------------------------------------------------------------- network level
def _ctl_model(dtype, arch, sd, C, K, seed=6):
    from centroids_reid_amd.bench_train import make_model
    model = make_model(num_classes=C, dtype=dtype, K=K, arch=arch)
    missing = model.backbone.base.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        model.center_loss.centers.copy_(torch.from_numpy(rng.standard_normal((C, 2048)).astype(np.float32)) * 0.3)
        model.fc_query.weight.copy_(torch.from_numpy((rng.standard_normal((C, 2048)) * 0.01).astype(np.float32)))
    return model


def test_bf16x3_step_at_the_benchmark_batch_vs_oracle():
    """tests/test_parity_full_size_gpu.py::test_fp32_step_at_the_benchmark_batch_vs_oracle in the bf16x3 mode (B = 64, 256 x 128):
    losses within the fp32 bars (measured: 5e-6 xent, 4.3e-5 triplet, 4.1e-5 total); embeddings 4.2e-4 max-abs, see BAR_BENCH_EMB."""
    from oracle import backbone_oracle as bo, reid_oracle as ro
    torch.set_num_threads(16)
    P, K, Cn, H, W = 16, 4, 751, 256, 128
    sd = bo.make_state_dict("resnet50", 1, seed=77)
    model = _ctl_model("bf16x3", "resnet50", sd, Cn, K)
    assert model.backbone.engine.x3_train
    centers0 = model.center_loss.centers.detach().cpu().clone(); fc0 = model.fc_query.weight.detach().cpu().clone()
    x = bo.synthetic_images(P * K, H, W, seed=3)
    labels = torch.from_numpy(np.repeat((np.arange(P) * 7) % Cn, K).astype(np.int64))
    is_real = torch.ones(P * K, dtype=torch.bool)
    out = model.forward_backward((x.cuda(), labels.cuda(), torch.zeros(P * K, dtype=torch.int64), is_real), 0)
    with torch.no_grad():
        _, feat = bo.backbone_forward(x, {k: v.clone() for k, v in sd.items()}, "resnet50", 1, training=True)
        o = ro.ctl_heads(feat, labels, is_real, torch.ones(2048), torch.zeros(2048), torch.zeros(2048), torch.ones(2048),
                         fc0, centers0, P, K)
        _, f = model.backbone.engine.forward(x.cuda(), True, False)
    err = float((f.cpu() - feat).abs().max())
    pairs = {n: (float(model.losses_dict[n][-1]), float(o[n])) for n in ("query_xent", "query_triplet", "query_center", "centroid_triplet")}
    print("bf16x3 B=64 embeddings max-abs vs oracle", err, "|feat|max", float(feat.abs().max()), pairs, float(out["loss"]), float(o["total"]))
    assert err <= BAR_BENCH_EMB
    for n, (got, ref) in pairs.items():
        assert abs(got - ref) <= 2e-4, (n, got, ref)
    assert abs(float(out["loss"]) - float(o["total"])) <= 4e-4


def _cfg(D, K, margin):
    from centroids_reid_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.MODEL.PRETRAINED = False
    cfg.MODEL.BACKBONE_EMB_SIZE = D
    cfg.DATALOADER.NUM_INSTANCE = K
    cfg.SOLVER.MARGIN = margin
    cfg.USE_MIXED_PRECISION = False
    return cfg


@pytest.mark.parametrize("name", ["full_step_r50_p4k4_64x32", "full_step_r50ibn_p4k4_64x64"])
def test_full_model_vs_reference_recording_bf16x3(golden, name):
    """tests/test_ctl_step_gpu.py::test_full_model_vs_reference_recording in the bf16x3 mode: the fp32 trajectory and after-four-steps
    bars (measured trajectory 1.3e-2 / 6.4e-3, centers 3.8e-3 / 3.1e-3); first-step losses see BAR_RECORDING_STEP1."""
    from oracle import backbone_oracle as bo
    from centroids_reid_amd.train_ctl_model import CTLModel
    g = golden(name)
    P, K, Cn, H, W = (int(g[k]) for k in ("P", "K", "C", "H", "W"))
    arch = str(g["arch"])
    cfg = _cfg(2048, K, 0.5)
    cfg.MODEL.NAME = arch
    model = CTLModel(cfg, num_classes=Cn, num_query=0, compute_dtype="bf16x3")
    missing = model.backbone.base.load_state_dict(bo.make_state_dict(arch, 1, seed=int(g["seed"])), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("fc.") for k in missing.missing_keys), missing
    rng = np.random.default_rng(5)
    with torch.no_grad():
        model.center_loss.centers.copy_(torch.from_numpy(rng.standard_normal((Cn, 2048)).astype(np.float32)) * 0.3)
        model.fc_query.weight.copy_(torch.from_numpy((rng.standard_normal((Cn, 2048)) * 0.01).astype(np.float32)))
    model = model.cuda().train()
    model.configure_optimizers()
    x = bo.synthetic_images(P * K, H, W, seed=3)
    labels = torch.from_numpy(np.repeat(np.arange(P) * 3 % Cn, K).astype(np.int64))
    is_real = torch.ones(P * K, dtype=torch.bool); is_real[6] = False
    out = model.training_step((x.cuda(), labels.cuda(), torch.zeros(P * K, dtype=torch.int64), is_real), 0)
    errs = {"loss_total": abs(float(out["loss"]) - float(g["f32_loss_total"]))}
    for n in ("query_xent", "query_triplet", "query_center", "centroid_triplet"):
        errs[n] = abs(float(model.losses_dict[n][-1]) - float(g[f"f32_{n}"]))
    print("bf16x3", name, {k: f"{v:.2e}" for k, v in errs.items()})
    traj = {}
    for st in range(1, 4):
        xs = bo.synthetic_images(P * K, H, W, seed=3 + st)
        out = model.training_step((xs.cuda(), labels.cuda(), torch.zeros(P * K, dtype=torch.int64), torch.ones(P * K, dtype=torch.bool)), st)
        traj[st] = {"loss_total": abs(float(out["loss"]) - float(g[f"f32_s{st}_loss_total"]))}
        for n in ("query_xent", "query_triplet", "query_center", "centroid_triplet"):
            traj[st][n] = abs(float(model.losses_dict[n][-1]) - float(g[f"f32_s{st}_{n}"]))
    base = model.backbone.base
    dc = np.abs(model.center_loss.centers.detach().cpu().numpy() - g["centers_after"]).max()
    drv = np.abs(model.bn.running_var.cpu().numpy() / g["bn_rv_after"] - 1).max()
    drm = np.abs(base.layer4[2].bn3.running_mean.cpu().numpy() - g["l4_bn3_rm_after"]).max()
    moved = np.abs(g["conv1_after_slice"] - base.conv1.weight.detach().cpu().numpy()[:8])
    print("trajectory", {st: f"{max(v.values()):.2e}" for st, v in traj.items()},
          f"centers {dc:.2e}, BNNeck running_var rel {drv:.2e}, layer4 bn3 running_mean {drm:.2e}, "
          f"conv1 slice max {moved.max():.2e}, fraction beyond 1e-4 {(moved > 1e-4).mean():.3f}")
    assert max(errs.values()) < BAR_RECORDING_STEP1, errs
    assert max(max(v.values()) for v in traj.values()) < 3e-2, traj
    assert dc < 5e-3 and drv < 5e-3 and drm < 2e-3 and (moved > 1e-4).mean() < 0.05, (dc, drv, drm, moved.max())


def _oracle_grads(sd, x, coef, arch, dtype):
    from oracle import backbone_oracle as bo
    params = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()
              if v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var"))}
    full = {**{k: (v.to(dtype) if v.dtype.is_floating_point else v).clone() for k, v in sd.items()}, **params}
    _, feat = bo.backbone_forward(x.to(dtype), full, arch, 1, training=True)
    (feat * coef.to(dtype)).sum().backward()
    return {k: p.grad.double() for k, p in params.items() if p.grad is not None}, feat.detach().double()


def _engine_grads(net, eng, x, coef):
    for p in net.parameters():
        p.grad = None
    _, feat = eng.forward(x.cuda(), training=True)
    eng.backward(coef.cuda())
    torch.cuda.synchronize()
    return {n: p.grad.detach().double().cpu() for n, p in net.named_parameters() if p.grad is not None}, feat.detach().double().cpu()


def test_ibn_a_gradient_error_vs_fp64():
    """tests/test_parity_full_size_gpu.py::test_ibn_a_gradient_error_is_at_the_fp32_noise_floor in the bf16x3 mode: within 5x the
    torch fp32 error (measured 7.4e-2 against 5 x 2.0e-2) and 10x its worst tensor; the absolute bar see BAR_IBN_GRAD."""
    from oracle import backbone_oracle as bo
    from centroids_reid_amd import backbone as bb
    torch.set_num_threads(16)
    B, H, W = 8, 128, 64
    x = bo.synthetic_images(B, H, W, seed=43)
    coef = torch.from_numpy(np.random.default_rng(8).standard_normal((B, 2048)).astype(np.float32))
    sd = bo.make_state_dict("resnet50_ibn_a", 1, seed=4322)
    net = bb.build_backbone("resnet50_ibn_a", 1)
    net.load_state_dict(sd, strict=False)
    net = net.cuda()
    g64, f64 = _oracle_grads(sd, x, coef, "resnet50_ibn_a", torch.float64)
    g32, f32 = _oracle_grads(sd, x, coef, "resnet50_ibn_a", torch.float32)
    gh, feat = _engine_grads(net, bb.BackboneEngine(net, "bf16x3", trainable=True), x, coef)
    names = [n for n in g64 if n in gh and n.endswith("weight") and g64[n].dim() == 4]
    assert len(names) == 53

    def rel(g):
        num = sum(float((g[n] - g64[n]).pow(2).sum()) for n in names)
        return (num / sum(float(g64[n].pow(2).sum()) for n in names)) ** 0.5
    err_hip, err_t32 = rel(gh), rel(g32)
    ferr_hip = float((feat - f64).abs().max()); ferr_t32 = float((f32 - f64).abs().max())
    worst = max((float((gh[n] - g64[n]).norm() / (g64[n].norm() + 1e-30)), n) for n in names)
    worst_t = max((float((g32[n] - g64[n]).norm() / (g64[n].norm() + 1e-30)), n) for n in names)
    print(f"IBN-a conv-weight gradients vs fp64: HIP bf16x3 {err_hip:.3e}, torch-CPU fp32 {err_t32:.3e}; embeddings max-abs vs fp64: "
          f"HIP {ferr_hip:.2e}, torch fp32 {ferr_t32:.2e}; worst tensor HIP {worst}, torch fp32 {worst_t}")
    assert err_hip < 5 * err_t32 + 2e-4, (err_hip, err_t32)
    assert err_hip < BAR_IBN_GRAD
    assert worst[0] < 10 * worst_t[0] + 1e-3, (worst, worst_t)


def test_gradients_against_the_fp32_mode():
    """Same network, weights and batch through the fp32 engine and the bf16x3 engine: aggregate relative L2 of the 53 conv-weight
    gradients.  The issue's guess was 1e-3; the emulation predicted 7.3e-2 and the MI355X measures 8.1e-2 (BAR_VS_FP32): the
    fp32 mode's rounding itself sits 1.2-2e-2 from fp64 here."""
    from oracle import backbone_oracle as bo
    from centroids_reid_amd import backbone as bb
    B, H, W = 8, 128, 64
    x = bo.synthetic_images(B, H, W, seed=43)
    coef = torch.from_numpy(np.random.default_rng(8).standard_normal((B, 2048)).astype(np.float32))
    net = bb.build_backbone("resnet50", 1)
    net.load_state_dict(bo.make_state_dict("resnet50", 1, seed=4322), strict=False)
    net = net.cuda()
    g32, f32 = _engine_grads(net, bb.BackboneEngine(net, torch.float32), x, coef)
    gx3, fx3 = _engine_grads(net, bb.BackboneEngine(net, "bf16x3", trainable=True), x, coef)
    names = [n for n in g32 if n.endswith("weight") and g32[n].dim() == 4]
    assert len(names) == 53
    num = sum(float((gx3[n] - g32[n]).pow(2).sum()) for n in names)
    rel = (num / sum(float(g32[n].pow(2).sum()) for n in names)) ** 0.5
    stem = float((gx3["conv1.weight"] - g32["conv1.weight"]).norm() / g32["conv1.weight"].norm())
    print(f"bf16x3 vs fp32 mode: conv-weight gradients aggregate rel. L2 {rel:.3e} (stem {stem:.3e}); embeddings max-abs "
          f"{float((fx3 - f32).abs().max()):.2e}")
    assert rel <= BAR_VS_FP32


def test_determinism_and_graph_replay():
    """The same step twice from the same state gives bit-identical gradients, and a captured-graph replay of the step equals the
    eager one bit for bit."""
    from oracle import backbone_oracle as bo
    from centroids_reid_amd import backbone as bb
    B, H, W = 16, 128, 64
    x = bo.synthetic_images(B, H, W, seed=5).cuda()
    coef = torch.from_numpy(np.random.default_rng(9).standard_normal((B, 2048)).astype(np.float32)).cuda()
    net = bb.build_backbone("resnet50", 1)
    net.load_state_dict(bo.make_state_dict("resnet50", 1, seed=11), strict=False)
    net = net.cuda()
    eng = bb.BackboneEngine(net, "bf16x3", trainable=True)
    params = [p for p in net.parameters() if p.requires_grad]

    def step():
        for p in params:
            if p.grad is not None:
                p.grad.zero_()
        _, f = eng.forward(x, training=True)
        eng.backward(coef)
        return f

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
        step()
    torch.cuda.current_stream().wait_stream(side)
    step()
    g1 = [p.grad.clone() for p in params]
    step()
    g2 = [p.grad.clone() for p in params]
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for p in params:
        p.grad.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, p.grad) for a, p in zip(g1, params))


def test_training_step_is_capturable():
    """The full CTLModel step in bf16x3 captures like the fp32 mode (bench_train.fp32_mode_step): replays run and move the loss."""
    from centroids_reid_amd.bench_train import make_model, synthetic_batch
    P, K, H, W = 4, 4, 128, 64
    model = make_model(num_classes=40, dtype="bf16x3", K=K)
    b0 = synthetic_batch(P, K, H, W, 0, num_classes=40)
    static = (b0[0].clone(), b0[1].clone(), b0[2], b0[3])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for s in range(2):
            model.training_step(static, s)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.training_step(static, 0)
    losses = []
    for _ in range(3):
        graph.replay()
        losses.append(float(out["loss"]))
    assert all(np.isfinite(losses)) and losses[0] != losses[2], losses


def test_weight_tracking_and_checkpoint_interchange():
    """After one training_step the next eval forward reflects the new weights and equals a freshly built bf16x3 model loaded from
    the same state_dict; that state_dict loads into an fp32-mode model whose eval embeddings are within 5e-5 of the bf16x3 ones."""
    from oracle import backbone_oracle as bo
    from centroids_reid_amd.train_ctl_model import CTLModel
    P, K, Cn, H, W = 4, 4, 20, 128, 64
    sd = bo.make_state_dict("resnet50", 1, seed=21)

    def model_of(dtype):
        m = CTLModel(_cfg(2048, K, 0.5), num_classes=Cn, num_query=0, compute_dtype=dtype)
        return m

    def embed(m, xe):
        m.backbone.eval()
        with torch.no_grad():
            _, f = m.backbone(xe)
        m.backbone.train()
        return f.clone()

    m = model_of("bf16x3")
    m.backbone.base.load_state_dict(sd, strict=False)
    m = m.cuda().train()
    m.configure_optimizers()
    xe = bo.synthetic_images(8, H, W, seed=30).cuda()
    f0 = embed(m, xe)
    x = bo.synthetic_images(P * K, H, W, seed=31).cuda()
    labels = torch.as_tensor(np.repeat(np.arange(P) * 3 % Cn, K).astype(np.int64)).cuda()
    m.training_step((x, labels, torch.zeros(P * K, dtype=torch.int64), torch.ones(P * K, dtype=torch.bool)), 0)
    f1 = embed(m, xe)
    assert not torch.equal(f0, f1)
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    fresh = model_of("bf16x3")
    fresh.load_state_dict(state)
    fresh = fresh.cuda()
    assert torch.equal(embed(fresh, xe), f1)
    m32 = model_of(torch.float32)
    m32.load_state_dict(state)
    m32 = m32.cuda()
    e32 = float((embed(m32, xe) - f1).abs().max())
    print(f"fp32-mode eval embeddings of the bf16x3-trained checkpoint vs its bf16x3 eval forward: {e32:.2e}")
    assert e32 <= 5e-5


# Bars of the network-level tests that differ from the fp32 mode's.  The layer-level error of the mode is 4.4e-6 relative L2
# (above: the resolution of the split, hi and lo each rounded to 8 significant bits, about 20x fp32's rounding).  Train-mode
# BatchNorm (batch statistics of 8-64 images) amplifies per-layer differences on the way through 50 layers: the fp32 mode's own
# rounding already ends 1-2e-2 from fp64 in the conv-weight gradients of these small batches.  tests/probes/bf16x3_train_emul.py
# predicted, before any GPU run, that the bf16x3 step lands ~16x further from fp64 than fp32 does, and therefore breaks these fp32
# bars (prediction -> MI355X measurement, deterministic):
#   embeddings, training-mode forward, max-abs    6.5e-4 (B=8, 128x64)  -> 4.2e-4 at B=64 256x128 against the oracle (fp32 bar 1e-4)
#   first-step losses, P4K4 64x32 recording       (embeddings 1.3e-3)    -> 2.8e-4 query_triplet, 2.4e-4 total (fp32 bar 2e-4);
#                                                                           IBN-a 64x64 1.4e-4 (inside the fp32 bar)
#   IBN-a conv-weight gradients vs fp64           7.2e-2                 -> 7.4e-2 (fp32 bar 5e-2; torch fp32 itself 2.0e-2)
#   conv-weight gradients vs the fp32 mode        7.3e-2                 -> 8.1e-2 (the issue's guessed 1e-3)
# The bars below sit above the measured values; every other bar (losses at B=64, the three-step trajectory, the after-four-steps
# state, the relative bars against torch fp32) is the fp32 mode's own.
BAR_BENCH_EMB = 1e-3
BAR_RECORDING_STEP1 = 1e-3
BAR_IBN_GRAD = 1e-1
BAR_VS_FP32 = 1.2e-1
