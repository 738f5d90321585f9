"""GPU: generalized-mean pooling with a trainable exponent -- creid_gem_fwd / creid_gem_bwd through the C ABI against the float64
reference of tests/gem_ref.py, then through the backbone engine and one whole training step.

Bounds.  `floor` is the largest relative error that the plain fp32 CPU composition of the same expression (u^p = exp2(p log2 u),
gem_ref.*_f32) shows against float64 ON THE SAME INPUTS; the kernels get 4 x floor: the hardware log2 / exp2 may be one unit in the
last place each where libm is about half, and the sums run in another order.
* y:  |y - y64| <= 4 floor |y64|, every output finite.
* dx: |dx - dx64| <= 1/2 ulp(output dtype) + 4 floor_dx |dx64|, against the float64 value itself: the kernel rounds its fp32 value
  once to the output type.  (Against the float64 value ROUNDED to the output type the half ulp could not hold for any kernel: two
  values 4 floor apart that straddle a rounding boundary land one whole ulp apart.)  Exact zeros where x < eps.
* dp: |dp - dp64| <= 4 floor (sum |t1| + sum |t2|) with the forward's floor and the reference's two terms, which nearly cancel.
Measured maxima as a share of these bounds: profiles/gem_pooling.md (the test prints them)."""
import numpy as np
import pytest
import torch

import gem_ref as gr

pytestmark = pytest.mark.gpu

EPS = 1e-6
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
PS = [1.0, 3.0, 6.5]
SHAPES = [(1, 1, 8),             # one position, one channel vector
          (3, 7, 64),            # HW below and off the eight row lanes
          (5, 33, 520),          # a partial last block of 32 channel vectors, ragged HW
          (2, 128, 2048)]        # the production row


def _L():
    from centroids_reid_amd import _lib as L
    return L


class _Pool:
    """One (shape, dtype, p) problem on the device: inputs, float64 reference and floors computed once."""
    cache = {}

    def __init__(self, shape, dtype, p):
        B, HW, C = shape
        self.shape, self.dtype, self.p = shape, dtype, p
        self.x, self.dy = gr.make_inputs(B, HW, C, dtype, seed=B * 1000 + HW)
        self.y64, _ = gr.fwd_f64(self.x, p, EPS)
        self.floor = gr.fwd_floor(self.x, p, EPS)
        self.xd, self.dyd = self.x.cuda(), self.dy.cuda()
        self.pd = torch.tensor([p], dtype=torch.float32, device="cuda")

    @classmethod
    def get(cls, shape, dtype, p):
        key = (shape, dtype, p)
        if key not in cls.cache:
            cls.cache[key] = cls(shape, dtype, p)
        return cls.cache[key]

    def fwd(self, save=True, counter=None):
        L = _L()
        B, HW, C = self.shape
        feat = torch.full((B, C), float("nan"), dtype=torch.float32, device="cuda")
        stats = torch.full((3, B, C), float("nan"), dtype=torch.float32, device="cuda") if save else None
        L.check(L.lib().creid_gem_fwd(L.ptr(self.xd), B, HW, C, L._DT[self.dtype], L.ptr(self.pd), EPS, L.ptr(feat), L.ptr(stats),
                                      L.ptr(counter), L.stream()), "gem_fwd")
        return feat, stats

    def bwd(self, stats, dy, pgrad):
        L = _L()
        B, HW, C = self.shape
        dx = torch.full((B, HW, C), float("nan"), dtype=self.dtype, device="cuda")
        n = L.lib().creid_gem_bwd_partials(B, C, L._DT[self.dtype])
        assert n == B * ((C // (4 if self.dtype == torch.float32 else 8) + 31) // 32)
        parts = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
        L.check(L.lib().creid_gem_bwd(L.ptr(self.xd), L.ptr(dy), L.ptr(stats), B, HW, C, L._DT[self.dtype], L.ptr(self.pd), EPS,
                                      L.ptr(dx), L.ptr(pgrad), L.ptr(parts), L.stream()), "gem_bwd")
        return dx


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_forward_against_float64(dtype, p, shape):
    pb = _Pool.get(shape, dtype, p)
    counter = torch.full((), 41, dtype=torch.long, device="cuda")
    feat, stats = pb.fwd(save=True, counter=counter)
    feat_eval, _ = pb.fwd(save=False)
    assert int(counter) == 42                                        # the training forward's step count rides in the launch
    assert torch.equal(feat, feat_eval)                              # saving changes nothing in y
    y = feat.cpu()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(stats).all())
    err = gr.rel_err(y, pb.y64)
    print(f"fwd {dtype} p={p} {shape}: rel err {err:.3e}, floor {pb.floor:.3e}, share of bound {err / (4 * pb.floor):.3f}")
    assert pb.floor > 0 and err <= 4 * pb.floor


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_backward_against_float64(dtype, p, shape):
    pb = _Pool.get(shape, dtype, p)
    _, stats = pb.fwd(save=True)
    pg = torch.tensor([0.625], dtype=torch.float32, device="cuda")
    dx = pb.bwd(stats, pb.dyd, pg)
    pg2 = torch.tensor([0.625], dtype=torch.float32, device="cuda")
    dx2 = pb.bwd(stats, pb.dyd, pg2)
    assert torch.equal(dx.view(torch.uint8), dx2.view(torch.uint8)) and torch.equal(pg.view(torch.int32), pg2.view(torch.int32))
    # dx
    dx64 = gr.dx_f64(pb.x, pb.dy, p, EPS)
    floor_dx = gr.dx_floor(pb.x, pb.dy, p, EPS)
    got = dx.cpu().double()
    assert bool(torch.isfinite(got).all())
    below = pb.x.double() < EPS
    assert bool((got[below] == 0).all()) and not bool(torch.signbit(dx.cpu().float()[below]).any())
    bound = 0.5 * gr.ulp_of(dtype, dx64) + 4 * floor_dx * dx64.abs()
    share = float(((got - dx64).abs()[~below] / bound[~below]).max()) if bool((~below).any()) else 0.0
    # dp
    dp64, abs_sum = gr.dp_f64(pb.x, pb.dy, p, EPS)
    dp_err = abs(float(pg.double()) - 0.625 - dp64)
    dp_bound = 4 * pb.floor * abs_sum + 2.0 ** -24 * (0.625 + abs(dp64))         # (+ adding dp to the 0.625 already in p.grad)
    print(f"bwd {dtype} p={p} {shape}: dx share of bound {share:.3f} (floor {floor_dx:.3e}); "
          f"dp err {dp_err:.3e}, share of bound {dp_err / dp_bound:.3f}")
    assert share <= 1.0
    assert dp_err <= dp_bound
    # dy = 0 leaves p.grad as it is; without p_grad no partials are needed and dx is the same
    pg3 = torch.tensor([0.625], dtype=torch.float32, device="cuda")
    dx0 = pb.bwd(stats, torch.zeros_like(pb.dyd), pg3)
    assert float(pg3) == 0.625 and not bool(dx0.float().abs().any())
    L = _L()
    B, HW, C = shape
    dx3 = torch.empty_like(dx)
    L.check(L.lib().creid_gem_bwd(L.ptr(pb.xd), L.ptr(pb.dyd), L.ptr(stats), B, HW, C, L._DT[dtype], L.ptr(pb.pd), EPS, L.ptr(dx3),
                                  None, None, L.stream()), "gem_bwd")
    assert torch.equal(dx3.view(torch.uint8), dx.view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_p_one_is_the_average_pool(dtype):
    """p = 1 with every input >= eps: the generalized mean IS the mean -- within the forward bound of creid_gap_fwd's output."""
    L = _L()
    B, HW, C = 3, 33, 520
    x = (torch.rand((B, HW, C), generator=torch.Generator().manual_seed(5)) * 30.0 + 1e-3).to(dtype)
    floor = gr.fwd_floor(x, 1.0, EPS)
    xd = x.cuda()
    p = torch.ones(1, dtype=torch.float32, device="cuda")
    gem = torch.empty((B, C), dtype=torch.float32, device="cuda")
    gap = torch.empty((B, C), dtype=torch.float32, device="cuda")
    L.check(L.lib().creid_gem_fwd(L.ptr(xd), B, HW, C, L._DT[dtype], L.ptr(p), EPS, L.ptr(gem), None, None, L.stream()), "gem_fwd")
    L.check(L.lib().creid_gap_fwd(L.ptr(xd), B, HW, C, L._DT[dtype], L.ptr(gap), L.stream()), "gap_fwd")
    err = gr.rel_err(gem.cpu(), gap.cpu())
    print(f"p = 1 vs average pool {dtype}: {err:.3e}, floor {floor:.3e}")
    assert floor > 0 and err <= 4 * floor


def test_refusals_before_any_launch():
    L = _L()
    lib = L.lib()
    x = torch.zeros((2, 4, 16), dtype=torch.bfloat16, device="cuda")
    p = torch.full((1,), 3.0, device="cuda")
    feat = torch.full((2, 16), 7.0, device="cuda")
    stats = torch.zeros((3, 2, 16), device="cuda")
    dx = torch.zeros_like(x)
    pg = torch.zeros(1, device="cuda")
    st = L.stream()
    E_ARG, E_DTYPE = -1, -2
    assert lib.creid_gem_fwd(None, 2, 4, 16, L.BF16, L.ptr(p), EPS, L.ptr(feat), None, None, st) == E_ARG
    assert lib.creid_gem_fwd(L.ptr(x), 2, 4, 16, L.BF16, None, EPS, L.ptr(feat), None, None, st) == E_ARG
    assert lib.creid_gem_fwd(L.ptr(x), 2, 4, 16, L.BF16, L.ptr(p), EPS, None, None, None, st) == E_ARG
    assert lib.creid_gem_fwd(L.ptr(x), 2, 4, 12, L.BF16, L.ptr(p), EPS, L.ptr(feat), None, None, st) == E_ARG      # C % 8
    assert lib.creid_gem_fwd(L.ptr(x), 2, 4, 6, L.F32, L.ptr(p), EPS, L.ptr(feat), None, None, st) == E_ARG        # C % 4
    assert lib.creid_gem_fwd(L.ptr(x), 2, 0, 16, L.BF16, L.ptr(p), EPS, L.ptr(feat), None, None, st) == E_ARG
    assert lib.creid_gem_fwd(L.ptr(x), 2, 4, 16, L.BF16, L.ptr(p), 0.0, L.ptr(feat), None, None, st) == E_ARG
    assert lib.creid_gem_fwd(L.ptr(x), 2, 4, 16, L.BF16X3, L.ptr(p), EPS, L.ptr(feat), None, None, st) == E_DTYPE
    a = (L.ptr(x), L.ptr(feat), L.ptr(stats), 2, 4, 16, L.BF16, L.ptr(p), EPS, L.ptr(dx), L.ptr(pg), L.ptr(stats), st)
    for slot in (0, 1, 2, 7, 9, 11):                     # x, dfeat, stats, p, dx; partials missing while p_grad is given
        assert lib.creid_gem_bwd(*[None if i == slot else v for i, v in enumerate(a)]) == E_ARG
    assert lib.creid_gem_bwd(*[12 if i == 5 else v for i, v in enumerate(a)]) == E_ARG
    assert lib.creid_gem_bwd(*[L.BF16X3 if i == 6 else v for i, v in enumerate(a)]) == E_DTYPE
    torch.cuda.synchronize()
    assert bool((feat == 7.0).all()) and float(pg) == 0.0 and not bool(dx.float().abs().any())
    assert lib.creid_gem_fwd(L.ptr(torch.zeros((2, 4, 12), device="cuda")), 2, 4, 12, L.F32, L.ptr(p), EPS, L.ptr(feat), None, None,
                             st) == 0                    # fp32 takes C % 4 == 0


# ------------------------------------------------------------------ through the network
ARCH, NB, NH, NW = "resnet50", 8, 64, 32


def _cfg(arch=ARCH, K=4):
    from centroids_reid_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.MODEL.PRETRAINED = False
    cfg.MODEL.NAME = arch
    cfg.DATALOADER.NUM_INSTANCE = K
    return cfg


@pytest.fixture(scope="module")
def net_oracle():
    """The oracle's training-mode forward / backward of sum(feat * w) with feat = GeM(base_out), in float64 and in fp32."""
    from oracle import backbone_oracle as bo
    torch.set_num_threads(16)
    sd = bo.make_state_dict(ARCH, 1, seed=77)
    x = bo.synthetic_images(NB, NH, NW, seed=12)
    coef = torch.from_numpy(np.random.default_rng(3).standard_normal((NB, 2048)).astype(np.float32))
    out = {"sd": sd, "x": x, "coef": coef}
    for dtype in (torch.float64, torch.float32):
        params = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()
                  if v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var"))}
        full = {**{k: (v.to(dtype) if v.dtype.is_floating_point else v).clone() for k, v in sd.items()}, **params}
        p = torch.tensor(3.0, dtype=dtype, requires_grad=True)
        base_out, _ = bo.backbone_forward(x.to(dtype), full, ARCH, 1, training=True)
        feat = gr.pool_nchw(base_out, p, EPS)
        (feat * coef.to(dtype)).sum().backward()
        out[dtype] = dict(feat=feat.detach().double(), grads={k: q.grad.double() for k, q in params.items()}, dp=float(p.grad))
    out["train_feat"] = out[torch.float32]["feat"]       # the oracle as the other network tests use it: its fp32 evaluation
    with torch.no_grad():
        base_out, _ = bo.backbone_forward(x, {k: v.clone() for k, v in sd.items()}, ARCH, 1, training=False)
        out["eval_feat"] = gr.pool_nchw(base_out, 3.0, EPS)
    return out


def _baseline(sd, dtype, **kw):
    from centroids_reid_amd.baseline import Baseline
    m = Baseline(_cfg(), compute_dtype=dtype, pooling="gem", **kw)
    m.base.load_state_dict(sd)
    return m.cuda()


def _own_map_check(base_out, feat, p):
    """feat against gem_ref applied to the engine's own final map (NCHW fp32 copy)"""
    B, C = feat.shape
    m = base_out.cpu().reshape(B, C, -1).permute(0, 2, 1).contiguous()
    err, floor = gr.rel_err(feat.cpu(), gr.fwd_f64(m, p, EPS)[0]), gr.fwd_floor(m, p, EPS)
    assert floor > 0 and err <= 4 * floor, (err, floor)


def test_network_fp32_forward_and_gradients(net_oracle):
    """fp32 mode through ResNet50 at 8 x 64 x 32: feat within the project's 1e-4 embedding bar of the oracle's base_out pooled by
    gem_ref (the oracle as every network test uses it, evaluated in fp32), eval mode (the folded forward) and train mode; feat
    inside the kernel's forward bound on the engine's own final map; gradients of sum(feat * w), dp included, no further from the
    float64 oracle than 5 x torch-fp32 + 2e-4 in relative L2.
    Measured: train 8.7e-5 from the fp32 oracle.  Against the oracle's float64 evaluation it is 1.4e-4 -- and torch-fp32 itself
    1.05e-4: at a 4 x 2 final map with batch-8 statistics the map carries 2.7e-4 of fp32 noise, which the mean over eight positions
    halves twice and a p = 3 pool, leaning on the largest of them, does not.  Gradients: conv weights 1.99e-2 (torch-fp32 1.80e-2),
    dp 3.1e-2 (4.1e-2)."""
    o = net_oracle
    model = _baseline(o["sd"], torch.float32)
    eng = model.engine
    assert eng.pooling == "gem"
    # eval mode first (the training forward below moves the running statistics): the folded forward
    model.eval()
    base_out, feat = model.engine_for(False).forward(o["x"].cuda(), False, want_base_out=True)
    ferr_eval = float((feat.cpu() - o["eval_feat"]).abs().max())
    print(f"GeM network fp32, eval (folded): feat max-abs vs the oracle {ferr_eval:.3e}")
    _own_map_check(base_out, feat, 3.0)
    model.train()
    base_out, feat = eng.forward(o["x"].cuda(), True, want_base_out=True)
    o64, o32 = o[torch.float64], o[torch.float32]
    ferr = float((feat.double().cpu() - o["train_feat"]).abs().max())
    ferr64 = float((feat.double().cpu() - o64["feat"]).abs().max())
    t32_64 = float((o32["feat"] - o64["feat"]).abs().max())
    print(f"GeM network fp32, train: feat max-abs vs the oracle (fp32) {ferr:.3e}, vs its fp64 evaluation {ferr64:.3e} "
          f"(torch fp32 vs fp64: {t32_64:.3e}); max |feat| {float(feat.abs().max()):.3f}")
    _own_map_check(base_out, feat, 3.0)
    eng.backward(o["coef"].cuda())
    gh = {n: q.grad.detach().double().cpu() for n, q in model.base.named_parameters() if q.grad is not None}
    names = [n for n in o64["grads"] if n in gh and n.endswith("weight") and o64["grads"][n].dim() == 4]
    assert len(names) == 53

    def rel(g):
        num = sum(float((g[n] - o64["grads"][n]).pow(2).sum()) for n in names)
        return (num / sum(float(o64["grads"][n].pow(2).sum()) for n in names)) ** 0.5
    err_hip, err_t32 = rel(gh), rel(o32["grads"])
    dp_hip = abs(float(model.gap.p.grad) - o64["dp"]) / abs(o64["dp"])
    dp_t32 = abs(o32["dp"] - o64["dp"]) / abs(o64["dp"])
    print(f"GeM network fp32: conv-weight gradients vs fp64: HIP {err_hip:.3e}, torch fp32 {err_t32:.3e}; "
          f"dp: HIP {dp_hip:.3e}, torch fp32 {dp_t32:.3e} (dp = {o64['dp']:.6f})")
    # the bar of test_whole_network_gradient_error_is_at_the_fp32_noise_floor (tests/test_backbone_gpu.py): 5 x torch-fp32 + 2e-4
    assert err_hip < 5 * err_t32 + 2e-4, (err_hip, err_t32)
    assert dp_hip < 5 * dp_t32 + 2e-4, (dp_hip, dp_t32)
    assert ferr_eval < 1e-4, ferr_eval
    assert ferr < 1e-4, ferr                             # the project's fp32 embedding bar, train mode


def test_network_bf16_forward():
    """The bar of the bf16 average-pool test, test_resnet50_bf16_vs_oracle (tests/test_backbone_gpu.py), at that test's own set-up
    (the bar was measured for it: 4 x 128 x 64, its seeds, training mode, against the fp32 oracle): cosine > 0.98, max error < 0.4
    of the largest value -- with both sides pooled by GeM."""
    from oracle import backbone_oracle as bo
    sd = bo.make_state_dict(ARCH, 1, seed=1234)
    x = bo.synthetic_images(4, 128, 64, seed=11)
    with torch.no_grad():
        ref_map, _ = bo.backbone_forward(x, {k: v.clone() for k, v in sd.items()}, ARCH, 1, training=True)
        ref = gr.pool_nchw(ref_map, 3.0, EPS).numpy()
    model = _baseline(sd, torch.bfloat16).train()
    base_out, feat = model.engine.forward(x.cuda(), True, want_base_out=True)
    f = feat.cpu().numpy()
    err = np.abs(f - ref).max() / np.abs(ref).max()
    cos = (f * ref).sum() / np.linalg.norm(f) / np.linalg.norm(ref)
    print(f"GeM network bf16: cosine {cos:.4f}, max error / max value {err:.3f}")
    assert cos > 0.98 and err < 0.4, (cos, err)
    _own_map_check(base_out, feat, 3.0)
    model.engine.backward(torch.ones_like(feat))
    assert bool(torch.isfinite(model.gap.p.grad).all()) and float(model.gap.p.grad) != 0.0
    assert all(bool(torch.isfinite(q.grad).all()) for q in model.parameters() if q.grad is not None)


def test_network_bf16x3_eval_and_basic_block():
    """Every engine of a GeM Baseline pools with GeM: the bf16x3 eval engine and a BasicBlock network (train, backward, eval)."""
    from centroids_reid_amd.baseline import Baseline
    from oracle import backbone_oracle as bo
    x = bo.synthetic_images(4, NH, NW, seed=2).cuda()
    m = Baseline(_cfg("resnet18"), compute_dtype=torch.float32, eval_precision="bf16x3", pooling="gem", gem_p=2.0)
    m.base.load_state_dict(bo.make_state_dict("resnet18", 1, seed=5))
    m.cuda().train()
    base_out, feat = m.engine.forward(x, True, want_base_out=True)
    _own_map_check(base_out, feat, 2.0)
    m.engine.backward(torch.ones_like(feat))
    assert float(m.gap.p.grad) != 0.0 and bool(torch.isfinite(m.gap.p.grad).all())
    m.eval()
    with torch.no_grad():
        base_out, feat = m(x)
    assert m.engine_for(False).x3
    _own_map_check(base_out, feat, 2.0)


# ------------------------------------------------------------------ the step
P_, K_ = 4, 4


def _ctl(dtype=torch.bfloat16, seed=0, **kw):
    from centroids_reid_amd.train_ctl_model import CTLModel
    torch.manual_seed(seed)
    cfg = _cfg()
    cfg.USE_MIXED_PRECISION = dtype != torch.float32
    model = CTLModel(cfg, num_classes=20, num_query=0, compute_dtype=dtype, **kw).cuda().train()
    model.configure_optimizers()
    return model


def _batches(steps):
    gen = torch.Generator(device="cuda").manual_seed(9)
    out = []
    for s in range(steps):
        ids = (np.arange(P_) * 3 + s) % 20
        x = torch.randn((P_ * K_, 3, NH, NW), generator=gen, device="cuda")
        out.append((x, torch.as_tensor(np.repeat(ids, K_).astype(np.int64), device="cuda"), torch.zeros(P_ * K_, dtype=torch.int64),
                    torch.ones(P_ * K_, dtype=torch.bool)))
    return out


def test_step_eager_and_captured_replay_agree(monkeypatch):
    from centroids_reid_amd import ops
    from centroids_reid_amd.bench_train import CAPTURE_MODE
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)          # single-pass classifier GEMMs: bit-reproducible steps
    batches = _batches(4)
    eager = _ctl(pooling="gem")
    p = eager.backbone.gap.p
    assert "backbone.gap.p" in eager.optimizers()[0].param_groups[0]["names"]
    p0 = p.detach().clone()
    out = eager.forward_backward(batches[0], 0)
    assert bool(torch.isfinite(out["loss"])) and float(p.grad) != 0.0 and bool(torch.isfinite(p.grad).all())
    eager.apply_optimizers()
    assert not torch.equal(p.detach(), p0) and bool(torch.isfinite(p).all())
    losses = [out["loss"].clone()] + [eager.training_step(batches[s], s)["loss"].clone() for s in range(1, 4)]
    assert all(bool(torch.isfinite(v)) for v in losses)
    model = _ctl(pooling="gem")
    sx, sl = batches[0][0].clone(), batches[0][1].clone()
    static = (sx, sl, batches[0][2], batches[0][3])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for s in range(2):
            sx.copy_(batches[s][0]); sl.copy_(batches[s][1])
            model.training_step(static, s)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
        gout = model.training_step(static, 0)
    for s in range(2, 4):
        sx.copy_(batches[s][0]); sl.copy_(batches[s][1])
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gout["loss"].reshape(()), losses[3].reshape(()))
    for (n, a), (_, b) in zip(eager.named_parameters(), model.named_parameters()):
        assert torch.equal(a, b), n
    assert float(model.backbone.gap.p.detach()) != 3.0


def test_avg_keyword_is_the_default_bit_for_bit(monkeypatch):
    from centroids_reid_amd import ops
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    batch = _batches(1)[0]
    a, b = _ctl(), _ctl(pooling="avg")
    assert list(a.state_dict()) == list(b.state_dict())
    oa, ob = a.training_step(batch, 0), b.training_step(batch, 0)
    assert torch.equal(oa["loss"], ob["loss"])
    for k in oa["other"]:
        assert torch.equal(oa["other"][k], ob["other"][k]), k
    for (n, u), (_, v) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(u, v), n


def test_f16_step_with_the_loss_scaler():
    model = _ctl(torch.float16, pooling="gem")
    sc = model.loss_scaler
    assert sc is not None
    sc.state.copy_(torch.tensor([1024.0, 1.0 / 1024.0]))       # a settled scale: GradScaler's 65536 is meant to back off at first
    p = model.backbone.gap.p
    for s, b in enumerate(_batches(2)):
        out = model.training_step(b, s)
    assert bool(torch.isfinite(out["loss"])) and sc.skipped_steps == 0 and model.optimizers()[0].step_count == 2
    assert bool(torch.isfinite(p).all()) and float(p.detach()) != 3.0 and sc.get_scale() == 1024.0
