"""CPU: the generalized-mean pooling reference (tests/gem_ref.py) checked against itself and against torch autograd, and the
public surface of the feature (keywords, refusals, state-dict key, checkpoint rules) -- no device needed."""
import pytest
import torch

import gem_ref as gr


def _cfg(arch="resnet50"):
    from centroids_reid_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.MODEL.PRETRAINED = False
    cfg.MODEL.NAME = arch
    return cfg


# ------------------------------------------------------------------ the reference against itself
@pytest.mark.parametrize("p", [1.0, 3.0, 6.5])
def test_analytic_gradients_equal_autograd_in_float64(p):
    x, dy = gr.make_inputs(3, 7, 16, torch.float32, seed=1)
    x[1, :, 5] = 3e-7                                   # a channel that lies below eps everywhere
    xd = x.double().requires_grad_(True)
    pd = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    y = xd.clamp(min=1e-6).pow(pd).mean(dim=1).pow(1.0 / pd)
    (y * dy.double()).sum().backward()
    y_ref, _ = gr.fwd_f64(x, p)
    assert torch.allclose(y.detach(), y_ref, rtol=1e-14, atol=0)
    dx = gr.dx_f64(x, dy, p)
    assert torch.allclose(dx, xd.grad, rtol=1e-12, atol=1e-300)
    assert bool((dx[x.double() < 1e-6] == 0).all())
    dp, abs_sum = gr.dp_f64(x, dy, p)
    assert abs(dp - float(pd.grad)) <= 1e-12 * abs_sum


def test_p_one_is_the_mean_of_the_clamped_values():
    x, _ = gr.make_inputs(2, 33, 8, torch.float32, seed=2)
    y, m = gr.fwd_f64(x, 1.0)
    ref = x.double().clamp(min=1e-6).mean(dim=1)
    assert torch.allclose(y, ref, rtol=1e-15, atol=0) and torch.equal(m, y)


def test_channel_below_eps_gives_eps_and_no_gradient():
    x = torch.full((1, 5, 4), 3e-7)
    x[0, :, 1] = 0.0
    x[0, :, 3] = 2.0
    dy = torch.ones(1, 4)
    for p in (1.0, 3.0, 8.0):
        y, _ = gr.fwd_f64(x, p)
        assert torch.allclose(y[0, :3], torch.full((3,), 1e-6, dtype=torch.float64), rtol=1e-14, atol=0)
        assert bool((gr.dx_f64(x, dy, p)[0, :, :3] == 0).all())
        t1, t2 = gr.dp_terms_f64(x, dy, p)
        assert float((t1 - t2)[0, :3].abs().max()) <= 1e-20          # y = eps whatever p is: the terms cancel
        assert abs(float((t1 - t2)[0, 3])) <= 1e-14                  # a constant channel does not depend on p either


def test_fp32_composition_is_close_but_not_exact():
    x, dy = gr.make_inputs(3, 7, 64, torch.float32, seed=3)
    for p in (1.0, 3.0, 6.5):                            # (eps^6.5 is subnormal in fp32: fewer bits, still a usable floor)
        assert 0 < gr.fwd_floor(x, p) < 1e-5 and gr.dx_floor(x, dy, p) < 1e-4


def test_ulp_helper():
    one = torch.tensor([1.0, 1.5, 0.75, 1e-30], dtype=torch.float64)
    assert gr.ulp_of(torch.float32, one)[:3].tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -24]
    assert gr.ulp_of(torch.bfloat16, one)[:3].tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -8]
    assert gr.ulp_of(torch.float16, one).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -11, 2.0 ** -24]


# ------------------------------------------------------------------ the public surface
def test_refusals():
    from centroids_reid_amd.baseline import Baseline
    cfg = _cfg()
    with pytest.raises(ValueError):
        Baseline(cfg, pooling="bogus")
    for bad in (0.5, 8.5):
        with pytest.raises(ValueError):
            Baseline(cfg, pooling="gem", gem_p=bad)
    for bad in (0.0, -1e-6):
        with pytest.raises(ValueError):
            Baseline(cfg, pooling="gem", gem_eps=bad)


def test_state_dict_key_only_in_gem_mode():
    from centroids_reid_amd.baseline import Baseline
    from centroids_reid_amd.train_ctl_model import CTLModel
    cfg = _cfg("resnet18")
    plain, avg, gem = Baseline(cfg), Baseline(cfg, pooling="avg"), Baseline(cfg, pooling="gem", gem_p=2.5)
    assert list(plain.state_dict()) == list(avg.state_dict()) and "gap.p" not in plain.state_dict()
    sd = gem.state_dict()
    assert list(sd) == list(plain.state_dict()) + ["gap.p"]
    assert sd["gap.p"].shape == (1,) and sd["gap.p"].dtype == torch.float32 and float(sd["gap.p"]) == 2.5
    m = CTLModel(cfg, num_classes=7, num_query=0, pooling="gem")
    assert "backbone.gap.p" in m.state_dict() and float(m.backbone.gap.p.detach()) == 3.0 and m.backbone.gap.eps == 1e-6
    assert "backbone.gap.p" not in CTLModel(cfg, num_classes=7, num_query=0).state_dict()
    assert "pooling" not in m.hparams and "gem_p" not in m.hparams              # keywords, not config keys
    # the exponent trains in the Adam group, behind the backbone's convolutions and inside the loss-scaled `backbone.` prefix
    opt, opt_center = m.configure_optimizers()[0]
    names = opt.param_groups[0]["names"]
    assert "backbone.gap.p" in names and names.index("backbone.gap.p") == max(i for i, n in enumerate(names) if n.startswith("backbone."))
    assert m.backbone.gap.p.grad.data_ptr() == opt.gflat[opt._offsets[names.index("backbone.gap.p")]:].data_ptr()


def test_checkpoint_round_trip_and_reference_layout(tmp_path):
    from centroids_reid_amd.train_ctl_model import CTLModel
    cfg = _cfg("resnet18")
    m = CTLModel(cfg, num_classes=7, num_query=0, pooling="gem", gem_p=4.25)
    with torch.no_grad():
        m.backbone.gap.p.fill_(2.718281828)
    path = tmp_path / "gem.ckpt"
    m.save_checkpoint(path, 1, 10)
    m2 = CTLModel.load_from_checkpoint(path)            # the key in the state dict selects GeM without being told
    assert m2.backbone.pooling == "gem"
    assert list(m2.state_dict()) == list(m.state_dict())
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k
    # a reference-layout checkpoint (no exponent) loads into a GeM model, strictly, and leaves p at gem_p
    ref = CTLModel(cfg, num_classes=7, num_query=0)
    ref_path = tmp_path / "ref.ckpt"
    ref.save_checkpoint(ref_path, 1, 10)
    assert CTLModel.load_from_checkpoint(ref_path).backbone.pooling == "avg"
    m3 = CTLModel.load_from_checkpoint(ref_path, pooling="gem", gem_p=5.0)
    assert float(m3.backbone.gap.p.detach()) == 5.0
    assert torch.equal(m3.backbone.base.conv1.weight, ref.backbone.base.conv1.weight)
    m4 = CTLModel(cfg, num_classes=7, num_query=0, pooling="gem", gem_p=5.0)
    m4.load_state_dict(ref.state_dict(), strict=True)
    assert float(m4.backbone.gap.p.detach()) == 5.0
    with pytest.raises(RuntimeError):                   # the other way round the key is unexpected
        ref.load_state_dict(m.state_dict(), strict=True)


def test_engine_takes_the_mode_and_the_parameter():
    from centroids_reid_amd import backbone as bb
    from centroids_reid_amd.baseline import Baseline, GemPool
    net = bb.build_backbone("resnet18", 1)
    with pytest.raises(ValueError):
        bb.BackboneEngine(net, torch.float32, pooling="max")
    with pytest.raises(ValueError):
        bb.BackboneEngine(net, torch.float32, pooling="gem")          # no parameter
    gem = GemPool(3.0, 1e-6)
    eng = bb.BackboneEngine(net, torch.float32, pooling="gem", gem=gem)
    assert eng.pooling == "gem" and eng.gem.p is gem.p
    assert bb.BackboneEngine(net, torch.float32).pooling == "avg"
    b = Baseline(_cfg("resnet18"), pooling="gem", eval_precision="bf16x3")
    assert b.engine.gem is b.gap and b.engine_for(False).gem is b.gap and b.engine_for(False) is not b.engine
