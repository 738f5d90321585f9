"""GPU: the BENCHMARKED configuration itself is pinned (BASELINE configs[1]: ResNet50 256x128 bf16, P=16 x K=4 = 64
images, fused head pass, hipGraph replay) -- not only the small fp32 parity cases."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P, K, C, H, W = 16, 4, 751, 256, 128


def _model(dtype, sd, seed=6):
    from centroids_reid_amd.bench_train import make_model
    model = make_model(num_classes=C, dtype=dtype, K=K)
    model.backbone.base.load_state_dict(sd)
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        model.center_loss.centers.copy_(torch.from_numpy(rng.standard_normal((C, 2048)).astype(np.float32)) * 0.3)
        model.fc_query.weight.copy_(torch.from_numpy((rng.standard_normal((C, 2048)) * 0.01).astype(np.float32)))
    return model


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_bf16_b64_fused_step_vs_fp32_oracle(dtype):
    """One bf16 training step at the benchmark size against the fp32 CPU oracle (train_ctl_model.py:38-152):
    per-image embedding cosine > 0.995 (measured 0.9977: bf16 storage of the raw conv outputs is amplified by every
    BatchNorm's (|mean| + std) / std -- the same drift an autocast run of the reference has), the four weighted
    losses within 5 % (+2e-3 absolute; measured 0.01-2.6 %).  Round 5: the same step in f16 (the reference's precision=16, loss
    scale on the device) against the same oracle: three more mantissa bits -> cosine > 0.9995, losses within 1 %."""
    from oracle import backbone_oracle as bo, reid_oracle as ro
    torch.set_num_threads(32)
    sd = bo.make_state_dict("resnet50", 1, seed=77)
    model = _model(dtype, sd)
    centers0 = model.center_loss.centers.detach().cpu().clone(); fc0 = model.fc_query.weight.detach().cpu().clone()
    x = bo.synthetic_images(P * K, H, W, seed=3)
    labels = torch.from_numpy(np.repeat((np.arange(P) * 7) % C, K).astype(np.int64))
    is_real = torch.ones(P * K, dtype=torch.bool)
    out = model.forward_backward((x.cuda(), labels.cuda(), torch.zeros(P * K, dtype=torch.int64), is_real), 0)
    assert model.fused_heads                                  # the hand-scheduled path the benchmark runs
    feat_dev = model.backbone.engine  # noqa: F841  (engine exists -> HIP path)
    with torch.no_grad():
        _, feat = bo.backbone_forward(x, {k: v.clone() for k, v in sd.items()}, "resnet50", 1, training=True)
        o = ro.ctl_heads(feat, labels, is_real, torch.ones(2048), torch.zeros(2048), torch.zeros(2048), torch.ones(2048),
                         fc0, centers0, P, K)
    # embeddings: recompute the bf16 forward (the step does not return them)
    with torch.no_grad():
        _, f16 = model.backbone.engine.forward(x.cuda(), True, False)
    f16 = f16.float().cpu().numpy(); f32 = feat.numpy()
    cos = (f16 * f32).sum(1) / np.linalg.norm(f16, axis=1) / np.linalg.norm(f32, axis=1)
    print("bf16 vs fp32-oracle embeddings: min cosine", cos.min(), "max rel err", np.abs(f16 - f32).max() / np.abs(f32).max())
    pairs = {n: (float(model.losses_dict[n][-1]), float(o[n])) for n in ("query_xent", "query_triplet", "query_center", "centroid_triplet")}
    print(pairs, float(out["loss"]), float(o["total"]))
    f16_mode = dtype == torch.float16
    assert cos.min() > (0.9995 if f16_mode else 0.995), cos.min()
    for n, (got, ref) in pairs.items():
        assert abs(got - ref) < (1e-2 if f16_mode else 5e-2) * abs(ref) + 2e-3, (n, got, ref)
    assert abs(float(out["loss"]) - float(o["total"])) < (5e-3 if f16_mode else 2e-2) * abs(float(o["total"]))
    if f16_mode:
        # gradients are finite and correctly unscaled: one optimiser step applies (no overflow at the settled scale) and moves the
        # classifier like the oracle's gradient says (same sign on the largest entries)
        model.loss_scaler.state.copy_(torch.tensor([1024.0, 1.0 / 1024.0]))
        model.forward_backward((x.cuda(), labels.cuda(), torch.zeros(P * K, dtype=torch.int64), is_real), 1)
        opt, _ = model.optimizers()
        n0 = opt.step_count
        model.apply_optimizers()
        assert opt.step_count == n0 + 1 and model.loss_scaler.get_scale() == 1024.0
        assert all(torch.isfinite(p).all() for p in model.parameters())


def test_graph_replays_equal_eager_steps(monkeypatch):
    """3 hipGraph replays of the captured step == 3 eager steps from the same state: loss trajectory, Adam's device
    step counter, centers, a backbone weight, BNNeck statistics.  The classifier GEMMs run in their single-pass form
    here (the default split-K combines partials with fp32 atomics, and Adam's first steps turn last-bit gradient noise
    into +-lr updates), so every kernel is deterministic and the two runs must agree to the last bit."""
    from oracle import backbone_oracle as bo
    from centroids_reid_amd import ops
    from centroids_reid_amd.bench_train import synthetic_batch
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    sd = bo.make_state_dict("resnet50", 1, seed=78)
    batches = [synthetic_batch(P, K, H, W, s) for s in range(3)]

    def run(use_graph):
        model = _model(torch.bfloat16, sd)
        opt, _ = model.optimizers()
        losses = []
        if not use_graph:
            for s in range(3):
                losses.append(float(model.training_step(batches[s], s)["loss"]))
        else:
            sx, sl = batches[0][0].clone(), batches[0][1].clone()
            static = (sx, sl, batches[0][2], batches[0][3])
            # capture WITHOUT advancing the state: snapshot, warm up + capture, restore
            snap = {k: v.detach().clone() for k, v in model.state_dict().items()}
            flat0, m0, v0, h0 = opt.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.hyper.clone()
            side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                model.training_step(static, 0)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                gout = model.training_step(static, 0)
            with torch.no_grad():
                model.load_state_dict(snap)
                opt.flat.copy_(flat0); opt.exp_avg.copy_(m0); opt.exp_avg_sq.copy_(v0)
                opt.hyper[1:].copy_(h0[1:])          # step counter back to 0; hyper[0] (the lr set by the warm-up step) stays
            model.backbone.engine.fold_counters()
            for s in range(3):
                sx.copy_(batches[s][0]); sl.copy_(batches[s][1])
                g.replay()
                losses.append(float(gout["loss"]))
        torch.cuda.synchronize()
        return (losses, opt.step_count, model.center_loss.centers.detach().cpu().numpy().copy(),
                model.backbone.base.layer3[2].conv2.weight.detach().cpu().numpy().copy(),
                model.bn.running_mean.detach().cpu().numpy().copy())

    le, se, ce, we, re_ = run(False)
    lg, sg, cg, wg, rg = run(True)
    print("eager", le, "graph", lg)
    assert se == sg == 3
    assert lg == le
    np.testing.assert_array_equal(cg, ce)
    np.testing.assert_array_equal(wg, we)
    np.testing.assert_array_equal(rg, re_)


def test_map_delta_of_bf16_backbone_on_clustered_identities():
    """BASELINE metric (iii): embed clustered synthetic identities with the SAME weights in fp32 (parity mode) and in
    bf16 (throughput mode), run the retrieval evaluation on both, and bound the mAP difference.  The identities are
    separable but not trivially so (mAP in 0.3..0.9), so the delta is informative."""
    from centroids_reid_amd.bench_train import map_delta_bf16
    r = map_delta_bf16()
    print(r)
    assert 0.3 < r["mAP_f32"] < 0.95, r
    assert abs(r["mAP_bf16_minus_f32"]) < 2e-2, r
    assert r["min_cosine"] > 0.99, r


def test_plain_bench_run_is_lean_and_dumps_the_last_step(tmp_path):
    """`bench.py --gpus 1 --steps N --warmup 1 --dump-outputs DIR` (deterministic kernels): ONE stdout line with the headline
    fields and none of the --full side measurements; the last timed step's outputs in DIR as float32 / float64 .npy files
    (64 MB at most) whose loss is the line's final_loss; the same arguments dump the same arrays bit for bit (seeded inputs);
    and --steps sets the number of timed steps: two more steps advance Adam's device step counter by exactly two."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["CREID_DETERMINISTIC"] = "1"

    def bench(steps, tag):
        d = tmp_path / tag
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                            "--dump-outputs", str(d)], cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        lines = [ln for ln in r.stdout.strip().splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        return json.loads(lines[0]), {n[:-4]: np.load(d / n) for n in sorted(os.listdir(d))}

    line, arrs = bench(3, "a")
    assert line["metric"] == "train_images_per_sec" and line["unit"] == "images/s" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert not {"eval", "embed", "roofline", "roofline_hbm_stages", "cpu_baseline", "fp32_mode", "f16_train"} & set(line), line.keys()
    assert {"loss", "adam_step", "centers", "params_sample", "buffers"} <= set(arrs), sorted(arrs)
    for n, a in arrs.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert float(arrs["loss"][0]) == line["final_loss"]
    line_b, arrs_b = bench(3, "b")
    assert sorted(arrs_b) == sorted(arrs)
    for n in arrs:
        assert np.array_equal(arrs_b[n], arrs[n]), f"{n} differs between two runs with the same arguments"
    line_c, arrs_c = bench(5, "c")
    assert line_c["steps"] == 5
    assert arrs_c["adam_step"][0] - arrs["adam_step"][0] == 2.0, (arrs["adam_step"], arrs_c["adam_step"])
