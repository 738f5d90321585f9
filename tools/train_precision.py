"""Training speed and accuracy per compute mode: bf16, bf16x3 (fp32 activations, three bf16 MFMAs per product in every non-stem
convolution's forward, data gradient and weight gradient) and fp32, at the benchmark config (ResNet50 256 x 128, P16 x K4, 751
classes), all in one process on one GPU.

    python tools/train_precision.py [--steps N] [--curve-steps N]      -> one JSON line

images/s: the graph-captured full CTL training step of bench_train.fp32_mode_step (a fresh synthetic batch copied into the captured
step's inputs before every replay).  Accuracy: the bench_train.train_curve_delta recipe (same seed, same clustered-identity
batches, full step) for bf16x3 against fp32 -- the largest and mean relative loss gap over the trajectory.
--only MODE times that mode alone (for a `rocprofv3 --kernel-trace --stats` pass); --kernels DB prints that pass's per-kernel
table (the training step's convolution kernels by name: forward and data gradient share igemm_x3_kernel)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from centroids_reid_amd import bench_train as bt  # noqa: E402

MODES = {"bf16": torch.bfloat16, "bf16x3": "bf16x3", "fp32": torch.float32}


def curve_gap(mode, P=16, K=4, H=256, W=128, steps=50, n_id=64, noise=0.6):
    """bench_train.train_curve_delta with `mode` in place of bf16: per-step loss of mode and fp32 on identical weights / batches."""
    gen = torch.Generator(device="cuda").manual_seed(1)
    base = torch.randn((n_id, 3, H // 16, W // 16), generator=gen, device="cuda")
    base = torch.nn.functional.interpolate(base, size=(H, W), mode="bilinear", align_corners=False)
    camid = torch.zeros(P * K, dtype=torch.int64)
    is_real = torch.ones(P * K, dtype=torch.bool)
    curves = {}
    for name, dt in (("fp32", torch.float32), (mode, MODES[mode])):
        torch.manual_seed(0)
        model = bt.make_model(num_classes=n_id, dtype=dt)
        g2 = torch.Generator(device="cuda").manual_seed(2)
        losses = []
        for s in range(steps):
            ids = (np.arange(P) * 5 + s * P) % n_id
            x = base[torch.as_tensor(ids, device="cuda")].repeat_interleave(K, 0) \
                + noise * torch.randn((P * K, 3, H, W), generator=g2, device="cuda")
            labels = torch.as_tensor(np.repeat(ids, K).astype(np.int64), device="cuda")
            losses.append(model.training_step((x, labels, camid, is_real), s)["loss"].detach().float().reshape(()))
        curves[name] = torch.stack(losses).cpu().numpy().astype(np.float64)
        del model
        torch.cuda.empty_cache()
    f, b = curves["fp32"], curves[mode]
    rel = np.abs(b - f) / np.abs(f)
    return {"steps": steps, "max_rel_loss_gap": float(rel.max()), "mean_rel_loss_gap": float(rel.mean()), "step_of_max": int(rel.argmax()),
            "loss_f32_first_last": [float(f[0]), float(f[-1])], f"loss_{mode}_first_last": [float(b[0]), float(b[-1])],
            "loss_f32_every_10th": [round(float(v), 4) for v in f[::10]], f"loss_{mode}_every_10th": [round(float(v), 4) for v in b[::10]]}


def kernel_table(db):
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, count(*), sum(end - start) from kernels group by name order by 3 desc").fetchall()
    tot = sum(r[2] for r in rows)
    print("| kernel | launches | ms total | share |\n|---|---|---|---|")
    for name, n, t in rows[:25]:
        print(f"| `{name.split('(')[0][:90]}` | {n} | {t * 1e-6:.2f} | {t / tot:.3f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--curve-steps", type=int, default=50)
    ap.add_argument("--only", default="", help="MODE: time that mode alone (profiling pass)")
    ap.add_argument("--kernels", default="", help="rocprofv3 database of an --only pass: per-kernel table")
    args = ap.parse_args()
    if args.kernels:
        kernel_table(args.kernels)
        return
    P, K, H, W = 16, 4, 256, 128
    out = {"metric": "graph-captured CTL training images/s per compute mode (ResNet50 256x128, P16xK4, 751 classes)"}
    for mode in ([args.only] if args.only else list(MODES)):
        r = bt.fp32_mode_step(P, K, H, W, steps=args.steps, warmup=3, dtype=MODES[mode])
        out[mode] = {"images_per_s": round(r["value"], 1), "ms_per_step": round(r["ms_per_step"], 3)}
        print(f"{mode:7s} {r['value']:9.1f} img/s ({r['ms_per_step']:.3f} ms)", file=sys.stderr, flush=True)
    if not args.only:
        out["bf16x3_over_fp32"] = round(out["bf16x3"]["images_per_s"] / out["fp32"]["images_per_s"], 3)
        out["curve_bf16x3_vs_fp32"] = curve_gap("bf16x3", steps=args.curve_steps)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
