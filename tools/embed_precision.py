"""Speed and accuracy of the eval-mode embedding forward per compute mode: bf16, bf16x3 (fp32 activations, three bf16 MFMAs per
product) and fp32, as graph-captured forwards (the way validation / inference replay them), on one GPU.

    python tools/embed_precision.py [--iters N]      -> one JSON line

embeddings/s: ResNet50 at 256 x 128, batch 128 and 512; ResNet50-IBN-a at 320 x 320, batch 256.  Error of each mode against the
fp32 mode on the same weights, B = 32 (R50 256 x 128): max-abs and max per-row relative L2 error of the L2-normalised BNNeck output
(eval BatchNorm1d with fixed statistics).  The per-layer kernel times come from a separate
`rocprofv3 --kernel-trace --stats` pass over this script (--only MODE,ARCH,B limits it to one configuration); --layers DB turns
that pass's database into the per-layer-class table of profiles/bf16x3_embed.md (ResNet50 256 x 128, batch 128):

    rocprofv3 --kernel-trace --stats -d OUT -o x3 -- python tools/embed_precision.py --only bf16x3,resnet50,128 --iters 5
    python tools/embed_precision.py --layers OUT/.../x3_results.db"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from centroids_reid_amd import backbone as bb  # noqa: E402
from oracle import backbone_oracle as bo  # noqa: E402   (deterministic weights / images only)

MODES = {"bf16": torch.bfloat16, "bf16x3": "bf16x3", "fp32": torch.float32}
CONFIGS = [("resnet50", 256, 128, 128), ("resnet50", 256, 128, 512), ("resnet50_ibn_a", 320, 320, 256)]


def make_net(arch):
    net = bb.build_backbone(arch, 1)
    net.load_state_dict(bo.make_state_dict(arch, 1, seed=11), strict=False)
    return net.cuda()


def rate(eng, x, iters):
    """Images per second of a graph-captured eval forward (median of `iters` timed replays)."""
    with torch.no_grad():
        for _ in range(2):
            eng.forward(x, False)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.forward(x, False)
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
    return x.shape[0] / float(np.median(ts)), float(np.median(ts))


def neck(feat):
    rng = np.random.default_rng(3)
    D = feat.shape[1]
    rm = torch.from_numpy(rng.standard_normal(D) * 0.1).cuda()
    rv = torch.from_numpy(rng.uniform(0.5, 2.0, D)).cuda()
    return F.normalize(F.batch_norm(feat.double(), rm, rv, None, None, False, 0.0, 1e-5), dim=1)


def eval_order_shapes(B, H, W):
    """(layer, (cin, cout, k, stride, Hin, Win)) of ResNet50's non-stem convolutions in the eval forward's launch order
    (per block: conv1, conv2, downsample, conv3)."""
    from centroids_reid_amd.bench_train import conv_shapes
    shapes, out, i = conv_shapes(B, H, W), [], 0
    for layer, n in enumerate((3, 4, 6, 3), start=1):
        for b in range(n):
            c1, c2, c3 = shapes[i:i + 3]
            ds = [shapes[i + 3]] if b == 0 else []
            out += [(layer, sh) for sh in [c1, c2] + ds + [c3]]
            i += 4 if b == 0 else 3
    return out


def layer_table(db, B=128, H=256, W=128):
    """Per layer class (layer, kernel size): us per forward, fraction of the bf16 MFMA peak for the 3x work, useful TF/s against
    the 157 TF f32 peak, and HBM-side bytes/s (fp32 activations in + out, both weight planes)."""
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, end - start from kernels where name like '%igemm_x3_kernel%' order by start").fetchall()
    shapes = eval_order_shapes(B, H, W)
    n = len(shapes)
    reps = len(rows) // n
    t = np.median(np.array([d for _, d in rows[len(rows) - reps * n:]], dtype=np.float64).reshape(reps, n), axis=0) * 1e-3   # us
    classes = {}
    for k, (layer, (cin, cout, kk, s, h, w)) in enumerate(shapes):
        oh, ow = (h + 2 * (kk // 2) - kk) // s + 1, (w + 2 * (kk // 2) - kk) // s + 1
        flops = 2.0 * B * oh * ow * cout * cin * kk * kk
        byts = 4.0 * B * (h * w * cin + oh * ow * cout) + 4.0 * cout * cin * kk * kk
        c = classes.setdefault((layer, f"{kk}x{kk}"), [0.0, 0.0, 0.0, 0])
        c[0] += t[k]; c[1] += flops; c[2] += byts; c[3] += 1
    print("| layer | conv | launches | us / forward | bf16 MFMA frac (3x work) | useful TF/s (frac of 157 TF f32) | GB/s |")
    print("|---|---|---|---|---|---|---|")
    tot = [0.0, 0.0, 0.0]
    for (layer, kind), (us, fl, by, cnt) in sorted(classes.items()):
        tot[0] += us; tot[1] += fl; tot[2] += by
        print(f"| {layer} | {kind} | {cnt} | {us:.0f} | {3 * fl / (us * 1e-6) / 2.5e15:.3f} | {fl / (us * 1e-6) / 1e12:.0f} "
              f"({fl / (us * 1e-6) / 157e12:.2f}) | {by / (us * 1e-6) / 1e9:.0f} |")
    us, fl, by = tot
    print(f"| all | | {n} | {us:.0f} | {3 * fl / (us * 1e-6) / 2.5e15:.3f} | {fl / (us * 1e-6) / 1e12:.0f} ({fl / (us * 1e-6) / 157e12:.2f}) "
          f"| {by / (us * 1e-6) / 1e9:.0f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="", help="rocprofv3 database of an --only bf16x3,resnet50,128 pass: per-layer table")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="", help="MODE,ARCH,B: time that configuration alone (profiling pass)")
    args = ap.parse_args()
    if args.layers:
        layer_table(args.layers)
        return
    out = {"metric": "eval-mode embeddings/s per compute mode (graph-captured forward) + embedding error vs fp32"}
    nets = {}
    if args.only:
        mode, arch, B = args.only.split(",")
        H, W = (320, 320) if arch.endswith("ibn_a") else (256, 128)
        eng = bb.BackboneEngine(make_net(arch), MODES[mode])
        r, t = rate(eng, bo.synthetic_images(int(B), H, W, seed=5).cuda(), args.iters)
        out[f"{mode}_{arch}_{H}x{W}_b{B}"] = {"emb_per_s": round(r, 1), "ms": round(t * 1e3, 3)}
        print(json.dumps(out), flush=True)
        return
    for arch, H, W, B in CONFIGS:
        net = nets.setdefault(arch, make_net(arch))
        x = bo.synthetic_images(B, H, W, seed=5).cuda()
        for mode, dt in MODES.items():
            r, t = rate(bb.BackboneEngine(net, dt), x, args.iters)
            out[f"{mode}_{arch}_{H}x{W}_b{B}"] = {"emb_per_s": round(r, 1), "ms": round(t * 1e3, 3)}
            print(f"{mode:7s} {arch} {H}x{W} B={B}: {r:9.1f} emb/s ({t * 1e3:.3f} ms)", file=sys.stderr, flush=True)
        del x
        torch.cuda.empty_cache()
    for arch, H, W, _ in CONFIGS[:1] + CONFIGS[2:]:
        net = nets[arch]
        x = bo.synthetic_images(32, H, W, seed=5).cuda()
        with torch.no_grad():
            ref = neck(bb.BackboneEngine(net, torch.float32).forward(x, False)[1])
            for mode in ("bf16", "bf16x3"):
                e = neck(bb.BackboneEngine(net, MODES[mode]).forward(x, False)[1])
                out[f"err_{mode}_{arch}_{H}x{W}"] = {"max_abs": float((e - ref).abs().max()),
                                                     "rel_l2_max": float((e - ref).norm(dim=1).max()),
                                                     "rel_l2_mean": float((e - ref).norm(dim=1).mean())}
    r128 = out["bf16x3_resnet50_256x128_b128"]["emb_per_s"] / out["fp32_resnet50_256x128_b128"]["emb_per_s"]
    out["bf16x3_over_fp32_b128"] = round(r128, 3)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
