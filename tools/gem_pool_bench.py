"""Generalized-mean pooling (creid_gem_fwd / creid_gem_bwd) beside the average pool (creid_gap_fwd_count / creid_gap_bwd), one
process, one session:
  1. launch times at the final map of the B = 64 and B = 128 training steps (HW = 128, C = 2048; bf16, and fp32 for the larger):
     >= 3 warm-up rounds, then ROUNDS timed rounds between device events, the two pools ALTERNATING round by round.  Every round
     walks a ring of maps larger than the 256 MB last-level cache, so each launch reads its map from HBM as it does inside a step
     (there the map was written a whole backward pass earlier);
  2. the byte floor of each launch -- the bytes it must move over the HBM peak of MI355X_BW TB/s -- and the time as a multiple;
  3. the training step (ResNet50, 256 x 128, P = 16, K = 4, bf16) with pooling="gem" against "avg", eager, alternating, with the
     library calls and the launches inside them counted on one step of each (torch's own fills and copies are not counted);
  4. the accuracy maxima that tests/test_gem_pool_gpu.py prints, as a share of their bounds (--test-log, the output of
     `pytest -s tests/test_gem_pool_gpu.py`).
Writes the markdown the README quotes:
    python tools/gem_pool_bench.py --out profiles/gem_pooling.md --test-log LOG
Needs a GPU; there is no fallback."""
import argparse
import collections
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from centroids_reid_amd import _lib as L           # noqa: E402

MI355X_BW = 8.0e12           # HBM3E peak, bytes / s
HW, C = 128, 2048
SHAPES = [(64, torch.bfloat16), (128, torch.bfloat16), (128, torch.float32)]
RING_BYTES = 640 << 20
ROUNDS = 12
# launches inside one library call (every other counted call is one launch)
LAUNCHES = {"creid_ctl_heads_fused": 6, "creid_gem_bwd": 2}
NO_LAUNCH = re.compile(r"(_bytes|_rows|_partials|_version|^creid_tune)")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3          # us


def pool_launches(B, dtype):
    """us per launch: {name: [per-round means]} for the four launches, over a ring of maps"""
    lib, st, dt = L.lib(), L.stream(), L._DT[dtype]
    esz = torch.empty((), dtype=dtype).element_size()
    n = max(2, RING_BYTES // (B * HW * C * esz))
    gen = torch.Generator(device="cuda").manual_seed(B)
    maps = [torch.relu(torch.randn((B * HW, C), generator=gen, device="cuda") * 2).to(dtype) for _ in range(n)]
    dxs = [torch.empty_like(m) for m in maps]
    feat = torch.empty((B, C), dtype=torch.float32, device="cuda")
    dfeat = torch.randn((B, C), generator=gen, device="cuda")
    stats = torch.empty((3, B, C), dtype=torch.float32, device="cuda")
    p = torch.full((1,), 3.0, device="cuda")
    pg = torch.zeros(1, device="cuda")
    parts = torch.empty(lib.creid_gem_bwd_partials(B, C, dt), dtype=torch.float32, device="cuda")
    counter = torch.zeros((), dtype=torch.long, device="cuda")
    calls = {
        "gap_fwd": lambda i: lib.creid_gap_fwd_count(L.ptr(maps[i]), B, HW, C, dt, L.ptr(feat), L.ptr(counter), st),
        "gem_fwd": lambda i: lib.creid_gem_fwd(L.ptr(maps[i]), B, HW, C, dt, L.ptr(p), 1e-6, L.ptr(feat), L.ptr(stats), L.ptr(counter), st),
        "gem_fwd_eval": lambda i: lib.creid_gem_fwd(L.ptr(maps[i]), B, HW, C, dt, L.ptr(p), 1e-6, L.ptr(feat), None, None, st),
        "gap_bwd": lambda i: lib.creid_gap_bwd(L.ptr(dfeat), B, HW, C, dt, L.ptr(dxs[i]), st),
        "gem_bwd": lambda i: lib.creid_gem_bwd(L.ptr(maps[i]), L.ptr(dfeat), L.ptr(stats), B, HW, C, dt, L.ptr(p), 1e-6, L.ptr(dxs[i]),
                                               L.ptr(pg), L.ptr(parts), st),
    }
    lib.creid_gem_fwd(L.ptr(maps[0]), B, HW, C, dt, L.ptr(p), 1e-6, L.ptr(feat), L.ptr(stats), None, st)     # stats for the backward
    out = collections.defaultdict(list)

    def ring(fn):
        for i in range(n):
            L.check(fn(i), "launch")
    for r in range(3 + ROUNDS):
        for name, fn in calls.items():                      # alternating: one ring of each per round
            t = timed(lambda: ring(fn)) / n
            if r >= 3:
                out[name].append(t)
    nbytes = B * HW * C * esz
    floors = {"gap_fwd": nbytes, "gem_fwd": nbytes, "gem_fwd_eval": nbytes, "gap_bwd": nbytes, "gem_bwd": 2 * nbytes}
    return out, floors, n


class _Counting:
    def __init__(self, h):
        self.h, self.calls = h, collections.Counter()

    def __getattr__(self, name):
        f = getattr(self.h, name)
        if NO_LAUNCH.search(name):
            return f

        def w(*a):
            self.calls[name] += 1
            return f(*a)
        return w


def train_steps():
    from centroids_reid_amd.config import get_cfg_defaults
    from centroids_reid_amd.train_ctl_model import CTLModel
    from centroids_reid_amd.bench_train import synthetic_batch
    P, K, H, W = 16, 4, 256, 128
    models = {}
    for mode in ("avg", "gem"):
        torch.manual_seed(0)
        cfg = get_cfg_defaults()
        cfg.MODEL.PRETRAINED = False
        cfg.DATALOADER.NUM_INSTANCE = K
        cfg.USE_MIXED_PRECISION = True
        m = CTLModel(cfg, num_classes=751, num_query=0, compute_dtype=torch.bfloat16, pooling=mode).cuda().train()
        m.configure_optimizers()
        models[mode] = m
    batches = [synthetic_batch(P, K, H, W, s) for s in range(4)]
    times = {k: [] for k in models}
    for r in range(3 + ROUNDS):
        for mode, m in models.items():
            t = timed(lambda: [m.training_step(b, 0) for b in batches]) / len(batches)
            if r >= 3:
                times[mode].append(t)
    counts = {}
    real = L.lib()
    for mode, m in models.items():
        L._lib = proxy = _Counting(real)
        try:
            m.training_step(batches[0], 0)
        finally:
            L._lib = real
        torch.cuda.synchronize()
        counts[mode] = (sum(proxy.calls.values()), sum(v * LAUNCHES.get(k, 1) for k, v in proxy.calls.items()), dict(proxy.calls))
    return times, counts, float(models["gem"].backbone.gap.p.detach())


def test_shares(path):
    """max share of bound per (kind, dtype) from the lines tests/test_gem_pool_gpu.py prints"""
    best = collections.defaultdict(float)
    if not path or not os.path.exists(path):
        return None
    for line in open(path):
        m = re.search(r"fwd torch\.(\w+) p=.*share of bound ([0-9.]+)", line)
        if m:
            best[("y", m.group(1))] = max(best[("y", m.group(1))], float(m.group(2)))
        m = re.search(r"bwd torch\.(\w+) p=.*dx share of bound ([0-9.]+).*share of bound ([0-9.]+)", line)
        if m:
            best[("dx", m.group(1))] = max(best[("dx", m.group(1))], float(m.group(2)))
            best[("dp", m.group(1))] = max(best[("dp", m.group(1))], float(m.group(3)))
    return best


def fmt(v):
    return f"{np.median(v):.1f} (min {np.min(v):.1f}, max {np.max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/gem_pooling.md")
    ap.add_argument("--test-log", default=None)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gem_pool_bench needs a GPU")
    lines = ["# Generalized-mean pooling beside the average pool", "",
             f"`python tools/gem_pool_bench.py` on an MI355X ({torch.cuda.get_device_properties(0).gcnArchName}), torch {torch.__version__}, HIP {torch.version.hip}; one "
             f"process, 3 warm-up rounds, then {ROUNDS} timed rounds between device events, the launches alternating round by round; "
             "every round walks a ring of maps larger than the last-level cache.  Median over the rounds (min, max), us per launch.", "",
             "## Launches", "",
             "| B x HW x C | type | launch | us | bytes moved | floor at 8 TB/s, us | time / floor |", "|---|---|---|---|---|---|---|"]
    med = {}
    for B, dtype in SHAPES:
        out, floors, n = pool_launches(B, dtype)
        med[(B, dtype)] = {k: float(np.median(v)) for k, v in out.items()}
        for name in ("gap_fwd", "gem_fwd", "gem_fwd_eval", "gap_bwd", "gem_bwd"):
            fl = floors[name] / MI355X_BW * 1e6
            lines.append(f"| {B} x {HW} x {C} | {str(dtype).split('.')[1]} | {name} | {fmt(out[name])} | {floors[name] / 2 ** 20:.0f} MiB | "
                         f"{fl:.1f} | {np.median(out[name]) / fl:.2f} |")
        print("\n".join(lines[-5:]), flush=True)
    lines += ["", "gap_fwd = creid_gap_fwd_count, gem_fwd = the training forward (counter and saved statistics), gem_fwd_eval = without "
              "them; gem_bwd = both of its launches (dx and the workgroup partials of dp, then the fixed-order sum).  The backward "
              "reads the map and writes a tensor of the same size; the average pool's backward only writes.", ""]
    if not a.skip_step:
        times, counts, p_end = train_steps()
        lines += ["## Training step (ResNet50, 256 x 128, P = 16, K = 4, bf16, eager)", "",
                  "| pooling | us per step | library calls | launches in them |", "|---|---|---|---|"]
        for mode in ("avg", "gem"):
            lines.append(f"| {mode} | {fmt(times[mode])} | {counts[mode][0]} | {counts[mode][1]} |")
        d = np.median(times["gem"]) - np.median(times["avg"])
        lines += ["", f"Difference of the medians: {d:+.1f} us per step.  `creid_ctl_heads_fused` counts as six launches and "
                  "`creid_gem_bwd` as two; torch's own fills and copies are not counted.  "
                  f"Calls that differ: " + ", ".join(f"{k} {counts['avg'][2].get(k, 0)} -> {counts['gem'][2].get(k, 0)}"
                                                       for k in sorted(set(counts['avg'][2]) | set(counts['gem'][2]))
                                                       if counts['avg'][2].get(k, 0) != counts['gem'][2].get(k, 0)) + ".",
                  f"(p after the timed steps: {p_end:.4f}, from 3.0.)", ""]
        m64 = med[(64, torch.bfloat16)]
        dk = m64["gem_fwd"] - m64["gap_fwd"] + m64["gem_bwd"] - m64["gap_bwd"]
        lines += [f"Of that difference the two pooling launches account for {dk:+.1f} us (table above, this batch); the rest, "
                  f"{d - dk:+.1f} us, is the separate-launch heads schedule in place of `creid_ctl_heads_fused`, whose last launch "
                  "also produced the first BatchNorm backward's column sums.", ""]
    sh = test_shares(a.test_log)
    if sh:
        lines += ["## Accuracy: measured maxima as a share of the tests' bounds", "",
                  "| quantity | fp32 | bf16 | f16 |", "|---|---|---|---|"]
        for q in ("y", "dx", "dp"):
            lines.append(f"| {q} | " + " | ".join(f"{sh[(q, d)]:.3f}" for d in ("float32", "bfloat16", "float16")) + " |")
        lines += ["", "Bounds: 4 x the error of the plain fp32 CPU composition against float64 on the same inputs (y, dx; dp against the "
                  "sum of the absolute terms), dx plus half a unit in the last place of its type.  In bf16 and f16 that half unit is "
                  "nearly all of dx's bound and the one rounding to the type nearly all of its error: a share near 1 there is the "
                  "rounding, the fp32 column shows the arithmetic.", ""]
    lines += ["## The scaled form and what it costs", "",
              "The sums are formed relative to the per-(b, c) maximum U: r = u / U (an IEEE division, so r = 1 exactly at the maximum and a "
              "constant channel pools to U with no rounding), S = sum r^p, y = U (S / HW)^(1/p) with the last power in fp64 per output.  "
              "Cost: the forward walks its slice of the map twice (maximum, then sums; the second walk finds the slice in the cache the "
              "first one filled), and per element one division, one v_log_f32 and one v_exp_f32 (the training forward one more "
              "multiply-add for the sum the dp coefficient needs); the backward one division, log and exp per element and no "
              "reduction over the map.  The time / floor column above is that cost: the average pool's forward does one add per "
              "element.  The alternative, an online rescale in the log2 domain, was not built and not measured.", "",
              "## Not measured", "",
              "* the step captured in a hipGraph (the table above is eager; tests/test_gem_pool_gpu.py checks that the captured step "
              "replays to the bits of the eager one);", "* any effect on mAP / mINP: no dataset.", ""]
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
