"""The streamed evaluation with a 16-bit pre-filter (reid_metric.R1_mAP(streamed=True, prefilter=...)) against the fp32 streamed
evaluation, in one process: the clustered features of tools/topk_prefilter_bench.py (un-normalised; the evaluation normalises),
D = 2048, at 2228 x 17661 and 6250 x 200 000, pid = the centre, with 0 %, 2 % and 10 % of the gallery labels randomised, cameras
uniform in 0..5:
  1. asserts pre-filtered == fp32 (valid, first, CMC and top-k equal; ap and mAP within 1e-12) for bf16 and f16;
  2. times whole compute() calls -- label upload, normalisation, plan, kernels, read-back -- of fp32, bf16 and f16, alternating:
     warm-ups, then timed calls on the host clock (every call ends in its read-back); median, min .. max;
  3. per-stage times of one call (last["prefilter"]["stage_ms"]), the listed pairs per row, fallback_rows, and
     torch.cuda.max_memory_allocated above the live inputs.
Prints the markdown tables profiles/eval_prefilter.md quotes (--out FILE writes them as well):
    python tools/eval_prefilter_bench.py --out tables.md
Needs a GPU; there is no fallback."""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from centroids_reid_amd import reid_metric as rm   # noqa: E402

SHAPES = [(2228, 17661), (6250, 200_000)]
D = 2048
NOISE = (0.0, 0.02, 0.10)
MODES = [("fp32", None), ("bf16", torch.bfloat16), ("f16", torch.float16)]


def features(nq, ng, seed):
    """Rows around (nq + ng) / 20 unit-norm centres (noise norm ~ 0.7 of the centre's): identities with ~20 images."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    nc = max(1, (nq + ng) // 20)
    centres = torch.randn((nc, D), generator=gen, device="cuda")
    centres /= centres.norm(dim=1, keepdim=True)
    which = torch.randint(0, nc, (nq + ng,), generator=gen, device="cuda")
    f = centres[which] + (0.7 / D ** 0.5) * torch.randn((nq + ng, D), generator=gen, device="cuda")
    return f, which.cpu().numpy(), nc


def labels(pids, nq, nc, noise, seed):
    rng = np.random.default_rng(seed)
    p = pids.copy()
    ng = len(p) - nq
    hit = nq + rng.choice(ng, int(round(noise * ng)), replace=False)
    p[hit] = rng.integers(0, nc, len(hit))
    return p, rng.integers(0, 6, len(p))


def quiet(fn):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn()


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    quiet(fn)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def run_case(f, pids, cams, nq, noise, warmup, reps):
    metrics = {name: rm.R1_mAP(num_query=nq, streamed=True, prefilter=dt) for name, dt in MODES}
    calls = {name: (lambda m=m: m.compute(f, pids, cams)) for name, m in metrics.items()}
    ref = quiet(calls["fp32"])
    ref_last = metrics["fp32"].last
    for name, dt in MODES[1:]:
        got = quiet(calls[name])
        last = metrics[name].last
        assert torch.equal(last["valid"], ref_last["valid"]) and torch.equal(last["first"], ref_last["first"]), name
        assert float((last["ap"] - ref_last["ap"]).abs().max()) <= 1e-12, name
        assert np.array_equal(got[0], ref[0]) and abs(got[1] - ref[1]) <= 1e-12 and np.array_equal(got[2], ref[2]), name
    for _ in range(warmup):
        for name in calls:
            quiet(calls[name])
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name in calls:
            times[name].append(timed(calls[name]))
    base = float(np.median(times["fp32"]))
    # the fp32 kernels alone (positives, count, finalize) on the same rows and plan: what the poslist + count + rescore stages replace
    fn, sq = rm.l2_normalize(f, return_sqnorm=True)
    plan = ref_last["plan"]
    fq, fg, qq, gg = fn[:nq], fn[nq:], sq[:nq].contiguous(), sq[nq:].contiguous()
    kern = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rm.stream_eval(fq, fg, qq, gg, plan)
        e1.record()
        e1.synchronize()
        kern.append(e0.elapsed_time(e1))
    kern_ms = float(np.median(kern[warmup:]))
    del fn, sq, fq, fg
    rows = []
    for name, dt in MODES:
        t = times[name]
        torch.cuda.synchronize()
        live = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        metrics[name].last = {"prefilter": {"timing": True}}
        quiet(calls[name])
        torch.cuda.synchronize()
        row = dict(shape=f"{nq} x {len(pids) - nq}", noise=noise, mode=name, ms=float(np.median(t)), lo=min(t), hi=max(t),
                   ratio=float(np.median(t)) / base, mem=torch.cuda.max_memory_allocated() - live, mAP=ref[1], kern_ms=kern_ms)
        info = metrics[name].last.get("prefilter")
        if info is not None:
            amb = info["ambiguous"].float()
            row.update(stage=info["stage_ms"], amb=(float(amb.mean()), float(amb.max())), fallback_rows=info["fallback_rows"],
                       margin_max=info["margin_max"], ran=info["dtype"])
        metrics[name].last = {}
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for nq, ng in (SHAPES[:1] if a.small_only else SHAPES):
        f, pids0, nc = features(nq, ng, seed=nq)
        for noise in NOISE:
            pids, cams = labels(pids0, nq, nc, noise, seed=nq + int(noise * 100))
            rows += run_case(f, pids, cams, nq, noise, a.warmup, a.reps)
        del f
    mib = lambda b: f"{b / 2**20:.0f}"                                        # noqa: E731
    out = [f"R1_mAP(streamed=True).compute, D = {D}, clustered features, {a.reps} timed calls per mode after {a.warmup} warm-ups, "
           "modes alternating in one process; ms = median (min .. max) of whole calls on the host clock; ratio = median / the fp32 "
           "median of the same shape and label noise.", "",
           "| shape | labels randomised | mode | ms | ratio to fp32 | peak MiB above inputs | listed pairs per row: mean / max | "
           "fallback_rows | margin_max | mAP |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        amb = f"{r['amb'][0]:.1f} / {r['amb'][1]:.0f}" if "amb" in r else "-"
        out.append(f"| {r['shape']} | {100 * r['noise']:.0f} % | {r['mode']} | {r['ms']:.3f} ({r['lo']:.3f} .. {r['hi']:.3f}) | "
                   f"{r['ratio']:.3f} | {mib(r['mem'])} | {amb} | {r.get('fallback_rows', '-')} | "
                   f"{r.get('margin_max', float('nan')):.3g} | {r['mAP']:.4f} |")
    names = ["pack", "poslist", "count", "rescore", "repair"]
    out += ["", "Stages of one pre-filtered call, ms between device events (pack: both packs and the margins; rescore: with the "
            "finalize; repair: with the reduction and the read-back; host waits fall inside the stage that caused them):", "",
            "| shape | labels randomised | mode | " + " | ".join(names) + " | fp32 poslist + count + finalize |",
            "|---|---|---|" + "---|" * (len(names) + 1)]
    for r in rows:
        if "stage" in r:
            out.append(f"| {r['shape']} | {100 * r['noise']:.0f} % | {r['mode']} | " +
                       " | ".join(f"{r['stage'].get(n, 0.0):.3f}" for n in names) + f" | {r['kern_ms']:.3f} |")
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
