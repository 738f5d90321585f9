"""Exact fp32 top-k with a 16-bit pre-filter (reid_metric.topk_stream(prefilter=...)) against the fp32 topk_stream, in one process:
clustered unit-norm features, D = 2048, at 2228 x 17661 and 6250 x 200 000, k = 50 and k = 21:
  1. asserts pre-filtered == fp32 (indices and distance bits) for bf16 and f16;
  2. times fp32, bf16, f16 and the two with a gallery pack made once (g_pack), alternating: warm-ups, then timed calls between
     device events (median, min .. max);
  3. per-stage times of one call (stats["stage_ms"]: pack of g and of q, sample, collect, re-score, repair), the distribution of
     kept entries per row, fallback_rows, and torch.cuda.max_memory_allocated above the live inputs;
  4. re_ranking's stage table at 2228 x 17661 with and without prefilter.
Prints the markdown tables profiles/topk_prefilter.md quotes (--out FILE writes them as well):
    python tools/topk_prefilter_bench.py --out tables.md
Needs a GPU; there is no fallback."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from centroids_reid_amd import reid_metric as rm   # noqa: E402

SHAPES = [(2228, 17661), (6250, 200_000)]
D, KS = 2048, (50, 21)
MODES = [("fp32", None, False), ("bf16", torch.bfloat16, False), ("f16", torch.float16, False),
         ("bf16 + g_pack", torch.bfloat16, True), ("f16 + g_pack", torch.float16, True)]


def features(nq, ng, seed):
    """Unit-norm rows around (nq + ng) / 20 unit-norm centres (noise norm ~ 0.7 of the centre's): identities with ~20 images."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    nc = max(1, (nq + ng) // 20)
    centres = torch.randn((nc, D), generator=gen, device="cuda")
    centres /= centres.norm(dim=1, keepdim=True)
    which = torch.randint(0, nc, (nq + ng,), generator=gen, device="cuda")
    f = centres[which] + (0.7 / D ** 0.5) * torch.randn((nq + ng, D), generator=gen, device="cuda")
    del centres
    fn, sq = rm.l2_normalize(f, return_sqnorm=True)
    del f
    return fn[:nq].contiguous(), fn[nq:].contiguous(), sq[:nq].contiguous(), sq[nq:].contiguous()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    live = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - live
    del out
    return peak


def run_shape(nq, ng, k, warmup, reps):
    q, g, qq, gg = features(nq, ng, seed=nq)
    packs = {dt: rm.prefilter_pack(g, dt) for dt in (torch.bfloat16, torch.float16)}
    calls = {}
    for name, dt, packed in MODES:
        kw = {} if dt is None else {"prefilter": dt, "g_pack": packs[dt] if packed else None}
        calls[name] = (lambda kw=kw: rm.topk_stream(q, g, k, qq, gg, **kw))
    ref = calls["fp32"]()
    rows = []
    for name, dt, packed in MODES:
        got = calls[name]()
        assert torch.equal(got[0], ref[0]), f"{name}: indices differ from the fp32 path"
        assert torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32)), f"{name}: distance bits differ"
        del got
    for _ in range(warmup):
        for name in calls:
            calls[name]()
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name in calls:
            times[name].append(timed(calls[name]))
    base = float(np.median(times["fp32"]))
    for name, dt, packed in MODES:
        t = times[name]
        row = dict(shape=f"{nq} x {ng}", k=k, mode=name, ms=float(np.median(t)), lo=min(t), hi=max(t), ratio=float(np.median(t)) / base,
                   mem=peak_above_inputs(calls[name]))
        st = {"timing": True}
        kw = {} if dt is None else {"prefilter": dt, "g_pack": packs[dt] if packed else None}
        rm.topk_stream(q, g, k, qq, gg, stats=st, **kw)
        row.update(fallback_rows=st["fallback_rows"], max_candidates=st["max_candidates"], stage=st.get("stage_ms"))
        if dt is not None:
            kept = st["kept"].float()
            row.update(kept=[float(v) for v in (kept.mean(), kept.median(), torch.quantile(kept, 0.99), kept.max())],
                       margin_max=st["margin_max"])
        rows.append(row)
    return rows


def rerank_rows(nq, ng):
    q, g, _, _ = features(nq, ng, seed=nq)
    out, ref = [], None
    for name, dt in (("fp32", None), ("bf16", torch.bfloat16), ("f16", torch.float16)):
        rm.re_ranking(q, g, prefilter=dt)                                     # warm-up
        st = {"timing": True}
        res = rm.re_ranking(q, g, prefilter=dt, stats=st)
        ref = res if ref is None else ref
        assert torch.equal(res.view(torch.int32), ref.view(torch.int32)), f"re_ranking(prefilter={name}) changed bits"
        out.append((name, st["stage_ms"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = SHAPES[:1] if a.small_only else SHAPES
    rows = [r for nq, ng in shapes for k in KS for r in run_shape(nq, ng, k, a.warmup, a.reps)]
    mib = lambda b: f"{b / 2**20:.0f}"                                        # noqa: E731
    out = [f"topk_stream, D = {D}, clustered unit-norm features, {a.reps} timed calls per mode after {a.warmup} warm-ups, modes "
           "alternating in one process; ms = median (min .. max); ratio = median / the fp32 median of the same shape and k.", "",
           "| shape | k | mode | ms | ratio to fp32 | peak MiB above inputs | fallback_rows | max_candidates | kept per row: mean / "
           "median / p99 / max | margin_max |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        kept = " / ".join(f"{v:.0f}" for v in r["kept"]) if "kept" in r else "-"
        out.append(f"| {r['shape']} | {r['k']} | {r['mode']} | {r['ms']:.3f} ({r['lo']:.3f} .. {r['hi']:.3f}) | {r['ratio']:.3f} | "
                   f"{mib(r['mem'])} | {r['fallback_rows']} | {r['max_candidates']} | {kept} | "
                   f"{r.get('margin_max', float('nan')):.3g} |")
    names = ["pack_g", "pack_q", "sample", "collect", "rescore", "repair"]
    out += ["", "Stages of one call, ms between device events (host waits fall inside the stage that caused them):", "",
            "| shape | k | mode | " + " | ".join(names) + " |", "|---|---|---|" + "---|" * len(names)]
    for r in rows:
        if r["stage"]:
            out.append(f"| {r['shape']} | {r['k']} | {r['mode']} | " + " | ".join(f"{r['stage'].get(n, 0.0):.3f}" for n in names) + " |")
    nq, ng = SHAPES[0]
    rr = rerank_rows(nq, ng)
    stages = list(rr[0][1])
    out += ["", f"re_ranking at {nq} x {ng} (k1 = 20, k2 = 6), ms per stage of one call:", "",
            "| prefilter | " + " | ".join(stages) + " | total |", "|---|" + "---|" * (len(stages) + 1)]
    for name, ms in rr:
        out.append(f"| {name} | " + " | ".join(f"{ms[s]:.3f}" for s in stages) + f" | {sum(ms.values()):.3f} |")
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
