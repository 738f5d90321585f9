"""Streamed top-k retrieval (reid_metric.topk_stream: no m x n matrix) against the materialised path (get_euclidean + topk_rows)
on seeded unit-norm random features, D = 2048, k = 50, at 2228 x 17661 and 6250 x 200 000:
  1. asserts streamed == materialised (indices and distance bits) and reports fallback_rows / max_candidates;
  2. times both paths in this process, alternating: >= 3 warm-ups each, then >= 20 timed calls each between device events;
  3. reports torch.cuda.max_memory_allocated above the live inputs for each path.
Writes the markdown table the README quotes:
    python tools/topk_stream_bench.py --out profiles/topk_stream.md
Needs a GPU; there is no fallback."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from centroids_reid_amd import reid_metric as rm   # noqa: E402

SHAPES = [(2228, 17661), (6250, 200_000)]
D, K = 2048, 50


def features(nq, ng, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    f = torch.randn((nq + ng, D), generator=gen, device="cuda", dtype=torch.float32)
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


def run_shape(nq, ng, warmup, reps):
    q, g, qq, gg = features(nq, ng, seed=nq)
    mat = lambda: rm.topk_rows(rm.get_euclidean(q, g, qq, gg), K)          # noqa: E731
    stats = {}
    stream = lambda: rm.topk_stream(q, g, K, qq, gg, stats=stats)          # noqa: E731
    ref, got = mat(), stream()
    assert torch.equal(got[0], ref[0]), "streamed indices differ from the materialised path"
    assert torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32)), "streamed distance bits differ"
    del ref, got
    first = dict(stats)
    mem_mat, mem_stream = peak_above_inputs(mat), peak_above_inputs(stream)
    for _ in range(warmup):
        mat(); stream()
    t_mat, t_stream = [], []
    for _ in range(reps):                                                   # alternating: both see the same clocks and caches
        t_mat.append(timed(mat))
        t_stream.append(timed(stream))
    t_mat, t_stream = np.asarray(t_mat), np.asarray(t_stream)
    med_m, med_s = float(np.median(t_mat)), float(np.median(t_stream))
    return {"shape": f"{nq} x {ng}", "mat_ms": med_m, "mat_min": float(t_mat.min()), "mat_max": float(t_mat.max()),
            "spread": float((t_mat.max() - t_mat.min()) / med_m), "stream_ms": med_s, "stream_min": float(t_stream.min()),
            "stream_max": float(t_stream.max()), "ratio": med_s / med_m, "mem_mat": mem_mat, "mem_stream": mem_stream,
            "matrix_bytes": nq * ng * 4, **first}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="markdown file to write (default: standard output only)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/topk_stream_bench.py needs a GPU")
    if a.warmup < 3 or a.reps < 20:
        sys.exit("at least 3 warm-ups and 20 timed calls per path")
    rows = [run_shape(nq, ng, a.warmup, a.reps) for nq, ng in SHAPES]
    mib = lambda b: f"{b / 2**20:.0f}"                                      # noqa: E731
    out = ["# Streamed top-k retrieval against the materialised path", "",
           f"`tools/topk_stream_bench.py` on {torch.cuda.get_device_name(0)}: seeded unit-norm random features, D = {D}, k = {K}; "
           f"both paths in one process, alternating, {a.warmup} warm-ups and {a.reps} timed calls each between device events "
           "(medians; min .. max in brackets).  Materialised = `get_euclidean` + `topk_rows`; streamed = `topk_stream` at its "
           "defaults (threshold sample, collect, select, host check of the flags).  Spread = (max - min) / median of the "
           "materialised timings.  Before timing, streamed == materialised was asserted (indices and distance bits).", "",
           "| shape | materialised ms | spread | streamed ms | streamed / materialised | peak MiB materialised | peak MiB streamed | "
           "matrix MiB | sample | capacity | fallback_rows | max_candidates |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['shape']} | {r['mat_ms']:.3f} ({r['mat_min']:.3f} .. {r['mat_max']:.3f}) | {100 * r['spread']:.1f} % | "
                   f"{r['stream_ms']:.3f} ({r['stream_min']:.3f} .. {r['stream_max']:.3f}) | {r['ratio']:.3f} | {mib(r['mem_mat'])} | "
                   f"{mib(r['mem_stream'])} | {mib(r['matrix_bytes'])} | {r['sample']} | {r['capacity']} | {r['fallback_rows']} | "
                   f"{r['max_candidates']} |")
    big = rows[-1]
    verdict = "meets" if big["ratio"] <= 1.0 + big["spread"] else "MISSES"
    out += ["", f"Acceptance at {big['shape']}: streamed / materialised = {big['ratio']:.3f} against 1 + spread = "
                f"{1.0 + big['spread']:.3f}: {verdict} the bar (not slower than the materialised path by more than its own "
                "run-to-run spread).  Peak MiB is `torch.cuda.max_memory_allocated` above the live inputs."]
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
