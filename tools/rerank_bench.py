"""k-reciprocal re-ranking on the device (reid_metric.re_ranking, csrc/rerank.hip) on seeded unit-norm clustered features
(identities of about 13 images, like Market-1501), k1 = 20, k2 = 6, lambda = 0.3, at 2228 x 17661 x 2048 and one small shape:
  1. per-stage times between device events (re_ranking's own stage clock; the host's waits fall inside the stage that causes
     them), median of `--reps` calls after `--warmup`, and the whole call on the host clock around a device synchronise;
  2. nnz of V and V', the longest rows, the temporaries of every stage, and torch.cuda.max_memory_allocated above the inputs;
  3. at the small shape, the deviation from the float64 reference of tests/rerank_ref.py fed with the device's own distances.
Writes the markdown the README quotes:
    python tools/rerank_bench.py --out profiles/rerank.md
Needs a GPU; there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from centroids_reid_amd import reid_metric as rm   # noqa: E402

SHAPES = [(2228, 17661, 2048), (160, 640, 2048)]
K1, K2, LAM = 20, 6, 0.3
STAGES = ["neighbours", "row_maxima", "reciprocal_sets", "weights", "expansion", "column_index", "blend"]


def features(nq, ng, D, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    n = nq + ng
    ids = max(2, n // 13)
    centres = torch.randn((ids, D), generator=gen, device="cuda")
    label = torch.randint(0, ids, (n,), generator=gen, device="cuda")
    f = rm.l2_normalize(centres[label] + 0.6 * torch.randn((n, D), generator=gen, device="cuda"))
    return f[:nq].contiguous(), f[nq:].contiguous()


def run_shape(nq, ng, D, warmup, reps):
    q, g = features(nq, ng, D, seed=nq)
    torch.cuda.synchronize()
    live = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    stats = {}
    out = rm.re_ranking(q, g, K1, K2, LAM, stats=stats)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - live
    first = out.clone()
    del out
    for _ in range(warmup):
        rm.re_ranking(q, g, K1, K2, LAM)
    per_stage, whole = {s: [] for s in STAGES}, []
    for _ in range(reps):
        st = {"timing": True}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = rm.re_ranking(q, g, K1, K2, LAM, stats=st)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3)
        assert torch.equal(out, first), "two runs differ"
        del out
        for s in STAGES:
            per_stage[s].append(st["stage_ms"][s])
    t_plain = []
    qq, gg = rm.row_sqnorm(q), rm.row_sqnorm(g)
    for _ in range(warmup + reps):                        # what the evaluation ranks without re-ranking
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rm.get_euclidean(q, g, qq, gg)
        torch.cuda.synchronize()
        t_plain.append((time.perf_counter() - t0) * 1e3)
    return {"shape": (nq, ng, D), "stage_ms": {s: float(np.median(v)) for s, v in per_stage.items()},
            "whole_ms": float(np.median(whole)), "whole_min": float(min(whole)), "whole_max": float(max(whole)),
            "plain_ms": float(np.median(t_plain[warmup:])), "peak": peak, "stats": stats, "q": q, "g": g, "out": first}


def deviation(r):
    """max |device - float64 reference| of the result and of V' at the small shape."""
    from rerank_ref import rerank_reference
    q, g = r["q"], r["g"]
    nq, N = q.shape[0], q.shape[0] + g.shape[0]
    X = torch.cat([q, g])
    d_all = rm.get_euclidean(X, X).cpu().numpy()
    dbg = {}
    out = rm.re_ranking(q, g, K1, K2, LAM, debug=dbg).cpu().numpy()
    ref, sets, ref_vq = rerank_reference(d_all, nq, K1, K2, LAM)
    rp, cols, vals = (dbg[k].cpu().numpy() for k in ("vprime_rowptr", "vprime_cols", "vprime_vals"))
    vq = np.zeros((N, N), np.float32)
    vq[np.repeat(np.arange(N), np.diff(rp)), cols] = vals
    rs, rc = dbg["rstar_rowptr"].cpu().numpy(), dbg["rstar_cols"].cpu().numpy()
    sets_equal = all(rc[rs[i]:rs[i + 1]].tolist() == sets[i].tolist() for i in range(N))
    return float(np.abs(out - ref).max()), float(np.abs(vq - ref_vq).max()), sets_equal


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="markdown file to write (default: standard output only)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/rerank_bench.py needs a GPU")
    rows = [run_shape(nq, ng, D, a.warmup, a.reps) for nq, ng, D in SHAPES]
    dev_out, dev_v, sets_equal = deviation(rows[-1])
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    mib = lambda b: f"{b / 2 ** 20:.1f}"                                    # noqa: E731
    lines = ["# k-reciprocal re-ranking on the device", "",
             f"`python tools/rerank_bench.py` on {torch.cuda.get_device_name(0)} ({arch}), one box, one session; seeded unit-norm clustered "
             f"features, k1 = {K1}, k2 = {K2}, lambda = {LAM}; median of {a.reps} calls after {a.warmup} warm-ups.  Stage times are "
             "between device events inside `reid_metric.re_ranking` and include the host's waits (the nnz read-backs); the whole "
             "call is the host clock around a device synchronise.", "",
             "| stage | " + " | ".join(f"{r['shape'][0]} x {r['shape'][1]} x {r['shape'][2]}" for r in rows) + " |",
             "|---|" + "---:|" * len(rows)]
    for s in STAGES:
        lines.append(f"| {s} (ms) | " + " | ".join(f"{r['stage_ms'][s]:.3f}" for r in rows) + " |")
    lines.append("| **whole call (ms, min .. max)** | " + " | ".join(
        f"**{r['whole_ms']:.2f}** ({r['whole_min']:.2f} .. {r['whole_max']:.2f})" for r in rows) + " |")
    lines.append("| get_euclidean(q, g) alone (ms) | " + " | ".join(f"{r['plain_ms']:.3f}" for r in rows) + " |")
    lines.append("| nnz V / V' | " + " | ".join(f"{r['stats']['nnz_v']} / {r['stats']['nnz_vprime']}" for r in rows) + " |")
    lines.append("| longest row V / V' | " + " | ".join(
        f"{r['stats']['max_row_v']} / {r['stats']['max_row_vprime']}" for r in rows) + " |")
    lines.append("| peak above the inputs (MiB) | " + " | ".join(mib(r["peak"]) for r in rows) + " |")
    lines.append("| output + distance matrix (MiB) | " + " | ".join(mib(2 * r["shape"][0] * r["shape"][1] * 4) for r in rows) + " |")
    lines.append("| an N x N fp32 matrix would be (MiB) | " + " | ".join(
        mib((r["shape"][0] + r["shape"][1]) ** 2 * 4) for r in rows) + " |")
    for s in STAGES[:-1]:
        lines.append(f"| temporaries, {s} (MiB) | " + " | ".join(mib(r["stats"]["temp_bytes"][s]) for r in rows) + " |")
    lines.append("")
    for r in rows:
        top = max(STAGES, key=lambda s: r["stage_ms"][s])
        total = sum(r["stage_ms"].values())
        lines.append(f"At {r['shape'][0]} x {r['shape'][1]} the stage `{top}` dominates: {r['stage_ms'][top]:.2f} of "
                     f"{total:.2f} ms ({100 * r['stage_ms'][top] / total:.0f} %).")
    nq, ng, _ = rows[-1]["shape"]
    lines += ["", f"Deviation from the float64 reference (`tests/rerank_ref.py`, fed the device's own fp32 distances) at {nq} x {ng}: "
              f"max |out - ref| = {dev_out:.3e}, max |V' - ref| = {dev_v:.3e}; R* rows equal: {sets_equal}.  "
              f"The tests' bound is max(4 x the float32 restatement's own deviation, 32 x 2^-23 = {32 * 2.0 ** -23:.3e})."]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
