"""Open-set operating points without the m x n matrix (reid_metric.roc_stream: three radix passes of the streamed contraction with
the histogram epilogue, three select steps) on seeded CLUSTERED unit rows, D = 2048, at 2228 x 17661 and 6250 x 200 000, fp32 and
bf16:
  1. asserts roc_stream == roc_matrix on the get_euclidean matrix of the same rows (where that matrix is formed anyway: 3.);
  2. per radix pass, times the histogram launch (creid_stream_dist_hist[_h16]) against the count launch of the streamed
     evaluation (creid_stream_count[_h16]: the same contraction with the count epilogue) on the same rows, in this process,
     alternating: >= 3 warm-ups each, then >= 10 timed calls each between device events.  Pass 1 (no prefix, one selector) is
     the contended one -- the keys of unit rows crowd into a few of its bins --, passes 2 and 3 run four selectors with the
     prefixes the select steps produced;
  3. times the whole roc_stream call (default rates) against the alternative it replaces -- get_euclidean, the impostor
     entries selected by a label mask, torch.sort -- with torch.cuda.max_memory_allocated above the live inputs for both.
Writes the markdown table the README quotes:
    python tools/roc_stream_bench.py --out profiles/roc_stream.md
Needs a GPU; there is no fallback."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from centroids_reid_amd import _lib as L           # noqa: E402
from centroids_reid_amd import reid_metric as rm   # noqa: E402

SHAPES = [(2228, 17661), (6250, 200_000)]
D = 2048
PASSES = ((0, 11), (11, 11), (22, 10))


def features(nq, ng, seed, dtype):
    """Clustered unit rows: ng // 24 identities, a row = its identity's centre + 0.7 N(0, 1) per element x |centre| / sqrt(D),
    normalised -- genuine pairs near squared distance 0.66, impostor pairs near 2, as a trained embedding gives them."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    n_id = max(4, ng // 24)
    centres = torch.randn((n_id, D), generator=gen, device="cuda")
    pids = torch.randint(0, n_id, (nq + ng,), generator=gen, device="cuda")
    cams = torch.randint(0, 8, (nq + ng,), generator=gen, device="cuda")
    f = centres[pids] + 0.7 * torch.randn((nq + ng, D), generator=gen, device="cuda")
    fn, sq = rm.l2_normalize(f, out_dtype=dtype, return_sqnorm=True)
    del f, centres
    junk = rm.JunkFilter(pids[:nq].contiguous(), cams[:nq].contiguous(), pids[nq:].contiguous(), cams[nq:].contiguous())
    return fn[:nq].contiguous(), fn[nq:].contiguous(), sq[:nq].contiguous(), sq[nq:].contiguous(), junk


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


def pass_prefixes(q, g, qq, gg, junk, rates):
    """The prefixes passes 2 and 3 of roc_stream run with for `rates` (at most four): the library's own select steps."""
    lib = L.lib()
    nt = len(rates)
    far_d = torch.tensor(rates, dtype=torch.float64).cuda()
    state = torch.zeros((nt, 8), dtype=torch.int64, device="cuda")
    prefix = torch.zeros(nt, dtype=torch.int32, device="cuda")
    out = [None]
    for level, (pb, bits) in enumerate(PASSES):
        h = rm.distance_histogram(q, g, junk, qq, gg, prefix=prefix if pb else None, prefix_bits=pb, bits=bits)
        L.check(lib.creid_roc_descend(L.ptr(h), nt, bits, level, L.ptr(far_d), L.ptr(state), L.ptr(prefix), L.stream()),
                "creid_roc_descend")
        if level < 2:
            out.append(prefix.clone())
    return out, h


def sort_alternative(q, g, qq, gg, junk, rates):
    """What a user does today: the matrix, the impostor entries, a full sort, the order statistics."""
    d = rm.get_euclidean(q, g, qq, gg)
    imp = d[junk.g_pids[None, :] != junk.q_pids[:, None]]
    del d
    imp = torch.sort(imp).values
    n = imp.numel()
    ks = [min(int(np.floor(np.float64(f) * np.float64(n))), n - 1) for f in rates]
    return imp[torch.tensor(ks, device=imp.device)].cpu().numpy()


def run_case(nq, ng, dtype, warmup, reps, alt_reps):
    q, g, qq, gg, junk = features(nq, ng, seed=nq, dtype=dtype)
    rates = rm.ROC_DEFAULT_FAR
    # the count launch of the streamed evaluation on the same rows
    plan = rm.StreamPlan(junk.q_pids.cpu().numpy(), junk.g_pids.cpu().numpy(), junk.q_cams.cpu().numpy(),
                         junk.g_cams.cpu().numpy(), q.device)
    if plan.cap is None:
        plan.finish()
    pl = rm._stream_poslist(q, g, qq, gg, plan)
    count = lambda: rm._stream_count(q, g, qq, gg, plan.q_pids, plan.g_pids, pl)                 # noqa: E731
    prefixes, _ = pass_prefixes(q, g, qq, gg, junk, rates + (0.1,))                            # four selectors
    outs = [torch.zeros((1 if pb == 0 else 4, 2, 1 << bits), dtype=torch.int64, device="cuda") for pb, bits in PASSES]
    hists = [(lambda i=i, pb=pb, bits=bits: rm.distance_histogram(q, g, junk, qq, gg, prefix=prefixes[i], prefix_bits=pb, bits=bits,
                                                                  out=outs[i])) for i, (pb, bits) in enumerate(PASSES)]
    whole = lambda: rm.roc_stream(q, g, junk, rates, qq, gg)                                     # noqa: E731
    got = whole()
    for _ in range(warmup):
        count()
        for h in hists:
            h()
        whole()
    t = {name: [] for name in ("count", "pass1", "pass2", "pass3", "whole")}
    for _ in range(reps):                                                   # alternating: all see the same clocks and caches
        t["count"].append(timed(count))
        for i, h in enumerate(hists):
            t[f"pass{i + 1}"].append(timed(h))
        t["whole"].append(timed(whole))
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in t.items()}
    row = {"shape": f"{nq} x {ng}", "dtype": str(dtype).replace("torch.", ""), "cap": plan.cap, **{k + "_ms": v for k, v in med.items()},
           "count_spread": spread["count"], "whole_spread": spread["whole"], "mem_whole": peak_above_inputs(whole),
           "matrix_bytes": nq * ng * 4, "tar": got["tar"], "thr": got["threshold"], "fa": got["false_accepts"],
           "n_imp": int(got["n_impostor"][0]), "n_gen": int(got["n_genuine"][0]),
           "bins1": int((got["hist"][1] > 0).sum()), "top1": float(got["hist"][1].max() / max(1, got["hist"][1].sum()))}
    del pl, outs
    try:
        alt = lambda: sort_alternative(q, g, qq, gg, junk, rates)                                # noqa: E731
        thr = alt()
        assert (thr.view(np.uint32) == got["threshold"].view(np.uint32)).all(), "roc_stream thresholds differ from the sorted matrix"
        d = rm.get_euclidean(q, g, qq, gg)
        ref = rm.roc_matrix(d, junk, rates)
        del d
        for key in ("threshold", "false_accepts", "true_accepts", "n_impostor", "n_genuine", "hist"):
            assert np.array_equal(np.asarray(ref[key]).view(np.uint8), np.asarray(got[key]).view(np.uint8)), key
        row["mem_alt"] = peak_above_inputs(alt)
        ta = [timed(alt) for _ in range(alt_reps)]
        row["alt_ms"] = float(np.median(ta))
    except torch.OutOfMemoryError:
        torch.cuda.empty_cache()
        row["mem_alt"] = row["alt_ms"] = None
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="markdown file to write (default: standard output only)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--alt-reps", type=int, default=3, help="timed calls of the matrix + sort alternative")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/roc_stream_bench.py needs a GPU")
    if a.warmup < 3 or a.reps < 10:
        sys.exit("at least 3 warm-ups and 10 timed calls per launch")
    rows = [run_case(nq, ng, dt, a.warmup, a.reps, a.alt_reps) for nq, ng in SHAPES for dt in (torch.float32, torch.bfloat16)]
    mib = lambda b: "does not fit" if b is None else f"{b / 2**20:.1f}"    # noqa: E731
    ms = lambda v: "-" if v is None else f"{v:.3f}"                         # noqa: E731
    out = ["# Open-set operating points: the histogram epilogue against the count epilogue", "",
           f"`tools/roc_stream_bench.py` on {torch.cuda.get_device_name(0)}, one process: seeded clustered unit rows (ng // 24 "
           f"identities, centre + 0.7 N(0, 1)), D = {D}; every launch alternating with the others, {a.warmup} warm-ups and "
           f"{a.reps} timed calls each between device events (medians).  count = `creid_stream_count[_h16]` of the streamed "
           "evaluation on the same rows (positive-list capacity in the table); pass 1 / 2 / 3 = `creid_stream_dist_hist[_h16]` "
           "with (prefix bits, digit bits) = (0, 11) one selector, (11, 11) and (22, 10) four selectors each, the prefixes the "
           "select steps produced for the rates 1e-4, 1e-3, 1e-2, 1e-1.  Ratios are pass / count.", "",
           "| shape | dtype | cap | count ms | spread | pass 1 ms | ratio | pass 2 ms | ratio | pass 3 ms | ratio | impostor bins of pass 1 "
           "| largest bin's share |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        c = r["count_ms"]
        out.append(f"| {r['shape']} | {r['dtype']} | {r['cap']} | {c:.3f} | {100 * r['count_spread']:.1f} % | {r['pass1_ms']:.3f} | "
                   f"{r['pass1_ms'] / c:.3f} | {r['pass2_ms']:.3f} | {r['pass2_ms'] / c:.3f} | {r['pass3_ms']:.3f} | "
                   f"{r['pass3_ms'] / c:.3f} | {r['bins1']} | {100 * r['top1']:.1f} % |")
    out += ["", "The whole call (`roc_stream`, rates 1e-4 / 1e-3 / 1e-2: three passes, three select steps, one read-back) against the "
                f"alternative it replaces (`get_euclidean`, the impostor entries by a label mask, `torch.sort`; {a.alt_reps} timed "
                "calls); peak MiB is `torch.cuda.max_memory_allocated` above the live inputs.  Before timing, the thresholds of both "
                "were asserted equal bit for bit, and `roc_stream` == `roc_matrix` on the matrix field for field.", "",
            "| shape | dtype | roc_stream ms | spread | matrix + sort ms | peak MiB roc_stream | peak MiB matrix + sort | matrix MiB | "
            "N_imp | N_gen | threshold @ 1e-4 / 1e-3 / 1e-2 | TAR | FA |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['shape']} | {r['dtype']} | {r['whole_ms']:.3f} | {100 * r['whole_spread']:.1f} % | {ms(r['alt_ms'])} | "
                   f"{mib(r['mem_whole'])} | {mib(r['mem_alt'])} | {mib(r['matrix_bytes'])} | {r['n_imp']} | {r['n_gen']} | "
                   f"{' / '.join(f'{v:.4f}' for v in r['thr'])} | {' / '.join(f'{v:.4f}' for v in r['tar'])} | "
                   f"{' / '.join(str(int(v)) for v in r['fa'])} |")
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
