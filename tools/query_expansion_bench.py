"""Query expansion on the device (reid_metric.query_expansion, csrc/neighbour_expand.hip) on seeded unit-norm clustered features
(identities of about 13 images, like Market-1501), k = 10, alpha = 3, at 2228 x 17661 x 2048 and 6250 x 200000 x 2048:
  1. the gather kernel alone (neighbour_expand on a fixed neighbour table of all N rows): median of `--reps` launches between
     device events, against its byte floor (m k + m) D 4 B / 6.3 TB/s and against the torch composition
     (w[:, :, None] * U[idx]).sum(1) in the same process (given the weights; in row chunks where the [m, k, D] temporary is large);
  2. every stage of query_expansion (its own stage clock: normalise, search, expand) for both scopes, with and without
     prefilter=bfloat16, and the whole call on the host clock around a device synchronise;
  3. the whole R1_mAP(streamed=True).compute with and without query_expansion;
  4. at a small shape, the largest |S - S_ref| / bound of tests/test_query_expansion_gpu.py's chain bound.
Writes the markdown profiles/query_expansion.md quotes:
    python tools/query_expansion_bench.py --out tables.md
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

SHAPES = [(2228, 17661, 2048), (6250, 200000, 2048)]
K, ALPHA = 10, 3.0
HBM = 6.3e12
STAGES = ["normalise", "search", "expand"]


def features(nq, ng, D, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    n = nq + ng
    ids = max(2, n // 13)
    centres = torch.randn((ids, D), generator=gen, device="cuda")
    label = torch.randint(0, ids, (n,), generator=gen, device="cuda")
    f = torch.empty((n, D), device="cuda")
    for r0 in range(0, n, 32768):                               # (bounded temporaries at the large shape)
        lab = label[r0:r0 + 32768]
        f[r0:r0 + 32768] = rm.l2_normalize(centres[lab] + 0.6 * torch.randn((len(lab), D), generator=gen, device="cuda"))
    return f, label


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def host_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def torch_composition(U, idx, w, rows):
    out = torch.empty_like(U[:idx.shape[0]])
    for r0 in range(0, idx.shape[0], rows):
        out[r0:r0 + rows] = (w[r0:r0 + rows, :, None] * U[idx[r0:r0 + rows]]).sum(1)
    return out


def kernel_section(U, lines, warmup, reps):
    N, D = U.shape
    idx, d = rm.topk_stream(U, U, K, prefilter=torch.bfloat16)
    floor = (N * K + N) * D * 4 / HBM * 1e3
    lines.append(f"| alpha | kernel ms (min .. max) | byte floor ms | floor / kernel | torch composition ms | torch / kernel |")
    lines.append("|---|---|---|---|---|---|")
    rows = max(1, (2 << 30) // (K * D * 4))                     # the [rows, k, D] temporary of the composition: 2 GiB
    for alpha in (0.0, 1.0, ALPHA):
        med, lo, hi = median_ms(lambda: rm._neighbour_expand(U, idx, d, alpha, None), warmup, reps)
        sim = (1.0 - 0.5 * d).clamp(0.0, 1.0)
        w = torch.ones_like(d) if alpha == 0 else sim if alpha == 1 else sim.double().pow(alpha).float()
        tmed, _, _ = median_ms(lambda: torch_composition(U, idx, w, rows), 1, max(2, reps // 4))
        got, ref = rm._neighbour_expand(U[:4096], idx[:4096], d[:4096], alpha, None), torch_composition(U, idx[:4096], w[:4096], rows)
        assert (got - ref).abs().max().item() < 1e-5, "kernel and composition disagree"
        lines.append(f"| {alpha:g} | {med:.3f} ({lo:.3f} .. {hi:.3f}) | {floor:.3f} | {floor / med:.2f} | {tmed:.2f} | {tmed / med:.1f}x |")
    idx9, d9 = idx[:, :K - 1].contiguous(), d[:, :K - 1].contiguous()
    med, lo, hi = median_ms(lambda: rm._neighbour_expand(U, idx9, d9, ALPHA, U), warmup, reps)
    lines.append(f"\nWith `self_rows` (k - 1 = {K - 1} neighbours and the row itself): {med:.3f} ms ({lo:.3f} .. {hi:.3f}).\n")


def stage_section(q, g, lines, warmup, reps):
    lines.append("| scope | prefilter | " + " | ".join(STAGES) + " | stages | whole call, host clock (min .. max) | fallback rows |")
    lines.append("|---|---|" + "---|" * (len(STAGES) + 3))
    for scope in ("all", "query"):
        for pf in (None, torch.bfloat16):
            kw = dict(k=K, alpha=ALPHA, scope=scope, prefilter=pf)
            first = rm.query_expansion(q, g, **kw)
            per = {s: [] for s in STAGES}
            st = {}
            for _ in range(reps):
                st = {"timing": True}
                out = rm.query_expansion(q, g, stats=st, **kw)
                assert torch.equal(out[0], first[0]) and torch.equal(out[1], first[1]), "two runs differ"
                del out
                for s in STAGES:
                    per[s].append(st["stage_ms"][0][s])
            del first
            med = {s: float(np.median(per[s])) for s in STAGES}
            whole, lo, hi = host_ms(lambda: rm.query_expansion(q, g, **kw), warmup, reps)
            lines.append(f"| {scope} | {'bf16' if pf else 'none'} | " + " | ".join(f"{med[s]:.2f}" for s in STAGES) +
                         f" | {sum(med.values()):.2f} | {whole:.2f} ({lo:.2f} .. {hi:.2f}) | {st['fallback_rows']} |")


def eval_section(X, label, nq, lines, warmup, reps):
    pids = label.cpu().numpy()
    cams = np.random.default_rng(0).integers(0, 6, len(pids))
    import contextlib
    import io
    lines.append("| R1_mAP(streamed=True) | compute ms, host clock (min .. max) | mAP |")
    lines.append("|---|---|---|")
    for name, kw in (("no expansion", {}), ("query_expansion=all", dict(query_expansion=dict(k=K, alpha=ALPHA))),
                     ("query_expansion=all, prefilter=bf16", dict(query_expansion=dict(k=K, alpha=ALPHA), prefilter=torch.bfloat16)),
                     ("query_expansion=query", dict(query_expansion=dict(k=K, alpha=ALPHA, scope="query")))):
        res = {}

        def run():
            with contextlib.redirect_stdout(io.StringIO()):
                res["r"] = rm.R1_mAP(num_query=nq, streamed=True, **kw).compute(X, pids, cams)
        med, lo, hi = host_ms(run, warmup, reps)
        lines.append(f"| {name} | {med:.2f} ({lo:.2f} .. {hi:.2f}) | {res['r'][1]:.4f} |")


def bound_section(lines):
    import qe_ref as R
    lines.append("| D | scope | max abs(S - S_ref) / bound |")
    lines.append("|---|---|---|")
    for D in (64, 2048):
        U = rm.l2_normalize(torch.from_numpy(R.clustered_unit_rows(300, D, 12, seed=D)).cuda())
        Uh = U.cpu().numpy()
        idx, d = rm.topk_stream(U, U, K)
        ref, B = R.expand(Uh, idx.cpu().numpy(), d.cpu().numpy(), ALPHA)
        got = rm.neighbour_expand(U, idx, d, ALPHA).cpu().numpy().astype(np.float64)
        lines.append(f"| {D} | all | {(np.abs(got - ref) / ((K + 2) * 2.0 ** -24 * B)).max():.3f} |")
        Uq, Ug = U[:60].contiguous(), U[60:].contiguous()
        idx, d = rm.topk_stream(Uq, Ug, K - 1)
        ref, B = R.expand(Uh[60:], idx.cpu().numpy(), d.cpu().numpy(), ALPHA, self_rows=Uh[:60])
        got = rm.neighbour_expand(Ug, idx, d, ALPHA, self_rows=Uq).cpu().numpy().astype(np.float64)
        lines.append(f"| {D} | query | {(np.abs(got - ref) / ((K + 2) * 2.0 ** -24 * B)).max():.3f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="0,1", help="indices into SHAPES")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    lines = [f"Device: {torch.cuda.get_device_name(0)}; k = {K}, alpha = {ALPHA:g}; medians of {args.reps} after {args.warmup} warm-up calls.\n"]
    for si in (int(v) for v in args.shapes.split(",")):
        nq, ng, D = SHAPES[si]
        reps = args.reps if (nq + ng) < 100000 else max(3, args.reps // 3)
        X, label = features(nq, ng, D, seed=nq)
        lines.append(f"## {nq} x {ng} x {D} (N = {nq + ng}, rows {(nq + ng) * D * 4 / 2 ** 20:.0f} MiB)\n")
        lines.append("### The gather kernel alone\n")
        kernel_section(X, lines, args.warmup, reps)
        lines.append("### query_expansion, per stage (ms between device events)\n")
        stage_section(X[:nq].contiguous(), X[nq:].contiguous(), lines, args.warmup, reps)
        lines.append("\n### R1_mAP.compute\n")
        eval_section(X, label, nq, lines, args.warmup, reps)
        lines.append("")
        del X
        torch.cuda.empty_cache()
        print(f"done: {nq} x {ng} x {D}", flush=True)
        if args.out:                                            # (a partial file is better than none if a later shape fails)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    lines.append("## Chain bound at 300 rows\n")
    bound_section(lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
