"""The 16-bit streamed paths (csrc/stream_h16.hip: bf16 / f16 features on the 16-bit MFMA) against the existing paths, on seeded
unit-norm random features, D = 2048, at 2228 x 17661 and 6250 x 200 000:
  top-k (k = 50)   materialised fp32 | streamed fp32 | materialised 16-bit | streamed 16-bit, per dtype; peak memory above the live
                   inputs; fallback_rows / max_candidates of the streamed calls;
  evaluation       R1_mAP(streamed=True) fp32 | R1_mAP(compute_dtype=dt) materialised | R1_mAP(compute_dtype=dt, streamed=True).
Equality (streamed == materialised of the same dtype: indices and distance bits; CMC / mAP) is asserted first.  The paths of a
table are alternated in one process: >= 3 warm-ups, then >= 20 timed calls each between device events; medians and the
run-to-run spread (max - min) / median are reported.
    python tools/stream_h16_bench.py --out profiles/stream_h16.md
The kernel breakdown comes from a run of its own under the profiler, one per shape (the program after `--`):
    rocprofv3 --kernel-trace --stats -d DIR_A -o t -- python tools/stream_h16_bench.py --trace-run 0
    rocprofv3 --kernel-trace --stats -d DIR_B -o t -- python tools/stream_h16_bench.py --trace-run 1
    python tools/stream_h16_bench.py --out profiles/stream_h16.md --kernels DB_A DB_B        (timing tables + kernel table)
Needs a GPU; there is no fallback."""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from centroids_reid_amd import reid_metric as rm   # noqa: E402

SHAPES = [(2228, 17661), (6250, 200_000)]
D, K = 2048, 50
DTYPES = [(torch.bfloat16, "bf16"), (torch.float16, "f16")]
PEAK_16 = 2.5e15                                   # dense bf16 / f16 MFMA peak of the MI355X, FLOP/s
PEAK_F32 = PEAK_16 / 16                            # the f32 MFMA peak
TRACE_REPS = 5


def raw_features(nq, ng, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((nq + ng, D), generator=gen, device="cuda", dtype=torch.float32)


def labels(nq, ng, seed):
    """2228 x 17661: the DukeMTMC-like label statistics of the evaluation benchmark (702 identities, 8 cameras); 6250 x 200 000:
    the per-rank shard of the large configuration (every query has 4 gallery matches in another camera)."""
    rng = np.random.default_rng(seed)
    if ng < 100_000:
        return rng.integers(0, 702, nq + ng), rng.integers(0, 8, nq + ng)
    pids = np.concatenate([rng.integers(0, 50_000, nq), np.arange(ng) % 50_000])
    cams = np.concatenate([np.zeros(nq, np.int64), np.ones(ng, np.int64)])
    return pids, cams


def split(f, nq, dt):
    fn, sq = rm.l2_normalize(f, out_dtype=dt, return_sqnorm=True)
    q, g = fn[:nq].contiguous(), fn[nq:].contiguous()
    return q, g, rm.row_sqnorm(q), rm.row_sqnorm(g)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    with contextlib.redirect_stdout(io.StringIO()):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    live = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with contextlib.redirect_stdout(io.StringIO()):
        out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - live
    del out
    return peak


def alternate(paths, warmup, reps):
    """paths: {name: callable}.  Returns {name: (median ms, min, max, spread)} with the calls of all paths interleaved."""
    for _ in range(warmup):
        for fn in paths.values():
            timed(fn)
    t = {k: [] for k in paths}
    for _ in range(reps):
        for k, fn in paths.items():
            t[k].append(timed(fn))
    out = {}
    for k, v in t.items():
        v = np.asarray(v)
        med = float(np.median(v))
        out[k] = (med, float(v.min()), float(v.max()), float((v.max() - v.min()) / med))
    return out


def topk_rows_of(f, nq, ng, warmup, reps):
    paths, info, mem = {}, {}, {}
    q32, g32, qq32, gg32 = split(f, nq, torch.float32)
    paths["materialised fp32"] = lambda: rm.topk_rows(rm.get_euclidean(q32, g32, qq32, gg32), K)
    info["streamed fp32"] = {}
    paths["streamed fp32"] = lambda: rm.topk_stream(q32, g32, K, qq32, gg32, stats=info["streamed fp32"])
    keep = [(q32, g32, qq32, gg32)]
    for dt, name in DTYPES:
        q, g, qq, gg = split(f, nq, dt)
        keep.append((q, g, qq, gg))
        info[f"streamed {name}"] = {}
        paths[f"materialised {name}"] = (lambda q=q, g=g, qq=qq, gg=gg: rm.topk_rows(rm.get_euclidean(q, g, qq, gg), K))
        paths[f"streamed {name}"] = (lambda q=q, g=g, qq=qq, gg=gg, s=info[f"streamed {name}"]:
                                     rm.topk_stream(q, g, K, qq, gg, stats=s))
    for name in ("fp32", "bf16", "f16"):                                   # equality first
        ref, got = paths[f"materialised {name}"](), paths[f"streamed {name}"]()
        assert torch.equal(got[0], ref[0]), f"{name}: streamed indices differ from the materialised path"
        assert torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32)), f"{name}: streamed distance bits differ"
        del ref, got
    for k, fn in paths.items():
        mem[k] = peak_above_inputs(fn)
    t = alternate(paths, warmup, reps)
    return [{"path": k, "t": t[k], "mem": mem[k], **{x: info.get(k, {}).get(x, "") for x in ("fallback_rows", "max_candidates")}}
            for k in paths]


def eval_rows_of(f, nq, ng, warmup, reps):
    pids, cams = labels(nq, ng, nq)
    paths = {"streamed fp32": lambda: rm.R1_mAP(num_query=nq, streamed=True).compute(f, pids, cams)}
    for dt, name in DTYPES:
        paths[f"materialised {name}"] = lambda dt=dt: rm.R1_mAP(num_query=nq, compute_dtype=dt).compute(f, pids, cams)
        paths[f"streamed {name}"] = lambda dt=dt: rm.R1_mAP(num_query=nq, compute_dtype=dt, streamed=True).compute(f, pids, cams)
    with contextlib.redirect_stdout(io.StringIO()):
        for _, name in DTYPES:                                             # equality first
            ref, got = paths[f"materialised {name}"](), paths[f"streamed {name}"]()
            assert np.array_equal(ref[0], got[0]) and abs(ref[1] - got[1]) < 1e-12 and np.array_equal(ref[2], got[2]), name
    t = alternate(paths, warmup, reps)
    return [{"path": k, "t": t[k]} for k in paths]


def trace_run(shape_index):
    """The workload of the profiler pass: the three streamed evaluations of one shape, TRACE_REPS times each after one warm-up."""
    nq, ng = SHAPES[shape_index]
    f = raw_features(nq, ng, nq)
    pids, cams = labels(nq, ng, nq)
    with contextlib.redirect_stdout(io.StringIO()):
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            for _ in range(1 + TRACE_REPS):
                rm.R1_mAP(num_query=nq, compute_dtype=dt, streamed=True).compute(f, pids, cams)
    torch.cuda.synchronize()


def kernel_table(dbs):
    import sqlite3
    out = ["", "## Kernel breakdown", "",
           "`rocprofv3 --kernel-trace --stats` over `--trace-run` (a run of its own per shape: the three streamed evaluations, "
           f"{TRACE_REPS} calls each after a warm-up); median duration per launch.  FLOP = 2 m n D; operand bytes = what the "
           "workgroups request from L2 / the Infinity Cache: per 64 x 256 tile and 64-deep k-tile (64 + 256) rows x 64 elements.  "
           "Peak = 2.5 PFLOP/s for the 16-bit MFMA, 1/16 of it for the f32 MFMA.", "",
           "| shape | kernel | launches | median ms | min .. max ms | TFLOP/s | of its MFMA peak | of the 16-bit peak | operand TB/s |",
           "|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for (nq, ng), db in zip(SHAPES, dbs):
        rows = sqlite3.connect(db).execute("select name, end - start from kernels order by start").fetchall()
        by = {}
        for name, ns in rows:
            by.setdefault(name, []).append(ns / 1e6)
        flop = 2.0 * nq * ng * D
        stats = {}
        for name, v in sorted(by.items()):
            short = name.split("(")[0]
            if "sqdist_count_f32_kernel" in name:
                label, esz, peak = "sqdist_count_f32_kernel (fp32)", 4, PEAK_F32
            elif "sqdist_stream_h16_kernel" in name:
                label, esz, peak = short, 2, PEAK_16
            elif "stream_poslist" in name:
                label, esz, peak = short, 0, 0
            else:
                continue
            v = np.asarray(v[1:] if len(v) > 1 else v)                     # in launch order: the first is the warm-up
            med = float(np.median(v))
            if esz:
                tiles = -(-nq // 64) * -(-ng // 256) * -(-D // 64)
                ob = tiles * (64 + 256) * 64 * esz
                rate = flop / (med * 1e-3)
                out.append(f"| {nq} x {ng} | `{label}` | {len(v)} | {med:.3f} | {v.min():.3f} .. {v.max():.3f} | {rate / 1e12:.1f} | "
                           f"{rate / peak:.3f} | {rate / PEAK_16:.3f} | {ob / (med * 1e-3) / 1e12:.2f} |")
                stats[label] = (med, float(v.max() - v.min()))
            else:
                out.append(f"| {nq} x {ng} | `{label}` | {len(v)} | {med:.3f} | {v.min():.3f} .. {v.max():.3f} | | | | |")
        f32 = stats.get("sqdist_count_f32_kernel (fp32)")
        for label, (med, _) in stats.items():
            if f32 and "h16" in label:
                ok = med < f32[0] - f32[1]
                verdicts.append(f"{nq} x {ng}: `{label}` {med:.3f} ms against the fp32 kernel's {f32[0]:.3f} ms (its spread "
                                f"{f32[1]:.3f} ms): {'meets' if ok else 'MISSES'} the bar.")
    out += ["", "Acceptance (the 16-bit streamed contraction faster than the fp32 one by more than the latter's run-to-run spread):", ""]
    out += [f"* {v}" for v in verdicts]
    return out


def fmt(t):
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f}) | {100 * t[3]:.1f} %"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="markdown file to write (default: standard output only)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace-run", type=int, default=None, metavar="SHAPE", help="profiler workload for shape 0 or 1 only")
    ap.add_argument("--kernels", nargs=2, default=None, metavar="DB", help="rocprofv3 databases of --trace-run 0 and 1")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/stream_h16_bench.py needs a GPU")
    if a.trace_run is not None:
        return trace_run(a.trace_run)
    if a.warmup < 3 or a.reps < 20:
        sys.exit("at least 3 warm-ups and 20 timed calls per path")
    mib = lambda b: f"{b / 2**20:.0f}"                                      # noqa: E731
    out = ["# The 16-bit streamed paths against the existing ones", "",
           f"`tools/stream_h16_bench.py` on {torch.cuda.get_device_name(0)}: seeded unit-norm random features, D = {D}; the paths of "
           f"a table alternated in one process, {a.warmup} warm-ups and {a.reps} timed calls each between device events (medians; "
           "min .. max in brackets; spread = (max - min) / median).  Before timing, streamed == materialised of the same dtype "
           "was asserted (top-k: indices and distance bits; evaluation: CMC, top-k, mAP within 1e-12).", ""]
    verdicts = []
    for nq, ng in SHAPES:
        f = raw_features(nq, ng, nq)
        out += [f"## {nq} x {ng}", "", f"Top-k retrieval, k = {K} (`get_euclidean` + `topk_rows` against `topk_stream` at its defaults; "
                f"the fp32 matrix would be {mib(nq * ng * 4)} MiB):", "",
                "| path | ms | spread | peak MiB above the inputs | fallback_rows | max_candidates |", "|---|---|---|---|---|---|"]
        for r in topk_rows_of(f, nq, ng, a.warmup, a.reps):
            out.append(f"| {r['path']} | {fmt(r['t'])} | {mib(r['mem'])} | {r['fallback_rows']} | {r['max_candidates']} |")
        torch.cuda.empty_cache()
        out += ["", "Evaluation (`R1_mAP(...).compute(device features, host labels)` -> host CMC / mAP; normalisation included):", "",
                "| path | ms | spread |", "|---|---|---|"]
        rows = eval_rows_of(f, nq, ng, a.warmup, a.reps)
        for r in rows:
            out.append(f"| {r['path']} | {fmt(r['t'])} |")
        out.append("")
        if (nq, ng) == SHAPES[0]:
            t = {r["path"]: r["t"] for r in rows}
            for _, name in DTYPES:
                s, m_ = t[f"streamed {name}"], t[f"materialised {name}"]
                ok = s[0] <= m_[0] * (1.0 + m_[3])
                verdicts.append(f"{nq} x {ng}, {name}: streamed evaluation {s[0]:.3f} ms against materialised {m_[0]:.3f} ms "
                                f"(spread {100 * m_[3]:.1f} %): {'meets' if ok else 'MISSES'} the bar.")
        del f
        torch.cuda.empty_cache()
    out += ["Acceptance (the 16-bit streamed evaluation not slower than the 16-bit materialised one by more than the latter's spread):", ""]
    out += [f"* {v}" for v in verdicts]
    if a.kernels:
        out += kernel_table(a.kernels)
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f_:
            f_.write(text)


if __name__ == "__main__":
    main()
