"""Ranked lists under the evaluation protocol (reid_metric.topk_stream(junk=...): the first k non-junk gallery entries per query,
no m x n matrix) on seeded clustered unit-norm features, D = 2048, k = 10 and 50, at 2228 x 17661 and 6250 x 200 000, with plain
camera ids and with camera sets:
  1. asserts topk_stream(junk=...) == get_euclidean + rank_rows + rank_keep_topk (indices, padding, distance bits);
  2. times, in this process and alternating, the plain topk_stream, topk_stream(junk=...) and the materialised route: whole
     calls between device events, medians of `--reps` calls after `--warmup` warm-ups;
  3. reports torch.cuda.max_memory_allocated above the live inputs for each.
--gate-lib PATH (another build of libcreid_hip.so, for instance the parent commit's): additionally times the plain topk_stream
(k = 50) and the streamed count (stream_eval: positives, contraction, finalize) with this build and with that one, in fresh
child processes that alternate, and reports the ratio of the medians: the existing kernels must not have changed.
Writes the markdown the README quotes:
    python tools/ranked_lists_bench.py --out profiles/ranked_lists.md [--gate-lib other/libcreid_hip.so]
Needs a GPU; there is no fallback."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from centroids_reid_amd import _lib as L             # noqa: E402
from centroids_reid_amd import reid_metric as rm    # noqa: E402

SHAPES = [(2228, 17661), (6250, 200_000)]
D, KS = 2048, (10, 50)


def case(nq, ng, seed):
    """Identities of about 13 gallery rows (centre + 0.6 N(0, 1) per element, then unit norm); every query's identity is in the
    gallery; cameras 0..5, camera-set masks 1..63."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    n_id = max(4, ng // 13)
    centres = torch.randn((n_id, D), generator=gen, device="cuda")
    pids = torch.cat([torch.randint(0, n_id, (nq,), generator=gen, device="cuda"),
                      torch.randint(0, n_id, (ng,), generator=gen, device="cuda")])
    f = centres[pids] + 0.6 * torch.randn((nq + ng, D), generator=gen, device="cuda")
    del centres
    fn, sq = rm.l2_normalize(f, return_sqnorm=True)
    del f
    cams = torch.randint(0, 6, (nq + ng,), generator=gen, device="cuda")
    masks = torch.randint(1, 64, (ng,), generator=gen, device="cuda")
    return fn[:nq].contiguous(), fn[nq:].contiguous(), sq[:nq].contiguous(), sq[nq:].contiguous(), pids, cams, masks


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


def med(ts):
    ts = np.asarray(ts)
    return f"{np.median(ts):.2f} ({ts.min():.2f} .. {ts.max():.2f})"


def run_shape(nq, ng, warmup, reps):
    q, g, qq, gg, pids, cams, masks = case(nq, ng, seed=nq)
    rows = []
    for camsets in (False, True):
        junk = rm.JunkFilter(pids[:nq], cams[:nq], pids[nq:], masks if camsets else cams[nq:], camsets=camsets)
        for k in KS:
            stats = {}
            plain = lambda: rm.topk_stream(q, g, k, qq, gg)                                    # noqa: E731
            keep = lambda: rm.topk_stream(q, g, k, qq, gg, junk=junk, stats=stats)             # noqa: E731

            def mat():
                d = rm.get_euclidean(q, g, qq, gg)
                idx = rm.rank_keep_topk(rm.rank_rows(d), k, junk)[0]
                return idx, rm.gather_ranked(d, idx)
            ref, got, unfiltered = mat(), keep(), plain()
            assert torch.equal(got[0], ref[0]), "streamed lists differ from the materialised route"
            assert torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32)), "streamed distance bits differ"
            differ = int((got[0] != unfiltered[0]).any(1).sum())
            del ref, got, unfiltered
            first = dict(stats)
            mem = [peak_above_inputs(f) for f in (plain, keep, mat)]
            for _ in range(warmup):
                plain(); keep(); mat()
            ts = [[], [], []]
            for _ in range(reps):                                       # alternating: all see the same clocks and caches
                for t, f in zip(ts, (plain, keep, mat)):
                    t.append(timed(f))
            m = [float(np.median(t)) for t in ts]
            rows.append(f"| {nq} x {ng} | {'sets' if camsets else 'ids'} | {k} | {med(ts[0])} | {med(ts[1])} | {m[1] / m[0]:.3f} | "
                        f"{med(ts[2])} | {m[1] / m[2]:.3f} | {mem[0] / 2**20:.0f} | {mem[1] / 2**20:.0f} | {mem[2] / 2**20:.0f} | "
                        f"{differ} | {first['fallback_rows']} | {first['max_candidates']} |")
            print(rows[-1], flush=True)
    return rows


# ---------------------------------------------------------------------------------------------- the gate: two builds, alternating
def gate_child(reps):
    """One build (CREID_LIB_PATH), both shapes: medians of the plain topk_stream (k = 50) and of stream_eval, as JSON."""
    have = ctypes.CDLL(L.LIB_PATH)
    for name in [n for n in L.SIGNATURES if not hasattr(have, n)]:     # an older build lacks the newer entry points
        del L.SIGNATURES[name]
    out = {}
    for nq, ng in SHAPES:
        q, g, qq, gg, pids, cams, _ = case(nq, ng, seed=nq)
        plan = rm.StreamPlan.on_device(pids.cpu().numpy(), cams.cpu().numpy(), nq, q.device).finish()
        topk = lambda: rm.topk_stream(q, g, 50, qq, gg)                 # noqa: E731
        count = lambda: rm.stream_eval(q, g, qq, gg, plan)              # noqa: E731
        for _ in range(3):
            topk(); count()
        tt, tc = [], []
        for _ in range(reps):
            tt.append(timed(topk)); tc.append(timed(count))
        out[f"{nq} x {ng}"] = {"topk_stream": float(np.median(tt)), "stream_eval": float(np.median(tc))}
        del q, g, qq, gg, plan
    print("GATE " + json.dumps(out), flush=True)


def gate(other, rounds, reps):
    libs = {"this build": L.LIB_PATH, "other build": os.path.abspath(other)}
    res = {name: [] for name in libs}
    for _ in range(rounds):
        for name, path in libs.items():                                 # fresh processes, alternating
            env = dict(os.environ, CREID_LIB_PATH=path)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--gate-child", "--reps", str(reps)], env=env,
                               capture_output=True, text=True, timeout=900)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("GATE ")]
            if r.returncode != 0 or not line:
                sys.exit(f"gate child failed ({name}):\n{r.stdout}\n{r.stderr}")
            res[name].append(json.loads(line[0][5:]))
            print(name, line[0], flush=True)
    rows = []
    for shape in res["this build"][0]:
        for what in ("topk_stream", "stream_eval"):
            a = [r[shape][what] for r in res["this build"]]
            b = [r[shape][what] for r in res["other build"]]
            ma, mb = float(np.median(a)), float(np.median(b))
            rows.append(f"| {shape} | {what} | {ma:.3f} ({min(a):.3f} .. {max(a):.3f}) | {mb:.3f} ({min(b):.3f} .. {max(b):.3f}) | "
                        f"{ma / mb:.4f} |")
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="markdown file to write (default: standard output only)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--gate-lib", default=None, help="another build of libcreid_hip.so to time the existing paths against")
    ap.add_argument("--gate-rounds", type=int, default=3)
    ap.add_argument("--gate-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/ranked_lists_bench.py needs a GPU")
    if a.gate_child:
        return gate_child(a.reps)
    rows = []
    for nq, ng in SHAPES:
        rows += run_shape(nq, ng, a.warmup, a.reps if nq * ng < 10**8 else max(3, a.reps // 3))
    out = ["# Ranked lists under the evaluation protocol: junk-free top-k, matrix-free", "",
           f"`python tools/ranked_lists_bench.py` on {torch.cuda.get_device_name(0)}, one box, one session: seeded clustered unit-norm "
           f"features (identities of about 13 rows, noise 0.6 per element before normalisation), D = {D}; cameras 0..5, camera-set "
           f"masks 1..63.  Whole calls between device events, the three routes alternating in one process; medians (min .. max) of "
           f"{a.reps} calls after {a.warmup} warm-ups ({max(3, a.reps // 3)} calls at 6250 x 200000).  plain = `topk_stream` (blind to "
           "labels); junk-free = `topk_stream(junk=...)`; materialised = `get_euclidean` + `rank_rows` + `rank_keep_topk` + gather.  "
           "Before timing, junk-free == materialised was asserted (indices, padding, distance bits).  Peak MiB is "
           "`torch.cuda.max_memory_allocated` above the live inputs.  `rows that differ`: queries whose junk-free list is not "
           "their plain list.", "",
           "| shape | cameras | k | plain ms | junk-free ms | junk-free / plain | materialised ms | junk-free / materialised | "
           "peak MiB plain | peak MiB junk-free | peak MiB materialised | rows that differ | fallback_rows | max_candidates |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"] + rows
    if a.gate_lib:
        out += ["", "## The existing paths against the other build", "",
                f"`--gate-lib`: {a.gate_rounds} fresh processes per build, alternating; in each, medians of {a.reps} calls between "
                "device events after 3 warm-ups; below, the median (min .. max) of the processes' medians.", "",
                "| shape | call | this build ms | other build ms | this / other |", "|---|---|---|---|---|"]
        out += gate(a.gate_lib, a.gate_rounds, a.reps)
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
