#!/usr/bin/env python
"""bench.py -- hot-path benchmark (contract: see the task statement / DESIGN.md "Measurement").

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload train|eval] [--full] [--dump-outputs DIR]

One "step" is one pass of the hot path over one batch of synthetic input already resident in HBM:
  train: one CTLModel.training_step (ResNet50 256x128 bf16, P=16 x K=4 = 64 images, all four
         losses, backward, Adam + center-SGD) -> metric train_images_per_sec  (BASELINE configs[1])
  eval : normalise + squared-L2 matrix + rank + CMC/mAP over 2228 x 17661 x 2048 fp32
         (DukeMTMC-shaped, BASELINE configs[4]) -> metric eval_dist_pairs_per_sec
Rank 0 prints ONE JSON line.  For N>1 launch with torch.distributed.run (one rank per GPU, RCCL).

A plain run sets up, warms up, times the K steps and prints the headline.  --full adds everything else the line used to
carry: per-kernel and in-situ rooflines, counter passes, CPU baselines, the other precisions, batch sizes and shapes, the
evaluation legs of a training run, the stock torch-ROCm yardstick.  --dump-outputs DIR writes what the timed path computed
in its last step as DIR/<name>.npy (float32 / float64; the inputs are seeded, so two builds compare output for output).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PMC_FILES = ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json")   # newest committed counter passes first (eval kernels only: the training families are measured live)
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_F32_TFLOPS = 157.3        # f32-input MFMA dense peak
MFMA_BF16_TFLOPS = 2500.0      # bf16 MFMA dense peak


def ddp_setup(n_gpus):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    force = os.environ.get("CREID_FORCE_DIST", "0") == "1"          # one-rank RCCL group: exercises the data-parallel path on one GPU
    if world > 1 or force:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if force and world == 1:
            os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        backend = os.environ.get("CREID_DIST_BACKEND", "nccl")      # "gloo" + CREID_SINGLE_DEVICE=1: control-flow
        if os.environ.get("CREID_SINGLE_DEVICE", "0") == "1":        # test of the N>1 path on a one-GPU box
            local = 0
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    else:
        torch.cuda.set_device(0)
    assert world == n_gpus, f"--gpus {n_gpus} but WORLD_SIZE={world}"
    return rank, world


def barrier_sync(world):
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()


def time_kernel(fn, iters, graph=True):
    """Average device time (ms) of fn() measured with HIP events on the launch stream.  With graph=True the
    `iters` launches are captured into one hipGraph first and the replay is timed: a Python/ctypes launch costs
    ~10 us of host time, so for kernels shorter than that an eager loop would time the host, not the kernel."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if graph:
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()                                   # allocations settle before capture
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):   # see bench_train.CAPTURE_MODE
                for _ in range(iters):
                    fn()
        torch.cuda.current_stream().wait_stream(side)
        g.replay()
        torch.cuda.synchronize()
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


# ----------------------------------------------------------------------------- eval workload
def eval_inputs(nq, ng, D, rank, world):
    gen = torch.Generator(device="cuda").manual_seed(0)
    feats = torch.randn((nq + ng, D), generator=gen, device="cuda", dtype=torch.float32)
    rng = np.random.default_rng(0)
    pids = rng.integers(0, 702, nq + ng)
    cams = rng.integers(0, 8, nq + ng)
    return feats, pids, cams


def pmc_traffic(key):
    """HBM-side bytes per launch from the committed rocprofv3 --pmc passes (profiles/r0x_pmc_traffic.json, falling back
    to the round-1 file: FETCH_SIZE + WRITE_SIZE collected in separate counter-only runs); None if absent."""
    here = os.path.dirname(os.path.abspath(__file__))
    for name in PMC_FILES:
        try:
            with open(os.path.join(here, "profiles", name)) as f:
                e = json.load(f)[key]
            return (e["fetch_bytes"] + e["write_bytes"]) / e["launches"]
        except (OSError, KeyError, ValueError):
            continue
    return None


def pmc_field(key, field):
    """A per-kernel field of the committed counter passes (profiles/r0x_pmc_traffic.json), e.g. "mfma_busy"."""
    for name in PMC_FILES:                                  # newest pass that has the kernel AND the field
        try:
            with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", name)) as f:
                return json.load(f)[key][field]
        except (OSError, KeyError, ValueError):
            continue
    return None


def inner_eval_trace():
    """Child of pmc_eval_insitu: the two fp32 contraction kernels of the evaluation on the configs[4] shape, a few launches each."""
    import torch
    from centroids_reid_amd import reid_metric as rm
    nq, ng, D = 2228, 17661, 2048
    feats, pids, cams = eval_inputs(nq, ng, D, 0, 1)
    plan = rm.StreamPlan.on_device(pids, cams, nq, "cuda").finish()
    fn, sq = rm.l2_normalize(feats, return_sqnorm=True)
    q, g = fn[:nq], fn[nq:]
    qq, gg = sq[:nq].contiguous(), sq[nq:].contiguous()
    L = rm.L
    lib = L.lib()
    cap = plan.cap
    pos_key = torch.empty((nq, cap), dtype=torch.int32, device="cuda"); pos_idx = torch.empty_like(pos_key)
    npos = torch.empty(nq, dtype=torch.int32, device="cuda"); hist = torch.zeros((nq, cap), dtype=torch.int32, device="cuda")
    L.check(lib.creid_stream_poslist(L.ptr(q), L.ptr(g), L.ptr(qq), L.ptr(gg), nq, ng, D, L.ptr(plan.q_slot), L.ptr(plan.csr_off),
                                     L.ptr(plan.g_order), L.ptr(plan.q_cams), L.ptr(plan.g_cams), cap, L.ptr(pos_key), L.ptr(pos_idx),
                                     L.ptr(npos), L.stream()), "poslist")
    for _ in range(4):
        L.check(lib.creid_stream_count(L.ptr(q), L.ptr(g), L.ptr(qq), L.ptr(gg), nq, ng, D, L.ptr(plan.q_pids), L.ptr(plan.g_pids),
                                       cap, L.ptr(pos_key), L.ptr(pos_idx), L.ptr(npos), L.ptr(hist), L.stream()), "count")
        rm.get_euclidean(q, g, qq, gg)
    torch.cuda.synchronize()


def pmc_eval_insitu(timeout_s=75):
    """HBM-side traffic and matrix-pipe occupancy of sqdist_count_f32_kernel / sqdist_f32_kernel measured in THIS run: three
    `rocprofv3 --kernel-trace --pmc` child runs of `bench.py --inner-eval-trace` (FETCH_SIZE, WRITE_SIZE, SQ_VALU_MFMA_BUSY_CYCLES
    + GRBM_GUI_ACTIVE, each in a pass of its own; counters only).  Per kernel and LAUNCH (first launch dropped): fetch_bytes =
    2 x FETCH_SIZE KiB (gfx950: the counter tallies 128-byte requests at 64), write_bytes = WRITE_SIZE KiB, mfma_busy = busy
    cycles / (GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs).  None when rocprofv3 or a pass is unavailable."""
    import glob
    import shutil
    import sqlite3
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe) or os.environ.get("CREID_BENCH_NO_PMC", "0") == "1" or os.environ.get("CREID_BENCH_PMC_FAILED") == "1":
        return None
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, TMPDIR="/tmp")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "CREID_FORCE_DIST"):
        env.pop(k, None)

    def one_pass(counters):
        tmp = tempfile.mkdtemp(prefix="creid_pmc_ev_", dir="/tmp")
        try:
            cmd = [exe, "--kernel-trace", "--pmc", *counters, "-d", tmp, "-o", "pmc", "--", sys.executable,
                   os.path.join(here, "bench.py"), "--inner-eval-trace"]
            r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout_s)
            dbs = glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True)
            if r.returncode != 0 or not dbs:
                print(f"[bench] eval counter pass {counters} failed (rc {r.returncode}): {r.stderr[-300:]}", file=sys.stderr)
                return None
            cur = sqlite3.connect(dbs[0]).cursor()
            rows = cur.execute("select kernel_name, counter_name, value, dispatch_id, start from counters_collection").fetchall()
            disp = {}
            for kn, cn, v, did, st in rows:
                d = disp.setdefault(did, {"name": kn, "start": st})
                d[cn] = d.get(cn, 0.0) + float(v)
            out = {}
            for key in ("sqdist_count_f32_kernel", "sqdist_f32_kernel"):
                ds = sorted((d for d in disp.values() if key in d["name"]), key=lambda d: d["start"])[1:]
                if ds:
                    out[key] = {c: sum(d.get(c, 0.0) for d in ds) / len(ds) for c in counters}
            return out or None
        except Exception as e:  # noqa: BLE001
            print(f"[bench] eval counter pass {counters} unavailable ({type(e).__name__}: {e})", file=sys.stderr)
            return None
        finally:
            shutil.rmtree(tmp, ignore_errors=True)

    F = one_pass(["FETCH_SIZE"])
    Wr = one_pass(["WRITE_SIZE"]) if F else None
    S = one_pass(["SQ_VALU_MFMA_BUSY_CYCLES", "GRBM_GUI_ACTIVE"]) if Wr else None
    if not (F and Wr):
        return None
    out = {}
    for key in F:
        e = {"fetch_bytes": 2.0 * F[key]["FETCH_SIZE"] * 1024.0, "write_bytes": Wr.get(key, {}).get("WRITE_SIZE", 0.0) * 1024.0}
        if S and key in S and S[key].get("GRBM_GUI_ACTIVE"):
            e["mfma_busy"] = S[key]["SQ_VALU_MFMA_BUSY_CYCLES"] / (S[key]["GRBM_GUI_ACTIVE"] / 8.0 * 1024.0)
        out[key] = e
    return out


def run_eval(args, rank, world, steps=None, warmup=None, shape=None, extras=True, full=True, outputs=None):
    """BASELINE configs[4]: normalise + squared-L2 + rank + CMC/mAP over 2228 x 17661 x 2048 fp32.  Timed twice:
    the METRIC-ONLY path the validation hook uses (streamed: the m x n matrix is never written; `value`) and the
    materialised path (distance matrix + int64 ranked indices, what get_similar / the rank-index goldens need).
    full=False: the streamed path alone (no materialised run, first-call timing or per-kernel figures).  `outputs` (a dict,
    rank 0): filled with the last timed step's (cmc, mAP, topk)."""
    from centroids_reid_amd import reid_metric as rm
    from centroids_reid_amd import parallel as par
    steps = steps or args.steps
    warmup = args.warmup if warmup is None else warmup
    nq, ng, D = shape or (2228, 17661, 2048)
    feats, pids, cams = eval_inputs(nq, ng, D, rank, world)
    # weak scaling: every rank ranks its own nq queries against the (all-gathered) gallery
    q_pids = torch.as_tensor(pids[:nq], device="cuda"); g_pids = torch.as_tensor(pids[nq:], device="cuda")
    q_cams = torch.as_tensor(cams[:nq], device="cuda"); g_cams = torch.as_tensor(cams[nq:], device="cuda")
    plan = rm.StreamPlan.on_device(pids, cams, nq, "cuda").finish()               # for the per-kernel timings below
    metric = rm.R1_mAP(num_query=nq, streamed=True)
    glo, ghi = par.shard_bounds(ng, rank, world)
    gal_shard = feats[nq + glo:nq + ghi].contiguous() if world > 1 else None
    gcounts = [par.shard_bounds(ng, r, world)[1] - par.shard_bounds(ng, r, world)[0] for r in range(world)]

    def gathered():
        if world > 1:  # node-level all-gather of (gallery) embeddings before the distance stage
            return torch.cat([feats[:nq], par.all_gather_rows(gal_shard, gcounts)])
        return feats

    def step_streamed():
        # END TO END: exactly what get_val_metrics calls (modelling/bases.py:264-297 -> utils/reid_metric.py:112-151): host label
        # vectors in, (cmc, mAP, topk) on the host out -- label upload, device index build, normalise, positives, streamed
        # contraction + count, finalize, means, read-back, every host synchronisation included
        cmc, m_ap, topk = metric.compute(gathered(), pids, cams)
        return cmc, torch.tensor([m_ap], dtype=torch.float64), topk

    def step_materialised():
        fn, sq = rm.l2_normalize(gathered(), return_sqnorm=True)
        d = rm.get_euclidean(fn[:nq], fn[nq:], sq[:nq].contiguous(), sq[nq:].contiguous())
        idx, valid, ap, first = rm.rank_rows_eval(d, q_pids, g_pids, q_cams, g_cams)     # ranked indices + per-query results, one pass
        return rm.eval_reduce_device(valid, ap, first, 50)

    def timed(step):
        for _ in range(warmup):
            out = step()
        barrier_sync(world)
        t0 = time.perf_counter()
        for _ in range(steps):
            out = step()
        barrier_sync(world)
        dt = time.perf_counter() - t0
        tmax = torch.tensor([dt], device="cuda", dtype=torch.float64)
        if world > 1:
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        return float(tmax.item()), out

    _quiet = open(os.devnull, "w")
    _so, sys.stdout = sys.stdout, _quiet                   # R1_mAP.compute mirrors the reference's banner print per call
    try:
        if full:
            dt_m, out_m = timed(step_materialised)
        # the FIRST streamed evaluation of a label-set shape in a process reads the index statistics back mid-pipeline (8 bytes,
        # one extra host synchronisation); calls 2..N speculate on that capacity (reid_metric._CAP_HINT) and verify it in the
        # final read-back.  The timed steps below are all "call >= 2": the first call is timed separately, kernels warm.
        step_streamed()
        if full:
            rm._CAP_HINT.clear()
            barrier_sync(world)
            t0 = time.perf_counter(); step_streamed(); barrier_sync(world)
            first_call_ms = (time.perf_counter() - t0) * 1e3
        dt, out = timed(step_streamed)
    finally:
        sys.stdout = _so
        _quiet.close()
    pairs = float(nq) * ng * world * steps
    mAP = float(out[1].item())
    if full:
        assert abs(mAP - float(out_m[1].item())) < 1e-12, "streamed and materialised evaluation disagree"
    if outputs is not None and rank == 0:
        outputs.update(cmc=out[0], mAP=out[1].cpu().numpy(), topk=out[2])

    # ---- per-kernel roofline (rank 0): dominant kernel = the distance contraction (MFMA-bound)
    res = {}
    if rank == 0 and full:
        fn, sq = rm.l2_normalize(feats, return_sqnorm=True)
        q, g = fn[:nq], fn[nq:]
        qq, gg = sq[:nq].contiguous(), sq[nq:].contiguous()
        L = rm.L
        lib = L.lib()
        cap = plan.cap
        pos_key = torch.empty((nq, cap), dtype=torch.int32, device="cuda"); pos_idx = torch.empty_like(pos_key)
        npos = torch.empty(nq, dtype=torch.int32, device="cuda"); hist = torch.zeros((nq, cap), dtype=torch.int32, device="cuda")

        def poslist():
            L.check(lib.creid_stream_poslist(L.ptr(q), L.ptr(g), L.ptr(qq), L.ptr(gg), nq, ng, D, L.ptr(plan.q_slot),
                                             L.ptr(plan.csr_off), L.ptr(plan.g_order), L.ptr(plan.q_cams), L.ptr(plan.g_cams),
                                             cap, L.ptr(pos_key), L.ptr(pos_idx), L.ptr(npos), L.stream()), "poslist")

        def count():
            L.check(lib.creid_stream_count(L.ptr(q), L.ptr(g), L.ptr(qq), L.ptr(gg), nq, ng, D, L.ptr(plan.q_pids),
                                           L.ptr(plan.g_pids), cap, L.ptr(pos_key), L.ptr(pos_idx), L.ptr(npos), L.ptr(hist),
                                           L.stream()), "count")
        poslist()
        t0 = time.perf_counter()
        for _ in range(5):
            rm.StreamPlan.on_device(pids, cams, nq, "cuda").finish()
        t_plan = (time.perf_counter() - t0) / 5 * 1e3           # host wall: upload + 5 launches + 8-byte read-back
        t_pos = time_kernel(poslist, 10)
        t_count = time_kernel(count, 10)
        t_dist = time_kernel(lambda: rm.get_euclidean(q, g, qq, gg), 10)
        d = rm.get_euclidean(q, g, qq, gg)
        t_rank = time_kernel(lambda: rm.rank_rows(d), 5)
        idx = rm.rank_rows(d)
        t_norm = time_kernel(lambda: rm.l2_normalize(feats, return_sqnorm=True), 10)
        t_cmc = time_kernel(lambda: rm.eval_func_device(idx, q_pids, g_pids, q_cams, g_cams, 50), 10)
        t_rank_eval = time_kernel(lambda: rm.rank_rows_eval(d, q_pids, g_pids, q_cams, g_cams), 5)
        flops = 2.0 * nq * ng * D
        live = pmc_eval_insitu() if (extras and world == 1 and shape is None) else None

        def traffic_of(key):
            if live and key in live:
                return live[key]["fetch_bytes"] + live[key]["write_bytes"]
            return pmc_traffic(key)
        src = ("THIS run: rocprofv3 --kernel-trace --pmc child passes (FETCH_SIZE, WRITE_SIZE, SQ_VALU_MFMA_BUSY_CYCLES + GRBM_GUI_ACTIVE, "
               "one pass each) over the same kernels on the same inputs; fetch = 2 x FETCH_SIZE (gfx950)") if live else \
            "profiles/r0x_pmc_traffic.json: committed rocprofv3 --pmc passes, NOT measured in this run"
        res["roofline"] = {"kernel": "sqdist_count_f32_kernel (contraction + in-register rank-by-counting epilogue)",
                           "bound": "mfma", "achieved": flops / (t_count * 1e-3) / 1e12, "peak": MFMA_F32_TFLOPS,
                           "unit": "TFLOP/s", "frac": flops / (t_count * 1e-3) / 1e12 / MFMA_F32_TFLOPS,
                           "traffic": traffic_of("sqdist_count_f32_kernel"), "ms": t_count, "traffic_source": src,
                           "mfma_busy_by_counter": (live or {}).get("sqdist_count_f32_kernel", {}).get("mfma_busy")
                           if live else pmc_field("sqdist_count_f32_kernel", "mfma_busy")}
        res["materialised"] = {
            "value": float(nq) * ng * world * steps / dt_m, "unit": "pairs/s", "ms_per_step": dt_m / steps * 1e3,
            "roofline": {"kernel": "sqdist_f32_kernel", "bound": "mfma", "achieved": flops / (t_dist * 1e-3) / 1e12,
                         "peak": MFMA_F32_TFLOPS, "unit": "TFLOP/s", "frac": flops / (t_dist * 1e-3) / 1e12 / MFMA_F32_TFLOPS,
                         "traffic": traffic_of("sqdist_f32_kernel"), "ms": t_dist},
            "stages_ms": {"l2norm": t_norm, "sqdist": t_dist, "rank_rows_eval": t_rank_eval,
                          "separately": {"rank_rows": t_rank, "cmc_ap": t_cmc}},
            "rank_rows_GBs": nq * ng * (4 + 8) / (t_rank * 1e-3) / 1e9}
        # BASELINE configs[4] asks for fp16 vs fp32: the same distance stage on f16-rounded embeddings (MFMA f16,
        # fp32 accumulate) and what the rounding does to the ranking metric
        fn16 = fn.half()
        t_dist16 = time_kernel(lambda: rm.get_euclidean(fn16[:nq], fn16[nq:]), 10)
        idx16 = rm.rank_rows(rm.get_euclidean(fn16[:nq], fn16[nq:]))
        _, map16, _, _, _, _, _ = rm.eval_func_device(idx16, q_pids, g_pids, q_cams, g_cams, 50)
        res["f16_vs_f32"] = {"sqdist_f16_ms": t_dist16, "sqdist_f16_TFLOPs": flops / (t_dist16 * 1e-3) / 1e12,
                             "sqdist_f32_ms": t_dist, "mAP_f16_minus_f32": float(map16.item()) - mAP,
                             "rank_index_agreement": float((idx16 == idx).float().mean().item())}
        res["stages_ms"] = {"l2norm": t_norm, "plan_device_build_wall": t_plan, "poslist": t_pos, "sqdist_count": t_count}
        res["timed_region"] = ("R1_mAP(streamed=True).compute(device feats, host pids, host camids) -> host (cmc, mAP, topk): "
                               "index build and every host sync inside the clock.  The timed steps are evaluations 2..N of one "
                               "label-set shape: they ASSUME the positive-list capacity of the previous call (verified in the final "
                               "read-back, redone synchronously if wrong) instead of reading 8 bytes back mid-pipeline; "
                               "first_call_ms = the same call without that hint (the first validation of a run)")
        res["first_call_ms"] = first_call_ms
        # BASELINE target line "HBM roofline on the distance matrix": the materialised fp32 matrix moves
        # (m + n) * D * 4 + m * n * 4 algorithmic bytes; the contraction is MFMA-bound (2 D FLOP per 4 output bytes), so this
        # fraction is capped at flops_floor / hbm_floor -- reported because the target is phrased in it
        alg_bytes = (nq + ng) * D * 4 + nq * ng * 4
        res["distance_matrix_hbm"] = {"kernel": "sqdist_f32_kernel (materialised matrix)", "bound": "hbm", "ms": t_dist,
                                      "achieved": alg_bytes / (t_dist * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                      "frac": alg_bytes / (t_dist * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                      "ceiling_frac": (alg_bytes / HBM_PEAK_GBS / 1e9) / (flops / MFMA_F32_TFLOPS / 1e12),
                                      "note": "MFMA-bound kernel: f32-MFMA floor is 1/ceiling_frac x the HBM floor"}
        res["roofline_hbm_stages"] = {"l2norm_GBs": (nq + ng) * D * 8 / (t_norm * 1e-3) / 1e9, "peak_GBs": HBM_PEAK_GBS}
        if not args.no_cpu_baseline and world == 1 and extras:  # the CPU leg is reported at N=1 only
            res["cpu_baseline"] = cpu_baseline_eval(feats, pids, cams, nq, ng)
        if not extras:
            for k in ("f16_vs_f32", "roofline_hbm_stages"):
                res.pop(k, None)
    if rank == 0:
        res["mAP"] = mAP
    return {
        "metric": "eval_dist_pairs_per_sec", "value": pairs / dt, "unit": "pairs/s",
        "ms_per_step": dt / steps * 1e3, "steps": steps, "dtype": "f32",
        "config": {"workload": f"{'DukeMTMC-shaped' if shape is None else 'north-star shape'} eval {nq}x{ng}x{D}: normalise + "
                               "squared-L2 + rank + CMC/mAP end to end, metric-only streamed path"
                               + (" (BASELINE configs[4])" if shape is None else " (BASELINE north_star 3000x15000)"),
                   "queries_per_rank": nq, "gallery": ng, "D": D,
                   "parallelism": f"query-shard x{world}, gallery all-gather" if world > 1 else "single"},
        **res}


def run_eval_configs3_shard(steps=2, warmup=1):
    """BASELINE configs[3], retrieval half: the per-rank shard of the 50k x 200k Street2Shop-shaped evaluation -- 6250 queries
    (50 000 / 8 ranks) x the all-gathered 200 000-row gallery x 2048 fp32 -- streamed END TO END (the 5 GB distance matrix and
    the 10 GB index matrix are never written; utils/reid_metric.py:93-110 is the reference's batched fallback for this size).
    Same timed region as run_eval; roofline of the counting contraction against the f32 MFMA peak."""
    from centroids_reid_amd import reid_metric as rm
    nq, ng, D, npid = 6250, 200_000, 2048, 50_000
    gen = torch.Generator(device="cuda").manual_seed(4)
    feats = torch.randn((nq + ng, D), generator=gen, device="cuda", dtype=torch.float32)
    rng = np.random.default_rng(4)
    pids = np.concatenate([rng.integers(0, npid, nq), np.arange(ng) % npid])       # every query has 4 gallery matches
    cams = np.concatenate([np.zeros(nq, np.int64), np.ones(ng, np.int64)])          # datasets/bases.py:226-229
    metric = rm.R1_mAP(num_query=nq, streamed=True)
    _quiet = open(os.devnull, "w")
    _so, sys.stdout = sys.stdout, _quiet
    try:
        for _ in range(warmup):
            metric.compute(feats, pids, cams)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            cmc, m_ap, topk = metric.compute(feats, pids, cams)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        sys.stdout = _so
        _quiet.close()
    plan = metric.last["plan"]
    fn, sq = rm.l2_normalize(feats, return_sqnorm=True)
    q, g = fn[:nq], fn[nq:]
    qq, gg = sq[:nq].contiguous(), sq[nq:].contiguous()
    L = rm.L
    lib = L.lib()
    cap = plan.cap
    pos_key = torch.empty((nq, cap), dtype=torch.int32, device="cuda"); pos_idx = torch.empty_like(pos_key)
    npos = torch.empty(nq, dtype=torch.int32, device="cuda"); hist = torch.zeros((nq, cap), dtype=torch.int32, device="cuda")
    L.check(lib.creid_stream_poslist(L.ptr(q), L.ptr(g), L.ptr(qq), L.ptr(gg), nq, ng, D, L.ptr(plan.q_slot), L.ptr(plan.csr_off),
                                     L.ptr(plan.g_order), L.ptr(plan.q_cams), L.ptr(plan.g_cams), cap, L.ptr(pos_key),
                                     L.ptr(pos_idx), L.ptr(npos), L.stream()), "poslist")

    def count():
        L.check(lib.creid_stream_count(L.ptr(q), L.ptr(g), L.ptr(qq), L.ptr(gg), nq, ng, D, L.ptr(plan.q_pids), L.ptr(plan.g_pids),
                                       cap, L.ptr(pos_key), L.ptr(pos_idx), L.ptr(npos), L.ptr(hist), L.stream()), "count")
    t_count = time_kernel(count, 2)
    flops = 2.0 * nq * ng * D
    return {"metric": "eval_dist_pairs_per_sec", "value": float(nq) * ng * steps / dt, "unit": "pairs/s",
            "ms_per_step": dt / steps * 1e3, "steps": steps, "warmup": warmup, "dtype": "f32", "mAP": float(m_ap),
            "config": {"workload": "per-rank shard of BASELINE configs[3] retrieval: 6250 queries (50 000 / 8 ranks) x 200 000 gallery "
                                   "x 2048, normalise + squared-L2 + rank + CMC/mAP end to end, streamed (no 5 GB matrix)",
                       "queries_per_rank": nq, "gallery": ng, "D": D, "positive_list_capacity": int(cap)},
            "roofline": {"kernel": "sqdist_count_f32_kernel", "bound": "mfma", "achieved": flops / (t_count * 1e-3) / 1e12,
                         "peak": MFMA_F32_TFLOPS, "unit": "TFLOP/s", "frac": flops / (t_count * 1e-3) / 1e12 / MFMA_F32_TFLOPS,
                         "ms": t_count, "traffic": None,
                         "algorithmic_bytes": (nq + ng) * D * 4, "note": "4096 FLOP per pair; operands 1.69 GB, read once by HBM and "
                         "re-read from L2 / Infinity Cache while MFMA-bound"}}


def cpu_baseline_eval(feats, pids, cams, nq, ng):
    """The CPU oracle (kind 'port') on a bounded sample of the same workload, all host cores."""
    from oracle import reid_oracle as ro
    cores = os.cpu_count() or 1
    torch.set_num_threads(cores)
    nqs = min(nq, 512)
    f = torch.cat([feats[:nqs], feats[nq:]]).cpu()
    p = np.concatenate([pids[:nqs], pids[nq:]]); c = np.concatenate([cams[:nqs], cams[nq:]])
    t0 = time.perf_counter()
    ro.r1_map(f, p, c, nqs)
    dt = time.perf_counter() - t0
    return {"value": nqs * ng / dt, "unit": "pairs/s", "cores": cores, "kind": "port",
            "sample": f"{nqs} of {nq} queries x {ng} gallery, vectorised numpy/torch-CPU restatement "
                      f"(the reference's own per-query Python loop is ~50x slower, BASELINE.md)", "seconds": dt}


def cpu_baseline_train(P, K, H, W):
    """The CPU oracle (kind 'port': torch-CPU restatement of backbone + heads, autograd backward, torch.optim Adam + SGD steps)
    on the host cores, same synthetic shapes.  Bounded sample: five full 64-image steps after one warm-up step, on at most 32
    threads (torch-CPU convolutions get slower, not faster, when oversubscribed across hundreds of cores)."""
    from oracle import backbone_oracle as bo, reid_oracle as ro
    cores = min(32, os.cpu_count() or 1)
    torch.set_num_threads(cores)
    sd = bo.make_state_dict("resnet50", 1, seed=1)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()
              if v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var"))}
    sd2 = {**{k: v.clone() for k, v in sd.items()}, **params}
    C = 751
    centers = torch.randn(C, 2048, requires_grad=True); fc = (torch.randn(C, 2048) * 0.001).requires_grad_(True)
    bw = torch.ones(2048, requires_grad=True)

    # the reference's two optimisers (solver/build.py:9-47): Adam(lr 3.5e-4, weight decay 5e-4) over everything but the centers,
    # SGD(lr 0.5) over the centers after the 1 / CENTER_LOSS_WEIGHT rescale (train_ctl_model.py:154-159) -- the GPU number
    # includes both steps, so does this one
    opt = torch.optim.Adam(list(params.values()) + [fc, bw], lr=3.5e-4, weight_decay=5e-4)
    opt_c = torch.optim.SGD([centers], lr=0.5)

    def step(p):
        x = torch.randn(p * K, 3, H, W)
        labels = torch.as_tensor(np.repeat((np.arange(p) * 7) % C, K).astype(np.int64))
        is_real = torch.ones(p * K, dtype=torch.bool)
        opt.zero_grad(); opt_c.zero_grad()
        _, feat = bo.backbone_forward(x, sd2, "resnet50", 1, training=True)
        o = ro.ctl_heads(feat, labels, is_real, bw, torch.zeros(2048), torch.zeros(2048), torch.ones(2048), fc, centers, p, K)
        o["total"].backward()
        opt.step()
        centers.grad.mul_(1.0 / 5e-4)
        opt_c.step()
    nsteps = int(os.environ.get("CREID_CPU_BASELINE_STEPS", "5"))     # >= 5 steps after 1 warm-up
    step(P)
    t0 = time.perf_counter()
    for _ in range(nsteps):
        step(P)
    dt = time.perf_counter() - t0
    return {"value": nsteps * P * K / dt, "unit": "images/s", "cores": cores, "kind": "port",
            "sample": f"{nsteps} full steps of {P * K} images (fwd + bwd + Adam + center SGD, like the GPU step) after 1 warm-up step, torch-CPU oracle; "
                      f"{cores} of {os.cpu_count()} host threads: torch-CPU (oneDNN) convolutions of a 64-image batch stop scaling past "
                      "one socket's worth of cores and get SLOWER when oversubscribed across all of them, so 32 is the fastest setting "
                      "for this baseline (the eval leg, a pure GEMM + sort, uses every core)",
            "seconds": dt}



def cpu_baseline_embed(B=64, H=256, W=128, reps=3):
    """The CPU oracle's eval-mode embedding forward (backbone + GAP + BNNeck, torch-CPU fp32) on <= 32 host threads: `reps` batches
    of B images after one warm-up batch -- the baseline beside the `embed` object."""
    from oracle import backbone_oracle as bo
    cores = min(32, os.cpu_count() or 1)
    torch.set_num_threads(cores)
    sd = bo.make_state_dict("resnet50", 1, seed=1)
    bn_w, bn_b, bn_rm, bn_rv = torch.ones(2048), torch.zeros(2048), torch.zeros(2048), torch.ones(2048)

    def fwd():
        with torch.no_grad():
            _, feat = bo.backbone_forward(torch.randn(B, 3, H, W), sd, "resnet50", 1, training=False)
            return bo.bnneck_forward(feat, bn_w, bn_b, bn_rm, bn_rv, False)
    fwd()
    t0 = time.perf_counter()
    for _ in range(reps):
        fwd()
    dt = time.perf_counter() - t0
    return {"value": reps * B / dt, "unit": "images/s", "cores": cores, "kind": "port",
            "sample": f"{reps} eval-mode forwards of {B} images after 1 warm-up, torch-CPU oracle ({cores} of {os.cpu_count()} host "
                      "threads, the fastest setting: see the training leg's note)", "seconds": dt}


def vendor_yardstick(timeout_s=None):
    """tools/vendor_step.py in a child process: the same training step / embedding forward on stock torch-ROCm modules (MIOpen,
    hipBLASLt, channels_last, bf16 autocast), same box -- a yardstick outside the product.  None when switched off; an `error`
    entry when the stock stack does not finish inside the budget (MIOpen's first-run kernel search can take minutes on a fresh
    box -- nothing the product depends on)."""
    import subprocess
    if os.environ.get("CREID_BENCH_NO_VENDOR", "0") == "1":
        return None
    timeout_s = timeout_s or int(os.environ.get("CREID_BENCH_VENDOR_TIMEOUT", "150"))
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vendor_step.py"), "--steps", "10"], capture_output=True, text=True,
                           timeout=timeout_s, env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if line:
            out = json.loads(line[-1])
            out["seconds_incl_kernel_search"] = time.perf_counter() - t0
            return out
        return {"error": f"rc {r.returncode}: {r.stderr[-300:]}"}
    except subprocess.TimeoutExpired:
        return {"error": f"stock torch-ROCm step did not finish in {timeout_s} s (MIOpen kernel search on a fresh box)"}
    except Exception as e:  # noqa: BLE001
        return {"error": f"{type(e).__name__}: {e}"}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, arrays):
    """--dump-outputs: one DIR/<name>.npy per array, float64 where the value is float64 or integral, float32 otherwise."""
    os.makedirs(path, exist_ok=True)
    conv = {}
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        conv[name] = a.astype(np.float64 if a.dtype == np.float64 or a.dtype.kind in "iub" else np.float32)
    total = sum(a.nbytes for a in conv.values())
    assert total <= DUMP_LIMIT_BYTES, f"outputs to dump are {total} bytes, over the {DUMP_LIMIT_BYTES} byte limit"
    for name, a in conv.items():
        np.save(os.path.join(path, name + ".npy"), a)


# ----------------------------------------------------------------------------- main
_REAL_STDOUT = sys.stdout
_REAL_FD = 1


def main():
    # the contract is ONE JSON line on stdout: library chatter (optimizer grouping notes, metric banners that mirror
    # the reference's prints) goes to stderr -- at the FILE-DESCRIPTOR level too: RCCL prints its version banner through C
    # stdio, buffered until exit, i.e. AFTER the result line of a data-parallel run
    global _REAL_FD
    sys.stdout.flush()
    _REAL_FD = os.dup(1)
    os.dup2(2, 1)
    sys.stdout = sys.stderr
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--workload", choices=["train", "eval"], default=None)
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="skip the CPU leg of a --full run (a --full run reports it by default)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run every side measurement (rooflines, counter passes, CPU baselines, other "
                         "precisions / sizes / shapes, the evaluation legs of a training run, the stock torch-ROCm yardstick)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step to DIR/<name>.npy")
    ap.add_argument("--inner-trace", action="store_true", help=argparse.SUPPRESS)   # child of bench_train.insitu_trace
    ap.add_argument("--inner-eval-trace", action="store_true", help=argparse.SUPPRESS)   # child of pmc_eval_insitu
    args = ap.parse_args()
    if (args.steps is not None and args.steps < 1) or (args.warmup is not None and args.warmup < 0):
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.inner_eval_trace:
        inner_eval_trace()
        return
    rank, world = ddp_setup(args.gpus)
    if args.inner_trace:
        from centroids_reid_amd import bench_train
        bench_train.inner_trace(args, barrier_sync)
        return
    workload = args.workload
    if workload is None:
        try:
            from centroids_reid_amd import bench_train  # noqa: F401
            workload = "train"
        except ImportError:
            workload = "eval"
    outputs = {} if args.dump_outputs else None
    if workload == "train":
        from centroids_reid_amd import bench_train
        args.steps = args.steps if args.steps is not None else 30
        args.warmup = args.warmup if args.warmup is not None else 5
        out = bench_train.run(args, rank, world, barrier_sync, time_kernel,
                              None if args.no_cpu_baseline else cpu_baseline_train, full=args.full, outputs=outputs)
        if rank == 0 and world == 1 and "embed" in out and not args.no_cpu_baseline:
            out["embed"]["cpu_baseline"] = cpu_baseline_embed()
        if rank == 0 and world == 1 and "embed" in out:
            vy = vendor_yardstick()
            if vy is not None:
                if "step" in vy:
                    vy["step"]["product_over_vendor"] = out["value"] / vy["step"]["images_per_s"]
                if "embed" in vy:
                    vy["embed"]["product_over_vendor"] = out["embed"]["value"] / vy["embed"]["images_per_s"]
                out["extra"] = {"vendor_yardstick": vy}
        if args.full and os.environ.get("CREID_BENCH_NO_EVAL", "0") != "1":
            # the other half of BASELINE.metric (eval query x gallery dist-pairs/s) rides in the same line, timed by
            # the same invocation: 5 steps after 2 warm-up of the configs[4] workload
            ev = run_eval(args, rank, world, steps=5, warmup=2)
            ns = run_eval(args, rank, world, steps=5, warmup=2, shape=(3000, 15000, 2048), extras=False) if world == 1 else None
            c3 = run_eval_configs3_shard() if (world == 1 and os.environ.get("CREID_BENCH_NO_CONFIGS3", "0") != "1") else None
            if rank == 0:
                ev["higher_is_better"] = True
                if ns is not None:
                    ev["north_star_3000x15000"] = ns
                if c3 is not None:
                    ev["configs3_shard"] = c3
                vy = out.get("extra", {}).get("vendor_yardstick")
                if vy and "eval" in vy:                      # stock torch to RANKED INDICES vs the product's materialised path (adds CMC / AP)
                    vy["eval"]["product_materialised_over_vendor"] = ev["materialised"]["value"] / vy["eval"]["pairs_per_s_to_ranked_indices"]
                    vy["eval"]["product_streamed_over_vendor"] = ev["value"] / vy["eval"]["pairs_per_s_to_ranked_indices"]
                out["eval"] = ev
    else:
        args.steps = args.steps if args.steps is not None else 5
        args.warmup = args.warmup if args.warmup is not None else 2
        out = run_eval(args, rank, world, full=args.full, outputs=outputs)
        out.pop("steps", None)
    if rank == 0:
        if outputs is not None:
            dump_outputs(args.dump_outputs, outputs)
        line = {"metric": out.pop("metric"), "value": out.pop("value"), "unit": out.pop("unit"),
                "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": out.pop("ms_per_step"), "higher_is_better": True, "scaling": "weak",
                "vs_baseline": None, "dtype": out.pop("dtype"), "data": "synthetic", "full": args.full, **out}
        os.write(_REAL_FD, (json.dumps(line) + "\n").encode())
    if dist.is_available() and dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
