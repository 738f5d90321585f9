"""The camera-aware centroid validation tail (MODEL.KEEP_CAMID_CENTROIDS, modelling/bases.py:205-297) in one process: the path on the
device -- centroid index by csrc/centroid_index.hip, camera-set streamed evaluation -- against the path it replaces, which stays
reachable: the host grouping loop (bases._camera_centroids_host) and R1_mAP(streamed=False) (distance matrix, full sort, scan).
Synthetic labels (pids and cameras uniform) of the DukeMTMC and Market-1501 shapes and of 6250 x 200 000, D = 2048:
  1. asserts that both paths return the same centroids (bit for bit), labels, camera sets, CMC, top-k and mAP (1e-12);
  2. times, alternating, whole calls on the host clock (each ends in its read-back): labels -> centroids
     (validation_create_centroids) and centroids -> CMC / mAP (R1_mAP.compute); median (min .. max);
  3. the device half alone between device events on the normalised rows: matrix + sort + scan against poslist + count + finalize;
  4. torch.cuda.max_memory_allocated above the live inputs, per stage.
Prints the markdown tables profiles/camset_eval.md quotes (--out FILE writes them as well):
    python tools/camset_eval_bench.py --out tables.md
Needs a GPU; there is no fallback."""
import argparse
import contextlib
import io
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from centroids_reid_amd import bases, reid_metric as rm   # noqa: E402
from centroids_reid_amd.config import get_cfg_defaults   # noqa: E402

SHAPES = [("Duke-shaped", 2228, 17661, 1110, 8), ("Market-shaped", 3368, 15913, 751, 6), ("6250 x 200 000", 6250, 200_000, 20_000, 8)]
D = 2048


def holder(nq):
    cfg = get_cfg_defaults()
    cfg.MODEL.USE_CENTROIDS = True
    cfg.MODEL.KEEP_CAMID_CENTROIDS = True
    cfg.num_query = nq
    return SimpleNamespace(hparams=cfg, trainer=SimpleNamespace(logger=None, current_epoch=0))


def quiet(fn):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn()


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = quiet(fn)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def peak_above_live(fn):
    torch.cuda.synchronize()
    live = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    quiet(fn)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - live


def events_ms(fn, warmup, reps):
    out = []
    for _ in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out[warmup:]))


def run_case(name, nq, ng, npid, ncam, warmup, reps):
    rng = np.random.default_rng(nq)
    pids = rng.integers(0, npid, nq + ng)
    cams = rng.integers(0, ncam, nq + ng)
    gen = torch.Generator(device="cuda").manual_seed(nq)
    emb = torch.randn((nq + ng, D), generator=gen, device="cuda")
    h = holder(nq)
    device_index = bases.camera_centroid_index

    def centroids(new):
        bases.camera_centroid_index = device_index if new else (lambda *a, **k: None)
        try:
            return bases.ModelBase.validation_create_centroids(h, emb, pids, cams, respect_camids=True)
        finally:
            bases.camera_centroid_index = device_index

    (e_new, l_new, c_new), (e_old, l_old, c_old) = quiet(lambda: centroids(True)), quiet(lambda: centroids(False))
    assert torch.equal(e_new, e_old) and np.array_equal(l_new, l_old) and list(c_new) == c_old
    n_cent = len(l_new) - nq
    m_new, m_old = rm.R1_mAP(num_query=nq, streamed=True), rm.R1_mAP(num_query=nq)
    evals = {"new": lambda: m_new.compute(e_new, l_new, c_new, respect_camids=True),
             "old": lambda: m_old.compute(e_old, l_old, c_old, respect_camids=True)}
    r_new, r_old = quiet(evals["new"]), quiet(evals["old"])
    assert np.array_equal(r_new[0], r_old[0]) and abs(r_new[1] - r_old[1]) <= 1e-12 and np.allclose(r_new[2], r_old[2], rtol=0, atol=1e-12)
    assert np.abs(m_new.last["single_performance"] - m_old.last["single_performance"]).max() <= 1e-12
    m_old.last = {}
    # the grouping loop is quadratic in the host path: fewer repetitions where one call takes seconds
    reps_old = reps if ng < 100_000 else max(2, reps // 10)
    t = {k: [] for k in ("cent_new", "cent_old", "eval_new", "eval_old")}
    for i in range(warmup + reps):
        for key, fn in (("cent_new", lambda: centroids(True)), ("eval_new", evals["new"])):
            ms, _ = timed(fn)
            if i >= warmup:
                t[key].append(ms)
        if i < min(warmup, 1) + reps_old:
            for key, fn in (("cent_old", lambda: centroids(False)), ("eval_old", evals["old"])):
                ms, _ = timed(fn)
                if i >= min(warmup, 1):
                    t[key].append(ms)
                m_old.last = {}
    mem = {"cent_new": peak_above_live(lambda: centroids(True)), "cent_old": peak_above_live(lambda: centroids(False)),
           "eval_new": peak_above_live(evals["new"]), "eval_old": peak_above_live(evals["old"])}
    m_old.last = {}
    # the device half alone, on the normalised rows
    fn_, sq = rm.l2_normalize(e_new, return_sqnorm=True)
    fq, fg, qq, gg = fn_[:nq], fn_[nq:], sq[:nq].contiguous(), sq[nq:].contiguous()
    plan = m_new.last["plan"]
    qp, gp = plan.q_pids, plan.g_pids
    qc = np.asarray(cams[:nq], np.int64)

    def old_device():
        idx = rm.rank_rows(rm.get_euclidean(fq, fg, qq, gg))
        rm.eval_func_device(idx, qp, gp, qc, plan.g_cams, camsets=True)

    dev_new = events_ms(lambda: rm.stream_eval(fq, fg, qq, gg, plan), warmup, reps)
    dev_old = events_ms(lambda: quiet(old_device), warmup, reps)
    med = lambda v: (float(np.median(v)), min(v), max(v))                       # noqa: E731
    return dict(name=name, shape=f"{nq} / {ng} / {npid} / {ncam}", n_cent=n_cent, t={k: med(v) for k, v in t.items()}, mem=mem,
                dev_new=dev_new, dev_old=dev_old, mAP=r_new[1], n=dict(new=len(t["cent_new"]), old=len(t["cent_old"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [run_case(*s, a.warmup, a.reps) for s in (SHAPES[:2] if a.small_only else SHAPES)]
    ms = lambda v: f"{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})"                      # noqa: E731
    mib = lambda b: f"{b / 2**20:.1f}"                                          # noqa: E731
    out = [f"Camera-aware centroid validation tail, D = {D}, synthetic labels (pids and cameras uniform), device {torch.cuda.get_device_name(0)}; "
           f"{a.reps} timed calls after {a.warmup} warm-ups, paths alternating in one process (the host path at 200 000: fewer, see "
           "the calls column); ms = median (min .. max) of whole calls on the host clock, read-back included.  new = device centroid "
           "index + camera-set streamed evaluation; old = host grouping loop + R1_mAP(streamed=False).", "",
           "| labels | q / g / pids / cams | centroids | stage | new ms | old ms | old / new | new MiB above inputs | old MiB above inputs | calls new / old |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        for stage, kn, ko in (("labels -> centroids", "cent_new", "cent_old"), ("centroids -> CMC / mAP", "eval_new", "eval_old")):
            out.append(f"| {r['name']} | {r['shape']} | {r['n_cent']} | {stage} | {ms(r['t'][kn])} | {ms(r['t'][ko])} | "
                       f"{r['t'][ko][0] / r['t'][kn][0]:.2f} | {mib(r['mem'][kn])} | {mib(r['mem'][ko])} | {r['n']['new']} / {r['n']['old']} |")
    out += ["", "The device half of the evaluation alone, ms between device events on the normalised rows (median): old = distance "
            "matrix + full sort + camera-set scan; new = positives + streamed count + finalize (index and read-back excluded on both "
            "sides):", "",
            "| labels | queries x centroids | matrix + sort + scan | poslist + count + finalize | old / new |", "|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['name']} | {r['shape'].split(' / ')[0]} x {r['n_cent']} | {r['dev_old']:.3f} | {r['dev_new']:.3f} | "
                   f"{r['dev_old'] / r['dev_new']:.2f} |")
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
