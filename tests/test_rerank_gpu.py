"""GPU: reid_metric.re_ranking (csrc/rerank.hip behind topk_stream / get_euclidean) against the float64 reference of
tests/rerank_ref.py, and its plumbing through R1_mAP and inference.get_similar.

Discrete results (neighbour table, R* rows, the pattern of V') must EQUAL the reference's.  Values are held to a tolerance
that each case computes for itself and that never looks at the device:
    tol = max(4 x max|float32 restatement - float64 reference|, 32 x 2^-23)
The restatement (`restate_f32` below) redoes steps 1-7 in NumPy float32 on the reference's sets, so its distance from the
reference is what fp32 arithmetic costs on this very input; the factor 4 covers the device's expf and division differing from
NumPy's by a few ulp and its different summation order.  The floor: out is in [0, 1] and |dJ/ds| <= 2, so the roundings of
exp, the division, the normalisation and the two levels of averaging fit inside 32 ulp of 1."""
import functools

import numpy as np
import pytest
import torch

from rerank_ref import clustered_int_features, int_sqdist, rerank_reference

pytestmark = pytest.mark.gpu

FLOOR = 32 * 2.0 ** -23
F32 = np.float32


def restate_f32(d_all, nq, k1, k2, lam, sets):
    """Steps 1-7 of rerank_ref.rerank_reference in float32, on the reference's own sets and neighbour order."""
    d = np.asarray(d_all).astype(F32)
    N = d.shape[0]
    order = np.argsort(np.asarray(d_all), axis=1, kind="stable")
    M = d.max(axis=1)
    od = np.where(M[:, None] == 0, F32(0), d / np.where(M == 0, F32(1), M)[:, None]).astype(F32)
    V = np.zeros((N, N), F32)
    for i, cols in enumerate(sets):
        if len(cols):
            w = np.exp(-od[i, cols])
            V[i, cols] = w / w.sum(dtype=F32)
    if k2 > 1:
        Vq = np.zeros((N, N), F32)
        for t in range(k2):
            Vq += V[order[:, t]]
        Vq /= F32(k2)
    else:
        Vq = V
    out = np.empty((nq, N - nq), F32)
    for i in range(nq):
        s = np.minimum(Vq[i][None, :], Vq[nq:]).sum(axis=1, dtype=F32)
        out[i] = (F32(1) - F32(lam)) * (F32(1) - s / (F32(2) - s)) + F32(lam) * od[i, nq:]
    assert out.dtype == F32 and Vq.dtype == F32
    return out, Vq


def _int_features(kind, nq, ng, D, k1):
    N = nq + ng
    X = clustered_int_features(N, D, max(4, N // 24), seed=N + D + k1)
    if kind == "dup":
        # k1 + 2 identical rows: the last copy is absent from every neighbour list, its own included
        X[nq + 5:nq + 5 + k1 + 2] = X[nq + 5]
        X[3:3 + k1 + 2] = X[3]
    if kind == "hub":
        # 120 rows spread far from one another around three hub rows near the origin: every spread row has the hubs as its
        # nearest neighbours, the hubs list only k1 + 1 rows back
        rng = np.random.default_rng(7)
        far = rng.integers(-20, 21, (120, D)).astype(np.float32)
        X[nq // 2:nq // 2 + 20] = far[:20]
        X[nq + 10:nq + 110] = far[20:]
        X[nq + 110:nq + 113] = 0
        X[nq + 111, 0], X[nq + 112, 0] = 1, -1
        assert int_sqdist(X).max() < 1 << 24
    return X


# name -> (kind, nq, ng, D, k1, k2, lambda)
CASES = {
    "int-37x203-k6-3": ("int", 37, 203, 8, 6, 3, 0.3),
    "int-37x203-k5-6-lam0": ("int", 37, 203, 16, 5, 6, 0.0),
    "int-37x203-k21-1-lam1": ("int", 37, 203, 16, 21, 1, 1.0),
    "int-160x640-k20-6": ("int", 160, 640, 32, 20, 6, 0.3),
    "int-60x300-k125-2": ("int", 60, 300, 8, 125, 2, 0.3),          # the largest k1 the set kernel's LDS takes: rows of ~200
    "dup-37x203-k6-3": ("dup", 37, 203, 8, 6, 3, 0.3),
    "hub-60x300-k20-6": ("hub", 60, 300, 8, 20, 6, 0.3),
    "audit-100x500-d2048": ("audit", 100, 500, 2048, 20, 6, 0.3),
}


@functools.lru_cache(maxsize=None)
def _run(name):
    """One case: device run, float64 reference and float32 restatement, computed once and shared by the tests below."""
    from centroids_reid_amd import reid_metric as rm
    kind, nq, ng, D, k1, k2, lam = CASES[name]
    if kind == "audit":
        rng = np.random.default_rng(11)
        centres = rng.standard_normal((40, D))
        X = centres[rng.integers(0, 40, nq + ng)] + 0.6 * rng.standard_normal((nq + ng, D))
        Xd = rm.l2_normalize(torch.from_numpy(X.astype(np.float32)).cuda())
        d_all = rm.get_euclidean(Xd, Xd).cpu().numpy()           # the bits topk_stream orders by
    else:
        X = _int_features(kind, nq, ng, D, k1)
        Xd = torch.from_numpy(X).cuda()
        d_all = int_sqdist(X)
    stats, debug = {}, {}
    out = rm.re_ranking(Xd[:nq].contiguous(), Xd[nq:].contiguous(), k1, k2, lam, stats=stats, debug=debug)
    ref_out, sets, ref_vq = rerank_reference(d_all, nq, k1, k2, lam)
    rs_out, rs_vq = restate_f32(d_all, nq, k1, k2, lam, sets)
    dev = {k: v.cpu().numpy() for k, v in debug.items()}
    N = nq + ng
    vq = np.zeros((N, N), np.float32)
    rp = dev["vprime_rowptr"]
    rows = np.repeat(np.arange(N), np.diff(rp))
    vq[rows, dev["vprime_cols"]] = dev["vprime_vals"]
    return dict(nq=nq, ng=ng, k1=k1, k2=k2, lam=lam, d_all=d_all, out_t=out, out=out.cpu().numpy(), stats=stats, dev=dev,
                vq=vq, ref_out=ref_out, sets=sets, ref_vq=ref_vq,
                tol_out=max(4 * float(np.abs(rs_out - ref_out).max()), FLOOR),
                tol_v=max(4 * float(np.abs(rs_vq - ref_vq).max()), FLOOR))


@pytest.mark.parametrize("name", list(CASES))
def test_sets_and_pattern_equal_the_reference(name):
    c = _run(name)
    dev, N, K = c["dev"], c["nq"] + c["ng"], c["k1"] + 1
    order = np.argsort(c["d_all"], axis=1, kind="stable")
    assert np.array_equal(dev["neighbours"], order[:, :K])
    assert np.array_equal(dev["rowmax"], c["d_all"].max(axis=1).astype(np.float32))
    rp, cols = dev["rstar_rowptr"], dev["rstar_cols"]
    assert rp.shape == (N + 1,) and rp[0] == 0 and rp[-1] == len(cols) == c["stats"]["nnz_v"]
    for i in range(N):
        assert cols[rp[i]:rp[i + 1]].tolist() == c["sets"][i].tolist(), i
    rp2, cols2 = dev["vprime_rowptr"], dev["vprime_cols"]
    assert rp2[-1] == len(cols2) == c["stats"]["nnz_vprime"]
    for i in range(N):
        assert cols2[rp2[i]:rp2[i + 1]].tolist() == np.nonzero(c["ref_vq"][i])[0].tolist(), i
    assert c["stats"]["max_row_v"] == max(len(s) for s in c["sets"])
    assert c["stats"]["max_row_vprime"] == int((c["ref_vq"] != 0).sum(axis=1).max())
    if name.startswith("dup"):
        last = c["nq"] + 5 + c["k1"] + 1
        assert last not in dev["neighbours"][last] and rp[last + 1] == rp[last]      # absent from its own list: empty R*


@pytest.mark.parametrize("name", list(CASES))
def test_values_within_the_computed_tolerance(name):
    c = _run(name)
    dv = float(np.abs(c["vq"] - c["ref_vq"]).max())
    do = float(np.abs(c["out"] - c["ref_out"]).max())
    print(f"{name}: max|V' - ref| = {dv:.3e} (tol {c['tol_v']:.3e}); max|out - ref| = {do:.3e} (tol {c['tol_out']:.3e}); "
          f"nnz V = {c['stats']['nnz_v']}, nnz V' = {c['stats']['nnz_vprime']}")
    assert np.isfinite(c["out"]).all()
    assert dv <= c["tol_v"]
    assert do <= c["tol_out"]


@pytest.mark.parametrize("name", list(CASES))
def test_pairs_sharing_no_column_are_bit_equal_to_the_dense_pass(name):
    """J is exactly 1 there: out = (1 - lambda) + lambda * (d / M_i) in fp32, one rounding per operation."""
    c = _run(name)
    nq, lam, dev = c["nq"], c["lam"], c["dev"]
    pat = (c["ref_vq"] != 0).astype(np.float32)
    unshared = (pat[:nq] @ pat[nq:].T) == 0
    assert np.array_equal(dev["dist"], c["d_all"][:nq, nq:].astype(np.float32))
    M = dev["rowmax"][:nq, None]
    od = np.where(M == 0, F32(0), dev["dist"] / np.where(M == 0, F32(1), M)).astype(F32)
    dense = (F32(1) - F32(lam)) + F32(lam) * od
    assert dense.dtype == F32
    assert unshared.any()
    assert np.array_equal(c["out"][unshared].view(np.int32), dense[unshared].view(np.int32))
    if lam == 1.0:
        assert np.array_equal(c["out"].view(np.int32), od.view(np.int32))


@pytest.mark.parametrize("name", list(CASES))
def test_device_ranking_is_ordered_under_the_reference(name):
    """rank_rows of the device's matrix, read through the REFERENCE's values: never descending by more than 2 tol, for every
    query and every position."""
    from centroids_reid_amd import reid_metric as rm
    c = _run(name)
    idx = rm.rank_rows(c["out_t"]).cpu().numpy()
    ranked = np.take_along_axis(c["ref_out"], idx, axis=1)
    assert (np.diff(ranked, axis=1) >= -2 * c["tol_out"]).all()


def test_two_runs_are_bit_identical():
    from centroids_reid_amd import reid_metric as rm
    c = _run("hub-60x300-k20-6")
    X = torch.from_numpy(_int_features("hub", 60, 300, 8, 20)).cuda()
    again = rm.re_ranking(X[:60].contiguous(), X[60:].contiguous(), 20, 6, 0.3)
    assert torch.equal(again, c["out_t"])
    rng = np.random.default_rng(5)
    q, g = (torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda() for s in ((50, 96), (400, 96)))
    assert torch.equal(rm.re_ranking(q, g), rm.re_ranking(q, g))


# ------------------------------------------------------------------------------------------------ plumbing
def _labelled(nq=40, ng=200, D=62, seed=2):
    rng = np.random.default_rng(seed)
    pids = np.concatenate([rng.integers(0, 12, nq), rng.integers(0, 12, ng)])
    camids = rng.integers(0, 4, nq + ng)
    centres = rng.standard_normal((12, D))
    feats = (centres[pids] + 0.8 * rng.standard_normal((nq + ng, D))).astype(np.float32)
    return feats, pids, camids


@pytest.mark.parametrize("reranking", [True, {"k1": 9, "k2": 4, "lambda_value": 0.5}], ids=["defaults", "dict"])
def test_r1_map_reranking_is_the_existing_evaluation_of_the_reranked_matrix(reranking):
    from centroids_reid_amd import reid_metric as rm
    feats, pids, camids = _labelled()
    nq = 40
    fd = torch.from_numpy(feats).cuda()
    metric = rm.R1_mAP(num_query=nq, reranking=reranking)
    cmc, mAP, topk = metric.compute(fd, pids, camids)
    f = rm.l2_normalize(rm._pad_width(fd))                       # D = 62 is padded to 64, feat_norm applies first
    rr = rm.re_ranking(f[:nq], f[nq:], **rm.rerank_options(reranking))
    assert torch.equal(metric.last["distmat"], rr)
    plain = rm.get_euclidean(f[:nq], f[nq:])
    assert not torch.equal(rr, plain)
    idx, valid, ap, first = rm.rank_rows_eval(rr, pids[:nq], pids[nq:], camids[:nq], camids[nq:])
    cmc2, mAP2, topk2, _ = rm.eval_reduce_device(valid, ap, first, 50)
    assert torch.equal(metric.last["indices"], idx)
    assert np.array_equal(cmc, cmc2.cpu().numpy()) and mAP == float(mAP2.item()) and np.array_equal(topk, topk2.cpu().numpy())
    # camera sets (respect_camids): rank_rows + eval_func on the same matrix
    camsets = [[int(c)] if i % 3 else [int(c), int((c + 1) % 4)] for i, c in enumerate(camids)]
    cmc3, mAP3, topk3 = metric.compute(fd, pids, camsets, respect_camids=True)
    assert torch.equal(metric.last["distmat"], rr)
    cmc4, mAP4, topk4, _ = rm.eval_func(rm.rank_rows(rr), pids[:nq], pids[nq:], camsets[:nq], camsets[nq:], 50, True)
    assert np.array_equal(cmc3, cmc4) and mAP3 == mAP4 and np.array_equal(topk3, topk4)


@pytest.mark.parametrize("topk", [10, 0])
def test_get_similar_reranking_is_topk_of_the_reranked_matrix(topk):
    from centroids_reid_amd import inference as inf
    from centroids_reid_amd import reid_metric as rm
    feats, _, _ = _labelled(D=64)
    q, g = feats[:40], feats[40:]
    qpaths, gpaths = [f"q{i}" for i in range(40)], np.array([f"g{i}" for i in range(200)])
    opts = {"k1": 8, "k2": 3, "lambda_value": 0.4}
    stats = {}
    res = inf.get_similar(q, qpaths, g, gpaths, topk=topk, reranking=opts, stats=stats, streamed="auto")
    assert stats["path"] == "reranked" and stats["nnz_vprime"] > 0
    rr = rm.re_ranking(rm.l2_normalize(torch.from_numpy(q).cuda()), rm.l2_normalize(torch.from_numpy(g).cuda()), **opts)
    if topk:
        idx, dist = rm.topk_rows(rr, topk)
    else:
        idx = rm.rank_rows(rr)
        dist = torch.gather(rr, 1, idx)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    for i, p in enumerate(qpaths):
        assert np.array_equal(res[p]["indices"], idx[i]) and np.array_equal(res[p]["distances"], dist[i])
        assert np.array_equal(res[p]["paths"], gpaths[idx[i]])
    plain = inf.get_similar(q, qpaths, g, gpaths, topk=10, stats=stats)
    assert stats["path"] == "materialised"
    assert any(not np.array_equal(plain[p]["distances"], res[p]["distances"][:10]) for p in qpaths)


def test_refusals():
    from centroids_reid_amd import _lib as L
    from centroids_reid_amd import inference as inf
    from centroids_reid_amd import reid_metric as rm
    q, g = torch.zeros(8, 8).cuda(), torch.randn(1100, 8).cuda()
    small = g[:40].contiguous()
    for args in ((q.cpu(), g), (q, g.cpu()),
                 (q, small, 48), (q, small, 100), (q, g, 1024),             # k1 + 1 > min(N, 1024)
                 (q, g, 126),                                               # a worst-case R* row beyond the set kernel's LDS
                 (q, g, 20, 0), (q, g, 20, 22), (q, g, 5, 7),               # k2 < 1, k2 > k1 + 1
                 (q, g, 20, 6, -0.01), (q, g, 20, 6, 1.01), (q, g, 20, 6, float("nan")),
                 (q.bfloat16(), g.bfloat16()), (q.half(), g.half()), (q, g[:, :4].contiguous())):
        with pytest.raises(L.CreidError):
            rm.re_ranking(*args)
    assert rm.re_ranking(q, small, 47, 6).shape == (8, 40)              # k1 + 1 == N is the limit, not beyond it
    for kw in (dict(streamed=True), dict(compute_dtype=torch.bfloat16), dict(compute_dtype=torch.float16),
               dict(dist_func="cosine")):
        with pytest.raises(L.CreidError):
            rm.R1_mAP(num_query=8, reranking=True, **kw)
    feats, pids, camids = _labelled()
    with pytest.raises(L.CreidError):
        rm.R1_mAP(num_query=40, reranking=True).compute_chunked(torch.from_numpy(feats).cuda(), pids, camids)
    paths = [f"q{i}" for i in range(40)]
    for kw in (dict(streamed=True), dict(compute_dtype=torch.bfloat16), dict(compute_dtype=torch.float16),
               dict(distance_func="cosine")):
        with pytest.raises(L.CreidError):
            inf.get_similar(feats[:40], paths, feats[40:], np.arange(200), topk=5, reranking=True, **kw)
    with pytest.raises(L.CreidError):
        inf.get_similar(feats[:40], paths, feats[40:], np.arange(200), topk=5, reranking={"k3": 1})


def test_no_quadratic_allocation():
    """N = 16384: everything above the inputs, the output and the [nq, ng] distance matrix stays under half of an N x N fp32
    matrix (the chunked row maxima and the streamed top-k's candidate lists are bounded by 256 MiB each, one at a time)."""
    from centroids_reid_amd import reid_metric as rm
    N, nq, D = 16384, 2048, 16
    gen = torch.Generator(device="cuda").manual_seed(3)
    X = torch.randn((N, D), device="cuda", generator=gen)
    q, g = X[:nq].contiguous(), X[nq:].contiguous()
    del X
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    stats = {}
    out = rm.re_ranking(q, g, stats=stats)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base - 2 * nq * (N - nq) * 4
    print(f"peak above inputs, output and distance matrix: {extra / 2 ** 20:.1f} MiB; stats {stats}")
    assert out.shape == (nq, N - nq) and bool(torch.isfinite(out).all())
    assert extra < N * N * 4 // 2
    assert max(stats["temp_bytes"].values()) < N * N * 4 // 2
