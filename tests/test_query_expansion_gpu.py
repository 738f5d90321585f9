"""GPU: neighbour expansion (csrc/neighbour_expand.hip) and reid_metric.query_expansion against tests/qe_ref.py, and the plumbing
through R1_mAP and inference.get_similar.

Exact cases (integer rows, dyadic weights): torch.equal against qe_ref.exact_sums.  Bounded cases: per element
    |S - S_ref| <= (k + 2) 2^-24 sum_t |w_t u_tc|      ((k + 3) with self_rows: one more term in the chain)
-- at most one fp32 rounding of each weight, the gamma_k of a k-term fmaf chain, one unit of slack for second-order terms; the
reference is fed the device's own (idx, d), so the neighbour search is not part of the error.  Everything above the kernel is
held bit for bit to the composition of the public pieces it is defined as."""
import numpy as np
import pytest
import torch

import qe_ref as R

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
DYADIC_D = np.array([-0.5, 0, 0.5, 1, 1.5, 2, 2.5], np.float32)            # -> sim 1, 1, .75, .5, .25, 0, 0


def _rm():
    from centroids_reid_amd import reid_metric as rm
    return rm


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------ 1. the kernel, exact
@pytest.mark.parametrize("D", [4, 8, 68, 260, 2048, 2052])
def test_kernel_exact_on_integer_rows(D):
    rm = _rm()
    rng = np.random.default_rng(D)
    n_src = 37
    x = rng.integers(-8, 9, (n_src, D)).astype(np.float32)
    xd = _dev(x)
    for m in (1, 5, 67):
        own = rng.integers(-8, 9, (m, D)).astype(np.float32)
        for k in (1, 2, 7, 16):
            idx = rng.integers(0, n_src, (m, k)).astype(np.int64)
            if k >= 2:
                idx[:, -1] = idx[:, 0]                                        # a repeat inside every row
            junk = rng.standard_normal((m, k)).astype(np.float32) * 3
            junk.flat[::5] = np.nan
            junk.flat[1::7] = np.inf
            dyad = DYADIC_D[rng.integers(0, len(DYADIC_D), (m, k))]
            for self_rows in (None, own):
                sd = None if self_rows is None else _dev(self_rows)
                # (a) alpha = 0: weight 1 whatever the distance is
                got = rm.neighbour_expand(xd, _dev(idx), _dev(junk), 0.0, self_rows=sd)
                want = R.exact_sums(x, idx, np.ones((m, k)), self_rows)
                assert got.dtype == torch.float32 and got.shape == (m, D)
                assert torch.equal(got.cpu(), torch.from_numpy(want)), (D, m, k, "alpha0", self_rows is not None)
                # (b) alpha = 1 on dyadic similarities
                got = rm.neighbour_expand(xd, _dev(idx), _dev(dyad), 1.0, self_rows=sd)
                want = R.exact_sums(x, idx, R.sim_f32(dyad), self_rows)
                assert torch.equal(got.cpu(), torch.from_numpy(want)), (D, m, k, "alpha1", self_rows is not None)


@pytest.mark.parametrize("D", [8, 2052])
def test_kernel_k0_returns_self_rows_or_zeros(D):
    rm = _rm()
    x = _dev(np.ones((5, D), np.float32))
    own = _dev(np.arange(3 * D, dtype=np.float32).reshape(3, D) - 7)
    idx = torch.empty((3, 0), dtype=torch.int64, device="cuda")
    d = torch.empty((3, 0), dtype=torch.float32, device="cuda")
    for alpha in (0.0, 1.0, 3.0):
        assert torch.equal(rm.neighbour_expand(x, idx, d, alpha, self_rows=own), own)
        assert torch.equal(rm.neighbour_expand(x, idx, d, alpha), torch.zeros_like(own))


def test_kernel_more_than_one_batch_of_neighbours():
    """k > 64: the indices and weights of a row come in batches of 64 lanes; the chain still runs in the order of t."""
    rm = _rm()
    rng = np.random.default_rng(5)
    x = rng.integers(-8, 9, (37, 264)).astype(np.float32)
    for k in (64, 65, 131):
        idx = rng.integers(0, 37, (6, k)).astype(np.int64)
        dyad = DYADIC_D[rng.integers(0, len(DYADIC_D), (6, k))]
        got = rm.neighbour_expand(_dev(x), _dev(idx), _dev(dyad), 1.0)
        assert torch.equal(got.cpu(), torch.from_numpy(R.exact_sums(x, idx, R.sim_f32(dyad))))


# ------------------------------------------------------------------------------------------ 2. the wrapper's checks
def test_wrapper_refuses_bad_indices_and_arguments():
    rm = _rm()
    from centroids_reid_amd import _lib as L
    x = _dev(np.ones((9, 8), np.float32))
    d = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
    for bad in (-1, 9):
        idx = torch.zeros((4, 3), dtype=torch.int64, device="cuda")
        idx[2, 1] = bad
        with pytest.raises(L.CreidError, match="outside"):
            rm.neighbour_expand(x, idx, d, 3.0)
    idx = torch.zeros((4, 3), dtype=torch.int64, device="cuda")
    for kw in (dict(alpha=-1.0), dict(alpha=float("nan")), dict(alpha=float("inf"))):
        with pytest.raises(L.CreidError):
            rm.neighbour_expand(x, idx, d, kw["alpha"])
    with pytest.raises(L.CreidError):
        rm.neighbour_expand(x, idx.int(), d, 3.0)
    with pytest.raises(L.CreidError):
        rm.neighbour_expand(x, idx, d[:, :2].contiguous(), 3.0)
    with pytest.raises(L.CreidError):
        rm.neighbour_expand(x, idx, None, 3.0)
    with pytest.raises(L.CreidError):
        rm.neighbour_expand(x, idx, d, 3.0, self_rows=torch.zeros((4, 12), device="cuda"))
    # the C entry point's own limits
    out = torch.empty((4, 6), dtype=torch.float32, device="cuda")
    x6 = torch.ones((9, 6), dtype=torch.float32, device="cuda")
    rc = L.lib().creid_neighbour_expand(L.ptr(x6), 9, L.ptr(idx), L.ptr(d), None, 4, 3, 6, 3.0, L.ptr(out), L.stream())
    assert rc == -4                                                            # CREID_E_SHAPE: D % 4 != 0
    assert L.lib().creid_neighbour_expand(L.ptr(x), 9, L.ptr(idx), L.ptr(d), None, 0, 3, 8, 3.0, None, L.stream()) == 0
    assert L.lib().creid_neighbour_expand(L.ptr(x), 9, L.ptr(idx), L.ptr(d), None, 4, 3, 8, -1.0, L.ptr(out), L.stream()) == -1


# ------------------------------------------------------------------------------------------ 3. the kernel, bounded
@pytest.mark.parametrize("D", [64, 2048])
def test_kernel_within_the_chain_bound(D):
    rm = _rm()
    k, alpha, n, m = 10, 3.0, 300, 60
    U = R.clustered_unit_rows(n, D, 12, seed=D)
    Ud = rm.l2_normalize(_dev(U))
    U = Ud.cpu().numpy()
    idx, d = rm.topk_stream(Ud, Ud, k)
    got = rm.neighbour_expand(Ud, idx, d, alpha).cpu().numpy().astype(np.float64)
    ref, B = R.expand(U, idx.cpu().numpy(), d.cpu().numpy(), alpha)
    ratio = np.abs(got - ref) / np.maximum((k + 2) * U24 * B, 1e-300)
    print(f"D={D} all: max |S - S_ref| / bound = {ratio.max():.3f}")
    assert (np.abs(got - ref) <= (k + 2) * U24 * B).all()
    # the "query" composition: self rows first, then k - 1 rows of the others
    Uq, Ug = Ud[:m].contiguous(), Ud[m:].contiguous()
    idx, d = rm.topk_stream(Uq, Ug, k - 1)
    got = rm.neighbour_expand(Ug, idx, d, alpha, self_rows=Uq).cpu().numpy().astype(np.float64)
    ref, B = R.expand(U[m:], idx.cpu().numpy(), d.cpu().numpy(), alpha, self_rows=U[:m])
    ratio = np.abs(got - ref) / np.maximum((k - 1 + 3) * U24 * B, 1e-300)
    print(f"D={D} query: max |S - S_ref| / bound = {ratio.max():.3f}")
    assert (np.abs(got - ref) <= (k - 1 + 3) * U24 * B).all()


# ------------------------------------------------------------------------------------------ 4. reproducibility
def test_kernel_is_reproducible_and_independent_of_the_split():
    rm = _rm()
    U = rm.l2_normalize(_dev(R.clustered_unit_rows(203, 2048, 9, seed=3)))
    idx, d = rm.topk_stream(U, U, 7)
    a = rm.neighbour_expand(U, idx, d, 3.0)
    b = rm.neighbour_expand(U, idx, d, 3.0)
    assert torch.equal(a, b)
    for cut in (1, 66, 130):
        parts = [rm.neighbour_expand(U, idx[s].contiguous(), d[s].contiguous(), 3.0, self_rows=U[s].contiguous())
                 for s in (slice(0, cut), slice(cut, 203))]
        whole = rm.neighbour_expand(U, idx, d, 3.0, self_rows=U)
        assert torch.equal(torch.cat(parts), whole)


# ------------------------------------------------------------------------------------------ 5. query_expansion
def _features(nq, ng, D, seed):
    X = R.clustered_unit_rows(nq + ng, D, max(4, (nq + ng) // 10), seed=seed) * np.float32(1.7)      # (not unit: normalised inside)
    return _dev(X[:nq]), _dev(X[nq:])


@pytest.mark.parametrize("D", [64, 70, 2048])
def test_query_expansion_is_the_composition_of_its_pieces(D):
    rm = _rm()
    q, g = _features(48, 192, D, seed=11)
    nq = 48
    U = rm.l2_normalize(rm._pad_width(torch.cat([q, g])))
    for k, alpha in ((10, 3.0), (5, 0.0), (3, 1.0)):
        st = {}
        q2, g2 = rm.query_expansion(q, g, k=k, alpha=alpha, scope="all", stats=st)
        want = rm.l2_normalize(rm.neighbour_expand(U, *rm.topk_stream(U, U, k), alpha))[:, :D]
        assert q2.shape == q.shape and g2.shape == g.shape and q2.is_contiguous() and g2.is_contiguous()
        assert torch.equal(torch.cat([q2, g2]), want)
        assert st["fallback_rows"] == 0 and len(st["rounds_stats"]) == 1
        Uq, Ug = U[:nq].contiguous(), U[nq:].contiguous()
        q3, g3 = rm.query_expansion(q, g, k=k, alpha=alpha, scope="query")
        want = rm.l2_normalize(rm.neighbour_expand(Ug, *rm.topk_stream(Uq, Ug, k - 1), alpha, self_rows=Uq))[:, :D]
        assert torch.equal(q3, want) and torch.equal(g3, Ug[:, :D])
    q4, g4 = rm.query_expansion(q, g, k=1, scope="query")                     # no neighbours: the rows, normalised again
    assert torch.equal(q4, rm.l2_normalize(U[:nq].contiguous())[:, :D]) and torch.equal(g4, U[nq:, :D])


@pytest.mark.parametrize("scope", ["all", "query"])
def test_query_expansion_rounds_prefilter_and_outputs(scope):
    rm = _rm()
    q, g = _features(48, 192, 64, seed=12)
    o = dict(k=6, alpha=3.0, scope=scope)
    one = rm.query_expansion(q, g, **o)
    two = rm.query_expansion(q, g, rounds=2, **o)
    again = rm.query_expansion(*one, **o)
    assert torch.equal(two[0], again[0]) and torch.equal(two[1], again[1])
    assert not torch.equal(two[0], one[0])
    for pf in (torch.bfloat16, torch.float16):
        st = {"timing": True}
        got = rm.query_expansion(q, g, prefilter=pf, stats=st, **o)
        assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1])
        assert st["prefilter"] == pf and set(st["stage_ms"][0]) == {"normalise", "search", "expand"}
    # 16-bit rows: the last normalisation's output, rounded once, with the norms of the rounded rows
    for dt in (torch.bfloat16, torch.float16):
        qh, gh, qq, gg = rm.query_expansion(q, g, out_dtype=dt, return_sqnorm=True, **o)
        assert qh.dtype == gh.dtype == dt and qq.dtype == torch.float32 and qq.shape == (48,) and gg.shape == (192,)
        assert (qh.float() - one[0]).abs().max().item() <= 2.0 ** -8
        assert (torch.cat([qq, gg]) - 1).abs().max().item() < 2.0 ** -7
    from centroids_reid_amd import _lib as L
    for bad in (dict(k=241, scope="all"), dict(k=194, scope="query")):
        with pytest.raises(L.CreidError, match="outside"):
            rm.query_expansion(q, g, **bad)
    rm.query_expansion(q, g, k=193, scope="query")                            # k - 1 = ng is the limit


# ------------------------------------------------------------------------------------------ 6. R1_mAP
def _labels(nq, ng, seed, n_pid=24, n_cam=4):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n_pid, nq + ng), rng.integers(0, n_cam, nq + ng)


def _assert_same_eval(a, ra, b, rb, ap_tol=0.0):
    np.testing.assert_array_equal(ra[0], rb[0])
    np.testing.assert_array_equal(ra[2], rb[2])
    assert torch.equal(a.last["valid"], b.last["valid"]) and torch.equal(a.last["first"], b.last["first"])
    if ap_tol:
        assert abs(ra[1] - rb[1]) <= ap_tol and (a.last["ap"] - b.last["ap"]).abs().max().item() <= ap_tol
    else:
        assert ra[1] == rb[1] and torch.equal(a.last["ap"], b.last["ap"])


@pytest.mark.parametrize("D,opts", [(64, dict(k=5, alpha=3.0)), (64, dict(k=4, scope="query", rounds=2)), (70, True),
                                    (2048, dict(k=10))], ids=["d64-all", "d64-query-r2", "d70-default", "d2048"])
def test_r1_map_equals_evaluation_of_the_expanded_rows(D, opts):
    rm = _rm()
    nq, ng = 48, 192
    q, g = _features(nq, ng, D, seed=21)
    X = torch.cat([q, g])
    pids, cams = _labels(nq, ng, 1)
    o = rm.expansion_options(opts)
    Xe = torch.cat(rm.query_expansion(q, g, **o))
    for streamed in (False, True):
        a = rm.R1_mAP(num_query=nq, streamed=streamed, query_expansion=opts)
        b = rm.R1_mAP(num_query=nq, streamed=streamed, feat_norm=False)
        ra, rb = a.compute(X, pids, cams), b.compute(Xe, pids, cams)
        _assert_same_eval(a, ra, b, rb)
        if not streamed:
            assert torch.equal(a.last["distmat"][:, :ng], b.last["distmat"])
        info = a.last["query_expansion"]
        assert {k: info[k] for k in o} == o and info["fallback_rows"] == 0 and "query_expansion" not in b.last
    c = rm.R1_mAP(num_query=nq, query_expansion=opts)
    rc = c.compute_chunked(X, pids, cams)
    _assert_same_eval(a, ra, c, rc)
    assert "distmat" not in c.last and c.last["query_expansion"]["k"] == o["k"]


def test_r1_map_expansion_composes_with_reranking_prefilter_and_cosine():
    rm = _rm()
    nq, ng = 48, 192
    q, g = _features(nq, ng, 64, seed=22)
    X = torch.cat([q, g])
    pids, cams = _labels(nq, ng, 2)
    o = dict(k=5, alpha=3.0)
    q2, g2 = rm.query_expansion(q, g, **o)
    rr = dict(k1=8, k2=3, lambda_value=0.3)
    a = rm.R1_mAP(num_query=nq, reranking=rr, query_expansion=o)
    a.compute(X, pids, cams)
    assert torch.equal(a.last["distmat"], rm.re_ranking(q2, g2, **rr))         # expansion first, then re-ranking
    plain = rm.R1_mAP(num_query=nq, streamed=True, query_expansion=o)
    rp = plain.compute(X, pids, cams)
    for pf in (torch.bfloat16, torch.float16):                                  # the expansion's search and the count pre-filtered
        b = rm.R1_mAP(num_query=nq, streamed=True, prefilter=pf, query_expansion=o)
        b.last = {"query_expansion": {"timing": True}}
        rb = b.compute(X, pids, cams)
        _assert_same_eval(plain, rp, b, rb, ap_tol=1e-12)
        assert b.last["query_expansion"]["prefilter"] == pf and len(b.last["query_expansion"]["stage_ms"]) == 1
    for streamed in (False, True):
        c = rm.R1_mAP(num_query=nq, dist_func="cosine", streamed=streamed, query_expansion=o)
        d = rm.R1_mAP(num_query=nq, dist_func="cosine", streamed=streamed, feat_norm=False)
        rc, rd = c.compute(X, pids, cams), d.compute(torch.cat([q2, g2]), pids, cams)
        _assert_same_eval(c, rc, d, rd)
        assert torch.equal(c.last["distmat"], d.last["distmat"])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_r1_map_expansion_16bit_streamed_equals_materialised(dtype):
    rm = _rm()
    nq, ng = 48, 192
    q, g = _features(nq, ng, 64, seed=23)
    X = torch.cat([q, g])
    pids, cams = _labels(nq, ng, 3)
    o = dict(k=5, alpha=3.0)
    mat = rm.R1_mAP(num_query=nq, compute_dtype=dtype, query_expansion=o)
    st = rm.R1_mAP(num_query=nq, compute_dtype=dtype, streamed=True, query_expansion=o)
    rmat, rst = mat.compute(X, pids, cams), st.compute(X, pids, cams)
    assert "distmat" in mat.last and "distmat" not in st.last
    _assert_same_eval(mat, rmat, st, rst, ap_tol=1e-12)
    fp = rm.R1_mAP(num_query=nq, query_expansion=o).compute(X, pids, cams)
    assert abs(fp[1] - rst[1]) < 0.05                                           # the same evaluation, on rows rounded once


def test_r1_map_expansion_with_camera_sets():
    """respect_camids=True on camera-set labels shaped like tests/golden/eval_camsets.npz's (one camera per query, a set of 1-4 of 8
    cameras per gallery entry): the streamed evaluation of the expanded rows equals the materialised one."""
    rm = _rm()
    nq, ng = 48, 192
    q, g = _features(nq, ng, 64, seed=24)
    X = torch.cat([q, g])
    rng = np.random.default_rng(24)
    pids = rng.integers(0, 24, nq + ng)
    camsets = [[int(c)] for c in rng.integers(0, 8, nq)] + [sorted(set(rng.integers(0, 8, rng.integers(1, 5)).tolist()))
                                                            for _ in range(ng)]
    o = dict(k=5, alpha=3.0)
    mat = rm.R1_mAP(num_query=nq, query_expansion=o)
    st = rm.R1_mAP(num_query=nq, streamed=True, query_expansion=o)
    rmat = mat.compute(X, pids, camsets, respect_camids=True)
    rst = st.compute(X, pids, camsets, respect_camids=True)
    _, _, _, _, valid, ap, first = rm.eval_func_device(mat.last["indices"], pids[:nq], pids[nq:], camsets[:nq], camsets[nq:],
                                                       camsets=True)
    assert torch.equal(valid, st.last["valid"]) and torch.equal(first, st.last["first"])
    assert (ap - st.last["ap"]).abs().max().item() <= 1e-12
    np.testing.assert_array_equal(rmat[0], rst[0])
    np.testing.assert_array_equal(rmat[2], rst[2])
    assert abs(rmat[1] - rst[1]) <= 1e-12
    assert mat.last["query_expansion"]["k"] == 5 and st.last["plan"].camsets
    plain = rm.R1_mAP(num_query=nq, streamed=True).compute(X, pids, camsets, respect_camids=True)
    assert plain[1] != rst[1]                                                   # the expansion took part


def test_model_base_hands_the_keyword_to_r1_map(capsys):
    """ModelBase(eval_query_expansion=...) -> get_val_metrics -> R1_mAP(query_expansion=...)."""
    from types import SimpleNamespace
    rm = _rm()
    from centroids_reid_amd.bases import ModelBase
    from centroids_reid_amd.config import get_cfg_defaults
    nq, ng = 48, 192
    q, g = _features(nq, ng, 64, seed=25)
    X = torch.cat([q, g])
    pids, cams = _labels(nq, ng, 5)
    cfg = get_cfg_defaults()
    cfg.num_query = nq
    o = dict(k=5, alpha=3.0, scope="query")
    h = SimpleNamespace(hparams=cfg, trainer=SimpleNamespace(logger=None, current_epoch=0), eval_prefilter=None,
                        eval_query_expansion=o)
    out = ModelBase.get_val_metrics(h, X, pids, cams)
    want = rm.R1_mAP(num_query=nq, streamed=True, query_expansion=o).compute(X, pids, cams)
    assert out["mAP"] == want[1] and h.r1_map_func.last["query_expansion"]["scope"] == "query"
    h.eval_query_expansion = None
    assert ModelBase.get_val_metrics(h, X, pids, cams)["mAP"] == rm.R1_mAP(num_query=nq, streamed=True).compute(X, pids, cams)[1]
    assert "query_expansion" not in h.r1_map_func.last


# ------------------------------------------------------------------------------------------ 7. get_similar
@pytest.mark.parametrize("opts", [dict(k=5, alpha=3.0), dict(k=4, scope="query")], ids=["all", "query"])
def test_get_similar_equals_search_on_the_expanded_rows(opts):
    rm = _rm()
    from centroids_reid_amd import inference
    nq, ng = 23, 160
    q, g = _features(nq, ng, 64, seed=31)
    qp, gp = [f"q{i}" for i in range(nq)], [f"g{i}" for i in range(ng)]
    q2, g2 = rm.query_expansion(q, g, **rm.expansion_options(opts))
    for kw, path in ((dict(streamed=False, topk=5), "materialised"), (dict(streamed=False, topk=0), "materialised"),
                     (dict(streamed=True, topk=5), "streamed"), (dict(streamed=True, topk=5, prefilter=torch.bfloat16), "streamed"),
                     (dict(topk=5, reranking=dict(k1=6, k2=3)), "reranked")):
        sa, sb = {}, {}
        a = inference.get_similar(q, qp, g, gp, query_expansion=opts, stats=sa, **kw)
        b = inference.get_similar(q2, qp, g2, gp, normalize_features=False, stats=sb, **kw)
        assert sa["path"] == sb["path"] == path
        assert sa["query_expansion"]["k"] == opts["k"] and "query_expansion" not in sb
        for name in qp:
            np.testing.assert_array_equal(a[name]["indices"], b[name]["indices"])
            np.testing.assert_array_equal(a[name]["distances"].view(np.uint32), b[name]["distances"].view(np.uint32))


def test_get_similar_expansion_on_the_chunked_path(monkeypatch):
    rm = _rm()
    from centroids_reid_amd import inference
    nq, ng = 23, 160
    q, g = _features(nq, ng, 64, seed=32)
    qp, gp = [f"q{i}" for i in range(nq)], [f"g{i}" for i in range(ng)]
    q2, g2 = rm.query_expansion(q, g, k=5)
    monkeypatch.setattr(inference, "STREAM_MATRIX_BYTES", 7 * ng * 4)          # 7 query rows at a time; topk = 0 cannot stream
    sa = {}
    a = inference.get_similar(q, qp, g, gp, query_expansion=dict(k=5), stats=sa)
    b = inference.get_similar(q2, qp, g2, gp, normalize_features=False, streamed=False)
    assert sa["path"] == "chunked"
    for name in qp:
        np.testing.assert_array_equal(a[name]["indices"], b[name]["indices"])
        np.testing.assert_array_equal(a[name]["distances"].view(np.uint32), b[name]["distances"].view(np.uint32))


# ------------------------------------------------------------------------------------------ 8. quality
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_expansion_improves_map_on_the_device(seed):
    rm = _rm()
    q, g, qp, gp, qc, gc = R.quality_set(seed)
    X = _dev(np.concatenate([q, g]).astype(np.float32))
    pids, cams = np.concatenate([qp, gp]), np.concatenate([qc, gc])
    nq = len(q)
    base = rm.R1_mAP(num_query=nq).compute(X, pids, cams)[1]
    both = rm.R1_mAP(num_query=nq, query_expansion=dict(k=5, alpha=3)).compute(X, pids, cams)[1]
    aqe = rm.R1_mAP(num_query=nq, query_expansion=dict(k=5, alpha=3, scope="query")).compute(X, pids, cams)[1]
    print(f"seed {seed}: mAP none {base:.4f}  all {both:.4f} ({both - base:+.4f})  query {aqe:.4f} ({aqe - base:+.4f})")
    assert both >= base + 0.05
    assert aqe >= base + 0.02
