"""GPU parity: the ranked lists of the evaluation protocol -- per query the first k gallery entries that are not junk (its pid
seen by its camera, or by a camera set that holds it), in distance order -- without the m x n matrix
(reid_metric.topk_stream(junk=...): creid_junk_mask_rows + creid_stream_topk_collect_keep[_h16] + creid_stream_topk_select) and
from ranked indices (reid_metric.rank_keep_topk: creid_rank_keep_topk), against the numpy reference of tests/ranked_ref.py on
the get_euclidean matrix of the same device tensors; then R1_mAP(ranked_topk=...), ModelBase.get_val_metrics with
TEST.VISUALIZE = "yes", and the C ABI."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ranked_ref as R

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _rm():
    from centroids_reid_amd import reid_metric as rm
    return rm


@pytest.fixture(params=["0", "1"], ids=["split-major", "equal-runs"])
def work_split(monkeypatch, request):
    """Both work splits of the streamed contraction (mode 0 = per-row slices, mode 1 = equal runs of 64-column units)."""
    monkeypatch.setenv("CREID_STREAM_BALANCE", request.param)
    return request.param


@functools.lru_cache(maxsize=None)
def _case(nq, ng, D, dup, camsets):
    return R.make_case(nq, ng, D, dup, camsets)


def _device(qh, gh, norm, dtype):
    """The rows of one dtype (16-bit: width padded to the kernels' 8-element chunks) and their norms."""
    rm = _rm()
    q, g = torch.from_numpy(qh).cuda(), torch.from_numpy(gh).cuda()
    if dtype != torch.float32:
        q, g = rm._pad_width(q, 8), rm._pad_width(g, 8)
    if norm:
        q, g = rm.l2_normalize(q, out_dtype=dtype), rm.l2_normalize(g, out_dtype=dtype)
    else:
        q, g = q.to(dtype), g.to(dtype)
    return q, g, rm.row_sqnorm(q), rm.row_sqnorm(g)


def _junk(labels, camsets):
    qp, qc, gp, gc = labels
    return _rm().JunkFilter(torch.from_numpy(qp).cuda(), torch.from_numpy(qc).cuda(), torch.from_numpy(gp).cuda(),
                            torch.from_numpy(gc).cuda(), camsets=camsets)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _assert_lists(idx, dist, ref):
    assert idx.dtype == torch.int64 and dist.dtype == torch.float32
    np.testing.assert_array_equal(idx.cpu().numpy(), ref[0])                       # indices and padding
    np.testing.assert_array_equal(_bits(dist.cpu().numpy()), _bits(ref[1]))        # bit for bit (+inf in the padding)


def _short_rows(labels, camsets, k):
    return int(((~R.junk_matrix(*labels, camsets)).sum(1) < k).sum())


@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("nq,ng,D,k,sample,dup", R.SHAPES)
def test_topk_stream_junk_equals_reference(nq, ng, D, k, sample, dup, dtype, work_split):
    """The shapes of test_topk_stream_equals_materialised_random (a 65th query row, a 4097th column, D % 16 != 0, D = 8,
    k = n), normalised and not, plain ids and camera sets: topk_stream(junk=...) == the numpy reference on the get_euclidean
    matrix of the same dtype (indices, padding, distance bits) == rank_keep_topk(rank_rows(d)); matched / count against the
    reference; the rows that needed the repair are exactly those with fewer than k non-junk entries (none in the first five
    shapes; 3 with plain ids and 5 with camera sets in the sixth, k = n = 40, which exercises padding and repair).  Counted on
    the CPU with this generator (float64 distances; normalised / not, plain ids then camera sets): largest candidate list
    395 / 397, 394 / 384 | 239 / 228, 249 / 226 | 203 / 240, 203 / 239 | 77 / 74, 80 / 75 | 984 / 911, 984 / 915 | 40, 39 -- far
    below the default capacity --, no infinite threshold outside the sixth shape; recounted on the device with the fp32 bits
    (max_candidates, printed per case): the same 24 figures."""
    rm = _rm()
    dt = DTYPES[dtype]
    for camsets in (False, True):
        qh, gh, *labels = _case(nq, ng, D, dup, camsets)
        junk = _junk(labels, camsets)
        short = _short_rows(labels, camsets, k)
        for norm in (True, False):
            q, g, qq, gg = _device(qh, gh, norm, dt)
            d = rm.get_euclidean(q, g, qq, gg)
            ref = R.ranked_ref(d.cpu().numpy(), *labels, k, camsets)
            stats = {}
            idx, dist = rm.topk_stream(q, g, k, qq, gg, sample=sample, stats=stats, junk=junk)
            print(f"{nq} x {ng} x {D} k={k} {dtype} camsets={camsets} norm={norm}: {stats} short={short}")
            _assert_lists(idx, dist, ref)
            assert stats["fallback_rows"] == short and stats["capacity"] == 4096 and stats["sample"] == sample
            assert stats["max_candidates"] <= 4096
            kidx, kmatched, kcount = rm.rank_keep_topk(rm.rank_rows(d), k, junk)
            assert kmatched.dtype == torch.bool and kcount.dtype == torch.int32
            np.testing.assert_array_equal(kidx.cpu().numpy(), ref[0])
            np.testing.assert_array_equal(kmatched.cpu().numpy(), ref[2])
            np.testing.assert_array_equal(kcount.cpu().numpy(), ref[3])
            np.testing.assert_array_equal(_bits(rm.gather_ranked(d, kidx).cpu().numpy()), _bits(ref[1]))
            np.testing.assert_array_equal(junk.matched(idx).cpu().numpy(), ref[2])
            assert int((ref[3] < k).sum()) == short


# rows whose filtered list is not their unfiltered one, counted on the CPU (float64 distances of the normalised rows, this
# generator): (nq, ng) -> (plain ids, camera sets)
CPU_DIFFER = {(300, 3000): (107, 125), (70, 513): (24, 41), (129, 1000): (42, 50), (33, 300): (13, 13), (65, 4097): (25, 29),
              (5, 40): (3, 5)}


@pytest.mark.parametrize("nq,ng,D,k,sample,dup", R.SHAPES)
def test_filter_is_exercised(nq, ng, D, k, sample, dup):
    """The filtered lists differ from the plain topk_stream lists in at least the rows the generator planted -- every even
    query that has junk sits 0.05 N(0, 1) from its first junk row, which is therefore rank 1 of its unfiltered list (planted
    rows, plain ids / camera sets: 105 / 121, 22 / 27, 41 / 48, 11 / 11, 24 / 26, 3 / 3; rows that differ, counted on the CPU in
    float64: 107 / 125, 24 / 41, 42 / 50, 13 / 13, 25 / 29, 3 / 5, and the same twelve counts on the device with the fp32 bits)
    -- and no returned index is junk."""
    rm = _rm()
    for camsets in (False, True):
        qh, gh, *labels = _case(nq, ng, D, dup, camsets)
        junk = _junk(labels, camsets)
        q, g, qq, gg = _device(qh, gh, True, torch.float32)
        idx = rm.topk_stream(q, g, k, qq, gg, sample=sample, junk=junk)[0].cpu().numpy()
        plain = rm.topk_stream(q, g, k, qq, gg, sample=sample)[0].cpu().numpy()
        differ = np.nonzero((idx != plain).any(1))[0]
        plant = R.planted(*labels, camsets)
        print(f"{nq} x {ng} camsets={camsets}: {len(differ)} rows differ, {len(plant)} planted")
        assert len(differ) >= CPU_DIFFER[(nq, ng)][int(camsets)]
        assert len(plant) >= 3 and np.isin(plant, differ).all()
        jm = R.junk_matrix(*labels, camsets)
        real = idx >= 0
        assert not jm[np.nonzero(real)[0], idx[real]].any()
        assert jm[np.arange(nq)[:, None], plain].any()                  # ... while the unfiltered lists do hold junk


@pytest.mark.parametrize("camsets", [False, True], ids=["ids", "camsets"])
def test_topk_stream_junk_overflow_is_repaired(camsets, work_split):
    """300 x 3000, k = 20, sample 256, capacity 64: every list overflows (the smallest holds more than 64 kept entries, as in
    test_topk_stream_overflow_is_detected_and_repaired), every row is redone through get_euclidean + rank_rows +
    rank_keep_topk and still equals the reference."""
    rm = _rm()
    qh, gh, *labels = _case(300, 3000, 256, True, camsets)
    q, g, qq, gg = _device(qh, gh, True, torch.float32)
    ref = R.ranked_ref(rm.get_euclidean(q, g, qq, gg).cpu().numpy(), *labels, 20, camsets)
    stats = {}
    idx, dist = rm.topk_stream(q, g, 20, qq, gg, sample=256, capacity=64, stats=stats, junk=_junk(labels, camsets))
    print(stats)
    _assert_lists(idx, dist, ref)
    assert stats["capacity"] == 64 and stats["fallback_rows"] == 300


def test_topk_stream_junk_massive_ties(work_split):
    """The case of test_topk_stream_massive_ties -- 5000 identical gallery rows, nearest to every query -- with every second of
    them (in gallery-index order) junk for every query: the kept ties come back in gallery-index order.  The threshold IS the
    tied distance, so a list holds the 2500 kept ties: inside the default capacity they are ordered by the select, with
    capacity 1024 every list overflows and the repair orders them."""
    rm = _rm()
    rng = np.random.default_rng(11)
    nq, ng, D, k = 40, 6000, 32, 10
    centre = rng.standard_normal(D).astype(np.float32)
    q = (centre + 0.01 * rng.standard_normal((nq, D))).astype(np.float32)
    g = (centre + 4.0 * rng.standard_normal((ng, D))).astype(np.float32)
    same = np.sort(rng.permutation(ng)[:5000])
    g[same] = centre
    g_pids = np.arange(1, ng + 1, dtype=np.int64)
    g_pids[same[::2]] = 0                                               # the queries' pid ...
    labels = (np.zeros(nq, np.int64), np.full(nq, 3, np.int64), g_pids, np.full(ng, 3, np.int64))     # ... and camera
    qd, gd = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    ref = R.ranked_ref(rm.get_euclidean(qd, gd).cpu().numpy(), *labels, k, False)
    np.testing.assert_array_equal(ref[0], same[1::2][None, :k].repeat(nq, 0))
    for capacity, repaired in ((None, 0), (1024, nq)):
        stats = {}
        idx, dist = rm.topk_stream(qd, gd, k, stats=stats, capacity=capacity, junk=_junk(labels, False))
        print(stats)
        assert stats["fallback_rows"] == repaired and stats["max_candidates"] == 2500
        _assert_lists(idx, dist, ref)


# ------------------------------------------------------------------------------------------ R1_mAP(ranked_topk=...)
def _eval_case(camsets):
    nq, ng = 70, 513
    qh, gh, qp, qc, gp, gc = _case(nq, ng, 104, False, camsets)     # (the materialised 16-bit kernels take D % 8 == 0 only)
    feats = torch.from_numpy(np.concatenate([qh, gh])).cuda()
    pids = np.concatenate([qp, gp])
    camids = R.camset_lists(qc, gc) if camsets else np.concatenate([qc, gc])
    return nq, feats, pids, camids, (qp, qc, gp, gc)


def _ranked_np(last):
    r = last["ranked"]
    assert sorted(r) == ["count", "distances", "indices", "matched"]
    assert r["indices"].dtype == torch.int64 and r["distances"].dtype == torch.float32
    assert r["matched"].dtype == torch.bool and r["count"].dtype == torch.int32
    return {key: v.cpu().numpy() for key, v in r.items()}


def _assert_same_ranked(a, b):
    for key in ("indices", "distances", "matched", "count"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def _assert_ranked_is_ref(r, ref):
    for key, want in zip(("indices", "distances", "matched", "count"), ref):
        np.testing.assert_array_equal(r[key], want, err_msg=key)


@pytest.mark.parametrize("camsets", [False, True], ids=["ids", "camsets"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_r1_map_ranked_topk_routes_agree(dtype, camsets, capsys):
    """streamed=True, streamed=False and compute_chunked give the same last["ranked"], array for array -- the reference
    applied to the materialised route's own distmat --, and the metrics of the same calls without the keyword."""
    rm = _rm()
    nq, feats, pids, camids, labels = _eval_case(camsets)
    kw = dict(num_query=nq, compute_dtype=DTYPES[dtype])
    mat = rm.R1_mAP(streamed=False, ranked_topk=10, **kw)
    res_mat = mat.compute(feats, pids, camids, respect_camids=camsets)
    want = _ranked_np(mat.last)
    _assert_ranked_is_ref(want, R.ranked_ref(mat.last["distmat"].cpu().numpy(), *labels, 10, camsets))
    assert want["indices"].shape == (nq, 10) and (want["count"] == 10).all()
    st = rm.R1_mAP(streamed=True, ranked_topk=10, **kw)
    res_st = st.compute(feats, pids, camids, respect_camids=camsets)
    assert "distmat" not in st.last and "indices" not in st.last
    _assert_same_ranked(_ranked_np(st.last), want)
    ch = rm.R1_mAP(streamed=False, ranked_topk=10, **kw)
    res_ch = ch.compute_chunked(feats, pids, camids, query_chunk=32, respect_camids=camsets)
    _assert_same_ranked(_ranked_np(ch.last), want)
    for streamed, got in ((False, res_mat), (True, res_st)):
        plain = rm.R1_mAP(streamed=streamed, **kw)
        ref = plain.compute(feats, pids, camids, respect_camids=camsets)
        assert "ranked" not in plain.last
        np.testing.assert_array_equal(got[0], ref[0]); assert got[1] == ref[1]; np.testing.assert_array_equal(got[2], ref[2])
    ref = rm.R1_mAP(streamed=False, **kw).compute_chunked(feats, pids, camids, query_chunk=32, respect_camids=camsets)
    np.testing.assert_array_equal(res_ch[0], ref[0]); assert res_ch[1] == ref[1]; np.testing.assert_array_equal(res_ch[2], ref[2])


def test_r1_map_ranked_topk_cosine_reranking_prefilter_and_clamp(capsys):
    """The cosine distance (compute and the query-chunk loop of compute_chunked) and reranking=True give the reference applied
    to their own distmat; prefilter= gives the lists of the plain streamed call; ranked_topk beyond the gallery is clamped."""
    rm = _rm()
    nq, feats, pids, camids, labels = _eval_case(False)
    cos = rm.R1_mAP(num_query=nq, dist_func="cosine", ranked_topk=10)
    res = cos.compute(feats, pids, camids)
    want = _ranked_np(cos.last)
    _assert_ranked_is_ref(want, R.ranked_ref(cos.last["distmat"].cpu().numpy(), *labels, 10, False))
    ref = rm.R1_mAP(num_query=nq, dist_func="cosine").compute(feats, pids, camids)
    np.testing.assert_array_equal(res[0], ref[0]); assert res[1] == ref[1]
    ch = rm.R1_mAP(num_query=nq, dist_func="cosine", ranked_topk=10)
    res_ch = ch.compute_chunked(feats, pids, camids, query_chunk=32)
    _assert_same_ranked(_ranked_np(ch.last), want)
    ref_ch = rm.R1_mAP(num_query=nq, dist_func="cosine").compute_chunked(feats, pids, camids, query_chunk=32)
    np.testing.assert_array_equal(res_ch[0], ref_ch[0]); assert res_ch[1] == ref_ch[1]
    rr = rm.R1_mAP(num_query=nq, reranking=True, ranked_topk=10)
    res = rr.compute(feats, pids, camids)
    _assert_ranked_is_ref(_ranked_np(rr.last), R.ranked_ref(rr.last["distmat"].cpu().numpy(), *labels, 10, False))
    assert res[1] == rm.R1_mAP(num_query=nq, reranking=True).compute(feats, pids, camids)[1]
    st = rm.R1_mAP(num_query=nq, streamed=True, ranked_topk=10)
    st.compute(feats, pids, camids)
    pf = rm.R1_mAP(num_query=nq, streamed=True, prefilter=torch.bfloat16, ranked_topk=10)
    pf.compute(feats, pids, camids)
    _assert_same_ranked(_ranked_np(pf.last), _ranked_np(st.last))
    # beyond the gallery: K' = n_gallery; every row is short by its junk entries, so every list ends in padding
    nqs, ngs = 5, 40
    qh, gh, qp, qc, gp, gc = _case(nqs, ngs, 32, False, False)
    f5, p5, c5 = torch.from_numpy(np.concatenate([qh, gh])).cuda(), np.concatenate([qp, gp]), np.concatenate([qc, gc])
    for streamed in (True, False):
        m = rm.R1_mAP(num_query=nqs, streamed=streamed, ranked_topk=1024)
        m.compute(f5, p5, c5)
        r = _ranked_np(m.last)
        assert r["indices"].shape == (nqs, ngs)
        dm = rm.R1_mAP(num_query=nqs, streamed=False)
        dm.compute(f5, p5, c5)
        _assert_ranked_is_ref(r, R.ranked_ref(dm.last["distmat"].cpu().numpy(), qp, qc, gp, gc, ngs, False))
        assert (r["count"] < ngs).sum() == 3 and (r["indices"][r["count"] < ngs, -1] == -1).all()


@pytest.mark.parametrize("camsets", [False, True], ids=["ids", "camsets"])
def test_get_val_metrics_visualize_keeps_the_lists(camsets, capsys):
    """TEST.VISUALIZE = "yes": last_ranked holds VISUALIZE_TOPK columns for the first min(num_query, VISUALIZE_MAX_NUMBER + 1)
    queries, equals the reference, and the metrics are those of the "no" run (which keeps no lists)."""
    rm = _rm()
    from centroids_reid_amd.bases import ModelBase
    from centroids_reid_amd.config import get_cfg_defaults
    nq, feats, pids, camids, labels = _eval_case(camsets)
    if camsets:
        camids = rm.CameraSets(camids, torch.from_numpy(labels[3]).cuda(), labels[1])
    cfg = get_cfg_defaults()
    cfg.num_query = nq
    cfg.MODEL.USE_CENTROIDS = cfg.MODEL.KEEP_CAMID_CENTROIDS = camsets
    h = SimpleNamespace(hparams=cfg, trainer=SimpleNamespace(logger=None, current_epoch=0), eval_prefilter=None)
    base = ModelBase.get_val_metrics(h, feats, pids, camids)
    assert not hasattr(h, "last_ranked") and "ranked" not in h.r1_map_func.last
    cfg.TEST.VISUALIZE, cfg.TEST.VISUALIZE_TOPK = "yes", 7
    out = ModelBase.get_val_metrics(h, feats, pids, camids)
    assert out == base
    f, sq = rm.l2_normalize(feats, return_sqnorm=True)                  # the rows and norms of R1_mAP
    d = rm.get_euclidean(f[:nq], f[nq:], sq[:nq].contiguous(), sq[nq:].contiguous()).cpu().numpy()
    ref = R.ranked_ref(d, *labels, 7, camsets)
    assert all(isinstance(v, np.ndarray) for v in h.last_ranked.values())
    _assert_ranked_is_ref(h.last_ranked, ref)
    assert h.last_ranked["indices"].shape == (nq, 7)
    cfg.TEST.VISUALIZE_MAX_NUMBER = 11                                   # utils/visrank.py:241 stops AFTER query 11
    assert ModelBase.get_val_metrics(h, feats, pids, camids) == base
    _assert_ranked_is_ref(h.last_ranked, [a[:12] for a in ref])
    assert h.last_ranked["count"].shape == (12,)


# ------------------------------------------------------------------------------------------ C ABI
def test_ranked_lists_abi_argument_checks():
    """creid_stream_topk_collect_keep / _h16, creid_rank_keep_topk and creid_junk_mask_rows refuse what the header rules out
    before any launch (CREID_E_ARG = -1, CREID_E_SHAPE = -4), and m == 0 is a no-op."""
    from centroids_reid_amd import _lib as L
    lib, st = L.lib(), L.stream()
    m, n, D, cap, k = 4, 128, 16, 64, 5
    q = torch.zeros((m, D), device="cuda"); g = torch.zeros((n, D), device="cuda")
    qh, gh = q.bfloat16(), g.bfloat16()
    qq = torch.zeros(m, device="cuda"); gg = torch.zeros(n, device="cuda"); tau = torch.zeros(m, device="cuda")
    qp = torch.zeros(m, dtype=torch.int64, device="cuda"); qc = torch.zeros(m, dtype=torch.int64, device="cuda")
    gp = torch.zeros(n, dtype=torch.int64, device="cuda"); gc = torch.ones(n, dtype=torch.int64, device="cuda")
    gc[::2] = 0                                                         # every second entry is junk for every query
    cand = torch.zeros((m, 8192), dtype=torch.int64, device="cuda")
    count = torch.zeros(m, dtype=torch.int32, device="cuda")
    ranked = torch.arange(n, device="cuda").repeat(m, 1)
    oidx = torch.full((m, 1024), -7, dtype=torch.int64, device="cuda")
    omat = torch.full((m, 1024), 9, dtype=torch.uint8, device="cuda")
    ocnt = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    dist = torch.zeros((m, n), device="cuda")
    P = L.ptr

    def collect(m_=m, D_=D, cap_=cap, q_=q, gc_=gc):
        return lib.creid_stream_topk_collect_keep(P(q_), P(g), P(qq), P(gg), m_, n, D_, P(tau), P(qp), P(gp), P(qc), P(gc_), 0, cap_,
                                                  P(cand), P(count), st)

    def collect_h16(m_=m, D_=D, cap_=cap, dt=L.BF16, qp_=qp):
        return lib.creid_stream_topk_collect_keep_h16(P(qh), P(gh), P(qq), P(gg), m_, n, D_, dt, P(tau), P(qp_), P(gp), P(qc), P(gc), 0,
                                                      cap_, P(cand), P(count), st)

    def keep(m_=m, k_=k, idx_=ranked, out_=oidx):
        return lib.creid_rank_keep_topk(P(idx_), m_, n, n, k_, P(qp), P(gp), P(qc), P(gc), 0, P(out_), P(omat), P(ocnt), st)

    def mask(m_=m, ld_=n, d_=dist):
        return lib.creid_junk_mask_rows(P(d_), m_, n, ld_, P(qp), P(gp), P(qc), P(gc), 0, st)
    E_ARG, E_SHAPE, E_DTYPE = -1, -4, -2
    for bad_cap in (96, 32, 16384, 0):
        assert collect(cap_=bad_cap) == E_SHAPE and collect_h16(cap_=bad_cap) == E_SHAPE
    assert collect(D_=18) == E_SHAPE and collect_h16(D_=12) == E_SHAPE
    assert collect_h16(dt=L.F32) == E_DTYPE
    assert collect(m_=-1) == E_ARG and collect_h16(m_=-1) == E_ARG
    assert collect(q_=None) == E_ARG and collect(gc_=None) == E_ARG and collect_h16(qp_=None) == E_ARG
    assert keep(k_=1025) == E_SHAPE and keep(k_=0) == E_ARG and keep(m_=-1) == E_ARG
    assert keep(idx_=None) == E_ARG and keep(out_=None) == E_ARG
    assert mask(ld_=n - 1) == E_ARG and mask(d_=None) == E_ARG and mask(m_=-1) == E_ARG
    assert lib.creid_stream_topk_collect_keep(None, None, None, None, 0, n, D, None, None, None, None, None, 0, cap, None, None,
                                              st) == 0
    assert lib.creid_stream_topk_collect_keep_h16(None, None, None, None, 0, n, D, L.BF16, None, None, None, None, None, 0, cap,
                                                  None, None, st) == 0
    assert lib.creid_rank_keep_topk(None, 0, n, n, k, None, None, None, None, 0, None, None, None, st) == 0
    assert lib.creid_junk_mask_rows(None, 0, n, n, None, None, None, None, 0, st) == 0
    torch.cuda.synchronize()
    assert int(count.sum()) == 0 and int(oidx.max()) == -7 and int(omat.min()) == 9 and int(ocnt.max()) == -7
    assert float(dist.abs().max()) == 0.0                               # nothing was launched
    # and the accepted calls: all-zero features, tau = 0 -> every NON-junk column (the odd ones) is a candidate
    assert collect() == 0 and keep() == 0 and mask() == 0
    torch.cuda.synchronize()
    assert count.tolist() == [n // 2] * m
    assert sorted((cand[0, :n // 2] & 0xffffffff).tolist()) == list(range(1, n, 2))
    got_idx, got_mat = oidx.flatten()[:m * k].view(m, k), omat.flatten()[:m * k].view(m, k)       # the outputs are [m][k], dense
    assert got_idx.tolist() == [[1, 3, 5, 7, 9]] * m and got_mat.tolist() == [[1] * k] * m and ocnt.tolist() == [k] * m
    assert int(oidx.flatten()[m * k:].max()) == -7                      # ... and nothing behind them was written
    assert torch.isinf(dist[:, ::2]).all() and float(dist[:, 1::2].abs().max()) == 0.0
    count.zero_()
    assert collect_h16() == 0
    torch.cuda.synchronize()
    assert count.tolist() == [n // 2] * m
