"""GPU parity: the open-set operating points (TAR @ FAR) -- reid_metric.distance_histogram / distance_histogram_matrix (one radix
pass over the distance keys, by class: creid_stream_dist_hist[_h16], creid_dist_hist_matrix), roc_stream / roc_matrix (three
passes and three select steps, creid_roc_descend), R1_mAP(roc=...) on every route and ModelBase(eval_roc=...) -- against the
numpy reference of tests/roc_ref.py on the get_euclidean matrix of the same device tensors (or on the route's own matrix).
Everything is integers and distance bits: every comparison is for equality."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ranked_ref as RR
import roc_ref as R

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SHAPES = [s[:3] + (s[5],) for s in RR.SHAPES[-5:]]       # nq, ng, D, dup: a 65th row, a 4097th column, D % 16 != 0, D = 8
FIELDS = ("target", "threshold", "false_accepts", "true_accepts", "n_impostor", "n_genuine", "far", "tar", "hist", "edges")


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
    return RR.make_case(nq, ng, D, dup, camsets)


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


def _assert_roc(got, ref, what=""):
    """Field for field; floats by their bits (nan == nan, -0 != +0)."""
    assert sorted(got) == sorted(FIELDS), sorted(got)
    for key in FIELDS:
        a, b = np.asarray(got[key]), np.asarray(ref[key])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, key, a.dtype, b.dtype, a.shape, b.shape)
        if a.dtype.kind == "f":
            a, b = a.view(f"u{a.dtype.itemsize}"), b.view(f"u{b.dtype.itemsize}")
        np.testing.assert_array_equal(a, b, err_msg=f"{what} {key}")


# ------------------------------------------------------------------------------------------ 1. histograms
@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("nq,ng,D,dup", SHAPES)
def test_histograms_equal_reference(nq, ng, D, dup, dtype, work_split):
    """distance_histogram == np.bincount of the keys of the get_euclidean matrix of the same device tensors, for the three
    passes (prefix bits, digit bits) = (0, 11), (11, 11), (22, 10); four selectors from the reference (the lowest and the most
    frequent impostor prefix, the lowest again, one no key has); plain ids and camera sets, normalised and not.  The class
    totals are the label counts; distance_histogram_matrix on that matrix gives the same integers; two calls over the two
    halves of the queries into one `out` equal one call."""
    rm = _rm()
    dt = DTYPES[dtype]
    for camsets in (False, True):
        qh, gh, *labels = _case(nq, ng, D, dup, camsets)
        junk = _junk(labels, camsets)
        jm = RR.junk_matrix(*labels, camsets)
        same = labels[2][None, :] == labels[0][:, None]
        for norm in (True, False):
            q, g, qq, gg = _device(qh, gh, norm, dt)
            d = rm.get_euclidean(q, g, qq, gg)
            gen, imp = R.class_keys(d.cpu().numpy(), *labels, camsets)
            assert len(gen) == (same & ~jm).sum() and len(imp) == (~same).sum() and len(gen) > 0
            for pb, bits in R.PASSES:
                prefix = R.probe_prefixes(imp, pb) if pb else None
                want = R.hist_of_keys(gen, imp, prefix, pb, bits)
                kw = dict(prefix=prefix, prefix_bits=pb, bits=bits)
                got = rm.distance_histogram(q, g, junk, qq, gg, **kw)
                assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (4 if pb else 1, 2, 1 << bits)
                what = f"{nq} x {ng} x {D} {dtype} camsets={camsets} norm={norm} pass=({pb}, {bits})"
                np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=what)
                if pb == 0:
                    assert want[0, 0].sum() == len(gen) and want[0, 1].sum() == len(imp)
                else:
                    assert want[3].sum() == 0 and want[0, 1].sum() > 0 and (want[0] == want[2]).all()
                np.testing.assert_array_equal(rm.distance_histogram_matrix(d, junk, **kw).cpu().numpy(), want, err_msg=what)
                h = nq // 2
                out = rm.distance_histogram(q[:h], g, junk.rows(slice(0, h)), qq[:h].contiguous(), gg, **kw)
                back = rm.distance_histogram(q[h:], g, junk.rows(slice(h, nq)), qq[h:].contiguous(), gg, out=out, **kw)
                assert back is out
                np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=what + " (two halves)")


def test_histogram_runs_repeat(work_split):
    """Integer atomics only: a second run gives the same integers (and both work splits the reference's, above)."""
    rm = _rm()
    qh, gh, *labels = _case(65, 4097, 64, False, False)
    q, g, qq, gg = _device(qh, gh, True, torch.float32)
    junk = _junk(labels, False)
    a = rm.distance_histogram(q, g, junk, qq, gg)
    b = rm.distance_histogram(q, g, junk, qq, gg)
    assert torch.equal(a, b) and int(a.sum()) == int((~RR.junk_matrix(*labels, False)).sum())


# ------------------------------------------------------------------------------------------ 2. operating points
@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("nq,ng,D,dup", SHAPES)
def test_operating_points_equal_reference(nq, ng, D, dup, dtype, work_split):
    """roc_stream and roc_matrix == the sort-based reference on the get_euclidean matrix of the same tensors, field for field,
    for the rates 1e-4 .. 1.0 (1.0: the clamp to N_imp - 1); plain ids and camera sets, normalised and not."""
    rm = _rm()
    dt = DTYPES[dtype]
    for camsets in (False, True):
        qh, gh, *labels = _case(nq, ng, D, dup, camsets)
        junk = _junk(labels, camsets)
        for norm in (True, False):
            q, g, qq, gg = _device(qh, gh, norm, dt)
            d = rm.get_euclidean(q, g, qq, gg)
            ref = R.roc_ref(d.cpu().numpy(), *labels, R.RATES, camsets)
            what = f"{nq} x {ng} x {D} {dtype} camsets={camsets} norm={norm}"
            assert ref["k"][-1] == ref["n_impostor"][0] - 1 and (ref["false_accepts"] <= ref["k"]).all()
            stats = {}
            _assert_roc(rm.roc_stream(q, g, junk, R.RATES, qq, gg, stats=stats), ref, what + " stream")
            assert stats == dict(passes=1 + 2 * 2, groups=2)               # five rates: two groups of up to four targets
            _assert_roc(rm.roc_matrix(d, junk, R.RATES), ref, what + " matrix")
    three = rm.roc_stream(q, g, junk, qq=qq, gg=gg, stats=stats)           # the default rates: one group, three passes
    assert stats == dict(passes=3, groups=1)
    np.testing.assert_array_equal(three["target"], [1e-4, 1e-3, 1e-2])
    for key in ("threshold", "false_accepts", "true_accepts"):
        np.testing.assert_array_equal(three[key], ref[key][:3])


# ------------------------------------------------------------------------------------------ 3. ties and the sign branch
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("nq,ng,D,dup", SHAPES)
def test_threshold_inside_a_run_of_ties(nq, ng, D, dup, dtype):
    """Integer features in [-2, 2] (exact in every dtype): squared distances are small integers and the threshold falls
    inside a run of equal keys, so FA < k for at least one target of every shape (asserted on the reference; the generator's
    seed base is the first under which the 5 x 40 shape, whose ranks are only 0, 0, 1, 15, 154, has a tie at one of them);
    at 5 x 40, N_imp = 155 and the rates 1e-4 and 1e-3 give k = 0."""
    rm = _rm()
    _, _, *labels = _case(nq, ng, D, dup, False)
    qh, gh = R.integer_features(nq, ng, D, 11000 + nq + ng)
    q, g, qq, gg = _device(qh, gh, False, DTYPES[dtype])
    d = rm.get_euclidean(q, g, qq, gg)
    dh = d.cpu().numpy()
    assert (dh == np.round(dh)).all()
    ref = R.roc_ref(dh, *labels, R.RATES)
    print(f"{nq} x {ng} x {D} {dtype}: k = {ref['k']}, FA = {ref['false_accepts']}, TA = {ref['true_accepts']}")
    assert (ref["false_accepts"] < ref["k"]).any() and (ref["false_accepts"] <= ref["k"]).all()
    if (nq, ng) == (5, 40):
        assert ref["n_impostor"][0] == 155 and (ref["k"][:2] == 0).all() and (ref["false_accepts"][:2] == 0).all()
    junk = _junk(labels, False)
    _assert_roc(rm.roc_stream(q, g, junk, R.RATES, qq, gg), ref, "stream")
    _assert_roc(rm.roc_matrix(d, junk, R.RATES), ref, "matrix")


SIGN_SHAPES = [s for s in SHAPES if s[0] >= 65]


@pytest.mark.parametrize("nq,ng,D,dup", SIGN_SHAPES)
def test_impostor_keys_on_both_sides_of_zero(nq, ng, D, dup):
    """Every fourth query is an exact copy of a gallery row of a DIFFERENT pid, then both sides are normalised: the impostor
    class holds squared distances that round to negative, zero and positive values, so impostor keys lie on both sides of
    0x80000000 (asserted on the device matrix) and the lowest operating points sit among them.  The three shapes with at least
    65 queries: the two smaller ones plant 9 and 2 copies, of which the numpy fp32 model sees none come out negative.  Planted
    pairs negative / zero / positive in the numpy fp32 model: 10 / 6 / 2, 15 / 8 / 18, 8 / 4 / 5; on the device matrix (printed):
    13 / 1 / 4, 13 / 6 / 22, 4 / 9 / 4: every shape has negative ones, so no un-normalised copies
    scaled by 3 were needed."""
    rm = _rm()
    qh, gh, *labels = _case(nq, ng, D, dup, False)
    qn, gn = R.plant_impostor_copies(qh, gh, labels[0], labels[2])
    q, g = torch.from_numpy(qn).cuda(), torch.from_numpy(gn).cuda()
    qq, gg = rm.row_sqnorm(q), rm.row_sqnorm(g)
    d = rm.get_euclidean(q, g, qq, gg)
    gen, imp = R.class_keys(d.cpu().numpy(), *labels)
    near = imp[(imp > 0x47ffffff) & (imp < 0xb8000000)]                    # |d| < 2^-15: the planted pairs
    neg, zero, pos = (near < 0x7fffffff).sum(), ((near == 0x7fffffff) | (near == 0x80000000)).sum(), (near > 0x80000000).sum()
    print(f"{nq} x {ng} x {D}: planted impostor pairs negative / zero / positive = {neg} / {zero} / {pos}")
    assert (imp < 0x80000000).any() and (imp > 0x80000000).any()
    junk = _junk(labels, False)
    ref = R.roc_ref(d.cpu().numpy(), *labels, R.RATES)
    _assert_roc(rm.roc_stream(q, g, junk, R.RATES, qq, gg), ref, "stream")
    _assert_roc(rm.roc_matrix(d, junk, R.RATES), ref, "matrix")
    pre = np.asarray([0x7fffffff >> 21, 0x80000000 >> 21, 0x7fffffff >> 21, 0], np.uint32)      # the two bins around zero
    np.testing.assert_array_equal(rm.distance_histogram(q, g, junk, qq, gg, prefix=pre, prefix_bits=11, bits=11).cpu().numpy(),
                                  R.hist_of_keys(gen, imp, pre, 11, 11))


def test_no_impostor_and_no_genuine():
    """Every gallery entry has its query's pid: CreidError (a false-accept rate is undefined).  No genuine pair: tar is nan."""
    rm = _rm()
    from centroids_reid_amd._lib import CreidError
    qh, gh = RR.make_features(5, 40, 32, False)
    q, g = torch.from_numpy(qh).cuda(), torch.from_numpy(gh).cuda()
    z5, z40 = np.zeros(5, np.int64), np.zeros(40, np.int64)
    with pytest.raises(CreidError, match="impostor"):
        rm.roc_stream(q, g, _junk((z5, z5, z40, z40 + 1), False))
    d = rm.get_euclidean(q, g)
    with pytest.raises(CreidError, match="impostor"):
        rm.roc_matrix(d, _junk((z5, z5, z40, z40 + 1), False))
    labels = (z5, z5, z40 + 1, z40)
    ref = R.roc_ref(d.cpu().numpy(), *labels, R.RATES)
    assert np.isnan(ref["tar"]).all() and ref["n_impostor"][0] == 200
    _assert_roc(rm.roc_stream(q, g, _junk(labels, False), R.RATES), ref)


# ------------------------------------------------------------------------------------------ 4. R1_mAP(roc=...)
def _eval_case(camsets):
    nq, ng = 70, 513
    qh, gh, qp, qc, gp, gc = _case(nq, ng, 104, False, camsets)     # (the materialised 16-bit kernels take D % 8 == 0 only)
    feats = torch.from_numpy(np.concatenate([qh, gh])).cuda()
    pids = np.concatenate([qp, gp])
    camids = RR.camset_lists(qc, gc) if camsets else np.concatenate([qc, gc])
    return nq, feats, pids, camids, (qp, qc, gp, gc)


def _same_metrics(a, b):
    np.testing.assert_array_equal(a[0], b[0]); assert a[1] == b[1]; np.testing.assert_array_equal(a[2], b[2])


@pytest.mark.parametrize("camsets", [False, True], ids=["ids", "camsets"])
@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
def test_r1_map_roc_streamed_and_materialised(dtype, camsets, capsys):
    """streamed=False: last["roc"] is the reference on its own distmat; streamed=True and compute_chunked (the streamed kernels:
    no matrix) give the same dict, which is the reference on the get_euclidean matrix of the rows in compute_dtype; the metrics
    are those of the same calls without the keyword, exactly, and those calls keep no "roc"."""
    rm = _rm()
    nq, feats, pids, camids, labels = _eval_case(camsets)
    kw = dict(num_query=nq, compute_dtype=DTYPES[dtype])
    mat = rm.R1_mAP(streamed=False, roc=R.RATES, **kw)
    res_mat = mat.compute(feats, pids, camids, respect_camids=camsets)
    ref = R.roc_ref(mat.last["distmat"].cpu().numpy(), *labels, R.RATES, camsets)
    _assert_roc(mat.last["roc"], ref, "streamed=False")
    st = rm.R1_mAP(streamed=True, roc=R.RATES, **kw)
    res_st = st.compute(feats, pids, camids, respect_camids=camsets)
    assert "distmat" not in st.last
    _assert_roc(st.last["roc"], ref, "streamed=True")
    ch = rm.R1_mAP(streamed=False, roc=R.RATES, **kw)
    res_ch = ch.compute_chunked(feats, pids, camids, query_chunk=32, respect_camids=camsets)
    _assert_roc(ch.last["roc"], ref, "compute_chunked")
    for streamed, got in ((False, res_mat), (True, res_st)):
        plain = rm.R1_mAP(streamed=streamed, **kw)
        _same_metrics(got, plain.compute(feats, pids, camids, respect_camids=camsets))
        assert "roc" not in plain.last
    _same_metrics(res_ch, rm.R1_mAP(streamed=False, **kw).compute_chunked(feats, pids, camids, query_chunk=32, respect_camids=camsets))
    if dtype == "fp32" and not camsets:
        default = rm.R1_mAP(streamed=True, roc=True, **kw)
        default.compute(feats, pids, camids)
        np.testing.assert_array_equal(default.last["roc"]["target"], [1e-4, 1e-3, 1e-2])
        np.testing.assert_array_equal(default.last["roc"]["threshold"], ref["threshold"][:3])


def test_r1_map_roc_cosine_reranking_expansion_prefilter(capsys):
    """Cosine (compute, and the query-chunk loop of compute_chunked, which counts the first pass chunk by chunk and forms the
    chunks' matrices again for the two later passes) and reranking=True: the reference on their own distmat.
    query_expansion=True, streamed or not: the reference on the materialised route's distmat of the expanded rows.
    prefilter=: the dict of the plain fp32 streamed call.  Every call returns the metrics of the call without the keyword."""
    rm = _rm()
    nq, feats, pids, camids, labels = _eval_case(False)
    cos = rm.R1_mAP(num_query=nq, dist_func="cosine", roc=R.RATES)
    res = cos.compute(feats, pids, camids)
    ref = R.roc_ref(cos.last["distmat"].cpu().numpy(), *labels, R.RATES)
    _assert_roc(cos.last["roc"], ref, "cosine")
    _same_metrics(res, rm.R1_mAP(num_query=nq, dist_func="cosine").compute(feats, pids, camids))
    ch = rm.R1_mAP(num_query=nq, dist_func="cosine", roc=R.RATES)
    res_ch = ch.compute_chunked(feats, pids, camids, query_chunk=32)
    _assert_roc(ch.last["roc"], ref, "cosine, chunked")
    plain_ch = rm.R1_mAP(num_query=nq, dist_func="cosine").compute_chunked(feats, pids, camids, query_chunk=32)
    np.testing.assert_array_equal(res_ch[0], plain_ch[0]); assert res_ch[1] == plain_ch[1]
    both = rm.R1_mAP(num_query=nq, dist_func="cosine", roc=R.RATES, ranked_topk=5)
    both.compute_chunked(feats, pids, camids, query_chunk=32)
    _assert_roc(both.last["roc"], ref, "cosine, chunked, with ranked_topk")
    assert both.last["ranked"]["indices"].shape == (nq, 5)
    rr = rm.R1_mAP(num_query=nq, reranking=True, roc=R.RATES)
    res = rr.compute(feats, pids, camids)
    _assert_roc(rr.last["roc"], R.roc_ref(rr.last["distmat"].cpu().numpy(), *labels, R.RATES), "reranking")
    _same_metrics(res, rm.R1_mAP(num_query=nq, reranking=True).compute(feats, pids, camids))
    qe_mat = rm.R1_mAP(num_query=nq, query_expansion=True, roc=R.RATES)
    res = qe_mat.compute(feats, pids, camids)
    ref_qe = R.roc_ref(qe_mat.last["distmat"].cpu().numpy(), *labels, R.RATES)
    _assert_roc(qe_mat.last["roc"], ref_qe, "query expansion")
    _same_metrics(res, rm.R1_mAP(num_query=nq, query_expansion=True).compute(feats, pids, camids))
    qe_st = rm.R1_mAP(num_query=nq, query_expansion=True, streamed=True, roc=R.RATES)
    res = qe_st.compute(feats, pids, camids)
    _assert_roc(qe_st.last["roc"], ref_qe, "query expansion, streamed")
    _same_metrics(res, rm.R1_mAP(num_query=nq, query_expansion=True, streamed=True).compute(feats, pids, camids))
    fp = rm.R1_mAP(num_query=nq, streamed=False)
    fp.compute(feats, pids, camids)
    ref_fp = R.roc_ref(fp.last["distmat"].cpu().numpy(), *labels, R.RATES)
    pf = rm.R1_mAP(num_query=nq, streamed=True, prefilter=torch.bfloat16, roc=R.RATES)
    res = pf.compute(feats, pids, camids)
    _assert_roc(pf.last["roc"], ref_fp, "prefilter")
    _same_metrics(res, rm.R1_mAP(num_query=nq, streamed=True, prefilter=torch.bfloat16).compute(feats, pids, camids))


@pytest.mark.parametrize("camsets", [False, True], ids=["ids", "camsets"])
def test_get_val_metrics_eval_roc_logs_the_operating_points(camsets, capsys):
    """Without eval_roc the logged dict has exactly today's keys; with it, TAR@FAR=<rate> and thr@FAR=<rate> per rate on top of
    the same values, last_roc keeps the dict (the reference on the matrix of R1_mAP's rows), and one line per rate is printed."""
    rm = _rm()
    from centroids_reid_amd.bases import ModelBase
    from centroids_reid_amd.config import get_cfg_defaults
    nq, feats, pids, camids, labels = _eval_case(camsets)
    if camsets:
        camids = rm.CameraSets(camids, torch.from_numpy(labels[3]).cuda(), labels[1])
    cfg = get_cfg_defaults()
    cfg.num_query = nq
    cfg.MODEL.USE_CENTROIDS = cfg.MODEL.KEEP_CAMID_CENTROIDS = camsets
    logged = []
    logger = SimpleNamespace(log_metrics=lambda data, step: logged.append(dict(data)))
    h = SimpleNamespace(hparams=cfg, trainer=SimpleNamespace(logger=logger, current_epoch=0), eval_prefilter=None)
    base = ModelBase.get_val_metrics(h, feats, pids, camids)
    assert sorted(base) == sorted(["mAP"] + [f"Top-{k}" for k in (1, 5, 10, 20, 50)]) and logged[-1] == base
    assert not hasattr(h, "last_roc")
    capsys.readouterr()
    h.eval_roc = (1e-3, 1e-2, 0.1)
    out = ModelBase.get_val_metrics(h, feats, pids, camids)
    printed = capsys.readouterr().out
    extra = [f"{name}@FAR={r}" for r in ("0.001", "0.01", "0.1") for name in ("TAR", "thr")]
    assert sorted(out) == sorted(list(base) + extra) and logged[-1] == out
    assert {k: out[k] for k in base} == base
    f, sq = rm.l2_normalize(feats, return_sqnorm=True)                  # the rows and norms of R1_mAP
    d = rm.get_euclidean(f[:nq], f[nq:], sq[:nq].contiguous(), sq[nq:].contiguous()).cpu().numpy()
    ref = R.roc_ref(d, *labels, (1e-3, 1e-2, 0.1), camsets)
    _assert_roc(h.last_roc, ref)
    for i, r in enumerate(("0.001", "0.01", "0.1")):
        assert out[f"TAR@FAR={r}"] == ref["tar"][i] and out[f"thr@FAR={r}"] == float(ref["threshold"][i])
        assert f"TAR@FAR={r}:" in printed


# ------------------------------------------------------------------------------------------ 5. memory
def test_roc_stream_allocates_no_matrix():
    """300 x 3000 x 256 (the matrix would be 3.6 MB): the peak of allocated device memory rises by less than 1 MiB across one
    roc_stream call -- three histograms of at most 4 x 2 x 2048 int64, the state, the prefixes, the rates."""
    rm = _rm()
    qh, gh, *labels = _case(300, 3000, 256, True, False)
    q, g, qq, gg = _device(qh, gh, True, torch.float32)
    junk = _junk(labels, False)
    rm.roc_stream(q[:64].contiguous(), g, junk.rows(slice(0, 64)), qq=qq[:64].contiguous(), gg=gg)      # (first-call set-up)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = rm.roc_stream(q, g, junk, qq=qq, gg=gg)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes")
    assert rise < (1 << 20)
    assert out["n_impostor"][0] + out["n_genuine"][0] == int((~RR.junk_matrix(*labels, False)).sum())
