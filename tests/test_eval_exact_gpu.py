"""GPU: the evaluation kernels against references that share nothing with them (tests/eval_exact.py).

Exact part: integer features below the exactness margin, so every distance, norm, rank, top-k prefix and per-query result must
EQUAL the int64 / stable-argsort / Market-1501 reference (the float64 AP and mAP within 1e-12: sums in another order).  No test
here compares one project kernel with another; tests/test_eval_exact_cpu.py proves that the inputs meet the margin and that the
mistakes the shapes are chosen for would change nearly every distance.

Bounded part: clustered and N(0, 1) features through the normalisation kernel, every output against fp64 on the operands the
kernel read, under bounds derived from the kernels' summation order (eval_exact's docstring), never fitted."""
import numpy as np
import pytest
import torch

import eval_exact as ee
from layer_audit import Audit

pytestmark = pytest.mark.gpu

TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MATRIX_DT = [(c.name, dt) for c in ee.MATRIX for dt in ee.DTYPES]
STREAM_DT = [(c.name, dt) for c in ee.STREAM for dt in ee.DTYPES]
_ids = lambda tab: [f"{n}-{d}" for n, d in tab]


@pytest.fixture(params=["0", "1"], ids=["split-major", "equal-runs"])
def work_split(monkeypatch, request):
    """both work splits of the streamed contractions (stream_split() in csrc/stream_common.hpp)"""
    monkeypatch.setenv("CREID_STREAM_BALANCE", request.param)
    return request.param


def _feats(ref):
    """[m + n, D] device features in the case's dtype (an exact cast: test_eval_exact_cpu) and the split"""
    f = torch.from_numpy(ref.feats).float().cuda().to(TORCH_DT[ref.dt])
    return f, f[:ref.case.m].contiguous(), f[ref.case.m:].contiguous()


def _eq(got, exp, what):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    exp = np.asarray(exp, np.float64)
    assert got.shape == exp.shape, what
    bad = got != exp
    if bad.any():
        i = np.unravel_index(int(np.flatnonzero(bad)[0]), bad.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ, first at {i}: got {got[i]!r}, expected {exp[i]!r}")


def _assert_per_query(ref, valid, ap, first):
    v = valid.cpu().numpy()
    np.testing.assert_array_equal(v == 1, ref.valid)
    assert set(np.unique(v).tolist()) <= {0, 1}
    np.testing.assert_array_equal(first.cpu().numpy()[ref.valid], ref.first[ref.valid])
    np.testing.assert_allclose(ap.cpu().numpy()[ref.valid], ref.ap[ref.valid], rtol=0, atol=1e-12)


def _assert_metric(ref, out):
    cmc, mAP, topk = out
    np.testing.assert_array_equal(cmc, ref.cmc)
    assert abs(mAP - ref.mAP) <= 1e-12
    np.testing.assert_array_equal(topk, ref.topk)


# ------------------------------------------------------------------------------------------------ materialised kernels
@pytest.mark.parametrize("name,dt", MATRIX_DT, ids=_ids(MATRIX_DT))
def test_row_sqnorm_equals_reference(name, dt):
    from centroids_reid_amd import reid_metric as rm
    ref = ee.reference(name, dt)
    _, q, g = _feats(ref)
    _eq(rm.row_sqnorm(q), ref.fnorm(ref.qq), "row_sqnorm(q)")
    _eq(rm.row_sqnorm(g), ref.fnorm(ref.gg), "row_sqnorm(g)")


@pytest.mark.parametrize("name,dt", MATRIX_DT, ids=_ids(MATRIX_DT))
def test_sqdist_matrix_equals_reference(name, dt):
    """the whole matrix, with the reference's norms handed in (the distance kernel alone) and with the norms computed inside"""
    from centroids_reid_amd import reid_metric as rm
    ref = ee.reference(name, dt)
    _, q, g = _feats(ref)
    qq = torch.from_numpy(ref.fnorm(ref.qq)).float().cuda()
    gg = torch.from_numpy(ref.fnorm(ref.gg)).float().cuda()
    _eq(rm.get_euclidean(q, g, qq, gg), ref.fdist, "creid_sqdist_matrix")
    _eq(rm.get_euclidean(q, g), ref.fdist, "get_euclidean")


@pytest.mark.parametrize("dt", ee.DTYPES)
def test_sqdist_matrix_row_pitch_beyond_n(dt):
    """ldo > n through the C ABI: the matrix lands at the pitch and the padding columns are not written"""
    from centroids_reid_amd import _lib as L
    ref = ee.reference("129x127", dt)
    _, q, g = _feats(ref)
    m, n, D = ref.case.m, ref.case.n, q.shape[1]
    qq = torch.from_numpy(ref.fnorm(ref.qq)).float().cuda()
    gg = torch.from_numpy(ref.fnorm(ref.gg)).float().cuda()
    ldo = n + 5
    out = torch.full((m, ldo), -7.0, device="cuda")
    L.check(L.lib().creid_sqdist_matrix(L.ptr(q), L.ptr(g), L.ptr(qq), L.ptr(gg), m, n, D, L.dtype_code(q), L.ptr(out), ldo,
                                        L.stream()), "creid_sqdist_matrix")
    _eq(out[:, :n], ref.fdist, "creid_sqdist_matrix, ldo = n + 5")
    assert bool((out[:, n:] == -7.0).all())


@pytest.mark.parametrize("name,dt", MATRIX_DT, ids=_ids(MATRIX_DT))
def test_topk_and_rank_eval_equal_reference(name, dt):
    """topk_rows and rank_rows_eval on the distance matrix: the prefix, the ranking and (valid, first, AP) of the reference"""
    from centroids_reid_amd import reid_metric as rm
    ref = ee.reference(name, dt)
    c, m = ref.case, ref.case.m
    _, q, g = _feats(ref)
    d = rm.get_euclidean(q, g)
    _eq(d, ref.fdist, "distance matrix")
    idx, dsel = rm.topk_rows(d, c.k)
    np.testing.assert_array_equal(idx.cpu().numpy(), ref.order[:, :c.k])
    _eq(dsel, np.take_along_axis(ref.fdist, ref.order[:, :c.k], 1), "topk_rows distances")
    order, valid, ap, first = rm.rank_rows_eval(d, *(a.copy() for a in (ref.pids[:m], ref.pids[m:], ref.cams[:m], ref.cams[m:])))
    np.testing.assert_array_equal(order.cpu().numpy(), ref.order)
    _assert_per_query(ref, valid, ap, first)


@pytest.mark.parametrize("name,dt", MATRIX_DT, ids=_ids(MATRIX_DT))
def test_r1_map_materialised_equals_reference(name, dt):
    from centroids_reid_amd import reid_metric as rm
    ref = ee.reference(name, dt)
    metric = rm.R1_mAP(num_query=ref.case.m, feat_norm=False, compute_dtype=TORCH_DT[dt])
    out = metric.compute(torch.from_numpy(ref.feats).float().cuda(), ref.pids.copy(), ref.cams.copy())
    _assert_metric(ref, out)
    _eq(metric.last["distmat"], ref.fdist, "last['distmat']")
    np.testing.assert_array_equal(metric.last["indices"].cpu().numpy(), ref.order)
    _assert_per_query(ref, metric.last["valid"], metric.last["ap"], metric.last["first"])
    vi = np.nonzero(ref.valid)[0]
    np.testing.assert_array_equal(metric.last["single_performance"][:, 0], vi)
    np.testing.assert_allclose(metric.last["single_performance"][:, 2], ref.ap[vi], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ streamed kernels
def _topk_stream(ref, **kw):
    from centroids_reid_amd import reid_metric as rm
    c = ref.case
    _, q, g = _feats(ref)
    stats = {}
    idx, dist = rm.topk_stream(q, g, c.k, sample=c.sample, stats=stats, **kw)
    print(f"{c.name} {ref.dt}: {stats}")
    np.testing.assert_array_equal(idx.cpu().numpy(), ref.order[:, :c.k])
    _eq(dist, np.take_along_axis(ref.fdist, ref.order[:, :c.k], 1), "topk_stream distances")
    assert idx.dtype == torch.int64 and dist.dtype == torch.float32
    return stats


@pytest.mark.parametrize("name,dt", STREAM_DT, ids=_ids(STREAM_DT))
def test_topk_stream_equals_reference(name, dt, work_split):
    """the streamed top-k itself produced the result: no row fell back, and the longest list the device collected is the one
    the reference counts by the same threshold rule (exact distances: the counts must agree to the entry)"""
    ref = ee.reference(name, dt)
    stats = _topk_stream(ref)
    assert stats["fallback_rows"] == 0 and stats["capacity"] == ee.STREAM_CAPACITY
    assert stats["max_candidates"] == int(ee.candidate_counts(ref).max())


@pytest.mark.parametrize("dt", ee.DTYPES)
def test_topk_stream_capacity_64_every_row_falls_back(dt, work_split):
    ref = ee.reference(ee.FALLBACK.name, dt)
    stats = _topk_stream(ref, capacity=ee.FALLBACK_CAPACITY)
    assert stats["capacity"] == ee.FALLBACK_CAPACITY and stats["fallback_rows"] == ref.case.m
    assert stats["max_candidates"] == int(ee.candidate_counts(ref).max())


def _streamed_eval(ref):
    from centroids_reid_amd import reid_metric as rm
    metric = rm.R1_mAP(num_query=ref.case.m, streamed=True, feat_norm=False, compute_dtype=TORCH_DT[ref.dt])
    out = metric.compute(torch.from_numpy(ref.feats).float().cuda(), ref.pids.copy(), ref.cams.copy())
    last = metric.last
    assert "distmat" not in last and "indices" not in last and "plan" in last
    _assert_metric(ref, out)
    _assert_per_query(ref, last["valid"], last["ap"], last["first"])
    np.testing.assert_array_equal(last["plan"].n_pos, ee.positive_counts(ref))
    return last["plan"]


@pytest.mark.parametrize("name,dt", STREAM_DT, ids=_ids(STREAM_DT))
def test_streamed_eval_equals_reference(name, dt, work_split):
    """per query, with an absent pid (query 0) and positives that all share the query's camera (query 1) in every labelled case"""
    ref = ee.reference(name, dt)
    plan = _streamed_eval(ref)
    assert len(plan.overflow) == 0
    if ref.case.labelled:
        assert not ref.valid[0] and not ref.valid[1]


@pytest.mark.parametrize("dt", ee.DTYPES)
def test_streamed_eval_overflow_queries(dt, work_split):
    """queries 4..7 have more than 128 positives: they leave through the general path, the others stay streamed"""
    ref = ee.reference(ee.OVERFLOW.name, dt)
    plan = _streamed_eval(ref)
    pos = ee.positive_counts(ref)
    fits = int(pos[pos <= ee.PL_MAX].max())
    assert plan.overflow.tolist() == [4, 5, 6, 7]
    assert fits <= plan.cap <= ee.PL_MAX and plan.cap & (plan.cap - 1) == 0         # the list holds every query that stayed


# ------------------------------------------------------------------------------------------------ bounded audit
AUDIT_M, AUDIT_N = 130, 300


@pytest.mark.parametrize("dt", ee.DTYPES)
@pytest.mark.parametrize("D", [2048, 104])
@pytest.mark.parametrize("kind", ["clustered", "normal"])
def test_audit_normalise_norms_distance(kind, D, dt):
    """l2_normalize -> the norms it returns -> row_sqnorm -> the distance matrix, each against fp64 on the operands the kernel
    read, under eval_exact's derived bounds (fp32 outputs: the relative-L2 bar is fed the bound itself, so the element-wise
    check is the binding one; 16-bit rows also get Audit's rounding-bias check)."""
    from centroids_reid_amd import reid_metric as rm
    tdt = TORCH_DT[dt]
    x = ee.audit_features(kind, AUDIT_M + AUDIT_N, D, seed=D + len(kind))
    a = Audit(f"eval {kind} D={D} {dt}")
    y, sq = rm.l2_normalize(x.cuda(), out_dtype=tdt, return_sqnorm=True)
    yc, sqc = y.cpu(), sq.cpu()
    yref, yb = ee.normalize_ref_bound(x)
    a.check("l2norm", "rows", yc, yref, yb, tdt, sigma=yb if dt == "fp32" else None)
    a.exact("l2norm", "zero row", bool((yc[7] == 0).all()) and float(sqc[7]) == 0.0)
    sref, sb = ee.sqnorm_ref_bound(yc, 4)
    a.check("l2norm", "returned sqnorm", sqc, sref, sb, torch.float32, sigma=sb)
    rref, rb = ee.sqnorm_ref_bound(yc, 1)
    a.check("row_sqnorm", "sqnorm", rm.row_sqnorm(y).cpu(), rref, rb, torch.float32, sigma=rb)
    d = rm.get_euclidean(y[:AUDIT_M], y[AUDIT_M:], sq[:AUDIT_M].contiguous(), sq[AUDIT_M:].contiguous()).cpu()
    dref, db = ee.dist_ref_bound(yc[:AUDIT_M], yc[AUDIT_M:], sqc[:AUDIT_M], sqc[AUDIT_M:])
    a.check("sqdist", "matrix", d, dref, db, torch.float32, sigma=db)
    print(a.table())
    print(a.op_summary())
    assert not a.failures, "\n".join(a.failures)


@pytest.mark.parametrize("dt", ee.DTYPES)
def test_audit_normalise_streamed_row(dt):
    """D = 4104: beyond the 4096 elements a wave keeps in registers, the normalisation reads its row twice"""
    from centroids_reid_amd import reid_metric as rm
    tdt = TORCH_DT[dt]
    x = ee.audit_features("normal", 9, 4104, seed=4104)
    a = Audit(f"eval wide {dt}")
    y, sq = rm.l2_normalize(x.cuda(), out_dtype=tdt, return_sqnorm=True)
    yref, yb = ee.normalize_ref_bound(x)
    a.check("l2norm", "rows", y.cpu(), yref, yb, tdt, sigma=yb if dt == "fp32" else None)
    a.exact("l2norm", "zero row", bool((y[7] == 0).all()) and float(sq[7]) == 0.0)
    sref, sb = ee.sqnorm_ref_bound(y.cpu(), 4)
    a.check("l2norm", "returned sqnorm", sq.cpu(), sref, sb, torch.float32, sigma=sb)
    print(a.table())
    assert not a.failures, "\n".join(a.failures)
