"""GPU parity: the streamed (matrix-free) evaluation with a bf16 / f16 compute dtype (csrc/stream_h16.hip) against the
MATERIALISED evaluation of the same dtype on the same device features (creid_sqdist_matrix + creid_rank_rows_eval): the
two run the same 16-bit MFMA in the same order, so ranks are identical and only the float64 AP sums differ in order."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]


def _both(feats, pids, cams, nq, dt, feat_norm=True):
    from centroids_reid_amd import reid_metric as rm
    f = feats.cuda()
    a = rm.R1_mAP(num_query=nq, feat_norm=feat_norm, compute_dtype=dt)
    ra = a.compute(f, pids, cams)
    b = rm.R1_mAP(num_query=nq, feat_norm=feat_norm, compute_dtype=dt, streamed=True)
    rb = b.compute(f, pids, cams)
    return a, ra, b, rb


def _per_query_from_indices(metric, pids, cams, nq):
    from centroids_reid_amd import reid_metric as rm
    _, _, _, _, valid, ap, first = rm.eval_func_device(metric.last["indices"], pids[:nq], pids[nq:], cams[:nq], cams[nq:], 50)
    return valid.cpu().numpy(), ap.cpu().numpy(), first.cpu().numpy()


def _assert_same(a, ra, b, rb, pids, cams, nq):
    # the streamed request really streamed (on a build without the 16-bit streamed kernels it silently materialises, and
    # everything below would compare the materialised path with itself)
    assert "distmat" not in b.last and "plan" in b.last
    assert "distmat" in a.last and a.last["distmat"].dtype == torch.float32
    v0, ap0, f0 = _per_query_from_indices(a, pids, cams, nq)
    v1, ap1, f1 = b.last["valid"].cpu().numpy(), b.last["ap"].cpu().numpy(), b.last["first"].cpu().numpy()
    np.testing.assert_array_equal(v1, v0)                       # bit-exact: same ranks on the same distance bits
    np.testing.assert_array_equal(f1, f0)
    np.testing.assert_allclose(ap1, ap0, rtol=0, atol=1e-12)    # float64 sums in a different order
    np.testing.assert_array_equal(rb[0], ra[0])                 # CMC curve
    assert abs(rb[1] - ra[1]) < 1e-12
    np.testing.assert_array_equal(rb[2], ra[2])
    np.testing.assert_allclose(b.last["single_performance"], a.last["single_performance"], rtol=0, atol=1e-12)


@pytest.fixture(params=["0", "1"], ids=["split-major", "equal-runs"])
def work_split(monkeypatch, request):
    """Both work splits of the counting contraction (stream_split(): mode 0 = per-row slices, mode 1 = equal runs of 64-column
    units that may cross query tiles); the default picks by gallery size."""
    monkeypatch.setenv("CREID_STREAM_BALANCE", request.param)
    return request.param


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", ["eval_small", "eval_d2048", "eval_tiny_gallery"])
def test_streamed_h16_equals_materialised_on_goldens(golden, name, dt, work_split):
    g = golden(name)
    nq = int(g["num_query"])
    feats = torch.from_numpy(g["feats"])
    for norm in (True, False):
        a, ra, b, rb = _both(feats, g["pids"], g["camids"], nq, dt, feat_norm=norm)
        _assert_same(a, ra, b, rb, g["pids"], g["camids"], nq)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nq,ng,D,npid,ncam,dup", [(300, 3000, 256, 60, 3, True), (70, 513, 104, 9, 2, False),
                                                    (129, 1000, 2048, 400, 5, True), (5, 40, 32, 3, 2, False),
                                                    (33, 300, 8, 5, 2, False), (64, 512, 48, 9, 2, False)])
def test_streamed_h16_equals_materialised_random(nq, ng, D, npid, ncam, dup, dt, work_split):
    """N(0,1) features (rounded to 16 bits: many exact ties), duplicated gallery rows (exact ties between a positive and a
    negative -> order by gallery index), a zero-distance positive, a query whose pid is absent from the gallery and one whose
    positives all share its camera; a second query tile, narrow last tiles, k-tiles with zero fill (104, 8, 48), D = 2048."""
    rng = np.random.default_rng(nq * 7 + ng)
    f = rng.standard_normal((nq + ng, D)).astype(np.float32)
    pids = rng.integers(0, npid, nq + ng)
    cams = rng.integers(0, ncam, nq + ng)
    if dup:
        src = rng.integers(nq, nq + ng, ng // 4); dst = rng.integers(nq, nq + ng, ng // 4)
        f[dst] = f[src]                                         # exact ties, possibly between a positive and a negative
        f[nq + 7] = f[3]; pids[nq + 7] = pids[3]; cams[nq + 7] = cams[3] + 1      # a zero-distance positive
    pids[0] = npid + 5                                          # pid absent from the gallery
    same = (pids[nq:] == pids[1])
    cams[nq:][same] = cams[1]                                   # every same-pid entry removed -> invalid query
    for norm in (True, False):
        a, ra, b, rb = _both(torch.from_numpy(f), pids, cams, nq, dt, feat_norm=norm)
        _assert_same(a, ra, b, rb, pids, cams, nq)
        assert b.last["valid"][0].item() == 0 and b.last["valid"][1].item() == 0


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_streamed_h16_overflow_rows_take_general_path(dt, work_split):
    """A pid with more than 128 positives does not fit the LDS list: those queries are routed through the 16-bit
    materialised kernels and merged; the rest stay streamed (100 positives: four MFMA blocks in the positives kernel)."""
    rng = np.random.default_rng(5)
    nq, ng, D = 40, 2000, 64
    f = rng.standard_normal((nq + ng, D)).astype(np.float32)
    pids = rng.integers(2, 30, nq + ng)
    pids[nq:nq + 400] = 0; pids[:6] = 0                         # 400 gallery entries of pid 0
    pids[nq + 400:nq + 500] = 1; pids[6:9] = 1                  # 100 of pid 1 (fits: cap 128)
    cams = rng.integers(0, 4, nq + ng)
    a, ra, b, rb = _both(torch.from_numpy(f), pids, cams, nq, dt)
    plan = b.last["plan"]
    assert set(plan.overflow.tolist()) == set(range(6)) and plan.cap == 128
    _assert_same(a, ra, b, rb, pids, cams, nq)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_compute_chunked_h16_streams(dt):
    """compute_chunked with a 16-bit compute dtype and the euclidean distance is the streamed evaluation (no query-chunk
    loop over distance tiles): the CMC curve and the top-k of compute(), mAP within the float64 summation order."""
    from centroids_reid_amd import reid_metric as rm
    rng = np.random.default_rng(12)
    nq, ng, D = 230, 1700, 128
    f = torch.from_numpy(rng.standard_normal((nq + ng, D)).astype(np.float32)).cuda()
    pids = rng.integers(0, 90, nq + ng); cams = rng.integers(0, 4, nq + ng)
    ref = rm.R1_mAP(num_query=nq, compute_dtype=dt).compute(f, pids, cams)
    m = rm.R1_mAP(num_query=nq, compute_dtype=dt)
    got = m.compute_chunked(f, pids, cams, query_chunk=100)
    assert "distmat" not in m.last and "plan" in m.last
    np.testing.assert_array_equal(got[0], ref[0])
    assert abs(got[1] - ref[1]) < 1e-12
    np.testing.assert_array_equal(got[2], ref[2])


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_streamed_h16_speculative_capacity(dt):
    """A second 16-bit streamed evaluation of the same shape takes the first one's capacity as a hint (no read-back in the
    middle of the pipeline) and returns the same numbers."""
    from centroids_reid_amd import reid_metric as rm
    rng = np.random.default_rng(77)
    nq, ng, D = 64, 1500, 96
    f = torch.from_numpy(rng.standard_normal((nq + ng, D)).astype(np.float32)).cuda()
    pids = rng.integers(0, 300, nq + ng); cams = rng.integers(0, 3, nq + ng)

    def run():
        m = rm.R1_mAP(num_query=nq, compute_dtype=dt, streamed=True)
        return m, m.compute(f, pids, cams)
    rm._CAP_HINT.clear()
    m0, r0 = run()                                        # synchronous: no hint yet
    assert rm._CAP_HINT[(nq, ng)] == m0.last["plan"].cap
    m1, r1 = run()                                        # speculative
    assert m1.last["plan"].cap == m0.last["plan"].cap
    np.testing.assert_array_equal(r1[0], r0[0]); assert r1[1] == r0[1]; np.testing.assert_array_equal(r1[2], r0[2])
    for k in ("valid", "ap", "first"):
        assert torch.equal(m1.last[k], m0.last[k]), k
    a = rm.R1_mAP(num_query=nq, compute_dtype=dt)
    ra = a.compute(f, pids, cams)
    _assert_same(a, ra, m1, r1, pids, cams, nq)
