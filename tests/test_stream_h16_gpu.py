"""GPU parity: stream top-k on bf16 / f16 features (reid_metric.topk_stream -> creid_stream_topk_collect_h16 in
csrc/stream_h16.hip + creid_stream_topk_select) against the MATERIALISED path of the same dtype on the same device tensors,
rm.topk_rows(rm.get_euclidean(q16, g16, qq, gg), k): the same indices and the same distance bits, ties by gallery index --
through the Python surface, inference.get_similar(compute_dtype=...) and the C ABI."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]


@pytest.fixture(params=["0", "1"], ids=["split-major", "equal-runs"])
def work_split(monkeypatch, request):
    """Both work splits of the streamed contraction (stream_split(): mode 0 = per-row slices, mode 1 = equal runs of 64-column
    units that may cross query tiles); the default picks by gallery size."""
    monkeypatch.setenv("CREID_STREAM_BALANCE", request.param)
    return request.param


def make_features(nq, ng, D, dup, seed=None):
    """N(0,1) queries and gallery; dup: a quarter of the gallery rows copied over others (exact ties, ordered by gallery
    index).  (Rounded to 16 bits the near-ties of the fp32 features become many exact ties.)"""
    rng = np.random.default_rng(nq * 7 + ng if seed is None else seed)
    q = rng.standard_normal((nq, D)).astype(np.float32)
    g = rng.standard_normal((ng, D)).astype(np.float32)
    if dup:
        src = rng.integers(0, ng, ng // 4); dst = rng.integers(0, ng, ng // 4)
        g[dst] = g[src]
    return q, g


def _device(q, g, norm, dt):
    """The 16-bit device tensors and their norms, as R1_mAP / get_similar produce them: normalised rows are rounded by the
    normalisation kernel, un-normalised ones by a cast."""
    from centroids_reid_amd import reid_metric as rm
    q, g = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    if norm:
        q, g = rm.l2_normalize(q, out_dtype=dt), rm.l2_normalize(g, out_dtype=dt)
    else:
        q, g = q.to(dt), g.to(dt)
    return q, g, rm.row_sqnorm(q), rm.row_sqnorm(g)


def _reference(q, g, qq, gg, k):
    from centroids_reid_amd import reid_metric as rm
    assert q.dtype in DTYPES and g.dtype == q.dtype
    return rm.topk_rows(rm.get_euclidean(q, g, qq, gg), k)


def _assert_equal(got, ref):
    np.testing.assert_array_equal(got[0].cpu().numpy(), ref[0].cpu().numpy())
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32
    np.testing.assert_array_equal(got[1].cpu().numpy().view(np.int32), ref[1].cpu().numpy().view(np.int32))     # bit-exact


PARITY = [(300, 3000, 256, 20, 256, True), (70, 513, 104, 50, 128, False), (129, 1000, 2048, 7, 64, True),
          (33, 300, 8, 5, 32, False), (65, 4097, 64, 100, 512, False), (5, 40, 32, 40, 40, False)]


def _parity(nq, ng, D, k, sample, dup, dt, seed=None):
    from centroids_reid_amd import reid_metric as rm
    qh, gh = make_features(nq, ng, D, dup, seed)
    for norm in (True, False):
        q, g, qq, gg = _device(qh, gh, norm, dt)
        ref = _reference(q, g, qq, gg, k)
        stats = {}
        got = rm.topk_stream(q, g, k, qq, gg, sample=sample, stats=stats)
        print(f"{dt} {nq} x {ng} x {D} k={k} norm={norm}: {stats}")
        _assert_equal(got, ref)
        assert stats["fallback_rows"] == 0 and stats["capacity"] == 4096 and stats["sample"] == sample
        assert k <= stats["max_candidates"] <= 4096
        _assert_equal(rm.topk_stream(q, g, k, sample=sample), ref)           # norms computed inside


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nq,ng,D,k,sample,dup", PARITY)
def test_topk_stream_h16_equals_materialised_random(nq, ng, D, k, sample, dup, dt, work_split):
    """A 65th query row (second query tile), a 4097th column (a one-unit narrow tile with column masking), D = 104 = 64 + 40 (a
    k-tile with zero fill), D = 8 (below one k-tile), D = 2048, k = n; `sample` is forced small, so the threshold is loose and
    the candidate lists are real supersets.  Largest list per case, counted on the CPU (features rounded to the dtype,
    distances in fp64 cast to fp32, the same stride sample): 390 / 241 / 208 / 77 / 983 / 40 (bf16) and 394 / 241 / 204 / 77 /
    984 / 40 (f16) normalised, 383 / 271 / 240 / 75 / 900 / 40 and 391 / 272 / 240 / 75 / 909 / 40 un-normalised -- far below the
    default capacity, so no row may need the repair (a device count may differ by a few: the assertions are the bounds)."""
    _parity(nq, ng, D, k, sample, dup, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", [2032, 2048])
def test_topk_stream_h16_adjacent_widths(D, dt, work_split):
    """Two shapes that differ by exactly one 16-deep step (2032 = 31 k-tiles + three steps; 2048 = 32 k-tiles): a k-loop
    that drops or repeats its last step fails one of them."""
    _parity(70, 600, D, 10, 128, False, dt, seed=2032)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_topk_stream_h16_overflow_is_detected_and_repaired(dt, work_split):
    """300 x 3000, k = 20, sample 256, capacity 64: the shortest list counted on the CPU holds 98 entries, so every row
    overflows, is flagged and is redone through the 16-bit materialised kernels."""
    from centroids_reid_amd import reid_metric as rm
    qh, gh = make_features(300, 3000, 256, True)
    q, g, qq, gg = _device(qh, gh, True, dt)
    ref = _reference(q, g, qq, gg, 20)
    stats = {}
    got = rm.topk_stream(q, g, 20, qq, gg, sample=256, capacity=64, stats=stats)
    print(stats)
    _assert_equal(got, ref)
    assert stats["capacity"] == 64 and stats["fallback_rows"] == 300


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_topk_stream_h16_massive_ties(dt, work_split):
    """5000 identical gallery rows, nearest to every query: the threshold IS the tied distance, every list overflows the
    capacity, and the repaired rows order the ties by gallery index like the stable rank."""
    from centroids_reid_amd import reid_metric as rm
    rng = np.random.default_rng(11)
    nq, ng, D, k = 40, 6000, 32, 10
    centre = rng.standard_normal(D).astype(np.float32)
    q = (centre + 0.01 * rng.standard_normal((nq, D))).astype(np.float32)
    g = (centre + 4.0 * rng.standard_normal((ng, D))).astype(np.float32)
    same = rng.permutation(ng)[:5000]
    g[same] = centre
    qd, gd = torch.from_numpy(q).cuda().to(dt), torch.from_numpy(g).cuda().to(dt)
    stats = {}
    idx, dist = rm.topk_stream(qd, gd, k, stats=stats)
    print(stats)
    assert stats["fallback_rows"] == nq and stats["max_candidates"] >= 5000
    d = rm.get_euclidean(qd, gd)
    ref = rm.rank_rows(d)[:, :k]
    np.testing.assert_array_equal(idx.cpu().numpy(), ref.cpu().numpy())
    np.testing.assert_array_equal(idx.cpu().numpy(), np.sort(same)[None, :k].repeat(nq, 0))
    np.testing.assert_array_equal(dist.cpu().numpy().view(np.int32), torch.gather(d, 1, ref).cpu().numpy().view(np.int32))


def _similar_case():
    rng = np.random.default_rng(41)
    q = rng.standard_normal((37, 256)).astype(np.float32)
    gal = rng.standard_normal((900, 256)).astype(np.float32)
    qpaths = np.array([f"q/{i:04d}.jpg" for i in range(37)])
    gpaths = np.array([f"g/{i % 90:03d}_{i:05d}.jpg" for i in range(900)])
    return q, qpaths, gal, gpaths


def _assert_same_dict(a, b):
    assert list(a.keys()) == list(b.keys())
    for p in a:
        assert list(a[p].keys()) == list(b[p].keys()) == ["indices", "paths", "distances"]
        for key in a[p]:
            assert a[p][key].dtype == b[p][key].dtype and a[p][key].shape == b[p][key].shape
        np.testing.assert_array_equal(a[p]["indices"], b[p]["indices"])
        np.testing.assert_array_equal(a[p]["paths"], b[p]["paths"])
        np.testing.assert_array_equal(a[p]["distances"].view(np.int32), b[p]["distances"].view(np.int32))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_get_similar_h16_streamed_equals_materialised(dt):
    """get_similar(compute_dtype=dt): streamed=True returns the dict of streamed=False, array for array and bit for bit, with
    and without normalisation; the result is the one of the 16-bit kernels on the once-rounded features."""
    from centroids_reid_amd import inference as inf, reid_metric as rm
    q, qpaths, gal, gpaths = _similar_case()
    for norm in (True, False):
        base = inf.get_similar(q, qpaths, gal, gpaths, topk=20, streamed=False, normalize_features=norm, compute_dtype=dt)
        stats = {}
        got = inf.get_similar(q, qpaths, gal, gpaths, topk=20, streamed=True, normalize_features=norm, compute_dtype=dt, stats=stats)
        assert stats["path"] == "streamed" and stats["fallback_rows"] == 0
        _assert_same_dict(got, base)
        qd, gd, qq, gg = _device(q, gal, norm, dt)
        idx, dist = _reference(qd, gd, qq, gg, 20)
        np.testing.assert_array_equal(np.stack([got[p]["indices"] for p in qpaths]), idx.cpu().numpy())
        np.testing.assert_array_equal(np.stack([got[p]["distances"] for p in qpaths]).view(np.int32),
                                      dist.cpu().numpy().view(np.int32))


def test_get_similar_default_compute_dtype_is_fp32_on_inference_golden(golden):
    """The default compute_dtype is today's fp32 arithmetic: the reference's own inference results
    (tests/golden/inference.npz), streamed and materialised, with the keyword left out and spelled out."""
    from centroids_reid_amd import inference as inf
    g = golden("inference")
    nq, topk = int(g["num_query"]), int(g["topk"])
    f = g["feats"]
    for kw in ({}, {"compute_dtype": torch.float32}):
        for streamed in (True, False):
            res = inf.get_similar(f[:nq], g["query_paths"], f[nq:], g["gallery_paths"], topk=topk, streamed=streamed, **kw)
            assert list(res.keys()) == list(g["query_paths"])
            for i, p in enumerate(g["query_paths"]):
                np.testing.assert_array_equal(res[p]["indices"], g["indices"][i])
                np.testing.assert_array_equal(res[p]["paths"], g["gallery_paths"][g["indices"][i]])
                np.testing.assert_allclose(res[p]["distances"], g["distances"][i], rtol=0, atol=3e-6)


def test_stream_h16_abi_argument_checks():
    """The three _h16 entry points refuse what the header rules out before any launch -- D % 8 != 0 and a capacity that is no
    power of two: CREID_E_SHAPE (-4); dtype = CREID_F32: CREID_E_DTYPE (-2) -- and m == 0 is a no-op."""
    from centroids_reid_amd import _lib as L
    lib, st = L.lib(), L.stream()
    m, n, D, cap = 4, 128, 16, 64
    q = torch.zeros((m, D), dtype=torch.bfloat16, device="cuda"); g = torch.zeros((n, D), dtype=torch.bfloat16, device="cuda")
    qq = torch.zeros(m, device="cuda"); gg = torch.zeros(n, device="cuda"); tau = torch.zeros(m, device="cuda")
    cand = torch.zeros((m, 8192), dtype=torch.int64, device="cuda")
    count = torch.zeros(m, dtype=torch.int32, device="cuda")
    i64 = lambda k: torch.zeros(k, dtype=torch.int64, device="cuda")
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device="cuda")
    q_slot, csr, order, qc, gc, qp, gp = i32(m), i64(2), i32(n), i64(m), i64(n), i64(m), i64(n)
    pos_key = torch.full((m, 128), 7, dtype=torch.int32, device="cuda")
    pos_idx, npos, hist = i32(m * 128), torch.full((m,), 7, dtype=torch.int32, device="cuda"), i32(m * 128)

    def collect(m_=m, D_=D, cap_=cap, dt_=L.BF16):
        return lib.creid_stream_topk_collect_h16(L.ptr(q), L.ptr(g), L.ptr(qq), L.ptr(gg), m_, n, D_, dt_, L.ptr(tau), cap_,
                                                 L.ptr(cand), L.ptr(count), st)

    def poslist(m_=m, D_=D, cap_=4, dt_=L.BF16):
        return lib.creid_stream_poslist_h16(L.ptr(q), L.ptr(g), L.ptr(qq), L.ptr(gg), m_, n, D_, dt_, L.ptr(q_slot), L.ptr(csr),
                                            L.ptr(order), L.ptr(qc), L.ptr(gc), cap_, L.ptr(pos_key), L.ptr(pos_idx), L.ptr(npos), st)

    def cnt(m_=m, D_=D, cap_=4, dt_=L.BF16):
        return lib.creid_stream_count_h16(L.ptr(q), L.ptr(g), L.ptr(qq), L.ptr(gg), m_, n, D_, dt_, L.ptr(qp), L.ptr(gp), cap_,
                                          L.ptr(pos_key), L.ptr(pos_idx), L.ptr(npos), L.ptr(hist), st)
    E_ARG, E_DTYPE, E_SHAPE = -1, -2, -4
    for fn in (collect, poslist, cnt):
        assert fn(D_=12) == E_SHAPE                             # D % 8 != 0 (a multiple of 4: the fp32 entry points take it)
        assert fn(dt_=L.F32) == E_DTYPE and fn(dt_=L.BF16X3) == E_DTYPE
        assert fn(m_=-1) == E_ARG
    for bad_cap in (96, 32, 16384, 0):
        assert collect(cap_=bad_cap) == E_SHAPE
    for bad_cap in (3, 96, 256, 1, 0):
        assert poslist(cap_=bad_cap) == E_SHAPE and cnt(cap_=bad_cap) == E_SHAPE
    assert lib.creid_stream_topk_collect_h16(None, None, None, None, 0, n, D, L.F16, None, cap, None, None, st) == 0
    assert lib.creid_stream_poslist_h16(None, None, None, None, 0, n, D, L.F16, None, None, None, None, None, 4, None, None,
                                        None, st) == 0
    assert lib.creid_stream_count_h16(None, None, None, None, 0, n, D, L.F16, None, None, 4, None, None, None, None, st) == 0
    assert lib.creid_stream_topk_collect_h16(None, L.ptr(g), L.ptr(qq), L.ptr(gg), m, n, D, L.BF16, L.ptr(tau), cap, L.ptr(cand),
                                             L.ptr(count), st) == E_ARG
    torch.cuda.synchronize()
    assert int(count.sum()) == 0 and int(hist.sum()) == 0 and npos.tolist() == [7] * m      # nothing was launched
    assert int(pos_key.min()) == 7
    # and the accepted call: all-zero features, tau = 0 -> every column is a candidate (count = n, beyond cap = 64)
    for dt_, t in ((L.BF16, torch.bfloat16), (L.F16, torch.float16)):
        count.zero_()
        q, g = q.view(torch.int16).view(t), g.view(torch.int16).view(t)
        assert collect(dt_=dt_) == 0
        torch.cuda.synchronize()
        assert count.tolist() == [n] * m


def test_topk_stream_refuses_mixed_and_other_dtypes():
    """q and g of different dtypes, or of a dtype no kernel takes: CreidError before anything is launched."""
    from centroids_reid_amd import _lib as L, reid_metric as rm
    q = torch.zeros((4, 8), device="cuda")
    g = torch.zeros((16, 8), device="cuda")
    for qd, gd in ((torch.float32, torch.bfloat16), (torch.bfloat16, torch.float16), (torch.float16, torch.float32),
                   (torch.float64, torch.float64), (torch.int8, torch.int8)):
        with pytest.raises(L.CreidError, match="one dtype"):
            rm.topk_stream(q.to(qd), g.to(gd), 2)
