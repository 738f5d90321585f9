"""GPU parity: top-k retrieval that never writes the m x n distance matrix (reid_metric.topk_stream:
creid_stream_topk_collect + creid_stream_topk_select in csrc/stream_eval.hip) against the materialised path
rm.topk_rows(rm.get_euclidean(q, g, qq, gg), k) on the same device tensors -- the same indices and the same distance
bits, ties by gallery index -- through the Python surface, inference.get_similar and the C ABI."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["0", "1"], ids=["split-major", "equal-runs"])
def work_split(monkeypatch, request):
    """Both work splits of the streamed contraction (csrc/stream_eval.hip: mode 0 = per-row slices, mode 1 = equal runs of
    64-column units that may cross query tiles); the default picks by gallery size."""
    monkeypatch.setenv("CREID_STREAM_BALANCE", request.param)
    return request.param


def make_features(nq, ng, D, dup, seed=None):
    """N(0,1) queries and gallery (dense near-ties in fp32); dup: a quarter of the gallery rows copied over others (exact
    ties, ordered by gallery index)."""
    rng = np.random.default_rng(nq * 7 + ng if seed is None else seed)
    q = rng.standard_normal((nq, D)).astype(np.float32)
    g = rng.standard_normal((ng, D)).astype(np.float32)
    if dup:
        src = rng.integers(0, ng, ng // 4); dst = rng.integers(0, ng, ng // 4)
        g[dst] = g[src]
    return q, g


def _device(q, g, norm):
    from centroids_reid_amd import reid_metric as rm
    q, g = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    if norm:
        q, g = rm.l2_normalize(q), rm.l2_normalize(g)
    return q, g, rm.row_sqnorm(q), rm.row_sqnorm(g)


def _reference(q, g, qq, gg, k):
    from centroids_reid_amd import reid_metric as rm
    return rm.topk_rows(rm.get_euclidean(q, g, qq, gg), k)


def _assert_equal(got, ref):
    np.testing.assert_array_equal(got[0].cpu().numpy(), ref[0].cpu().numpy())
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32
    np.testing.assert_array_equal(got[1].cpu().numpy().view(np.int32), ref[1].cpu().numpy().view(np.int32))     # bit-exact


PARITY = [(300, 3000, 256, 20, 256, True), (70, 513, 100, 50, 128, False), (129, 1000, 2048, 1, 64, True),
          (129, 1000, 2048, 7, 64, True), (33, 300, 8, 5, 32, False), (65, 4097, 64, 100, 512, False),
          (5, 40, 32, 40, 40, False)]


@pytest.mark.parametrize("nq,ng,D,k,sample,dup", PARITY)
def test_topk_stream_equals_materialised_random(nq, ng, D, k, sample, dup, work_split):
    """A 65th query row (second query tile), a 4097th column (a one-unit narrow tile with column masking), D % 16 != 0 (the
    zero-fill k-loop), D = 8, k = n; `sample` is forced small, so the threshold is loose and the candidate lists are real
    supersets (largest list per case, counted on the CPU with this generator: 394 / 239 / 72 / 204 / 77 / 984 / 40 normalised,
    389 / 229 / 97 / 240 / 76 / 909 / 40 un-normalised) -- far below the default capacity, so no row may need the repair."""
    from centroids_reid_amd import reid_metric as rm
    qh, gh = make_features(nq, ng, D, dup)
    for norm in (True, False):
        q, g, qq, gg = _device(qh, gh, norm)
        ref = _reference(q, g, qq, gg, k)
        stats = {}
        got = rm.topk_stream(q, g, k, qq, gg, sample=sample, stats=stats)
        print(f"{nq} x {ng} x {D} k={k} norm={norm}: {stats}")
        _assert_equal(got, ref)
        assert stats["fallback_rows"] == 0 and stats["capacity"] == 4096 and stats["sample"] == sample
        assert k <= stats["max_candidates"] <= 4096
        _assert_equal(rm.topk_stream(q, g, k, sample=sample), ref)           # norms computed inside


@pytest.mark.parametrize("capacity", [64, 256])
def test_topk_stream_overflow_is_detected_and_repaired(capacity, work_split):
    """300 x 3000, k = 20, sample 256: the lists hold 98 .. 394 entries (mean 233, 92 of them above 256; counted on the
    CPU).  Capacity 64 overflows in every row, capacity 256 in some: those rows are flagged and redone through the
    materialised kernels."""
    from centroids_reid_amd import reid_metric as rm
    qh, gh = make_features(300, 3000, 256, True)
    q, g, qq, gg = _device(qh, gh, True)
    ref = _reference(q, g, qq, gg, 20)
    stats = {}
    got = rm.topk_stream(q, g, 20, qq, gg, sample=256, capacity=capacity, stats=stats)
    print(stats)
    _assert_equal(got, ref)
    assert stats["capacity"] == capacity
    if capacity == 64:
        assert stats["fallback_rows"] == 300
    else:
        assert 0 < stats["fallback_rows"] < 300


def test_topk_stream_massive_ties(work_split):
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
    qd, gd = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    stats = {}
    idx, dist = rm.topk_stream(qd, gd, k, stats=stats)
    print(stats)
    assert stats["fallback_rows"] == nq and stats["max_candidates"] >= 5000
    d = rm.get_euclidean(qd, gd)
    ref = rm.rank_rows(d)[:, :k]
    np.testing.assert_array_equal(idx.cpu().numpy(), ref.cpu().numpy())
    np.testing.assert_array_equal(idx.cpu().numpy(), np.sort(same)[None, :k].repeat(nq, 0))
    np.testing.assert_array_equal(dist.cpu().numpy().view(np.int32), torch.gather(d, 1, ref).cpu().numpy().view(np.int32))


def test_get_similar_streamed_on_inference_golden(golden):
    """get_similar(streamed=True) against the reference's own inference helpers (tests/golden/inference.npz): the assertions of
    test_centroid_eval_gpu.py::test_inference_golden."""
    from centroids_reid_amd import inference as inf
    g = golden("inference")
    nq, topk = int(g["num_query"]), int(g["topk"])
    f = g["feats"]
    stats = {}
    res = inf.get_similar(f[:nq], g["query_paths"], f[nq:], g["gallery_paths"], topk=topk, streamed=True, stats=stats)
    assert stats["path"] == "streamed"
    assert list(res.keys()) == list(g["query_paths"])
    for i, p in enumerate(g["query_paths"]):
        np.testing.assert_array_equal(res[p]["indices"], g["indices"][i])
        np.testing.assert_array_equal(res[p]["paths"], g["gallery_paths"][g["indices"][i]])
        np.testing.assert_allclose(res[p]["distances"], g["distances"][i], rtol=0, atol=3e-6)


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


def test_get_similar_streamed_equals_materialised(monkeypatch):
    """The 37 x 900 case of test_get_similar_matches_oracle: streamed=True returns the dict of streamed=False, array for array;
    calls that cannot stream raise; "auto" on a matrix inside the byte budget never touches the streamed path."""
    from centroids_reid_amd import _lib as L, inference as inf, reid_metric as rm
    q, qpaths, gal, gpaths = _similar_case()
    base = inf.get_similar(q, qpaths, gal, gpaths, topk=20, streamed=False)
    _assert_same_dict(inf.get_similar(q, qpaths, gal, gpaths, topk=20, streamed=True), base)
    _assert_same_dict(inf.get_similar(q, qpaths, gal, gpaths, topk=20, streamed=True, normalize_features=False),
                      inf.get_similar(q, qpaths, gal, gpaths, topk=20, streamed=False, normalize_features=False))
    with pytest.raises(L.CreidError):
        inf.get_similar(q, qpaths, gal, gpaths, topk=20, distance_func="cosine", streamed=True)
    with pytest.raises(L.CreidError):
        inf.get_similar(q, qpaths, gal, gpaths, topk=0, streamed=True)

    def boom(*a, **kw):
        raise AssertionError("auto streamed a matrix inside the byte budget")
    monkeypatch.setattr(rm, "topk_stream", boom)
    stats = {}
    _assert_same_dict(inf.get_similar(q, qpaths, gal, gpaths, topk=20, stats=stats), base)            # streamed="auto"
    assert stats["path"] == "materialised"
    full = inf.get_similar(q, qpaths, gal, gpaths, topk=0, distance_func="cosine", stats=stats)
    assert stats["path"] == "materialised" and full[qpaths[0]]["indices"].shape == (900,)


def test_get_similar_auto_beyond_the_byte_budget(monkeypatch):
    """"auto" with the matrix beyond the budget (the budget lowered instead of the problem raised): a streamable call with a
    sample of at most a quarter of the gallery streams; any other call runs the matrix path over chunks of query rows.  The
    returned dict is the one of streamed=False either way."""
    from centroids_reid_amd import inference as inf
    q, qpaths, gal, gpaths = _similar_case()
    rng = np.random.default_rng(43)
    big = rng.standard_normal((8192, 256)).astype(np.float32)
    bpaths = np.array([f"g/{i:05d}.jpg" for i in range(8192)])
    monkeypatch.setattr(inf, "STREAM_MATRIX_BYTES", 10 * 900 * 4)
    stats = {}
    res = inf.get_similar(q, qpaths, big, bpaths, topk=20, stats=stats)
    assert stats["path"] == "streamed" and stats["sample"] == 1024 and stats["fallback_rows"] == 0
    _assert_same_dict(res, inf.get_similar(q, qpaths, big, bpaths, topk=20, streamed=False))
    res = inf.get_similar(q, qpaths, gal, gpaths, topk=20, stats=stats)                             # sample 900 > 900 // 4
    assert stats["path"] == "chunked"
    _assert_same_dict(res, inf.get_similar(q, qpaths, gal, gpaths, topk=20, streamed=False))
    res = inf.get_similar(q, qpaths, gal, gpaths, topk=0, distance_func="cosine", stats=stats)      # not streamable
    assert stats["path"] == "chunked"
    _assert_same_dict(res, inf.get_similar(q, qpaths, gal, gpaths, topk=0, distance_func="cosine", streamed=False))


def test_topk_stream_allocates_no_matrix():
    """2048 x 65 536 (the matrix would be 512 MB): peak allocation above the live inputs stays below half of it (candidate
    lists 64 MB + the 2048 x 1280 sample slice at the defaults); results equal the reference computed in four query chunks."""
    from centroids_reid_amd import reid_metric as rm
    m, n, D, k = 2048, 65536, 64, 20
    gen = torch.Generator(device="cuda").manual_seed(3)
    q = torch.randn((m, D), generator=gen, device="cuda")
    g = torch.randn((n, D), generator=gen, device="cuda")
    qq, gg = rm.row_sqnorm(q), rm.row_sqnorm(g)
    torch.cuda.synchronize()
    live = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    stats = {}
    idx, dist = rm.topk_stream(q, g, k, qq, gg, stats=stats)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - live
    print(stats, f"peak above inputs {peak / 2**20:.1f} MiB")
    assert peak < m * n * 4 // 2
    assert stats["sample"] == 1280 and stats["fallback_rows"] == 0
    for c in range(4):
        r = slice(c * 512, (c + 1) * 512)
        _assert_equal((idx[r], dist[r]), _reference(q[r], g, qq[r], gg, k))


def test_stream_topk_abi_argument_checks():
    """creid_stream_topk_collect / _select refuse what the header rules out before any launch (CREID_E_SHAPE = -4), and
    m == 0 is a no-op."""
    from centroids_reid_amd import _lib as L
    lib, st = L.lib(), L.stream()
    m, n, D, cap, k = 4, 128, 16, 64, 5
    q = torch.zeros((m, D), device="cuda"); g = torch.zeros((n, D), device="cuda")
    qq = torch.zeros(m, device="cuda"); gg = torch.zeros(n, device="cuda"); tau = torch.zeros(m, device="cuda")
    cand = torch.zeros((m, 8192), dtype=torch.int64, device="cuda")
    count = torch.zeros(m, dtype=torch.int32, device="cuda")
    idx = torch.full((m, 1024), -1, dtype=torch.int64, device="cuda")
    dist = torch.zeros((m, 1024), device="cuda")
    flags = torch.full((m,), 7, dtype=torch.uint8, device="cuda")

    def collect(m_=m, D_=D, cap_=cap):
        return lib.creid_stream_topk_collect(L.ptr(q), L.ptr(g), L.ptr(qq), L.ptr(gg), m_, n, D_, L.ptr(tau), cap_, L.ptr(cand),
                                             L.ptr(count), st)

    def select(m_=m, cap_=cap, k_=k):
        return lib.creid_stream_topk_select(L.ptr(cand), L.ptr(count), m_, cap_, k_, L.ptr(idx), L.ptr(dist), L.ptr(flags), st)
    E_ARG, E_SHAPE = -1, -4
    for bad_cap in (96, 32, 16384, 0):
        assert collect(cap_=bad_cap) == E_SHAPE and select(cap_=bad_cap) == E_SHAPE
    assert collect(D_=18) == E_SHAPE
    assert select(cap_=2048, k_=1025) == E_SHAPE                # k > 1024
    assert select(cap_=64, k_=65) == E_SHAPE                    # k > cap
    assert select(k_=0) == E_ARG and collect(m_=-1) == E_ARG
    assert lib.creid_stream_topk_collect(None, None, None, None, 0, n, D, None, cap, None, None, st) == 0
    assert lib.creid_stream_topk_select(None, None, 0, cap, k, None, None, None, st) == 0
    assert lib.creid_stream_topk_collect(None, L.ptr(g), L.ptr(qq), L.ptr(gg), m, n, D, L.ptr(tau), cap, L.ptr(cand),
                                         L.ptr(count), st) == E_ARG
    torch.cuda.synchronize()
    assert int(count.sum()) == 0 and int(flags.min()) == 7 and int(idx.max()) == -1      # nothing was launched
    # and the accepted call: all-zero features, tau = 0 -> every column is a candidate (128 > cap = 64 -> flagged)
    assert collect() == 0 and select() == 0
    torch.cuda.synchronize()
    assert count.tolist() == [n] * m and flags.tolist() == [1] * m


# ------------------------------------------------------------------------------------------ more than one row chunk
CHUNK_M, CHUNK_N, CHUNK_K = 150, 700, 5
CHUNK_BYTES = 32768          # row chunks of 64 (150 = 64 + 64 + 22), repair chunks of 32768 // (700 * 4) = 11 rows, 2 with junk
CHUNK_SETTINGS = {"streamed": dict(sample=64), "repair": dict(sample=5, capacity=64)}
# (case, D): D = 40 is a multiple of the 16-bit kernels' 8-element chunk; the pre-filter also runs at D = 44, where topk_stream
# pads the fp32 rows to 48 columns
CHUNK_CASES = [("fp32", 40), ("bf16", 40), ("f16", 40), ("prefilter", 40), ("prefilter", 44), ("junk", 40), ("junk-bf16", 40),
               ("junk-camsets", 40)]


@functools.lru_cache(maxsize=None)
def _chunk_case(case, D):
    """(q, g, qq, gg, keywords, materialised reference) of one case: seeded N(0, 1) rows, 40 pids over 3 cameras (camera sets:
    masks over the same 3).  Computed once, shared by both settings, never written."""
    from centroids_reid_amd import reid_metric as rm
    rng = np.random.default_rng(CHUNK_M * 7 + CHUNK_N + D)
    qh = rng.standard_normal((CHUNK_M, D)).astype(np.float32)
    gh = rng.standard_normal((CHUNK_N, D)).astype(np.float32)
    q_pids, g_pids = rng.integers(0, 40, CHUNK_M), rng.integers(0, 40, CHUNK_N)
    q_cams, g_cams, g_masks = rng.integers(0, 3, CHUNK_M), rng.integers(0, 3, CHUNK_N), rng.integers(1, 8, CHUNK_N)
    dtype = torch.bfloat16 if case.endswith("bf16") else torch.float16 if case == "f16" else torch.float32
    q, g = torch.from_numpy(qh).cuda().to(dtype), torch.from_numpy(gh).cuda().to(dtype)
    qq, gg = rm.row_sqnorm(q), rm.row_sqnorm(g)
    d = rm.get_euclidean(q, g, qq, gg)
    kw = {}
    if case == "prefilter":
        kw["prefilter"] = torch.bfloat16
    if case.startswith("junk"):
        camsets = case == "junk-camsets"
        dev = lambda a: torch.from_numpy(a.astype(np.int64)).cuda()
        kw["junk"] = rm.JunkFilter(dev(q_pids), dev(q_cams), dev(g_pids), dev(g_masks if camsets else g_cams), camsets=camsets)
        ridx = rm.rank_keep_topk(rm.rank_rows(d), CHUNK_K, kw["junk"])[0]
        ref = (ridx, rm.gather_ranked(d, ridx))
    else:
        ref = rm.topk_rows(d, CHUNK_K)
    return q, g, qq, gg, kw, ref


@pytest.mark.parametrize("setting", list(CHUNK_SETTINGS))
@pytest.mark.parametrize("case,D", CHUNK_CASES, ids=[f"{c}-{D}" for c, D in CHUNK_CASES])
def test_topk_stream_in_several_row_chunks(case, D, setting, monkeypatch):
    """150 x 700, k = 5 with the temporaries bounded to 32 KiB instead of 256 MiB: three row chunks (64, 64, 22), repair chunks
    of 11 rows (2 with junk).  "streamed": sample 64 at the default capacity; "repair": sample 5 and capacity 64 -- the threshold
    is the largest of five columns, so the lists overflow and the repair runs in many chunks.  Either way the result is the
    materialised reference and the result of the same call in ONE chunk, indices and distance bits, with the same counters."""
    from centroids_reid_amd import reid_metric as rm
    q, g, qq, gg, kw, ref = _chunk_case(case, D)
    one, chunked = {}, {}
    whole = rm.topk_stream(q, g, CHUNK_K, qq, gg, stats=one, **CHUNK_SETTINGS[setting], **kw)
    monkeypatch.setattr(rm, "_STREAM_TOPK_CHUNK_BYTES", CHUNK_BYTES)
    got = rm.topk_stream(q, g, CHUNK_K, qq, gg, stats=chunked, **CHUNK_SETTINGS[setting], **kw)
    print(f"{case} D={D} {setting}: fallback_rows {chunked['fallback_rows']} max_candidates {chunked['max_candidates']}")
    _assert_equal(got, ref)
    _assert_equal(got, whole)
    assert chunked["fallback_rows"] == one["fallback_rows"] and chunked["max_candidates"] == one["max_candidates"]
    if setting == "repair":
        assert chunked["fallback_rows"] > 11


def test_stage_times_are_summed_over_row_chunks(monkeypatch):
    """The pre-filtered search in three row chunks marks pack_q / sample / collect / rescore once per chunk: stage_ms holds one
    entry per name.  re_ranking's stage names are unique."""
    from centroids_reid_amd import reid_metric as rm
    q, g, qq, gg, kw, _ = _chunk_case("prefilter", 40)
    monkeypatch.setattr(rm, "_STREAM_TOPK_CHUNK_BYTES", CHUNK_BYTES)
    stats = {"timing": True}
    rm.topk_stream(q, g, CHUNK_K, qq, gg, sample=64, stats=stats, **kw)
    print(stats["stage_ms"])
    assert set(stats["stage_ms"]) == {"pack_g", "pack_q", "sample", "collect", "rescore", "repair"}
    assert all(isinstance(v, float) and np.isfinite(v) and v >= 0 for v in stats["stage_ms"].values())
    monkeypatch.undo()
    gen = torch.Generator(device="cuda").manual_seed(7)
    stats = {"timing": True}
    rm.re_ranking(torch.randn((20, 32), generator=gen, device="cuda"), torch.randn((120, 32), generator=gen, device="cuda"),
                  k1=6, k2=3, stats=stats)
    print(stats["stage_ms"])
    assert list(stats["stage_ms"]) == ["neighbours", "row_maxima", "reciprocal_sets", "weights", "expansion", "column_index",
                                       "blend"]
    assert all(isinstance(v, float) and np.isfinite(v) and v >= 0 for v in stats["stage_ms"].values())
