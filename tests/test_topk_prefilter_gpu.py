"""GPU: exact fp32 top-k with the contraction on the 16-bit MFMA (reid_metric.topk_stream(prefilter=...): creid_prefilter_pack +
creid_stream_topk_collect_h16 + creid_stream_topk_rescore, csrc/stream_prefilter.hip).  The result must EQUAL the fp32
topk_stream and topk_rows(get_euclidean(...)) -- indices, and distances as int32 bit patterns -- and the re-scored set must be the
proven superset, not "everything": its size is bounded by a float64 count made on the CPU from the same rows."""
import numpy as np
import pytest
import torch

from test_stream_topk_gpu import PARITY, _assert_equal, _assert_same_dict, _device, _reference, make_features

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(params=["0", "1"], ids=["split-major", "equal-runs"])
def work_split(monkeypatch, request):
    """Both work splits of the streamed contraction (mode 0 = per-row slices, mode 1 = equal runs of 64-column units)."""
    monkeypatch.setenv("CREID_STREAM_BALANCE", request.param)
    return request.param


def _cpu_stats(x, dtype):
    """float64 |x - xh|^2, |xh|^2, |x|^2 per row of a device fp32 tensor, xh = torch's CPU rounding to dtype"""
    x = x.cpu()
    xh = x.to(dtype).double().numpy()
    x = x.double().numpy()
    return np.stack([((x - xh) ** 2).sum(1), (xh ** 2).sum(1), (x ** 2).sum(1)], 1)


def _superset_bound(q, g, k, dtype):
    """max_i c_i, c_i = #{ j : D_ij <= D_(k) + 5 m_i } in float64 on the CPU (D: the distance of the device rows, m_i:
    prefilter_margin of their float64 statistics): kept is inside { d <= d_(k) + 4 m }, the fifth m covers fp64 against fp32."""
    from centroids_reid_amd import reid_metric as rm
    sq, sg = _cpu_stats(q, dtype), _cpu_stats(g, dtype)
    D8 = -(-q.shape[1] // 8) * 8
    m = rm.prefilter_margin(sq[:, 0], sq[:, 1], sq[:, 2], sg[:, 0].max(), sg[:, 1].max(), sg[:, 2].max(), sg[:, 2].max(), D8)
    q64, g64 = q.cpu().double().numpy(), g.cpu().double().numpy()
    dist = sq[:, 2][:, None] + sg[:, 2][None, :] - 2.0 * q64 @ g64.T
    kth = np.sort(dist, axis=1)[:, k - 1]
    return int((dist <= (kth + 5.0 * m)[:, None]).sum(1).max()), float(m.max())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("nq,ng,D,k,sample,dup", PARITY)
def test_prefilter_equals_fp32_and_rescored_set_is_the_proven_superset(nq, ng, D, k, sample, dup, dtype, work_split):
    """The geometries of test_topk_stream_equals_materialised_random (exact ties; D % 8 != 0 and the zero-padded width; a second
    query tile; a one-unit narrow tile; k = n), normalised and not, forced small sample.  Counted on the CPU with this generator
    (numpy normalisation), per case the largest c_i = #{ j : D_ij <= D_(k) + 5 m_i } for bf16 / f16 and, for orientation, the
    largest kept set #{ dh <= dh_(k) + 2 m_i } and the largest collected list:
        300 x 3000 x 256 k 20    c 72 / 31 (un-normalised 68 / 30)      kept 40 / 26 (44 / 25)      list 474 / 407 (460 / 399)
        70 x 513 x 100 k 50      c 79 / 57 (84 / 57)                    kept 66 / 54 (68 / 54)      list 259 / 242 (245 / 233)
        129 x 1000 x 2048 k 1    c 52 / 7 (39 / 8)                      kept 15 / 4 (18 / 5)        list 119 / 80 (153 / 103)
        129 x 1000 x 2048 k 7    c 110 / 21 (93 / 19)                   kept 42 / 15 (38 / 13)      list 305 / 225 (335 / 251)
        33 x 300 x 8 k 5         c 10 / 6 (10 / 6)                      kept 7 / 6 (9 / 6)          list 78 / 77 (77 / 77)
        65 x 4097 x 64 k 100     c 171 / 109 (172 / 112)                kept 132 / 105 (132 / 107)  list 1070 / 994 (993 / 923)
        5 x 40 x 32 k 40         c 40 / 40 (40 / 40)                    kept 40 / 40                list 40 / 40
    -- every c far below the re-score capacity of 1024 and every list below the capacity of 4096, so no row may need the repair."""
    from centroids_reid_amd import reid_metric as rm
    qh, gh = make_features(nq, ng, D, dup)
    for norm in (True, False):
        q, g, qq, gg = _device(qh, gh, norm)
        ref = _reference(q, g, qq, gg, k)
        _assert_equal(rm.topk_stream(q, g, k, qq, gg, sample=sample), ref)
        stats = {}
        got = rm.topk_stream(q, g, k, qq, gg, sample=sample, stats=stats, prefilter=dtype)
        c_max, m_max = _superset_bound(q, g, k, dtype)
        print(f"{nq} x {ng} x {D} k={k} norm={norm} {dtype}: {stats} c_max={c_max} m_max={m_max:.3g}")
        _assert_equal(got, ref)
        assert stats["prefilter"] == dtype and stats["sample"] == sample and stats["capacity"] == 4096
        assert stats["rescore_capacity"] == rm.STREAM_RESCORE_CAPACITY >= 1024
        assert k <= stats["max_rescored"] <= c_max
        assert stats["max_rescored"] <= stats["max_candidates"] <= 4096
        assert c_max <= stats["rescore_capacity"] and stats["fallback_rows"] == 0
        # the device statistics are the CPU's; |q|^2 enters as max(itself, the fp32 norm passed): within (D / 64 + 6) 2^-24 of it
        assert m_max * (1 - 1e-9) <= stats["margin_max"] <= m_max * (1 + 1e-5)
        _assert_equal(rm.topk_stream(q, g, k, sample=sample, prefilter=dtype), ref)           # norms computed inside
        pack = rm.prefilter_pack(g, dtype)
        _assert_equal(rm.topk_stream(q, g, k, qq, gg, sample=sample, prefilter=dtype, g_pack=pack), ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_prefilter_pack_rounds_like_torch_and_sums_in_double(dtype):
    """The 16-bit copy has the bits of x.to(dtype) (width 100 is zero-padded to 104); the statistics equal float64 sums made on
    the CPU; rows scaled by 2^-20 (f16: subnormals, underflow) keep exact statistics; a row that overflows f16 or holds an Inf /
    NaN is reported through non-finite statistics."""
    from centroids_reid_amd import reid_metric as rm
    rng = np.random.default_rng(17)
    x = rng.standard_normal((70, 100)).astype(np.float32)
    x[10:20] *= np.float32(2.0 ** -20)
    x[20:30] *= np.float32(300)
    xd = torch.from_numpy(x).cuda()
    pack = rm.prefilter_pack(xd, dtype)
    assert pack.rounded.shape == (70, 104) and pack.rounded.dtype == dtype and pack.width == 100
    assert pack.stats.shape == (70, 3) and pack.stats.dtype == torch.float64
    np.testing.assert_array_equal(pack.rounded[:, :100].cpu().view(torch.int16).numpy(), xd.to(dtype).cpu().view(torch.int16).numpy())
    assert int(pack.rounded[:, 100:].cpu().view(torch.int16).abs().max()) == 0
    np.testing.assert_allclose(pack.stats.cpu().numpy(), _cpu_stats(xd, dtype), rtol=1e-13, atol=0)
    assert all(np.isfinite(v) for v in pack.maxima())
    bad = x.copy()
    bad[3] *= np.float32(1e5)
    bad[5, 7] = np.inf
    bad[6, 99] = np.nan
    st = rm.prefilter_pack(torch.from_numpy(bad).cuda(), dtype).stats.cpu().numpy()
    finite = np.isfinite(st).all(1)
    assert not finite[5] and not finite[6] and finite[[0, 1, 2, 4, 7]].all()
    assert finite[3] == (dtype == torch.bfloat16)                                 # 1e5-scaled rows overflow f16 only
    with pytest.raises(rm.L.CreidError):
        rm.prefilter_pack(xd, torch.float32)
    with pytest.raises(rm.L.CreidError):
        rm.prefilter_pack(xd.half(), torch.float16)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_rows_below_16_bit_resolution(dtype, work_split):
    """40 gallery rows = one base row + distinct multiples (0 .. 3 on each of three elements) of 2^-14: distinct in fp32, EQUAL after
    rounding to bf16 or f16 (the base's elements are 16-bit values of magnitude 0.5 .. 1, half a 16-bit spacing there is 2^-9 /
    2^-12 > 3 * 2^-14).  The base is nearest to every query, so the pre-filter cannot order the 40: all of them must be kept
    and the fp32 re-score decides."""
    from centroids_reid_amd import reid_metric as rm
    rng = np.random.default_rng(23)
    nq, ng, D, k = 16, 600, 64, 10
    base = (rng.uniform(0.55, 0.95, D) * rng.choice([-1.0, 1.0], D)).astype(np.float32)
    base = torch.from_numpy(base).to(torch.bfloat16).float().numpy()
    q = (base + 0.01 * rng.standard_normal((nq, D))).astype(np.float32)
    g = (base + 4.0 * rng.standard_normal((ng, D))).astype(np.float32)
    near = np.sort(rng.permutation(ng)[:40])
    for t, j in enumerate(near):
        g[j] = base
        g[j, :3] += np.float32(2.0 ** -14) * np.array([t % 4, (t // 4) % 4, t // 16], np.float32)
    assert len({g[j].tobytes() for j in near}) == 40
    gt = torch.from_numpy(g)
    assert int((gt[near].to(dtype) != torch.from_numpy(base).to(dtype)).sum()) == 0
    qd, gd = torch.from_numpy(q).cuda(), gt.cuda()
    ref = rm.topk_stream(qd, gd, k)
    _assert_equal(ref, _reference(qd, gd, rm.row_sqnorm(qd), rm.row_sqnorm(gd), k))
    assert np.isin(ref[0].cpu().numpy(), near).all()
    stats = {}
    got = rm.topk_stream(qd, gd, k, stats=stats, prefilter=dtype)
    print(stats)
    _assert_equal(got, ref)
    assert stats["fallback_rows"] == 0 and 40 <= stats["max_rescored"] <= rm.STREAM_RESCORE_CAPACITY


def _tie_case(ntied):
    rng = np.random.default_rng(11)
    nq, ng, D = 40, 6000, 32
    centre = rng.standard_normal(D).astype(np.float32)
    q = (centre + 0.01 * rng.standard_normal((nq, D))).astype(np.float32)
    g = (centre + 4.0 * rng.standard_normal((ng, D))).astype(np.float32)
    same = rng.permutation(ng)[:ntied]
    g[same] = centre
    return torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda(), np.sort(same)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("ntied", [5000, 2000])
def test_overflow_is_flagged_and_repaired(ntied, dtype, work_split):
    """The construction of test_topk_stream_massive_ties.  5000 identical gallery rows nearest to every query: every candidate
    list overflows the capacity of 4096.  2000 of them: the lists (the tie group and nothing near it) fit, but every row keeps more
    than the re-score capacity of 1024 -- only the re-score stage flags.  Either way every row is repaired through the
    materialised fp32 kernels and orders the ties by gallery index."""
    from centroids_reid_amd import reid_metric as rm
    qd, gd, same = _tie_case(ntied)
    k = 10
    stats = {}
    idx, dist = rm.topk_stream(qd, gd, k, stats=stats, prefilter=dtype)
    print(stats)
    assert stats["prefilter"] == dtype and stats["fallback_rows"] == 40
    assert stats["rescore_capacity"] < stats["capacity"]
    if ntied == 5000:
        assert stats["max_candidates"] >= 5000
    else:
        assert 2000 <= stats["max_candidates"] <= stats["capacity"] and stats["max_rescored"] >= 2000
    d = rm.get_euclidean(qd, gd)
    ref = rm.rank_rows(d)[:, :k]
    np.testing.assert_array_equal(idx.cpu().numpy(), ref.cpu().numpy())
    np.testing.assert_array_equal(idx.cpu().numpy(), same[None, :k].repeat(40, 0))
    np.testing.assert_array_equal(dist.cpu().numpy().view(np.int32), torch.gather(d, 1, ref).cpu().numpy().view(np.int32))


def test_range_f16_overflow_takes_the_fp32_path():
    """Un-normalised features x 1e5 overflow f16: the gallery's statistics are not finite and the whole call takes the fp32 path
    (stats["prefilter"] is None); bf16 has the range and pre-filters.  A single overflowing QUERY row goes to the repair."""
    from centroids_reid_amd import reid_metric as rm
    qh, gh = make_features(70, 513, 100, False)
    q, g = torch.from_numpy(qh * np.float32(1e5)).cuda(), torch.from_numpy(gh * np.float32(1e5)).cuda()
    ref = rm.topk_stream(q, g, 20, sample=128)
    stats = {}
    _assert_equal(rm.topk_stream(q, g, 20, sample=128, stats=stats, prefilter=torch.float16), ref)
    assert stats["prefilter"] is None and not np.isfinite(stats["margin_max"]) and stats["max_rescored"] == 0
    _assert_equal(rm.topk_stream(q, g, 20, sample=128, stats=stats, prefilter=torch.bfloat16), ref)
    assert stats["prefilter"] == torch.bfloat16 and stats["fallback_rows"] == 0
    q2, g2 = torch.from_numpy(qh).cuda(), torch.from_numpy(gh).cuda()
    q2[3] *= 1e5
    ref = rm.topk_stream(q2, g2, 20, sample=128)
    _assert_equal(rm.topk_stream(q2, g2, 20, sample=128, stats=stats, prefilter=torch.float16), ref)
    assert stats["prefilter"] == torch.float16 and stats["fallback_rows"] == 1 and not np.isfinite(stats["margin_max"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_range_tiny_features(dtype, work_split):
    """Features x 2^-20: in f16 every element is a subnormal or zero, so the pre-filter sees almost nothing and the margin (from
    the rows themselves) is as large as the distances -- the result is still the fp32 one."""
    from centroids_reid_amd import reid_metric as rm
    qh, gh = make_features(70, 513, 100, False)
    s = np.float32(2.0 ** -20)
    q, g = torch.from_numpy(qh * s).cuda(), torch.from_numpy(gh * s).cuda()
    ref = rm.topk_stream(q, g, 20, sample=128)
    _assert_equal(ref, _reference(q, g, rm.row_sqnorm(q), rm.row_sqnorm(g), 20))
    stats = {}
    _assert_equal(rm.topk_stream(q, g, 20, sample=128, stats=stats, prefilter=dtype), ref)
    print(stats)
    assert stats["prefilter"] == dtype and stats["fallback_rows"] == 0 and 20 <= stats["max_rescored"] <= 513


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_get_similar_prefilter_on_inference_golden(golden, dtype):
    """get_similar(prefilter=...) equals get_similar() entry by entry on the inference golden, and "auto" streams."""
    from centroids_reid_amd import inference as inf
    g = golden("inference")
    nq, topk = int(g["num_query"]), int(g["topk"])
    f = g["feats"]
    base = inf.get_similar(f[:nq], g["query_paths"], f[nq:], g["gallery_paths"], topk=topk)
    stats = {}
    res = inf.get_similar(f[:nq], g["query_paths"], f[nq:], g["gallery_paths"], topk=topk, stats=stats, prefilter=dtype)
    assert stats["path"] == "streamed" and stats["prefilter"] == dtype
    _assert_same_dict(res, base)
    _assert_same_dict(inf.get_similar(f[:nq], g["query_paths"], f[nq:], g["gallery_paths"], topk=topk, streamed=True,
                                      prefilter=dtype), base)


def test_surface_errors():
    from centroids_reid_amd import _lib as L, inference as inf, reid_metric as rm
    rng = np.random.default_rng(41)
    q = rng.standard_normal((37, 256)).astype(np.float32)
    gal = rng.standard_normal((900, 256)).astype(np.float32)
    qp, gp = np.array([f"q/{i}" for i in range(37)]), np.array([f"g/{i}" for i in range(900)])
    for kw in (dict(streamed=False), dict(compute_dtype=torch.bfloat16), dict(compute_dtype=torch.float16), dict(reranking=True),
               dict(distance_func="cosine"), dict(topk=0), dict(prefilter=torch.float32)):
        args = dict(topk=20, prefilter=torch.float16)
        args.update(kw)
        with pytest.raises(L.CreidError):
            inf.get_similar(q, qp, gal, gp, **args)
    qd, gd = torch.from_numpy(q).cuda(), torch.from_numpy(gal).cuda()
    with pytest.raises(L.CreidError):
        rm.topk_stream(qd.half(), gd.half(), 5, prefilter=torch.float16)             # needs fp32 features
    with pytest.raises(L.CreidError):
        rm.topk_stream(qd, gd, 5, prefilter=torch.float32)
    with pytest.raises(L.CreidError):
        rm.topk_stream(qd, gd, 5, g_pack=rm.prefilter_pack(gd, torch.float16))        # g_pack without prefilter
    with pytest.raises(L.CreidError):
        rm.topk_stream(qd, gd, 5, prefilter=torch.bfloat16, g_pack=rm.prefilter_pack(gd, torch.float16))
    with pytest.raises(L.CreidError):
        rm.topk_stream(qd, gd, 5, prefilter=torch.float16, g_pack=rm.prefilter_pack(gd[:100].contiguous(), torch.float16))
    with pytest.raises(L.CreidError):
        rm.re_ranking(qd, gd, prefilter=torch.float32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_re_ranking_keeps_its_bits(dtype):
    from centroids_reid_amd import reid_metric as rm
    rng = np.random.default_rng(29)
    centres = rng.standard_normal((25, 64)).astype(np.float32)
    x = (centres[rng.integers(0, 25, 220)] + 0.3 * rng.standard_normal((220, 64))).astype(np.float32)
    q, g = torch.from_numpy(x[:20]).cuda(), torch.from_numpy(x[20:]).cuda()
    q, g = rm.l2_normalize(q), rm.l2_normalize(g)
    base = rm.re_ranking(q, g)
    got = rm.re_ranking(q, g, prefilter=dtype)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.int32), base.cpu().numpy().view(np.int32))


def test_prefilter_allocates_no_matrix():
    """The method of test_topk_stream_allocates_no_matrix, 2048 x 65 536 (the matrix would be 512 MB): peak allocation above the
    live inputs stays below half of it (candidate lists 64 MB, the 16-bit gallery copy 8 MB, the sample slice)."""
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
    idx, dist = rm.topk_stream(q, g, k, qq, gg, stats=stats, prefilter=torch.bfloat16)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - live
    print(stats, f"peak above inputs {peak / 2**20:.1f} MiB")
    assert peak < m * n * 4 // 2
    assert stats["sample"] == 1280 and stats["fallback_rows"] == 0
    for c in range(4):
        r = slice(c * 512, (c + 1) * 512)
        _assert_equal((idx[r], dist[r]), _reference(q[r], g, qq[r], gg, k))


def test_prefilter_abi_argument_checks():
    """creid_prefilter_pack / creid_stream_topk_rescore refuse what the header rules out before any launch, and zero rows are a
    no-op; then one accepted call of each."""
    from centroids_reid_amd import _lib as L
    lib, st = L.lib(), L.stream()
    m, n, D, cap, k = 4, 128, 16, 64, 5
    q = torch.zeros((m, D), device="cuda"); g = torch.zeros((n, D), device="cuda")
    qq = torch.zeros(m, device="cuda"); gg = torch.zeros(n, device="cuda"); mg = torch.zeros(m, device="cuda")
    cand = torch.zeros((m, 8192), dtype=torch.int64, device="cuda")
    count = torch.zeros(m, dtype=torch.int32, device="cuda")
    idx = torch.full((m, 1024), -1, dtype=torch.int64, device="cuda")
    dist = torch.zeros((m, 1024), device="cuda")
    flags = torch.full((m,), 7, dtype=torch.uint8, device="cuda")
    kept = torch.full((m,), -1, dtype=torch.int32, device="cuda")
    y = torch.full((m, D), 3, dtype=torch.int16, device="cuda")
    stt = torch.full((m, 3), -1.0, dtype=torch.float64, device="cuda")

    def pack(rows=m, D_=D, dt=L.F16, x=q):
        return lib.creid_prefilter_pack(L.ptr(x), rows, D_, dt, L.ptr(y), L.ptr(stt), st)

    def rescore(m_=m, cap_=cap, k_=k, D_=D, n_=n, q_=q):
        return lib.creid_stream_topk_rescore(L.ptr(cand), L.ptr(count), m_, cap_, k_, L.ptr(q_), L.ptr(g), L.ptr(qq), L.ptr(gg), n_,
                                             D_, L.ptr(mg), L.ptr(idx), L.ptr(dist), L.ptr(flags), L.ptr(kept), st)
    E_ARG, E_DTYPE, E_SHAPE = -1, -2, -4
    assert pack(D_=12) == E_SHAPE and pack(D_=(1 << 20) + 8) == E_SHAPE
    assert pack(dt=L.F32) == E_DTYPE and pack(dt=L.BF16X3) == E_DTYPE
    assert pack(rows=-1) == E_ARG and pack(D_=0) == E_ARG and pack(x=None) == E_ARG
    assert lib.creid_prefilter_pack(None, 0, D, L.BF16, None, None, st) == 0
    for bad_cap in (96, 32, 16384, 0):
        assert rescore(cap_=bad_cap) == E_SHAPE
    assert rescore(cap_=2048, k_=1025) == E_SHAPE and rescore(cap_=64, k_=65) == E_SHAPE
    assert rescore(D_=18) == E_SHAPE
    assert rescore(k_=0) == E_ARG and rescore(m_=-1) == E_ARG and rescore(n_=0) == E_ARG and rescore(q_=None) == E_ARG
    assert lib.creid_stream_topk_rescore(None, None, 0, cap, k, None, None, None, None, n, D, None, None, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert int(flags.min()) == 7 and int(idx.max()) == -1 and int(kept.max()) == -1 and int(y.min()) == 3      # nothing launched
    # accepted: ones rounded to f16; lists of 6 entries (row r: columns r .. r + 5, 16-bit keys of distance 0) with k = 5, an
    # empty list, and a column outside the gallery
    q.fill_(1.0)
    assert pack() == 0
    key0 = -(1 << 63)                                 # key 0x80000000 (distance +0.0) << 32 as an int64
    flat = cand.view(-1)                              # the kernel's rows are `cap` words apart
    for r in range(3):
        flat[r * cap:r * cap + 6] = torch.tensor([key0 | (r + 5 - t) for t in range(6)], dtype=torch.int64)
    flat[2 * cap] = key0 | n
    count.copy_(torch.tensor([6, 6, 6, 0], dtype=torch.int32))
    assert rescore() == 0
    torch.cuda.synchronize()
    assert (y.view(torch.float16) == 1).all() and stt.tolist() == [[0.0, float(D), float(D)]] * m
    assert flags.tolist() == [0, 0, 1, 1] and kept.tolist() == [6, 6, 6, 0]
    assert idx.view(-1)[:2 * k].tolist() == [0, 1, 2, 3, 4, 1, 2, 3, 4, 5]       # rows of k entries
    assert dist.view(-1)[:2 * k].tolist() == [0.0] * (2 * k)                     # <1, 0> = 0, qq = gg = 0
    assert int(idx.view(-1)[2 * k:].max()) == -1                                 # flagged rows: nothing written
