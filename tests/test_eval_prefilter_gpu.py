"""GPU: exact fp32 CMC / mAP with the counting contraction on the 16-bit MFMA (reid_metric.R1_mAP(streamed=True, prefilter=...):
creid_prefilter_pack + creid_stream_poslist + creid_stream_count_band_h16 + creid_stream_count_rescore).  The result must EQUAL
the fp32 streamed evaluation -- valid and first bit for bit, ap within the order of its float64 additions -- without passing
through the fp32 fallback and without re-scoring everything: the number of listed pairs is bounded by what the numpy model of
tests/eval_prefilter_model.py counts for the same generator."""
import numpy as np
import pytest
import torch

import eval_prefilter_model as M

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]
_REF = {}                                                  # (input, feat_norm) -> the fp32 streamed evaluation, computed once


@pytest.fixture(params=["0", "1"], ids=["split-major", "equal-runs"])
def work_split(monkeypatch, request):
    """Both work splits of the counting contraction (mode 0 = per-row slices, mode 1 = equal runs of 64-column units)."""
    monkeypatch.setenv("CREID_STREAM_BALANCE", request.param)
    return request.param


def _edge_cases(f, pids, cams, nq):
    """as test_stream_h16_eval_gpu.py builds them: a pid absent from the gallery (query 0), a zero-distance positive (of query 3)
    and a query whose positives all share its camera (query 1)"""
    f, pids, cams = np.array(f, np.float32), np.array(pids), np.array(cams)
    ng = len(f) - nq
    pids[0] = pids.max() + 5
    k = nq + min(7, ng - 1)
    f[k] = f[3]; pids[k] = pids[3]; cams[k] = cams[3] + 1
    cams[nq:][pids[nq:] == pids[1]] = cams[1]
    return f, pids, cams


def _fp32(key, f, pids, cams, nq, norm):
    from centroids_reid_amd import reid_metric as rm
    if key is None or (key, norm) not in _REF:
        a = rm.R1_mAP(num_query=nq, feat_norm=norm, streamed=True)
        ra = a.compute(f, pids, cams)
        out = (a.last["valid"].cpu().numpy(), a.last["ap"].cpu().numpy(), a.last["first"].cpu().numpy(),
               a.last["single_performance"], ra)
        if key is None:
            return out
        _REF[(key, norm)] = out
    return _REF[(key, norm)]


def _assert_equals_fp32(ref, b, rb):
    v0, ap0, f0, single0, ra = ref
    assert "distmat" not in b.last and "plan" in b.last and "prefilter" in b.last
    np.testing.assert_array_equal(b.last["valid"].cpu().numpy(), v0)
    np.testing.assert_array_equal(b.last["first"].cpu().numpy(), f0)
    np.testing.assert_allclose(b.last["ap"].cpu().numpy(), ap0, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(rb[0], ra[0])                 # CMC curve
    assert abs(rb[1] - ra[1]) <= 1e-12
    np.testing.assert_array_equal(rb[2], ra[2])                 # top-k values
    np.testing.assert_allclose(b.last["single_performance"], single0, rtol=0, atol=1e-12)


def _run(f, pids, cams, nq, dt, norm, key=None, **kw):
    from centroids_reid_amd import reid_metric as rm
    fd = f if isinstance(f, torch.Tensor) else torch.from_numpy(f).cuda()
    ref = _fp32(key, fd, pids, cams, nq, norm)
    b = rm.R1_mAP(num_query=nq, feat_norm=norm, streamed=True, prefilter=dt, **kw)
    rb = b.compute(fd, pids, cams)
    _assert_equals_fp32(ref, b, rb)
    return b


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", ["eval_small", "eval_d2048", "eval_tiny_gallery"])
def test_prefilter_equals_fp32_on_goldens(golden, name, dt, work_split):
    """The goldens with the three edge cases added.  No row may need the fallback, some pairs are listed and at most a quarter
    of them, with the two exceptions the numpy model (eval_prefilter_model.emulate + banded_count on these inputs) shows: it lists
    33.5 % (raw) and 35.2 % (normalised) of eval_d2048's pairs in bf16 -- 24 x 200 rows of 26 identities, most negatives lie among
    the positives -- where the bound is a half, and none of eval_tiny_gallery's 320 normalised pairs in f16 (4 of the raw ones),
    where nothing has to be listed.  The other combinations: 1.3 .. 11.2 % of the pairs, at least 4 pairs."""
    from centroids_reid_amd import reid_metric as rm
    g = golden(name)
    nq = int(g["num_query"])
    f, pids, cams = _edge_cases(g["feats"], g["pids"], g["camids"], nq)
    for norm in (True, False):
        b = _run(f, pids, cams, nq, dt, norm, key=name)
        info = b.last["prefilter"]
        amb = info["ambiguous"].cpu().numpy()
        print(name, norm, dt, "ambiguous max", amb.max(), "sum", amb.sum(), "of", nq * (len(f) - nq), "margin", info["margin_max"])
        assert info["dtype"] == dt and info["capacity"] == rm.EVAL_PREFILTER_CAPACITY == 1024 and info["fallback_rows"] == 0
        if not (name == "eval_tiny_gallery" and dt == torch.float16 and norm):
            assert amb.sum() > 0
        share = 0.5 if (name == "eval_d2048" and dt == torch.bfloat16) else 0.25
        assert amb.sum() <= share * nq * (len(f) - nq)
        assert b.last["valid"][0].item() == 0 and b.last["valid"][1].item() == 0


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("nq,ng,D", [(300, 3000, 256), (129, 1000, 2048), (130, 1000, 64), (70, 513, 104), (33, 300, 8)])
def test_prefilter_equals_fp32_and_lists_few_pairs(nq, ng, D, seed, dt, work_split):
    """Clustered rows with 10 % of the gallery labels randomised (eval_prefilter_model.clustered): a second query tile, narrow last
    tiles, zero-filled k-tiles (104, 8), D = 2048.  The numpy model (proven margin, emulated 16-bit dot) lists, over these shapes
    and seeds, at most 773 pairs of a row in bf16 and 106 in f16 -- below the default capacity, so no row may take the fallback --
    and at most 12.3 % of all pairs; the device must list some (else nothing was re-scored) and at most a quarter."""
    f, pids, cams = M.clustered(nq, ng, D, seed)
    for norm in (True, False):
        b = _run(f, pids, cams, nq, dt, norm, key=(nq, ng, D, seed))
        info = b.last["prefilter"]
        amb = info["ambiguous"].cpu().numpy()
        print(nq, ng, D, seed, norm, dt, "ambiguous max", amb.max(), "sum", amb.sum(), "of", nq * ng, "margin", info["margin_max"])
        assert info["dtype"] == dt and info["capacity"] == 1024
        assert amb.dtype == np.int32 and amb.shape == (nq,)
        assert info["fallback_rows"] == 0
        assert amb.sum() > 0
        assert amb.sum() <= 0.25 * nq * ng
        assert b.last["valid"][0].item() == 0 and b.last["valid"][1].item() == 0


def _dense(nq=300, ng=3000, D=256):
    rng = np.random.default_rng(nq * 7 + ng)
    f = rng.standard_normal((nq + ng, D)).astype(np.float32)
    pids = rng.integers(0, 60, nq + ng); cams = rng.integers(0, 3, nq + ng)
    src = rng.integers(nq, nq + ng, ng // 4); dst = rng.integers(nq, nq + ng, ng // 4)
    f[dst] = f[src]                                             # exact ties, possibly between a positive and a negative
    return _edge_cases(f, pids, cams, nq)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_dense_ties_overflow_the_lists_and_are_repaired(dt, work_split):
    """N(0,1) rows with random pids: every negative lies among the positives, and the numpy model lists 1060 .. 2381 pairs of a row
    in bf16 (205 .. 598 in f16).  At capacity 64 every query that has positives overflows and is redone by the fp32 count; the
    result is the fp32 one at either capacity."""
    f, pids, cams = _dense()
    nq = 300
    for norm in (True, False):
        b = _run(f, pids, cams, nq, dt, norm, key="dense", prefilter_capacity=64)
        info = b.last["prefilter"]
        amb = info["ambiguous"].cpu().numpy()
        print(norm, dt, "capacity 64: fallback", info["fallback_rows"], "ambiguous min", amb.min(), "max", amb.max())
        assert info["capacity"] == 64 and info["fallback_rows"] > 0 and info["dtype"] == dt
        assert info["fallback_rows"] == int((amb > 64).sum())
        if dt == torch.bfloat16:
            assert info["fallback_rows"] > nq // 2
        b = _run(f, pids, cams, nq, dt, norm, key="dense")
        print(norm, dt, "capacity 1024: fallback", b.last["prefilter"]["fallback_rows"])
        assert b.last["prefilter"]["fallback_rows"] == int((b.last["prefilter"]["ambiguous"].cpu().numpy() > 1024).sum())


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_overflow_queries_take_the_general_path(dt, work_split):
    """The label set of test_streamed_h16_overflow_rows_take_general_path: six queries with 400 positives go through the fp32
    materialised kernels, the others (100 positives among them) stay streamed and pre-filtered."""
    rng = np.random.default_rng(5)
    nq, ng, D = 40, 2000, 64
    f = rng.standard_normal((nq + ng, D)).astype(np.float32)
    pids = rng.integers(2, 30, nq + ng)
    pids[nq:nq + 400] = 0; pids[:6] = 0
    pids[nq + 400:nq + 500] = 1; pids[6:9] = 1
    cams = rng.integers(0, 4, nq + ng)
    b = _run(f, pids, cams, nq, dt, True)
    plan = b.last["plan"]
    assert set(plan.overflow.tolist()) == set(range(6)) and plan.cap == 128
    assert (b.last["prefilter"]["ambiguous"][:6] == 0).all()


def test_overflow_queries_with_a_gallery_out_of_range(work_split):
    """Both fallbacks together: the label set above on features x 1e6, which overflow f16.  Every query with a positive list is
    redone by the fp32 count; the six queries without one keep the general path's results and are not counted as redone."""
    rng = np.random.default_rng(5)
    nq, ng, D = 40, 2000, 64
    f = rng.standard_normal((nq + ng, D)).astype(np.float32) * np.float32(1e6)
    pids = rng.integers(2, 30, nq + ng)
    pids[nq:nq + 400] = 0; pids[:6] = 0
    pids[nq + 400:nq + 500] = 1; pids[6:9] = 1
    cams = rng.integers(0, 4, nq + ng)
    b = _run(f, pids, cams, nq, torch.float16, False)
    info = b.last["prefilter"]
    assert set(b.last["plan"].overflow.tolist()) == set(range(6))
    assert info["dtype"] is None and info["fallback_rows"] == nq - 6
    assert (b.last["valid"][:6] == 1).all() and (b.last["first"][:6] >= 0).all()
    b = _run(f, pids, cams, nq, torch.bfloat16, False)
    assert b.last["prefilter"]["dtype"] == torch.bfloat16


def test_range_f16_overflow_takes_the_fp32_path(work_split):
    """Un-normalised features x 1e6 overflow f16: the gallery's statistics are not finite, every row is redone by the fp32 count
    and last["prefilter"]["dtype"] is None; bf16 has the range and pre-filters.  A single overflowing QUERY row has a margin that is
    not finite: every negative of it is listed and re-scored (513 fit the capacity)."""
    f, pids, cams = M.clustered(70, 513, 104, 0)
    big = f * np.float32(1e6)                                   # elements around 1e5: beyond f16's 65504, fine in bf16 and fp32
    b = _run(big, pids, cams, 70, torch.float16, False)
    info = b.last["prefilter"]
    assert info["dtype"] is None and not np.isfinite(info["margin_max"]) and info["fallback_rows"] == 70
    b = _run(big, pids, cams, 70, torch.bfloat16, False)
    assert b.last["prefilter"]["dtype"] == torch.bfloat16 and b.last["prefilter"]["fallback_rows"] == 0
    npos = ((pids[70:][None, :] == pids[:70, None]) & (cams[70:][None, :] != cams[:70, None])).sum(1)
    r = int(np.nonzero(npos > 0)[0][0])                         # a query with positives
    one = f.copy(); one[r] *= np.float32(1e6)
    b = _run(one, pids, cams, 70, torch.float16, False)
    info = b.last["prefilter"]
    assert info["dtype"] == torch.float16 and info["fallback_rows"] == 0 and not np.isfinite(info["margin_max"])
    assert b.last["valid"][r].item() == 1 and info["ambiguous"][r].item() == int((pids[70:] != pids[r]).sum())


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_range_tiny_features(dt, work_split):
    """Features x 2^-20: in f16 every element is a subnormal or zero, the margin (from the rows themselves) is as large as the
    distances and most pairs are listed or repaired -- the result is still the fp32 one."""
    f, pids, cams = M.clustered(70, 513, 104, 1)
    b = _run(f * np.float32(2.0 ** -20), pids, cams, 70, dt, False)
    print(dt, {k: v for k, v in b.last["prefilter"].items() if k != "ambiguous"}, int(b.last["prefilter"]["ambiguous"].max()))
    assert b.last["prefilter"]["dtype"] == dt and np.isfinite(b.last["prefilter"]["margin_max"])


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_compute_chunked_and_model_return_the_fp32_numbers(dt, work_split):
    from centroids_reid_amd import reid_metric as rm
    from centroids_reid_amd.config import get_cfg_defaults
    from centroids_reid_amd.train_ctl_model import CTLModel
    nq = 130
    f, pids, cams = M.clustered(nq, 1000, 64, 0)
    fd = torch.from_numpy(f).cuda()
    ref = rm.R1_mAP(num_query=nq, streamed=True).compute(fd, pids, cams)
    m = rm.R1_mAP(num_query=nq, streamed=True, prefilter=dt)
    got = m.compute_chunked(fd, pids, cams, query_chunk=50)
    assert "distmat" not in m.last and m.last["prefilter"]["dtype"] == dt
    np.testing.assert_array_equal(got[0], ref[0]); assert abs(got[1] - ref[1]) <= 1e-12; np.testing.assert_array_equal(got[2], ref[2])
    cfg = get_cfg_defaults()
    cfg.MODEL.PRETRAINED = False
    base = CTLModel(cfg, num_classes=10, num_query=nq).get_val_metrics(fd, pids, cams)
    model = CTLModel(cfg, num_classes=10, num_query=nq, eval_prefilter=dt)
    out = model.get_val_metrics(fd, pids, cams)
    assert model.r1_map_func.last["prefilter"]["dtype"] == dt
    assert abs(out["mAP"] - base["mAP"]) <= 1e-12 and all(out[k] == base[k] for k in base if k != "mAP")
    assert abs(base["mAP"] - ref[1]) <= 1e-12


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_speculative_second_call_returns_the_same_bits(dt, work_split):
    from centroids_reid_amd import reid_metric as rm
    nq, ng = 64, 1500
    f, pids, cams = M.clustered(nq, ng, 96, 2)
    fd = torch.from_numpy(f).cuda()

    def run():
        m = rm.R1_mAP(num_query=nq, streamed=True, prefilter=dt)
        return m, m.compute(fd, pids, cams)
    rm._CAP_HINT.clear()
    m0, r0 = run()                                        # synchronous: no hint yet
    assert rm._CAP_HINT[(nq, ng)] == m0.last["plan"].cap
    m1, r1 = run()                                        # speculative
    np.testing.assert_array_equal(r1[0], r0[0]); assert r1[1] == r0[1]; np.testing.assert_array_equal(r1[2], r0[2])
    for k in ("valid", "ap", "first"):
        assert torch.equal(m1.last[k], m0.last[k]), k
    assert torch.equal(m1.last["prefilter"]["ambiguous"], m0.last["prefilter"]["ambiguous"])
    _assert_equals_fp32(_fp32(None, fd, pids, cams, nq, True), m1, r1)
    # a hint that is too small: the contraction is redone with the plan's capacity, same bits
    rm._CAP_HINT[(nq, ng)] = 2
    m2, r2 = run()
    assert m2.last["plan"].cap == m0.last["plan"].cap > 2
    for k in ("valid", "ap", "first"):
        assert torch.equal(m2.last[k], m0.last[k]), k


def test_stage_times_on_request():
    from centroids_reid_amd import reid_metric as rm
    f, pids, cams = M.clustered(70, 513, 104, 0)
    fd = torch.from_numpy(f).cuda()
    m = rm.R1_mAP(num_query=70, streamed=True, prefilter=torch.bfloat16)
    m.compute(fd, pids, cams)
    assert "stage_ms" not in m.last["prefilter"]
    m.last = {"prefilter": {"timing": True}}
    m.compute(fd, pids, cams)
    st = m.last["prefilter"]["stage_ms"]
    assert list(st) == ["pack", "poslist", "count", "rescore", "repair"] and all(v >= 0 for v in st.values())


def test_prefilter_allocates_no_matrix():
    """The method of test_prefilter_allocates_no_matrix (top-k), 2048 x 65 536 x 64: the matrix would be 512 MiB.  What the call
    allocates above its inputs: the normalised fp32 rows and the upload copy (2 x 16.5 MiB, as the fp32 path), the packed rows
    (8.3 MiB) and their statistics (1.5 MiB), the ambiguous lists (2048 x 1024 x 4 = 8 MiB), positive lists and histogram
    (3 x 2048 x cap x 4 <= 3 MiB), the plan (< 1 MiB), per-row results: under 56 MiB; the bound is 64 MiB, an eighth of the matrix."""
    from centroids_reid_amd import reid_metric as rm
    nq, ng, D = 2048, 65536, 64
    f, pids, cams = M.clustered(nq, ng, D, 0)
    fd = torch.from_numpy(f).cuda()
    ref = rm.R1_mAP(num_query=nq, streamed=True).compute(fd, pids, cams)
    torch.cuda.synchronize()
    live = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    m = rm.R1_mAP(num_query=nq, streamed=True, prefilter=torch.bfloat16)
    got = m.compute(fd, pids, cams)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - live
    info = m.last["prefilter"]
    print({k: v for k, v in info.items() if k != "ambiguous"}, "ambiguous max", int(info["ambiguous"].max()),
          f"peak above inputs {peak / 2**20:.1f} MiB")
    assert peak < 64 << 20 < nq * ng * 4 // 8 + 1
    assert len(m.last["plan"].overflow) == 0
    np.testing.assert_array_equal(got[0], ref[0]); assert abs(got[1] - ref[1]) <= 1e-12


def test_band_abi_argument_checks():
    """creid_stream_count_band_h16 / creid_stream_count_rescore refuse what the header rules out before any launch, and zero rows
    are a no-op; then one accepted call of each on a hand-made problem."""
    from centroids_reid_amd import _lib as L
    lib, st = L.lib(), L.stream()
    m, n, D, cap, acap = 4, 128, 16, 4, 64
    q = torch.zeros((m, D), device="cuda"); g = torch.zeros((n, D), device="cuda")
    qh, gh = q.half(), g.half()
    qq = torch.zeros(m, device="cuda"); gg = torch.zeros(n, device="cuda"); mg = torch.zeros(m, device="cuda")
    qp = torch.arange(m, dtype=torch.int64, device="cuda"); gp = torch.full((n,), 99, dtype=torch.int64, device="cuda")
    pos_key = torch.full((m, 128), -1, dtype=torch.int32, device="cuda")
    pos_idx = torch.full((m, 128), 0x7fffffff, dtype=torch.int32, device="cuda")
    npos = torch.zeros(m, dtype=torch.int32, device="cuda")
    amb = torch.full((m, 8192), -7, dtype=torch.int32, device="cuda")
    count = torch.zeros(m, dtype=torch.int32, device="cuda")
    hist = torch.zeros((m, 128), dtype=torch.int32, device="cuda")
    flags = torch.full((m,), 7, dtype=torch.uint8, device="cuda")

    def band(m_=m, n_=n, D_=D, dt=L.F16, cap_=cap, acap_=acap, q_=qh, mg_=mg):
        return lib.creid_stream_count_band_h16(L.ptr(q_), L.ptr(gh), L.ptr(qq), L.ptr(gg), m_, n_, D_, dt, L.ptr(qp), L.ptr(gp), cap_,
                                               L.ptr(pos_key), L.ptr(pos_idx), L.ptr(npos), L.ptr(mg_), acap_, L.ptr(amb),
                                               L.ptr(count), L.ptr(hist), st)

    def rescore(m_=m, n_=n, D_=D, cap_=cap, acap_=acap, q_=q, fl=flags):
        return lib.creid_stream_count_rescore(L.ptr(amb), L.ptr(count), m_, acap_, L.ptr(q_), L.ptr(g), L.ptr(qq), L.ptr(gg), n_, D_,
                                              cap_, L.ptr(pos_key), L.ptr(pos_idx), L.ptr(npos), L.ptr(hist), L.ptr(fl), st)
    E_ARG, E_DTYPE, E_SHAPE = -1, -2, -4
    for bad in (96, 32, 16384, 0):
        assert band(acap_=bad) == E_SHAPE and rescore(acap_=bad) == E_SHAPE
    for bad in (3, 256, 0, 1):
        assert band(cap_=bad) == E_SHAPE and rescore(cap_=bad) == E_SHAPE
    assert band(D_=12) == E_SHAPE and band(D_=(1 << 20) + 8) == E_SHAPE and rescore(D_=18) == E_SHAPE
    assert band(dt=L.F32) == E_DTYPE and band(dt=L.BF16X3) == E_DTYPE
    assert band(m_=-1) == E_ARG and band(n_=0) == E_ARG and band(D_=0) == E_ARG and band(q_=None) == E_ARG and band(mg_=None) == E_ARG
    assert rescore(m_=-1) == E_ARG and rescore(n_=0) == E_ARG and rescore(q_=None) == E_ARG and rescore(fl=None) == E_ARG
    assert lib.creid_stream_count_band_h16(None, None, None, None, 0, n, D, L.F16, None, None, cap, None, None, None, None, acap,
                                           None, None, None, st) == 0
    assert lib.creid_stream_count_rescore(None, None, 0, acap, None, None, None, None, n, D, cap, None, None, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert int(flags.min()) == 7 and int(amb.max()) == -7 and int(count.max()) == 0 and int(hist.max()) == 0      # nothing launched
    # accepted.  Rows of ones against a gallery of e_0 .. (distance D + 1 - 2 = D - 1 with these norms) and two positives per query
    # with fp32 keys at D - 2 and D: margin 0 decides every negative into slot 1; margin 1.5 reaches both positives: all listed.
    q.fill_(1.0); qh.copy_(q); g.zero_(); g[:, 0] = 1.0; gh.copy_(g)
    qq.fill_(float(D)); gg.fill_(1.0)
    key = lambda v: int(np.array([v], np.float32).view(np.uint32)[0] ^ 0x80000000) - (1 << 32)
    pos_key.view(-1)[:m * cap].view(m, cap)[:, 0] = key(D - 2.0)
    pos_key.view(-1)[:m * cap].view(m, cap)[:, 1] = key(float(D))
    npos.fill_(2)
    assert band() == 0
    torch.cuda.synchronize()
    assert int(count.max()) == 0 and (hist.view(-1)[:m * cap].view(m, cap)[:, 1] == n).all()
    assert int(hist.view(-1)[:m * cap].view(m, cap)[:, 0].max()) == 0
    hist.zero_(); mg.fill_(1.5)
    mg[3] = 0.0
    assert band() == 0 and rescore() == 0
    torch.cuda.synchronize()
    assert count[:3].tolist() == [n] * 3 and count[3].item() == 0
    assert flags.tolist() == [1, 1, 1, 0]                       # 128 listed pairs > capacity 64: nothing added for those rows
    h = hist.view(-1)[:m * cap].view(m, cap)
    assert h[:3].sum().item() == 0 and h[3, 1].item() == n
    count.zero_(); hist.zero_()
    assert band(acap_=128) == 0 and rescore(acap_=128) == 0
    torch.cuda.synchronize()
    assert flags.tolist() == [0, 0, 0, 0]
    assert (hist.view(-1)[:m * cap].view(m, cap)[:, 1] == n).all()      # the re-score places them where the decided ones went
    cols = amb.view(-1)[:m * 128].view(m, 128)[:3].sort(dim=1).values
    assert (cols == torch.arange(n, device="cuda", dtype=torch.int32)).all()
    # a listed column outside the gallery: flagged, nothing added
    hist.zero_()
    amb.view(-1)[5] = n
    assert rescore(acap_=128) == 0
    torch.cuda.synchronize()
    assert flags.tolist() == [1, 0, 0, 0] and hist.view(-1)[:cap].sum().item() == 0
