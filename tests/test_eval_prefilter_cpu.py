"""CPU: the rule of the banded count behind R1_mAP(streamed=True, prefilter=...) on a numpy model (tests/eval_prefilter_model.py):
a negative whose 16-bit distance, widened by the proven margin and rounded outwards, falls between two positives' fp32 keys is
placed where the fp32 count places it; the others are listed, and placing those with their fp32 distance completes the fp32
histogram.  Plus the outward rounding helpers and the argument errors of the Python surface."""
import numpy as np
import pytest
import torch

import eval_prefilter_model as M


def _labels(rng, nq, ng, npid, ncam):
    return rng.integers(0, npid, nq + ng), rng.integers(0, ncam, nq + ng)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("norm", [True, False], ids=["unit", "raw"])
@pytest.mark.parametrize("kind", ["clustered", "normal-dup"])
def test_rule_places_decided_pairs_where_fp32_does(kind, norm, dt):
    """Clustered rows (few pairs ambiguous) and N(0,1) rows with random pids and a quarter of the gallery duplicated (exact ties
    between a positive and a negative, a zero-distance positive; most pairs ambiguous in bf16).  banded_count asserts, pair by pair,
    that a decided slot is the fp32 slot, that a skipped pair is one the fp32 count skips, and that decided + exactly placed
    ambiguous pairs == the full histogram."""
    nq, ng, D = 24, 400, 72
    if kind == "clustered":
        f, pids, cams = M.clustered(nq, ng, D, 3)
    else:
        rng = np.random.default_rng(11)
        f = rng.standard_normal((nq + ng, D)).astype(np.float32)
        pids, cams = _labels(rng, nq, ng, 12, 3)
        src = rng.integers(nq, nq + ng, ng // 4); dst = rng.integers(nq, nq + ng, ng // 4)
        f[dst] = f[src]
        f[nq + 7] = f[3]; pids[nq + 7] = pids[3]; cams[nq + 7] = cams[3] + 1
    if norm:
        f = M.l2n(f)
    d, dh, m32 = M.emulate(f[:nq], f[nq:], dt)
    full, decided, amb = M.banded_count(d, dh, m32, pids[:nq], pids[nq:], cams[:nq], cams[nq:])
    print(kind, norm, dt, "ambiguous per row: mean %.1f max %d of %d; decided %d of %d counted" %
          (amb.mean(), amb.max(), ng, decided.sum(), full.sum()))
    assert full.sum() > 0 and decided.sum() > 0 and amb.sum() > 0                # the rule decides some and lists some
    assert decided.sum() + amb.sum() >= full.sum()


def test_rule_with_exact_ties_and_a_zero_margin():
    """Margin 0 and dh == d: the band is one step wide on either side, so only a negative within a step of a positive is listed --
    the exact ties of duplicated rows among them -- and everything else is decided."""
    rng = np.random.default_rng(5)
    nq, ng, D = 8, 200, 16
    f = rng.standard_normal((nq + ng, D)).astype(np.float32)
    pids, cams = _labels(rng, nq, ng, 4, 2)
    f[nq + 50:nq + 100] = f[nq:nq + 50]                                          # exact ties, positives against negatives among them
    d, _, _ = M.emulate(f[:nq], f[nq:], "f16")
    full, decided, amb = M.banded_count(d, d, np.zeros(nq, np.float32), pids[:nq], pids[nq:], cams[:nq], cams[nq:])
    assert amb.sum() > 0 and decided.sum() > 0.8 * full.sum()


def test_non_finite_band_is_ambiguous():
    rng = np.random.default_rng(6)
    nq, ng, D = 4, 64, 8
    f = rng.standard_normal((nq + ng, D)).astype(np.float32)
    pids, cams = _labels(rng, nq, ng, 3, 2)
    d, dh, m32 = M.emulate(f[:nq], f[nq:], "bf16")
    m32 = m32.copy(); m32[0] = np.inf; m32[1] = np.nan
    dh = dh.copy(); dh[2, ::3] = np.nan; dh[3, ::2] = np.inf
    full, decided, amb = M.banded_count(d, dh, m32, pids[:nq], pids[nq:], cams[:nq], cams[nq:])
    assert amb[0] == (pids[nq:] != pids[0]).sum() and amb[1] == (pids[nq:] != pids[1]).sum()
    assert decided[:2].sum() == 0


EDGES = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.17549435e-38, 1.0, -1.0, 3.4028235e38, -3.4028235e38,
                  1.5, 2.0 ** -24, 1e30, -1e30], np.float32)


def test_outward_rounding_never_rounds_inward():
    """add_up(a, b) >= a + b and sub_down(a, b) <= a - b in exact arithmetic (float64 holds the sum of two fp32 numbers whose
    exponents are within 2^29 of each other exactly; the random pairs here stay within that, the edge pairs are compared through
    exact fractions), strictly outward in key order past either zero, by at most two steps; a result that is not finite -- the
    sum overflowed, or FLT_MAX stepped to inf -- makes the pair ambiguous, and non-finite inputs stay."""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = (rng.standard_normal(20000) * np.exp2(rng.integers(-12, 12, 20000))).astype(np.float32)
    b = (rng.standard_normal(20000) * np.exp2(rng.integers(-12, 12, 20000))).astype(np.float32)
    b[:5000] = np.abs(b[:5000]) * np.float32(2.0 ** -10)                      # the margin's shape: small and non-negative
    up, dn = M.add_up(a, b), M.sub_down(a, b)
    s, t = a.astype(np.float64) + b.astype(np.float64), a.astype(np.float64) - b.astype(np.float64)
    assert (up.astype(np.float64) > s).all() and (dn.astype(np.float64) < t).all()
    rn_s, rn_t = (a + b).astype(np.float32), (a - b).astype(np.float32)
    assert (np.abs(M.mono_key(up).astype(np.int64) - M.mono_key(rn_s).astype(np.int64)) <= 2).all()
    assert (np.abs(M.mono_key(dn).astype(np.int64) - M.mono_key(rn_t).astype(np.int64)) <= 2).all()
    below_max = Fraction(float(np.nextafter(M.FLT_MAX, np.float32(0))))     # only a result at FLT_MAX steps to inf
    for x in EDGES:
        for y in EDGES:
            u, v = M.add_up(x, y), M.sub_down(x, y)
            exact_s, exact_t = Fraction(float(x)) + Fraction(float(y)), Fraction(float(x)) - Fraction(float(y))
            if np.isfinite(u):                                 # (a non-finite end makes the pair ambiguous: nothing to prove)
                assert Fraction(float(u)) > exact_s, (x, y, u)
            else:
                assert abs(exact_s) > below_max
            if np.isfinite(v):
                assert Fraction(float(v)) < exact_t, (x, y, v)
            else:
                assert abs(exact_t) > below_max
            # in key order the band's ends lie outside BOTH zeros
            if exact_s == 0:
                assert M.mono_key(u) > M.mono_key(np.float32(0.0))
            if exact_t == 0:
                assert M.mono_key(v) < M.mono_key(np.float32(-0.0))
    for bad in (np.inf, -np.inf, np.nan):
        for f in (M.add_up, M.sub_down):
            r = f(np.float32(bad), np.float32(1.0))
            assert (np.isnan(r) and np.isnan(bad)) or r == bad
    assert M.add_up(np.float32(3.4028235e38), np.float32(0.0)) == np.inf         # FLT_MAX steps to inf: not finite, ambiguous
    assert M.sub_down(np.float32(-3.4028235e38), np.float32(0.0)) == -np.inf
    assert M.add_up(np.float32(0), np.float32(0)).view(np.uint32) == 1 and M.sub_down(np.float32(0), np.float32(0)).view(np.uint32) == 0x80000001


def test_surface_errors_need_no_device():
    from centroids_reid_amd import _lib as L, reid_metric as rm
    assert rm.EVAL_PREFILTER_CAPACITY == 1024
    ok = rm.R1_mAP(num_query=2, streamed=True, prefilter=torch.bfloat16)
    assert ok.prefilter == torch.bfloat16 and ok.prefilter_capacity == 1024
    assert rm.R1_mAP(num_query=2, streamed=True).prefilter is None
    for kw in (dict(streamed=False), dict(compute_dtype=torch.bfloat16), dict(compute_dtype=torch.float16),
               dict(dist_func="cosine"), dict(reranking=True), dict(prefilter=torch.float32), dict(prefilter_capacity=96),
               dict(prefilter_capacity=32), dict(prefilter_capacity=16384)):
        args = dict(num_query=2, streamed=True, prefilter=torch.float16)
        args.update(kw)
        with pytest.raises(L.CreidError):
            rm.R1_mAP(**args)

    class _Feats(torch.Tensor):                            # passes compute()'s device test without a device
        is_cuda = True
    with pytest.raises(L.CreidError, match="respect_camids"):
        ok.compute(torch.zeros(4, 8).as_subclass(_Feats), [0, 0, 1, 1], [[0], [1], [0], [1]], respect_camids=True)
