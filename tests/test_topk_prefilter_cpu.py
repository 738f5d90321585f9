"""CPU: reid_metric.prefilter_margin -- the per-row bound m_i >= |16-bit distance - fp32 distance| that
topk_stream(prefilter=...) widens its thresholds by -- against float64 on the rows themselves.  The rounding to bf16 / f16 is
torch's on the CPU (round to nearest even, the bits creid_prefilter_pack must produce); the statistics are float64 sums."""
import numpy as np
import pytest
import torch

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
M, N = 8, 64
U = 2.0 ** -24


def _rounded(x, dt):
    """fp32 -> dt -> float64 (exact)"""
    return torch.from_numpy(x).to(DTYPES[dt]).to(torch.float64).numpy()


def _stats(x, xh):
    x = x.astype(np.float64)
    return ((x - xh) ** 2).sum(1), (xh ** 2).sum(1), (x ** 2).sum(1)


def _rows(kind, D, dt, seed):
    rng = np.random.default_rng(seed)
    if kind == "aligned":                                   # q = g = a * ones, a a quarter of a 16-bit spacing above 1
        a = np.float32(1 + 2.0 ** (-9 if dt == "bf16" else -12))
        return np.full((M, D), a, np.float32), np.full((N, D), a, np.float32)
    q = rng.standard_normal((M, D)).astype(np.float32)
    g = rng.standard_normal((N, D)).astype(np.float32)
    if kind == "unit":
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        g /= np.linalg.norm(g, axis=1, keepdims=True)
    elif kind == "tiny":                                    # f16: subnormals and underflow to zero
        q *= np.float32(2.0 ** -20)
        g *= np.float32(2.0 ** -20)
    elif kind == "big":
        q *= np.float32(300)
        g *= np.float32(300)
    return q, g


def _margin_parts(q, g, qh, gh, D):
    from centroids_reid_amd import reid_metric as rm
    e2, h2, x2 = _stats(q, qh)
    ge2, gh2, gx2 = (v.max() for v in _stats(g, gh))
    return rm.prefilter_margin(e2, h2, x2, ge2, gh2, gx2, gx2, D, parts=True)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("D", [8, 64, 100])
@pytest.mark.parametrize("kind", ["normal", "unit", "tiny", "big", "aligned"])
def test_data_part_bounds_the_rounding_of_the_operands(kind, D, dt):
    """Dh and D: float64 distances qq + gg - 2 dot of the rounded and of the unrounded rows with the SAME norms (the fp32 rows'
    own), so they differ by 2 (q.g - qh.gh): |Dh - D| <= the data part everywhere; on the aligned rows Cauchy-Schwarz is an
    equality -- D 2^-9 (a + 1) on both sides, doubled (bf16; 2^-12 for f16) -- so a margin that is merely huge fails."""
    q, g = _rows(kind, D, dt, 100 * D + len(kind))
    qh, gh = _rounded(q, dt), _rounded(g, dt)
    if kind == "tiny" and dt == "f16":
        assert (qh == 0).any() and (np.abs(qh[qh != 0]) < 2.0 ** -14).all()     # underflow and subnormals, nothing else
    q64, g64 = q.astype(np.float64), g.astype(np.float64)
    diff = np.abs(2.0 * (q64 @ g64.T - qh @ gh.T))                               # |Dh - D|: the norms cancel
    data, arith = _margin_parts(q, g, qh, gh, D)
    assert data.shape == (M,) and arith.shape == (M,)
    scale = 2.0 * (np.abs(q64) @ np.abs(g64).T).max()
    assert (diff <= data[:, None] * (1 + 1e-12) + 1e-15 * scale).all()
    assert (arith > 0).all()
    if kind == "aligned":
        a = float(q[0, 0])
        step = 2.0 ** (-9 if dt == "bf16" else -12)
        assert qh[0, 0] == 1.0
        np.testing.assert_allclose(diff, 2.0 * D * step * (a + 1), rtol=1e-12)
        np.testing.assert_allclose(data, 2.0 * D * step * (a + 1), rtol=1e-12)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["normal", "unit", "tiny", "big"])
def test_full_margin_covers_fp32_emulations_of_both_kernels(kind, dt):
    """Both kernels emulated in numpy fp32 with the same fp32 norms: the fp32 kernel as the k-ordered chain (product and sum
    rounded separately here, fused on the device: both inside the 2 D u rule), the 16-bit kernel as fp32 accumulation of the
    exact products of the rounded rows in blocks of 16.  |dh - d| <= m_i for every pair."""
    from centroids_reid_amd import reid_metric as rm
    D = 100
    q, g = _rows(kind, D, dt, 7)
    qh, gh = _rounded(q, dt).astype(np.float32), _rounded(g, dt).astype(np.float32)
    qq = (q.astype(np.float64) ** 2).sum(1).astype(np.float32)
    gg = (g.astype(np.float64) ** 2).sum(1).astype(np.float32)
    acc = np.zeros((M, N), np.float32)
    for k in range(D):
        acc = (np.outer(q[:, k], g[:, k]).astype(np.float32) + acc).astype(np.float32)
    acch = np.zeros((M, N), np.float32)
    for k0 in range(0, D, 16):
        blk = qh[:, k0:k0 + 16].astype(np.float64) @ gh[:, k0:k0 + 16].astype(np.float64).T
        acch = (acch.astype(np.float64) + blk).astype(np.float32)
    s = (qq[:, None] + gg[None, :]).astype(np.float32)
    d = (s.astype(np.float64) - 2.0 * acc.astype(np.float64)).astype(np.float32)
    dh = (s.astype(np.float64) - 2.0 * acch.astype(np.float64)).astype(np.float32)
    e2, h2, x2 = _stats(q, qh.astype(np.float64))
    ge2, gh2, gx2 = (v.max() for v in _stats(g, gh.astype(np.float64)))
    x2 = np.maximum(x2, qq.astype(np.float64))
    margin = rm.prefilter_margin(e2, h2, x2, ge2, gh2, gx2, max(gx2, float(gg.max())), D)
    assert (np.abs(dh.astype(np.float64) - d.astype(np.float64)) <= margin[:, None]).all()


def test_margin_is_monotone_in_every_argument():
    from centroids_reid_amd import reid_metric as rm
    rng = np.random.default_rng(5)
    base = [rng.uniform(0.1, 2.0, 16) for _ in range(3)] + [float(v) for v in rng.uniform(0.1, 2.0, 4)] + [64]
    ref = rm.prefilter_margin(*base)
    d_ref, a_ref = rm.prefilter_margin(*base, parts=True)
    np.testing.assert_array_equal(ref, d_ref + a_ref)
    for i in range(len(base)):
        for factor in (1.0 + 2.0 ** -20, 1.5, 1e6):
            args = list(base)
            args[i] = base[i] * factor if i < 7 else int(base[i] * factor) + 1
            assert (rm.prefilter_margin(*args) > ref).all(), (i, factor)
    zero = rm.prefilter_margin(np.zeros(4), np.zeros(4), np.zeros(4), 0.0, 0.0, 0.0, 0.0, 2048)
    np.testing.assert_array_equal(zero, np.zeros(4))


def test_non_finite_statistics_give_a_non_finite_margin():
    from centroids_reid_amd import reid_metric as rm
    base = [np.array([1e-6, 1e-6]), np.array([1.0, 1.0]), np.array([1.0, 1.0]), 1e-6, 1.0, 1.0, 1.0, 2048]
    assert np.isfinite(rm.prefilter_margin(*base)).all()
    for i in range(7):
        for bad in (np.inf, np.nan):
            args = list(base)
            if i < 3:
                args[i] = np.array([bad, base[i][1]])
                out = rm.prefilter_margin(*args)
                assert not np.isfinite(out[0]) and np.isfinite(out[1])            # per row
            else:
                args[i] = bad
                assert not np.isfinite(rm.prefilter_margin(*args)).any()
    # the same with zeros on the other side of the product (inf * 0)
    with np.errstate(invalid="ignore"):
        assert not np.isfinite(rm.prefilter_margin(np.array([np.inf]), np.array([0.0]), np.array([0.0]), 0.0, 0.0, 0.0, 0.0, 8)).any()
    # rows that overflow f16: the statistics of the rounded rows are infinite
    q, g = _rows("normal", 64, "f16", 3)
    q, g = q * np.float32(1e5), g * np.float32(1e5)
    qh, gh = _rounded(q, "f16"), _rounded(g, "f16")
    assert np.isinf(qh).any() and np.isinf(gh).any()
    with np.errstate(invalid="ignore", over="ignore"):
        data, arith = _margin_parts(q, g, qh, gh, 64)
    assert not np.isfinite(data + arith).any()                                   # the gallery maxima enter every row


def test_margin_accepts_tensors_and_numpy_alike():
    from centroids_reid_amd import reid_metric as rm
    q, g = _rows("unit", 64, "bf16", 9)
    qh, gh = _rounded(q, "bf16"), _rounded(g, "bf16")
    e2, h2, x2 = _stats(q, qh)
    gm = [float(v.max()) for v in _stats(g, gh)]
    ref = rm.prefilter_margin(e2, h2, x2, *gm, gm[2], 64)
    got = rm.prefilter_margin(torch.from_numpy(e2), torch.from_numpy(h2), torch.from_numpy(x2), *gm, gm[2], 64)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64
    np.testing.assert_allclose(got.numpy(), ref, rtol=1e-15)
    # sizes of the issue's simulation: unit rows, D = 2048 -- about 7.5e-3 for bf16 and 1.3e-3 for f16, dominated by the data part
    for dt, lo, hi in (("bf16", 2e-3, 2e-2), ("f16", 3e-4, 3e-3)):
        q, g = _rows("unit", 2048, dt, 11)
        data, arith = _margin_parts(q, g, _rounded(q, dt), _rounded(g, dt), 2048)
        assert (lo < data + arith).all() and (data + arith < hi).all(), (dt, data + arith)
