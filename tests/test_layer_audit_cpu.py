"""CPU: the per-layer audit's comparison (tests/layer_audit.py) on torch emulations of the kernels' arithmetic.  Each unmutated
emulation passes; each mutation a kernel could plausibly carry -- truncating bf16 rounding, a dropped 32-wide k-slice, a dropped
128-row statistics tile, a 1 / (rows * 128) count, one channel's ReLU bits shifted in the packed bytes, a dropped bf16x3 cross
term -- is caught, the tile, truncation and k-slice mutations also at a production row count (131072 rows, 1/1024 of them in
the dropped tile) and depth (1/16 of K).  The same functions judge the real training step in tests/test_layer_audit_gpu.py."""
import math

import pytest
import torch

import layer_audit as la

BF = torch.bfloat16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _trunc_bf16(v):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero)"""
    return (v.float().contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).to(BF)


def _conv32(x, w, s, p):
    """the kernels' accumulation: products of the stored operands summed in fp32"""
    k, cout, cin = w.shape[2], w.shape[0], w.shape[1]
    xp = torch.nn.functional.pad(x.float(), (0, 0, p, p, p, p))
    oh, ow = (xp.shape[1] - k) // s + 1, (xp.shape[2] - k) // s + 1
    y = torch.zeros(xp.shape[0] * oh * ow, cout)
    for r, c, (sr, sc) in la._taps(k, s, oh, ow):
        y += xp[:, sr, sc, :].reshape(-1, cin) @ w.float()[:, :, r, c].t()
    return y.view(xp.shape[0], oh, ow, cout)


def _conv_case(seed=0, B=2, H=10, W=6, cin=96, cout=64, k=3, s=1):
    g = _gen(seed)
    x = torch.randn(B, H, W, cin, generator=g).to(BF)
    w = (torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)).to(BF)
    return x, w, k, s, k // 2


def _audit_conv(got, x, w, k, s, p, dt=BF, split=False):
    a = la.Audit("cpu")
    ref = la.conv_fwd(x, w.double(), s, p)
    mag = la.conv_fwd(x.double().abs(), w.double().abs(), s, p)
    K = w.shape[1] * k * k
    b = K * la.U * mag + (la.SPLIT * mag if split else 0.0)
    a.check("conv", "fwd", got, ref, b, dt, sigma=math.sqrt(K) * la.U * mag + (la.SPLIT * mag if split else 0.0),
            rel_bar=2e-5 if split else None, max_rms=1e-4 if split else None)
    return a


def test_conv_forward_passes_and_truncation_is_caught():
    x, w, k, s, p = _conv_case()
    acc = _conv32(x, w, s, p)
    assert not _audit_conv(acc.to(BF), x, w, k, s, p).failures
    bad = _audit_conv(_trunc_bf16(acc), x, w, k, s, p)
    assert any("bias" in f for f in bad.failures), bad.failures


def test_dropped_k_slice_is_caught():
    x, w, k, s, p = _conv_case(seed=1, k=1)
    xm = x.clone()
    xm[..., 32:64] = 0                                    # the kernel skips the second 32-wide slice of the k loop
    assert not _audit_conv(_conv32(x, w, s, p).to(BF), x, w, k, s, p).failures
    assert _audit_conv(_conv32(xm, w, s, p).to(BF), x, w, k, s, p).failures


def _stats_emul(y32, rows_per_tile=128, drop_tile=None, count=None):
    """conv-epilogue statistics: fp32 (sum, sumsq) per 128-row tile, fp64 over the tiles, divided by the row count"""
    M = y32.shape[0]
    rows = (M + rows_per_tile - 1) // rows_per_tile
    s1 = torch.zeros(y32.shape[1], dtype=torch.float64)
    s2 = torch.zeros_like(s1)
    for t in range(rows):
        if t == drop_tile:
            continue
        blk = y32[t * rows_per_tile:(t + 1) * rows_per_tile]
        s1 += blk.sum(0).double()
        s2 += (blk * blk).sum(0).double()
    n = count or M
    mean = s1 / n
    var = (s2 / n - mean * mean).clamp_min(0)
    return mean.float(), (1.0 / torch.sqrt(var + 1e-5)).float()


def _audit_stats(mean, invstd, x, w, k, s, p):
    a = la.Audit("cpu")
    ref = la.conv_fwd(x, w.double(), s, p).reshape(-1, w.shape[0])
    mag = la.conv_fwd(x.double().abs(), w.double().abs(), s, p).reshape(-1, w.shape[0])
    m_ref, _, i_ref = la.batch_stats(ref, 1e-5)
    dm, di, _, _ = la.stats_bound(ref, w.shape[1] * k * k * la.U * mag, 1e-5)
    a.check("conv", "mean", mean, m_ref, dm, torch.float32, sigma=dm, bias=False)
    a.check("conv", "invstd", invstd, i_ref, di, torch.float32, sigma=di, bias=False)
    return a


def test_statistics_tile_and_count_mutations_are_caught():
    x, w, k, s, p = _conv_case(seed=2, B=3, H=10, W=10, cin=64, k=1)     # M = 300: a partial third tile
    # a constant input channel gives every output a mean the statistics must get right
    x2 = torch.cat([x, torch.ones(*x.shape[:3], 1, dtype=BF)], 3)
    w2 = torch.cat([w, torch.full((w.shape[0], 1, 1, 1), 0.5).to(BF)], 1)
    y32 = _conv32(x2, w2, s, p).reshape(-1, w.shape[0])
    assert not _audit_stats(*_stats_emul(y32), x2, w2, k, s, p).failures
    assert _audit_stats(*_stats_emul(y32, drop_tile=1), x2, w2, k, s, p).failures
    assert _audit_stats(*_stats_emul(y32, count=3 * 128), x2, w2, k, s, p).failures


def _apply_emul(x, mean, invstd, gamma, beta):
    """bn2d_apply_mask: fp32 scale / shift, fma, ReLU, the bits of the fp32 value, one rounding"""
    sc = invstd * gamma
    sh = beta - mean * sc
    v = torch.clamp_min(x.float() * sc + sh, 0.0)
    bits = (v > 0).view(-1, 8).to(torch.uint8)
    packed = (bits << torch.arange(8, dtype=torch.uint8)).sum(1).to(torch.uint8)
    return v.to(BF), packed


def test_relu_bits_shifted_channel_is_caught():
    g = _gen(3)
    M, Cc = 256, 64
    x = torch.randn(M, Cc, generator=g).to(BF)
    mean, invstd = x.float().mean(0), 1.0 / x.float().std(0)
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1
    a_out, packed = _apply_emul(x, mean, invstd, gamma, beta)
    ref = torch.clamp_min((x.double() - mean.double()) * invstd.double() * gamma.double() + beta.double(), 0.0)
    b = la.affine_bound(x.double(), (invstd * gamma).double(), (beta - mean * invstd * gamma).double(), [])
    au = la.Audit("cpu")
    au.check("bn", "apply", a_out, ref, b, BF, sigma=b)
    au.relu_bits("bn", packed, a_out, ref, BF)
    assert not au.failures, au.failures
    shifted = packed.view(M, Cc // 8).clone()
    b5 = (shifted[:, 0] >> 5) & 1
    b6 = (shifted[:, 0] >> 6) & 1
    assert bool((b5 != b6).any())
    shifted[:, 0] = (shifted[:, 0] & ~(1 << 5)) | (b6 << 5)              # channel 5 carries channel 6's bits
    bad = la.Audit("cpu")
    assert bad.relu_bits("bn", shifted.reshape(-1), a_out, ref, BF) > 0 and bad.failures


def test_relu_bits_f16_underflow_exemption_is_narrow():
    """f16: a bit set over an activation that rounded to 0 is accepted only where the value is below 2^-24"""
    M, Cc = 8, 8
    a = torch.ones(M, Cc, dtype=torch.float16)
    a[3, 2] = 0
    packed = torch.full((M,), 0xFF, dtype=torch.uint8)                 # every bit set
    ref = torch.ones(M, Cc, dtype=torch.float64)
    ref[3, 2] = 2.0 ** -26                                             # rounds to 0 in f16 after a positive fp32 value
    au = la.Audit("cpu")
    assert au.relu_bits("bn", packed, a, ref, torch.float16) == 0 and not au.failures
    ref[3, 2] = 1e-3                                                   # a real value: the stored 0 is wrong
    bad = la.Audit("cpu")
    assert bad.relu_bits("bn", packed, a, ref, torch.float16) == 1 and bad.failures
    bf = la.Audit("cpu")                                               # bf16 has no such exemption
    ref[3, 2] = 2.0 ** -26
    assert bf.relu_bits("bn", packed, a.to(BF), ref, BF) == 1


def _x3_emul(x, w, s, p, drop_cross=False):
    """bf16x3: hi = bf16(v), lo = bf16(v - hi) for both operands; lo*hi + hi*lo + hi*hi in fp32"""
    xh = x.to(BF); xl = (x - xh.float()).to(BF)
    wh = w.to(BF); wl = (w - wh.float()).to(BF)
    y = _conv32(xh, wh, s, p) + _conv32(xl, wh, s, p)
    if not drop_cross:
        y = y + _conv32(xh, wl, s, p)
    return y


def test_x3_dropped_cross_term_is_caught():
    g = _gen(4)
    x = torch.randn(2, 8, 6, 64, generator=g)
    w = torch.randn(32, 64, 3, 3, generator=g) / 24.0
    assert not _audit_conv(_x3_emul(x, w, 1, 1), x, w, 3, 1, 1, dt=torch.float32, split=True).failures
    assert _audit_conv(_x3_emul(x, w, 1, 1, drop_cross=True), x, w, 3, 1, 1, dt=torch.float32, split=True).failures


@pytest.mark.parametrize("M", [300, 512])
def test_bn_backward_bound_holds_for_the_emulated_kernel(M):
    """bn2d_bwd: fp32 per-128-row partials of (dy, dy xhat), fp64 over them, fp32 coefficients, one rounding; truncating that
    rounding is caught"""
    g = _gen(5 + M)
    Cc = 64
    x = (torch.randn(M, Cc, generator=g) * 2 + 1).to(BF)
    dy32 = torch.randn(M, Cc, generator=g) * 1e-3
    dy = dy32.to(BF)
    mean, invstd = x.float().mean(0), (1.0 / x.float().std(0))
    gamma = torch.rand(Cc, generator=g) + 0.5
    xhat = (x.float() - mean) * invstd
    s1 = torch.zeros(Cc, dtype=torch.float64); s2 = torch.zeros_like(s1)
    for t in range(0, M, 128):
        s1 += dy[t:t + 128].float().sum(0).double()                    # (every route sums the stored, rounded gradient)
        s2 += (dy[t:t + 128].float() * xhat[t:t + 128]).sum(0).double()
    k1 = gamma * invstd
    a1, a2 = (s1 / M).float(), (s2 / M).float()
    dx32 = k1 * dy.float() + (-k1 * invstd * a2) * x.float() + (-k1 * a1 + k1 * invstd * a2 * mean)
    ref, r1, r2, parts = la.bn_bwd(x, dy, mean, invstd, gamma)
    b, ds1, ds2 = la.bn_bwd_bound(x, dy, parts, M)
    au = la.Audit("cpu")
    au.check("bn", "dx", dx32.to(BF), ref, b, BF, sigma=b / 4)
    au.check("bn", "dbeta", s1.float(), r1.view(-1), ds1.view(-1), torch.float32, sigma=ds1.view(-1), bias=False)
    au.check("bn", "dgamma", s2.float(), r2.view(-1), ds2.view(-1), torch.float32, sigma=ds2.view(-1), bias=False)
    assert not au.failures, au.failures
    bad = la.Audit("cpu")
    bad.check("bn", "dx", _trunc_bf16(dx32), ref, b, BF, sigma=b / 4)
    assert bad.failures


def test_mutations_are_caught_at_production_size():
    """layer1's 1 x 1 64 -> 64 convolution at the benchmark batch (M = 64 x 64 x 32 = 131072 rows): one dropped 128-row
    statistics tile (1/1024 of the rows), statistics of bf16-truncated outputs, a truncated output; and one dropped 32-wide
    k-slice of a 512-deep reduction (1/16 of K)"""
    g = _gen(7)
    x = torch.randn(64, 64, 32, 64, generator=g).to(BF)
    x = torch.cat([x, torch.ones(64, 64, 32, 1, dtype=BF)], 3)          # a constant channel: outputs with a mean
    w = torch.cat([torch.randn(64, 64, 1, 1, generator=g) / 8.0, torch.full((64, 1, 1, 1), 0.5)], 1).to(BF)
    y32 = _conv32(x, w, 1, 0).reshape(-1, 64)
    assert not _audit_stats(*_stats_emul(y32), x, w, 1, 1, 0).failures
    assert _audit_stats(*_stats_emul(y32, drop_tile=517), x, w, 1, 1, 0).failures
    assert _audit_stats(*_stats_emul(_trunc_bf16(y32).float()), x, w, 1, 1, 0).failures
    assert not _audit_conv(y32.view(64, 64, 32, 64).to(BF), x, w, 1, 1, 0).failures
    assert any("bias" in f for f in _audit_conv(_trunc_bf16(y32).view(64, 64, 32, 64), x, w, 1, 1, 0).failures)
    xk, wk, k, s, p = _conv_case(seed=8, B=2, H=16, W=8, cin=512, k=1)
    xm = xk.clone()
    xm[..., 256:288] = 0
    assert not _audit_conv(_conv32(xk, wk, s, p).to(BF), xk, wk, k, s, p).failures
    assert _audit_conv(_conv32(xm, wk, s, p).to(BF), xk, wk, k, s, p).failures
