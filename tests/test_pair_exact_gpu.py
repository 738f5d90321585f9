"""GPU: the block-boundary kernel (conv_pair.hip: creid_bottleneck_c3_c1_fwd_affine / creid_bottleneck_c3_c1_fwd_stats), exactly,
in the convention of tests/conv_exact.py: small-integer operands, an fp64 reference that is exact, 16-bit outputs equal to the one
correctly rounded value.  Both ABI entry points are called directly, for bf16 and f16.

Operands: a2, w3, w1 in {-2..2}, folded scales from {-1, 0.5, 1, 2}, integer shifts and residuals.  |a2 . w3| <= 256, so the
affine result is a multiple of 1/2 below 2^10: exact in fp32.  The reference applies the kernel's documented arithmetic: exact
accumulate, exact affine, round to the storage type, add the residual, ReLU, round; the second convolution runs on that STORED
value (multiples of 1/2; sum |o| |w1| < 2^23 is asserted, so every partial sum is exact in fp32 in any order), then affine, ReLU,
round.  Outputs are compared as values, bit for bit (+0 == -0): a missing, duplicated or misplaced product term moves a result by
at least 1/2.  The weights have distinct rows and distinct columns (asserted): a wrong swizzle key or k-chunk order cannot cancel.

Statistics variant: {-1, 0, 1} operands with eight non-zeros per weight row keep every tile's column sum and sum of squares a
multiple of 1/4 below 2^22 (asserted on the host), so the [tiles][2][64] partials must be bit-equal in any summation order.

Every output has 128 guard rows of a sentinel bit pattern behind row M (they must stay untouched) and is pre-filled with NaN.
Refusals (other channel counts, fp32, M % 128 != 0 for the statistics variant) return their documented codes and write nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF, F16 = torch.bfloat16, torch.float16
GUARD, SENT16, SENT32 = 128, 0x5A5A, 0x5A5A5A5A
NAN16 = {BF: 0x7FC0, F16: 0x7E00}
AFFINE_CASES = [(M, 0) for M in (1, 127, 128, 129, 255, 257)] + [(641, w) for w in (1, 2, 3)]    # 641: six tiles, the last of one row
STATS_CASES = [(M, w) for M in (128, 384, 1280) for w in (0, 1, 3)]


def _rd(t, dt):
    return t.float().to(dt).double()


def _distinct(w):
    return len(torch.unique(w, dim=0)) == w.shape[0] and len(torch.unique(w.t(), dim=0)) == w.shape[1]


def _guarded(M, C, dt):
    """[M + GUARD, C] of the 16-bit type: NaN in the M rows the kernel owns, the sentinel behind them"""
    buf = torch.full((M + GUARD, C), SENT16, dtype=torch.int16, device="cuda")
    buf[:M] = NAN16[dt]
    return buf


def _operands(M, dt, sparse, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def ints(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=g, device="cuda").double()

    def pick(vals, n):
        return torch.tensor(vals, dtype=torch.float64, device="cuda")[torch.randint(0, len(vals), (n,), generator=g, device="cuda")]

    if sparse:
        a2, res = ints((M, 64), -1, 1), ints((M, 256), -1, 1)
        w3 = torch.zeros(256, 64, dtype=torch.float64, device="cuda")
        idx = torch.rand(256, 64, generator=g, device="cuda").argsort(1)[:, :8]               # eight non-zeros per row
        w3.scatter_(1, idx, pick([-1.0, 1.0], 256 * 8).view(256, 8))
        # w1 [64][256]: column c is non-zero in rows c % 64 and (c % 64 + 1 + c // 64) % 64: eight per row, all columns distinct
        w1 = torch.zeros(64, 256, dtype=torch.float64, device="cuda")
        c = torch.arange(256, device="cuda")
        w1[c % 64, c] = pick([-1.0, 1.0], 256)
        w1[(c % 64 + 1 + c // 64) % 64, c] = pick([-1.0, 1.0], 256)
        assert bool(((w3 != 0).sum(1) == 8).all()) and bool(((w1 != 0).sum(1) == 8).all())
        sh3 = ints((256,), -2, 2)
    else:
        a2, res = ints((M, 64), -2, 2), ints((M, 256), -4, 4)
        w3, w1 = ints((256, 64), -2, 2), ints((64, 256), -2, 2)
        sh3 = ints((256,), -8, 8)
    assert _distinct(w3) and _distinct(w1), "weights need distinct rows and columns"
    ss3 = torch.stack([pick([-1.0, 0.5, 1.0, 2.0], 256), sh3])
    ss1 = torch.stack([pick([-1.0, 0.5, 1.0, 2.0], 64), ints((64,), -8, 8)])
    return a2, res, w3, w1, ss3, ss1


def _reference(a2, res, w3, w1, ss3, ss1, dt, stats):
    acc = a2 @ w3.t()
    assert float((a2.abs() @ w3.abs().t()).max()) < 2.0 ** 24
    v = acc * ss3[0] + ss3[1]                                   # exact: dyadic scale, integer shift, |v| < 2^10
    out3 = _rd(torch.relu(_rd(v, dt) + res), dt)                # rounded, + residual, ReLU, rounded
    assert 2.0 * float((out3.abs() @ w1.abs().t()).max()) < 2.0 ** 24, "the second multiply must be exact in fp32"
    acc2 = out3 @ w1.t()
    if not stats:
        out1 = _rd(torch.relu(acc2 * ss1[0] + ss1[1]), dt)
        assert float(out1.max()) < 65504.0
        return out3, out1, None
    t = acc2.view(-1, 128, 64)
    assert 4.0 * float((t * t).sum(1).max()) < 2.0 ** 24 and 4.0 * float(t.abs().sum(1).max()) < 2.0 ** 24, \
        "tile sums must be exact in fp32 in any order"
    return out3, _rd(acc2, dt), torch.stack([t.sum(1), (t * t).sum(1)], 1)


def _set_wgs(monkeypatch, wgs):
    if wgs:
        monkeypatch.setenv("CREID_STREAM1X1_WGS", str(wgs))
    else:
        monkeypatch.delenv("CREID_STREAM1X1_WGS", raising=False)


def _same(got, exp, what):
    bad = got.double() != exp                                   # as values: +0 == -0, a NaN left behind differs
    n = int(bad.sum())
    if n:
        i = int(bad.reshape(-1).nonzero()[0])
        r, c = divmod(i, exp.shape[-1])
        raise AssertionError(f"{what}: {n} of {exp.numel()} differ, first at (row, col) ({r}, {c}): got "
                             f"{float(got.reshape(-1)[i])} expected {float(exp.reshape(-1)[i])}")


@pytest.mark.parametrize("dt", [BF, F16])
@pytest.mark.parametrize("M,wgs", AFFINE_CASES)
def test_pair_affine_exact(M, wgs, dt, monkeypatch):
    from centroids_reid_amd import _lib as L
    lib = L.lib()
    a2, res, w3, w1, ss3, ss1 = _operands(M, dt, False, 1000 * M + wgs)
    e3, e1, _ = _reference(a2, res, w3, w1, ss3, ss1, dt, False)
    a2d, resd, w3d, w1d = (t.to(dt).contiguous() for t in (a2, res, w3, w1))
    f3, f1 = ss3.float().contiguous(), ss1.float().contiguous()
    o3, o1 = _guarded(M, 256, dt), _guarded(M, 64, dt)
    _set_wgs(monkeypatch, wgs)
    L.check(lib.creid_bottleneck_c3_c1_fwd_affine(M, 64, 256, 64, L.ptr(a2d), L.ptr(w3d), L.ptr(f3), L.ptr(resd), L.ptr(o3), L.ptr(w1d),
                                                  L.ptr(f1), L.ptr(o1), L._DT[dt], L.stream()), "pair affine")
    torch.cuda.synchronize()
    assert bool((o3[M:] == SENT16).all()) and bool((o1[M:] == SENT16).all()), "guard rows behind row M were written"
    _same(o3[:M].view(dt), e3, "block output")
    _same(o1[:M].view(dt), e1, "conv1 output")


@pytest.mark.parametrize("dt", [BF, F16])
@pytest.mark.parametrize("M,wgs", STATS_CASES)
def test_pair_stats_exact(M, wgs, dt, monkeypatch):
    from centroids_reid_amd import _lib as L
    lib = L.lib()
    a2, res, w3, w1, ss3, ss1 = _operands(M, dt, True, 2000 * M + wgs)
    e3, e1, ep = _reference(a2, res, w3, w1, ss3, None, dt, True)
    a2d, resd, w3d, w1d = (t.to(dt).contiguous() for t in (a2, res, w3, w1))
    f3 = ss3.float().contiguous()
    o3, o1 = _guarded(M, 256, dt), _guarded(M, 64, dt)
    tiles = M // 128
    part = torch.full((tiles + GUARD, 2, 64), SENT32, dtype=torch.int32, device="cuda")
    part[:tiles] = 0x7FC00000                                   # NaN
    _set_wgs(monkeypatch, wgs)
    L.check(lib.creid_bottleneck_c3_c1_fwd_stats(M, 64, 256, 64, L.ptr(a2d), L.ptr(w3d), L.ptr(f3), L.ptr(resd), L.ptr(o3), L.ptr(w1d),
                                                 L.ptr(o1), L.ptr(part), L._DT[dt], L.stream()), "pair stats")
    torch.cuda.synchronize()
    assert bool((o3[M:] == SENT16).all()) and bool((o1[M:] == SENT16).all()) and bool((part[tiles:] == SENT32).all()), \
        "guard rows behind the outputs were written"
    _same(o3[:M].view(dt), e3, "block output")
    _same(o1[:M].view(dt), e1, "raw conv1 output")
    _same(part[:tiles].view(torch.float32), ep, "statistics partials [tiles][2][64]")


@pytest.mark.parametrize("dt", [BF, F16])
def test_pair_refusals_write_nothing(dt):
    """c_mid / c_out / c_next other than 64 / 256 / 64: -4; fp32: -2; M % 128 != 0 with statistics: -4; no output is touched"""
    from centroids_reid_amd import _lib as L
    lib = L.lib()
    M = 256
    a2, res, w3, w1, ss3, ss1 = _operands(M, dt, False, 7)
    a2d, resd, w3d, w1d = (t.to(dt).contiguous() for t in (a2, res, w3, w1))
    f3, f1 = ss3.float().contiguous(), ss1.float().contiguous()
    o3, o1 = _guarded(M, 256, dt), _guarded(M, 64, dt)
    part = torch.full((M // 128 + GUARD, 2, 64), SENT32, dtype=torch.int32, device="cuda")
    snap = [t.clone() for t in (o3, o1, part)]
    st = L.stream()

    def affine(m, cm, co, cn, code):
        return lib.creid_bottleneck_c3_c1_fwd_affine(m, cm, co, cn, L.ptr(a2d), L.ptr(w3d), L.ptr(f3), L.ptr(resd), L.ptr(o3), L.ptr(w1d),
                                                     L.ptr(f1), L.ptr(o1), code, st)

    def stats(m, cm, co, cn, code):
        return lib.creid_bottleneck_c3_c1_fwd_stats(m, cm, co, cn, L.ptr(a2d), L.ptr(w3d), L.ptr(f3), L.ptr(resd), L.ptr(o3), L.ptr(w1d),
                                                    L.ptr(o1), L.ptr(part), code, st)

    code = L._DT[dt]
    for fn in (affine, stats):
        for cm, co, cn in ((128, 512, 128), (64, 256, 128), (64, 512, 64), (32, 256, 64)):
            assert fn(M, cm, co, cn, code) == -4, (fn.__name__, cm, co, cn)
        assert fn(M, 64, 256, 64, L._DT[torch.float32]) == -2, fn.__name__
    for m in (M - 1, M - 64, 1):
        assert stats(m, 64, 256, 64, code) == -4, m
    torch.cuda.synchronize()
    for t, s in zip((o3, o1, part), snap):
        assert torch.equal(t, s), "a refused call wrote to an output"
