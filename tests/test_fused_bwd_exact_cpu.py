"""CPU: the reference helpers of tests/fused_bwd_exact.py against straightforward fp64 autograd and loops on two tiny shapes, the
mask packing against ew_ref.relu_bits / bits_to_mask, and the exactness assertions firing on operand sets that break them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ew_ref
import fused_bwd_exact as fx

TINY = [(2, 8, 16, 3, 1, 5, 3), (3, 16, 8, 1, 2, 4, 6)]               # (B, cin, cout, k, stride, h, w): odd / even extents


def _autograd_dx(o):
    B, cin, cout, k, s, h, w = o.geom
    x = torch.zeros(B, cin, h, w, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, o.w8.double(), stride=s, padding=k // 2)
    y.backward(o.dy8.double().permute(0, 3, 1, 2))
    return x.grad.permute(0, 2, 3, 1).reshape(-1, cin)


@pytest.mark.parametrize("geom", TINY, ids=fx.gid)
def test_expected_dx_and_partials_against_autograd_and_loops(geom):
    o = fx.operands(geom, "cpu")
    B, cin, cout, k, s, h, w = geom
    acc = _autograd_dx(o)
    assert torch.equal(o.acc, acc) and float(acc.abs().max()) > 2
    keep_b, keep_a = o.bn_keep.reshape(-1, cin), o.add_keep.reshape(-1, cin)
    add, x = o.add8.reshape(-1, cin).double(), o.x8.reshape(-1, cin).double()
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        r = lambda t: t.float().to(dtype).double()
        g, part = fx.expected(o, dtype, "5_mask_add_addmask")
        want = r(r(acc) + add * keep_a)                                # two roundings; the add only where its bit is set
        assert torch.equal(g, want)
        rows = -(-o.M // 128)
        loop = torch.zeros(rows, 2, cin, dtype=torch.float64)
        for m in range(o.M):
            for c in range(cin):
                if keep_b[m, c]:
                    loop[m // 128, 0, c] += want[m, c]
                    loop[m // 128, 1, c] += want[m, c] * (x[m, c] - o.mean[c]) * o.invstd[c]
        assert torch.equal(part, loop) and float(loop[:, 1].abs().max()) > 0
        # act form: keep = act > 0; plain sums: no mask at all
        g1, p1 = fx.expected(o, dtype, "1_act")
        assert torch.equal(g1, r(acc))
        assert torch.equal(p1[:, 0].sum(0), (g1 * (o.act8.reshape(-1, cin) > 0)).sum(0))
        g3, p3 = fx.expected(o, dtype, "3_plain_sums")
        assert torch.equal(p3[:, 0].sum(0), g3.sum(0))
        assert torch.equal(p3[:, 1].sum(0), (g3 * (x - o.mean.double()) * o.invstd.double()).sum(0))
        assert fx.expected(o, dtype, "7_addmask_only")[1] is None
    if h % 2 == 0 and w % 2 == 0:
        g6, _ = fx.expected(o, torch.bfloat16, "6_mask_compact_add")
        want = o.acc.float().to(torch.bfloat16).double().view(B, h, w, cin).clone()
        for b in range(B):
            for y in range(0, h, 2):
                for xx in range(0, w, 2):
                    want[b, y, xx] = (want[b, y, xx] + o.addc8[b, y // 2, xx // 2].double()).float().to(torch.bfloat16).double()
        assert torch.equal(g6.view(B, h, w, cin), want)


def test_per_image_partials_use_each_image_s_statistics():
    gen = torch.Generator().manual_seed(5)
    B, rows, c = 3, 256, 8
    g = torch.randint(-9, 10, (B * rows, c), generator=gen).double()
    x = torch.randint(-2, 3, (B * rows, c), generator=gen).double()
    keep = torch.randint(0, 2, (B * rows, c), generator=gen).bool()
    mean = torch.randint(-2, 3, (B, c), generator=gen).double()
    invstd = 2.0 ** torch.randint(-1, 2, (B, c), generator=gen).double()
    part = fx.ref_bn_partials(g, keep, x, mean, invstd, image_rows=rows)
    assert part.shape == (B * rows // 128, 2, c)
    for b in range(B):
        sl = slice(b * rows, (b + 1) * rows)
        dy = g[sl] * keep[sl]
        assert torch.equal(part[2 * b:2 * b + 2, 0].sum(0), dy.sum(0))
        assert torch.equal(part[2 * b:2 * b + 2, 1].sum(0), (dy * (x[sl] - mean[b]) * invstd[b]).sum(0))
    other = fx.ref_bn_partials(g, keep, x, mean.roll(1, 0), invstd, image_rows=rows)
    assert not torch.equal(other[:, 1], part[:, 1]), "a wrong image index must change the sums"


def test_mask_packing_is_the_layout_of_the_apply_kernels():
    gen = torch.Generator().manual_seed(3)
    y = torch.randint(-2, 3, (21, 64), generator=gen).float()
    bits = fx.pack_bits(y > 0)
    assert bits.dtype == torch.uint8 and bits.numel() == 21 * 64 // 8
    assert np.array_equal(bits.numpy(), ew_ref.relu_bits(y.numpy()))
    assert torch.equal(fx.unpack_bits(bits, y.shape), ew_ref.bits_to_mask(bits.numpy(), y.shape))
    assert torch.equal(fx.unpack_bits(bits, y.shape), y > 0)
    # bit c % 8 of byte (pixel * C + c) / 8
    one = torch.zeros(3, 64, dtype=torch.bool)
    one[2, 13] = True
    b1 = fx.pack_bits(one)
    assert int(b1[(2 * 64 + 13) // 8]) == 1 << (13 % 8) and int(b1.sum()) == 1 << 5


@pytest.mark.parametrize("bn_c,rows", [(8, 1), (24, 7), (16, 1024)])
def test_finalize_reference_against_the_plain_formulas(bn_c, rows):
    f = fx.fin_operands(bn_c, rows, 0, "cpu")
    assert bool((f.dgamma0 != 0).all()) and bool((f.dbeta0 != 0).all()) and f.count & (f.count - 1) == 0
    ref = fx.ref_finalize(f.partial, f.count, f.mean, f.invstd, f.gamma, f.dgamma0, f.dbeta0)
    s1 = sum(f.partial[r, 0].double() for r in range(rows))
    s2 = sum(f.partial[r, 1].double() for r in range(rows))
    g, is_, mu = f.gamma.double(), f.invstd.double(), f.mean.double()
    m1, m2 = s1 / f.count, s2 / f.count
    # dx = k1 dy - k1 is m2 x + (k1 is m2 mu - k1 m1) = gamma is (dy - m1 - xhat m2)
    assert torch.equal(ref["sums"][0], g * is_)
    assert torch.equal(ref["sums"][1], -g * is_ * is_ * m2)
    assert torch.equal(ref["sums"][2], -g * is_ * m1 + g * is_ * is_ * m2 * mu)
    assert torch.equal(ref["dgamma"], f.dgamma0.double() + s2) and torch.equal(ref["dbeta"], f.dbeta0.double() + s1)
    dy, x = torch.tensor(3.0, dtype=torch.float64), torch.tensor(-1.5, dtype=torch.float64)
    lhs = ref["sums"][0] * dy + ref["sums"][1] * x + ref["sums"][2]
    assert torch.allclose(lhs, g * is_ * (dy - m1 - (x - mu) * is_ * m2), rtol=1e-12, atol=1e-12)


def test_exactness_assertions_fire():
    ok = torch.full((128, 4), 2.0 ** 16, dtype=torch.float64)          # 128 x 2^16 = 2^23 units: holds
    assert fx.assert_tile_sums_exact(ok) == 1.0
    assert fx.assert_tile_sums_exact(ok * 0.5 + 0.5) == 0.5
    with pytest.raises(AssertionError, match="not below 2\\^24"):
        fx.assert_tile_sums_exact(ok * 2)                              # 2^24 units in one tile
    with pytest.raises(AssertionError, match="not below 2\\^24"):
        fx.assert_tile_sums_exact(ok + 0.5)                            # the unit halves, the count doubles
    two_tiles = torch.cat([ok, ok])                                    # the bound is per tile, not over all rows
    assert fx.assert_tile_sums_exact(two_tiles) == 1.0
    with pytest.raises(AssertionError, match="power-of-two unit"):
        fx.assert_tile_sums_exact(torch.full((4, 4), 1.0 / 3.0, dtype=torch.float64))
    g = torch.full((128, 8), 2.0 ** 20, dtype=torch.float64)
    with pytest.raises(AssertionError):
        fx.ref_bn_partials(g, None, torch.ones(128, 8), torch.zeros(8), torch.ones(8))
    f = fx.fin_operands(8, 7, 0, "cpu")
    f.gamma[0] = 0.75                                                  # (at least one channel with a non-zero gamma)
    for name, val in (("gamma", f.gamma.double() / 3.0), ("invstd", f.invstd.double() + 2.0 ** -20),
                      ("partial", f.partial.double() + 1.0 + 2.0 ** -30)):
        args = {k: getattr(f, k) for k in ("partial", "count", "mean", "invstd", "gamma", "dgamma0", "dbeta0")}
        args[name] = val
        with pytest.raises(AssertionError, match="not an fp32 value"):
            fx.ref_finalize(**args)
    with pytest.raises(AssertionError, match="not an fp32 value"):
        fx.ref_finalize(f.partial, 3, f.mean, f.invstd, f.gamma, f.dgamma0, f.dbeta0)


def test_operands_narrow_dy_where_the_sums_would_not_be_exact(monkeypatch):
    calls = []
    monkeypatch.setattr(fx, "_sums_hold", lambda o: calls.append(o.dy_hi) or o.dy_hi == 1)
    o = fx.operands.__wrapped__((1, 8, 8, 3, 1, 3, 3), "cpu")
    assert calls == [2, 1] and o.dy_hi == 1 and int(o.dy8.abs().max()) == 1
    monkeypatch.undo()
    o = fx.operands.__wrapped__((1, 8, 8, 3, 1, 3, 3), "cpu")
    assert o.dy_hi == 2 and int(o.dy8.abs().max()) == 2
