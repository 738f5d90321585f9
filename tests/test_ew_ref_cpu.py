"""tests/ew_ref.py checked on the CPU, without the library:

  1. the float64 reference against independent evaluations -- torch.autograd in float64 (BatchNorm, IBN as instance_norm ||
     batch_norm, max_pool2d with its indices, adaptive_avg_pool2d), ties of the pool against torch, one example per operation
     worked out by hand;
  2. the bounds hold for a faithful emulation: the column pass of the kernels in numpy fp32 (lane chains, then the lane adds, then
     float64 across the blocks), the finalize expressions and the fmaf apply, at mean / std in {0.5, 16, 256} and at every (M, C)
     of the GPU sweep with M <= 4096;
  3. the comparator has teeth: the same emulation with ONE fault injected fails it, for each of six faults;
  4. the grid arithmetic of the grid-stride apply kernels: no chunk on another channel's coefficients for any (C, cap) of the
     sweep.  Before ew_blocks_cap rounded to mult / gcd(mult, 256) blocks, C = 40 in 16-bit storage (5 chunks per row) with
     600000 chunks under a cap of 2048 workgroups put 75712 chunks on another channel's coefficients (206784 at a cap of 1536);
     C = 24 was wrong at 2048 and right by luck at 1536, C = 72 wrong at both.

The emulated fma rounds the exact product-plus-addend twice (float64, then fp32): it differs from a real fma only where the
float64 sum lands within 2^-29 ulp of an fp32 tie, which is far below what the bounds resolve."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ew_ref as er

f32, f64 = np.float32, np.float64
MOM, EPS = float(f32(0.1)), float(f32(1e-5))          # the fp32 values the ABI receives


def n32(t):
    return np.asarray(er.t64(t).numpy(), f32)


def fma32(a, b, c):
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


# ------------------------------------------------------------------------------------------------ the emulation
def emu_col(t1, a, b, C, kind, drop_last=False):
    """col_stats_kernel / bn2d_bwd_reduce_kernel: per 128-row block, row lane rl adds rows rl, rl + nrl, ... (s1 += t1; s2 =
    fma(a, b, s2)), then the nrl lane partials are added in lane order; blocks meet in float64.  [M, C] fp32 -> (S1, S2)."""
    M = t1.shape[0]
    _, nrl = er.lanes(C, kind)
    nb, chain = -(-M // 128), -(-128 // nrl)

    def blocks(v):
        p = np.zeros((nb * 128, C), f32)
        p[:M] = v
        if drop_last:
            for k in range(nb):
                p[min(M, (k + 1) * 128) - 1] = 0
        q = np.zeros((nb, chain * nrl, C), f32)
        q[:, :128] = p.reshape(nb, 128, C)
        return q.reshape(nb, chain, nrl, C)
    t1, a, b = blocks(t1), blocks(a), blocks(b)
    s1, s2 = np.zeros((nb, nrl, C), f32), np.zeros((nb, nrl, C), f32)
    for j in range(chain):
        s1 = s1 + t1[:, j]
        s2 = fma32(a[:, j], b[:, j], s2)
    a1, a2 = np.zeros((nb, C), f32), np.zeros((nb, C), f32)
    for q in range(nrl):
        a1 = a1 + s1[:, q]
        a2 = a2 + s2[:, q]
    return a1.astype(f64).sum(0), a2.astype(f64).sum(0)


def emu_finalize(S1, S2, count, gamma, beta, rm, rv, guard=True):
    """bn2d_finalize_kernel, training."""
    mean = S1 / count
    var = np.maximum(S2 / count - mean * mean, 0.0)
    mu, inv = mean.astype(f32), (1.0 / np.sqrt(var + f64(f32(EPS)))).astype(f32)
    sc = inv * n32(gamma)
    sh = n32(beta) - mu * sc
    m = f32(MOM)
    with np.errstate(all="ignore"):
        unb = (var * count / (count - 1.0) if (count > 1 or not guard) else var).astype(f32)
    return dict(mean=mu, invstd=inv, ss=np.stack([sc, sh]), rmean=(f32(1) - m) * n32(rm) + m * mean.astype(f32),
                rvar=(f32(1) - m) * n32(rv) + m * unb)


def emu_apply(x, ss, res, ss2, relu, kind, drift_threads=None):
    """bn2d_apply_kernel; drift_threads: chunks past the first grid-stride trip of a grid of that many threads use the
    coefficients of channel chunk (c + 2) % cpr."""
    M, C = x.shape
    sc, sh = np.broadcast_to(ss[0], (M, C)), np.broadcast_to(ss[1], (M, C))
    if drift_threads is not None:
        V = er.VEC[kind]
        cpr = C // V
        rolled = [np.roll(v.reshape(cpr, V), -2, axis=0).reshape(C) for v in ss]
        late = (np.arange(M)[:, None] * cpr + np.arange(C)[None, :] // V) >= drift_threads
        sc, sh = np.where(late, rolled[0], sc), np.where(late, rolled[1], sh)
    v = fma32(x, sc, sh)
    if res is not None:
        v = v + (fma32(res, np.broadcast_to(ss2[0], (M, C)), np.broadcast_to(ss2[1], (M, C))) if ss2 is not None else res)
    if relu:
        v = np.maximum(v, f32(0))
    return er.round_to(torch.from_numpy(v.astype(f64)), kind)


def emu_forward(d, drop_last=False, guard=True, drift_threads=None):
    kind, C, M = d["kind"], d["C"], d["M"]
    x = n32(d["x"])
    S1, S2 = emu_col(x, x, x, C, kind, drop_last)
    dev = emu_finalize(S1, S2, float(M), d["gamma"], d["beta"], d["rmean"], d["rvar"], guard)
    res, ss2 = None, None
    if d["res"] is not None:
        res = n32(d["res"])
    if d["res_mode"] == "dual":
        T1, T2 = emu_col(res, res, res, C, kind)
        ss2 = emu_finalize(T1, T2, float(M), d["gamma2"], d["beta2"], np.zeros(C), np.ones(C))["ss"]
        dev["ss2"] = ss2
    dev["y"] = emu_apply(x, dev["ss"], res, ss2, d["relu"], kind, drift_threads)
    dev["bits"] = er.relu_bits(dev["y"].numpy()) if kind != "fp32" else None
    return dev


def emu_backward(d, fwd, dg0, db0):
    """bn2d_bwd_reduce_kernel -> bn2d_bwd_finalize_kernel -> bn2d_bwd_apply_kernel."""
    kind, C, M = d["kind"], d["C"], d["M"]
    x, g = n32(d["x"]), n32(d["g"])
    dy = g * (fwd["y"].numpy() > 0).astype(f32) if d["relu"] else g
    mu, inv = fwd["mean"], fwd["invstd"]
    xhat = (x - mu) * inv
    S1, S2 = emu_col(dy, dy, xhat, C, kind)
    invM = f32(1.0 / M)
    k1 = n32(d["gamma"]) * inv
    a1, a2 = S1.astype(f32) * invM, S2.astype(f32) * invM
    sums = np.stack([k1, -k1 * inv * a2, -k1 * a1 + k1 * inv * a2 * mu])
    dx = fma32(np.broadcast_to(sums[0], x.shape), dy, fma32(np.broadcast_to(sums[1], x.shape), x, np.broadcast_to(sums[2], x.shape)))
    return dict(sums=sums, dgamma=n32(dg0) + S2.astype(f32), dbeta=n32(db0) + S1.astype(f32),
                dx=er.round_to(torch.from_numpy(dx.astype(f64)), kind), gm=torch.from_numpy(dy.astype(f64)))


def emu_ibn_forward(d, second_group_bug=False):
    """ibn_col_stats_kernel per image -> ibn_finalize_kernel -> ibn_apply_kernel (training)."""
    kind, C, c_in, B, HW = d["kind"], d["C"], d["c_in"], d["B"], d["HW"]
    x = n32(d["x"])
    S = [emu_col(x[n], x[n], x[n], C, kind) for n in range(B)]
    S1, S2 = np.stack([s[0] for s in S]), np.stack([s[1] for s in S])
    w, b = np.concatenate([n32(d["in_w"]), n32(d["bn_w"])]), np.concatenate([n32(d["in_b"]), n32(d["bn_b"])])
    mean, inv, ss = np.zeros((B, C), f32), np.zeros((B, C), f32), np.zeros((B, 2, C), f32)
    for n in range(B):
        src = n - 16 if (second_group_bug and n >= 16) else n
        fi = emu_finalize(S1[src], S2[src], float(HW), w, b, np.zeros(C), np.ones(C))
        fb = emu_finalize(S1.sum(0), S2.sum(0), float(B * HW), w, b, np.concatenate([np.zeros(c_in), n32(d["rmean"])]),
                          np.concatenate([np.ones(c_in), n32(d["rvar"])]))
        for out, key in ((mean, "mean"), (inv, "invstd")):
            out[n, :c_in], out[n, c_in:] = fi[key][:c_in], fb[key][c_in:]
        ss[n, :, :c_in], ss[n, :, c_in:] = fi["ss"][:, :c_in], fb["ss"][:, c_in:]
    y = torch.stack([emu_apply(x[n], ss[n], None, None, d["relu"], kind) for n in range(B)])
    return dict(mean=mean, invstd=inv, ss=ss, rmean=fb["rmean"][c_in:], rvar=fb["rvar"][c_in:], y=y,
                bits=er.relu_bits(y.numpy()) if kind != "fp32" else None)


def emu_pool(x, last_wins=False, pad_zero=False):
    """maxpool_fwd_kernel, one window at a time."""
    x = x.numpy()
    B, H, W, C = x.shape
    y, tap = np.zeros((B, H // 2, W // 2, C)), np.zeros((B, H // 2, W // 2, C), np.uint8)
    for b in range(B):
        for oy in range(H // 2):
            for ox in range(W // 2):
                best, bi = np.full(C, -np.inf), np.zeros(C, np.uint8)
                for r in range(3):
                    for s in range(3):
                        iy, ix = 2 * oy + r - 1, 2 * ox + s - 1
                        inb = 0 <= iy < H and 0 <= ix < W
                        if not inb and not pad_zero:
                            continue
                        v = x[b, iy, ix] if inb else np.zeros(C)
                        win = (v >= best) if last_wins else (v > best)
                        best, bi = np.where(win, v, best), np.where(win, r * 3 + s, bi).astype(np.uint8)
                y[b, oy, ox], tap[b, oy, ox] = best, bi
    return torch.from_numpy(y), torch.from_numpy(tap)


# ------------------------------------------------------------------------------------------------ 1. the reference
def test_round_to_is_one_correct_rounding():
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.standard_normal(4000) * 10.0 ** rng.integers(-9, 5, 4000), [0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 2.0 ** -25,
                        3 * 2.0 ** -25, 2.0 ** -140, 65504.0, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11]])
    v = v[np.abs(v) < 6e4]
    t = torch.from_numpy(v)
    assert np.array_equal(er.round_to(t, "fp32").numpy(), v.astype(f32).astype(f64))
    assert np.array_equal(er.round_to(t, "f16").numpy(), v.astype(np.float16).astype(f64))
    v32 = torch.from_numpy(v.astype(f32))                       # fp32 values: torch's cast to bf16 is then a single rounding
    assert torch.equal(er.round_to(v32, "bf16"), v32.bfloat16().double())
    # 1 + 2^-8 + 2^-30 lies above the bf16 tie; through fp32 it would first fall onto the tie and then to even (1.0)
    t = lambda v: torch.tensor([v], dtype=er.F64)   # noqa: E731
    assert float(er.round_to(t(1 + 2.0 ** -8 + 2.0 ** -30), "bf16")) == 1 + 2.0 ** -7
    assert float(t(1 + 2.0 ** -8 + 2.0 ** -30).float().bfloat16()) == 1.0
    assert float(er.round_to(t(1 + 2.0 ** -8), "bf16")) == 1.0 and float(er.round_to(t(1 + 3 * 2.0 ** -8), "bf16")) == 1 + 2.0 ** -6
    # unit roundoff = half the spacing above 1: 8, 11 and 24 significand bits
    assert er.UNIT == {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "fp32": 2.0 ** -24}
    for kind in er.KINDS:
        assert float(er.round_to(t(1 + er.UNIT[kind]), kind)) == 1.0 and float(er.round_to(t(1 + 1.5 * er.UNIT[kind]), kind)) == 1 + 2 * er.UNIT[kind]


@pytest.mark.parametrize("res_mode,relu", [("none", True), ("plain", True), ("dual", False), ("dual", True)])
def test_bn_reference_vs_autograd(res_mode, relu):
    d = er.bn_inputs(37, 16, "fp32", 3, res_mode=res_mode, relu=relu, momentum=MOM, eps=EPS)
    x = d["x"].clone().requires_grad_(True)
    gam_, bet_ = d["gamma"].clone().requires_grad_(True), d["beta"].clone().requires_grad_(True)
    rm, rv = d["rmean"].clone(), d["rvar"].clone()
    y = F.batch_norm(x, rm, rv, gam_, bet_, True, MOM, EPS)
    sc2 = sh2 = None
    if res_mode == "plain":
        y = y + d["res"]
    elif res_mode == "dual":
        y = y + F.batch_norm(d["res"], None, None, d["gamma2"], d["beta2"], True, MOM, EPS)
        r2 = er.bn_forward_ref(d["res"], d["gamma2"], d["beta2"], rm, rv, MOM, EPS)
        sc2, sh2 = r2["sc"], r2["sh"]
    if relu:
        y = y.relu()
    (y * d["g"]).sum().backward()
    ref = er.bn_forward_ref(d["x"], d["gamma"], d["beta"], d["rmean"], d["rvar"], MOM, EPS)
    yr, z, _ = er.bn_apply(d["x"], ref["sc"], ref["sh"], d["res"], sc2, sh2, relu)
    tol = dict(rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(yr, y.detach(), **tol)
    torch.testing.assert_close(ref["rmean"], rm, **tol)
    torch.testing.assert_close(ref["rvar"], rv, **tol)
    s = er.bn_backward_sums(d["x"], d["g"], (z > 0) if relu else None, ref["mean"], ref["invstd"])
    A, B, Cc = er.bn_backward_coef(s["s1"], s["s2"], ref["mean"], ref["invstd"], d["gamma"], 37)
    dx, _ = er.bn_dx(d["x"], s["dy"], A, B, Cc)
    torch.testing.assert_close(dx, x.grad, **tol)
    torch.testing.assert_close(s["s2"], gam_.grad, **tol)
    torch.testing.assert_close(s["s1"], bet_.grad, **tol)


def test_bn_by_hand():
    """x = (1, 3): mean 2, biased variance 1, unbiased 2; gamma 2, beta 1, eps 0 -> y = (-1, 3), ReLU (0, 3).  One sample: the
    variance 0 stays 0 in the running statistic (var * 1 / 0 is never formed)."""
    x = torch.tensor([[1.0], [3.0]], dtype=er.F64)
    one = torch.ones(1, dtype=er.F64)
    r = er.bn_forward_ref(x, 2 * one, one, 0 * one, one, 0.5, 0.0)
    assert float(r["mean"]) == 2 and float(r["var"]) == 1 and float(r["invstd"]) == 1 and float(r["sc"]) == 2 and float(r["sh"]) == -3
    assert float(r["rmean"]) == 1.0 and float(r["rvar"]) == 0.5 * 1 + 0.5 * 2
    y, z, mag = er.bn_apply(x, r["sc"], r["sh"], relu=True)
    assert y.flatten().tolist() == [0.0, 3.0] and z.flatten().tolist() == [-1.0, 3.0] and mag.flatten().tolist() == [5.0, 9.0]
    bits = er.relu_bits(np.array([0, 3, -1, 2, 0, 0, 0, 1, 5, 0.0]))
    assert bits.tolist() == [0b10001010, 0b00000001]
    assert torch.equal(er.bits_to_mask(bits, (10,)), torch.tensor([0, 1, 0, 1, 0, 0, 0, 1, 1, 0], dtype=torch.bool))
    # backward of y = 2 xhat + 1 with g = (1, 0): S1 = 1, S2 = -1; dx = 2 (dy - 1/2 - xhat * (-1/2)) = (0, 0)
    s = er.bn_backward_sums(x, torch.tensor([[1.0], [0.0]]), None, r["mean"], r["invstd"])
    assert float(s["s1"]) == 1 and float(s["s2"]) == -1
    dx, _ = er.bn_dx(x, s["dy"], *er.bn_backward_coef(s["s1"], s["s2"], r["mean"], r["invstd"], 2 * one, 2))
    assert dx.flatten().tolist() == [0.0, 0.0]
    r1 = er.bn_forward_ref(x[:1], one, one, 0 * one, one, 0.5, 1e-5)
    assert float(r1["var"]) == 0 and float(r1["rvar"]) == 0.5


@pytest.mark.parametrize("training", [True, False])
def test_ibn_reference_vs_autograd(training):
    B, H, W, C, c_in = 3, 5, 4, 16, 8
    d = er.ibn_inputs(B, H * W, C, c_in, "fp32", 5, relu=True, training=training, momentum=MOM, eps=EPS)
    x = d["x"].reshape(B, H, W, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
    p = [d[k].clone().requires_grad_(True) for k in ("in_w", "in_b", "bn_w", "bn_b")]
    rm, rv = d["rmean"].clone(), d["rvar"].clone()
    y = torch.cat([F.instance_norm(x[:, :c_in], None, None, p[0], p[1], True, MOM, EPS),
                   F.batch_norm(x[:, c_in:], rm, rv, p[2], p[3], training, MOM, EPS)], 1).relu()
    g = d["g"].reshape(B, H, W, C).permute(0, 3, 1, 2)
    (y * g).sum().backward()
    ref = er.ibn_forward_ref(d["x"], c_in, d["in_w"], d["in_b"], d["bn_w"], d["bn_b"], d["rmean"], d["rvar"], MOM, EPS, training)
    yr, z, _ = er.bn_apply(d["x"], ref["sc"][:, None, :], ref["sh"][:, None, :], relu=True)
    tol = dict(rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(yr.reshape(B, H, W, C).permute(0, 3, 1, 2), y.detach(), **tol)
    if not training:
        return                                       # (the kernels' backward is the training one)
    torch.testing.assert_close(ref["rmean"], rm, **tol)
    torch.testing.assert_close(ref["rvar"], rv, **tol)
    s = er.ibn_backward_ref(d["x"], d["g"], z > 0, ref["mean"], ref["invstd"], c_in, torch.cat([d["in_w"], d["bn_w"]]))
    dx, _ = er.bn_dx(d["x"], s["dy"], s["A"][:, None, :], s["B"][:, None, :], s["Cc"][:, None, :])
    torch.testing.assert_close(dx.reshape(B, H, W, C).permute(0, 3, 1, 2), x.grad, **tol)
    for key, q in zip(("d_in_w", "d_in_b", "d_bn_w", "d_bn_b"), p):
        torch.testing.assert_close(s[key], q.grad, **tol)


def test_ibn_by_hand():
    """Two images of two pixels, channel 0 per image, channel 1 over the batch: image 0 = (0, 2 | 1, 1), image 1 = (4, 8 | 3, 7)."""
    x = torch.tensor([[[0.0, 1.0], [2.0, 1.0]], [[4.0, 3.0], [8.0, 7.0]]], dtype=er.F64)
    one = torch.ones(1, dtype=er.F64)
    r = er.ibn_forward_ref(x, 1, one, 0 * one, one, 0 * one, 0 * one, one, 0.5, 0.0)
    assert r["mean"].tolist() == [[1.0, 3.0], [6.0, 3.0]] and r["var"].tolist() == [[1.0, 6.0], [4.0, 6.0]]
    assert float(r["rmean"]) == 1.5 and float(r["rvar"]) == 0.5 + 0.5 * 8.0
    assert r["count"].tolist() == [2.0, 4.0]


def _torch_taps(idx, W):
    """max_pool2d's flat input index -> tap code r * 3 + s."""
    B, C, OH, OW = idx.shape
    iy, ix = idx // W, idx % W
    oy = torch.arange(OH).view(1, 1, OH, 1)
    ox = torch.arange(OW).view(1, 1, 1, OW)
    return ((iy - (2 * oy - 1)) * 3 + (ix - (2 * ox - 1))).permute(0, 2, 3, 1).to(torch.uint8)


@pytest.mark.parametrize("mode", er.POOL_MODES)
@pytest.mark.parametrize("shape", er.POOL_SHAPES[:4])
def test_pool_reference_vs_torch(shape, mode):
    x = er.pool_inputs(shape, "bf16", mode, 11)
    B, H, W, C = shape
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y, idx = F.max_pool2d(xn, 3, 2, 1, return_indices=True)
    ry, rt = er.maxpool_fwd(x)
    assert torch.equal(ry, y.detach().permute(0, 2, 3, 1))
    assert torch.equal(rt, _torch_taps(idx, W)), "tie-breaking differs from torch's first maximum in scan order"
    dy = er.pool_grad(ry.shape, 12)
    (y * dy.permute(0, 3, 1, 2)).sum().backward()
    assert torch.equal(er.maxpool_bwd(dy, rt, H, W, "fp32"), xn.grad.permute(0, 2, 3, 1))
    if mode == "relu":
        assert float((x == 0).double().mean()) >= 0.5 and bool((x[0, :2, :2] == 0).all())


def test_pool_ties_and_by_hand():
    z = torch.zeros(1, 1, 4, 4, dtype=er.F64)
    _, idx = F.max_pool2d(z, 3, 2, 1, return_indices=True)
    assert idx.flatten().tolist() == [0, 1, 4, 5]                       # the first in-bounds tap of each window
    _, tap = er.maxpool_fwd(z.permute(0, 2, 3, 1))
    assert tap.flatten().tolist() == [4, 3, 1, 0] and torch.equal(tap, _torch_taps(idx, 4))
    # a 2 x 2 map: one window, in-bounds taps 4 (1), 5 (5), 7 (5), 8 (2): the first 5 wins; its gradient lands on pixel (0, 1)
    x = torch.tensor([[1.0, 5.0], [5.0, 2.0]], dtype=er.F64).view(1, 2, 2, 1)
    y, tap = er.maxpool_fwd(x)
    assert float(y) == 5 and int(tap) == 5
    assert er.maxpool_bwd(torch.full((1, 1, 1, 1), 0.75), tap, 2, 2, "bf16").flatten().tolist() == [0.0, 0.75, 0.0, 0.0]
    y, tap = er.maxpool_fwd(-x)                                         # all negative: padding must not win
    assert float(y) == -1 and int(tap) == 4
    g = er.pool_grad((2, 3, 5, 8), 1)
    assert bool((g * 16 == torch.round(g * 16)).all()) and float(g.abs().max()) <= 8 and torch.equal(er.round_to(g, "bf16"), g)


def test_gap_and_layout_reference():
    rng = np.random.default_rng(2)
    x = torch.from_numpy(rng.standard_normal((2, 12, 24)))
    m, ma = er.gap_fwd(x)
    ref = F.adaptive_avg_pool2d(x.permute(0, 2, 1).reshape(2, 24, 3, 4), 1).flatten(1)
    torch.testing.assert_close(m, ref, rtol=1e-13, atol=1e-13)
    assert bool((ma >= m.abs()).all())
    assert er.gap_fwd(torch.tensor([[[1.0], [2.0], [6.0]]]))[0].item() == 3.0
    df = torch.from_numpy(rng.standard_normal((2, 24)).astype(f32))
    dx = er.gap_bwd(df.numpy(), 12, "fp32")
    assert dx.shape == (2, 12, 24)
    torch.testing.assert_close(dx[:, 5], df.double() / 12, rtol=2 * er.U32, atol=0)
    # by hand, in bf16: 3 * (1.0f / 3) = 1.0000000298 in fp32 -> 1 in bf16
    assert er.gap_bwd(np.array([[3.0]], f32), 3, "bf16").flatten().tolist() == [1.0, 1.0, 1.0]
    t = torch.arange(12, dtype=er.F64).reshape(1, 2, 6)
    assert torch.equal(er.nhwc_to_nchw(t), t.permute(0, 2, 1).float()) and er.nhwc_to_nchw(t)[0, 1].tolist() == [1.0, 7.0]
    assert er.gap_fwd_bound(torch.tensor(2.0), 9).item() == (2 + 8) * er.U32 * 2.0


# ------------------------------------------------------------------------------------------------ 2. bounds vs the emulation
SMALL = [(M, C) for M, C, _, _ in er.BN_SHAPES if M <= 4096]
EMU_CASES = [(M, C, 0.5) for M, C in SMALL] + [(M, C, r) for M, C in er.RATIO_SHAPES for r in (16.0, 256.0)]
RATIOS = er.Ratios()


@pytest.mark.parametrize("kind", er.KINDS)
@pytest.mark.parametrize("M,C,ratio", EMU_CASES)
def test_emulation_stays_within_the_bounds(M, C, ratio, kind):
    modes = ("none", "plain", "dual")
    d = er.bn_inputs(M, C, kind, 100 + M + C, ratio=ratio, res_mode=modes[(M + C // 8) % 3], relu=ratio == 0.5, momentum=MOM, eps=EPS)
    fwd = emu_forward(d)
    er.check_bn_forward(RATIOS, d, fwd)
    rng = np.random.default_rng(M)
    dg0, db0 = rng.standard_normal(C).astype(f32), rng.standard_normal(C).astype(f32)
    er.check_bn_backward(RATIOS, d, fwd, emu_backward(d, fwd, dg0, db0), dg0, db0)


def test_variance_bound_tracks_the_one_pass_error():
    """The relative error of the emulated one-pass variance grows like 2^-24 (1 + ratio^2) and the bound stays above it."""
    seen = []
    for ratio in (16.0, 256.0):
        d = er.bn_inputs(1000, 72, "fp32", 7, ratio=ratio, relu=False, momentum=MOM, eps=EPS)
        x = n32(d["x"])
        S1, S2 = emu_col(x, x, x, 72, "fp32")
        var = np.maximum(S2 / 1000 - (S1 / 1000) ** 2, 0)
        ref = er.bn_forward_ref(d["x"], d["gamma"], d["beta"], d["rmean"], d["rvar"], MOM, EPS)
        b = er.stat_bounds(ref["sum_abs"], ref["sum_sq"], ref["mean"], ref["var"], 1000, EPS, er.gamma_cols(72, "fp32", 1000))
        rel = np.abs(var - ref["var"].numpy()) / ref["var"].numpy()
        assert bool((torch.from_numpy(np.abs(var - ref["var"].numpy())) <= b["var"]).all())
        seen.append(rel.max())
        assert rel.max() < 40 * 2.0 ** -24 * (1 + ratio ** 2) and bool(torch.isfinite(b["invstd"]).all())
    assert seen[1] > 20 * seen[0]


# ------------------------------------------------------------------------------------------------ 3. injected faults
def _small(kind="bf16", **kw):
    return er.bn_inputs(300, 40, kind, 41, momentum=MOM, eps=EPS, **kw)


def test_fault_last_row_of_a_block_dropped():
    d = _small()
    er.check_bn_forward(er.Ratios(), d, emu_forward(d))
    with pytest.raises(AssertionError, match="mean|invstd"):
        er.check_bn_forward(er.Ratios(), d, emu_forward(d, drop_last=True))


@pytest.mark.parametrize("kind", er.KINDS)
def test_fault_coefficients_of_another_chunk_past_the_first_trip(kind):
    d = _small(kind, res_mode="plain")
    with pytest.raises(AssertionError, match="y: "):
        er.check_bn_forward(er.Ratios(), d, emu_forward(d, drift_threads=1024))


def test_fault_tie_resolved_to_the_last_maximum():
    x = er.pool_inputs((2, 4, 6, 8), "bf16", "levels", 5)
    dy = er.pool_grad((2, 2, 3, 8), 6)
    y, tap = emu_pool(x)
    er.check_pool(er.Ratios(), x, y, tap, dy, er.maxpool_bwd(dy, tap, 4, 6, "bf16"), "bf16")
    y, tap = emu_pool(x, last_wins=True)
    with pytest.raises(AssertionError, match="tap codes"):
        er.check_pool(er.Ratios(), x, y, tap, dy, None, "bf16")


def test_fault_padding_read_as_zero():
    x = er.pool_inputs((2, 4, 6, 8), "bf16", "negative", 5)
    y, tap = emu_pool(x, pad_zero=True)
    with pytest.raises(AssertionError, match="pooled values"):
        er.check_pool(er.Ratios(), x, y, tap, None, None, "bf16")


def test_fault_unbiased_factor_at_count_one():
    d = er.bn_inputs(1, 8, "f16", 9, relu=False, momentum=MOM, eps=EPS)
    er.check_bn_forward(er.Ratios(), d, emu_forward(d))
    with pytest.raises(AssertionError, match="running_var"):
        er.check_bn_forward(er.Ratios(), d, emu_forward(d, guard=False))


def test_fault_ibn_second_image_group_gets_the_first_groups_statistics():
    d = er.ibn_inputs(17, 9, 16, 8, "bf16", 13, momentum=MOM, eps=EPS)
    er.check_ibn_forward(er.Ratios(), d, emu_ibn_forward(d))
    with pytest.raises(AssertionError, match="mean|invstd"):
        er.check_ibn_forward(er.Ratios(), d, emu_ibn_forward(d, second_group_bug=True))


# ------------------------------------------------------------------------------------------------ 4. the grid arithmetic
CAPS = (1536, 2048, 1024, 2304)          # 6 and 8 workgroups per compute unit on 256 units, and two others


def test_no_chunk_drifts_to_another_channel():
    n = 0
    for M, C, kinds, _ in er.BN_SHAPES:
        for V in sorted({er.VEC[k] for k in kinds}):
            cpr, total = C // V, M * C // V
            for cap in CAPS:
                blocks = er.ew_blocks_cap(total, cpr, cap)
                assert (blocks * 256) % cpr == 0
                assert er.drifted_chunks(total, cpr, blocks) == 0, (M, C, V, cap, blocks)
                if cpr & (cpr - 1) == 0:            # a power of two keeps the grid it had
                    assert blocks == er.ew_blocks_cap(total, cpr, cap, fixed=False)
                n += 1
    assert n >= 4 * len(er.BN_SHAPES)


def test_the_old_rule_drifted():
    """The motivation, pinned: C = 40 in 16-bit storage, 600000 chunks."""
    old = lambda total, cpr, cap: er.drifted_chunks(total, cpr, er.ew_blocks_cap(total, cpr, cap, fixed=False))   # noqa: E731
    assert old(600000, 5, 2048) == 75712 and old(600000, 5, 1536) == 206784
    assert old(600000, 3, 2048) > 0 and old(600000, 3, 1536) == 0              # C = 24: right by luck at 1536
    assert old(630000, 9, 2048) > 0 and old(630000, 9, 1536) > 0               # C = 72
    for cpr in (5, 10, 9):                                                     # the past-the-cap cases of the sweep, both caps
        for M, C, kinds, _ in er.BN_SHAPES:
            if M >= 60000 and C // er.VEC[kinds[0]] == cpr:
                for cap in (1536, 2048):
                    assert old(M * cpr, cpr, cap) > 1000, (M, C, cap)
