"""The tap-fused weight-gradient kernel (csrc/conv_wgrad.hip wgrad_bf16_taps_kernel) on the GPU: exact against an fp64 reference
with small-integer operands (any summation order gives the same bits, so it cannot be wrong together with the tile kernel it is
also compared to), inside the fp32 summation bound with continuous operands, taken exactly where the coverage rule says
(creid_wgrad_taps_launches), carrying the BatchNorm-backward finalize with the bits of the stand-alone launch, and invisible in a
backbone's backward pass except for the rounding of the covered weight gradients."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import test_wgrad_taps_cpu as tc

DTYPES = [torch.bfloat16, torch.float16]
CASES = [(cin, cout, h, w, B) for cin, cout in tc.CHANNELS for h, w in tc.SIZES for B in tc.BATCHES]
# workgroup targets (CREID_WGRAD_TAPS_WGS; None: the built-in one): the default gives these small shapes one k-step per workgroup; 2 -> two splits of
# unequal length ((3, 2) k-steps at B = 5), 1 -> one split of B k-steps, so the 3-deep LDS ring wraps
TARGETS = [None, "2", "1"]
U = 2.0 ** -24


def _ids(c):
    return f"{c[0]}to{c[1]}_{c[2]}x{c[3]}_B{c[4]}"


def _target(monkeypatch, target):
    if target is None:
        monkeypatch.delenv("CREID_WGRAD_TAPS_WGS", raising=False)
    else:
        monkeypatch.setenv("CREID_WGRAD_TAPS_WGS", target)


def _launches():
    from centroids_reid_amd import _lib as L
    return int(L.lib().creid_wgrad_taps_launches())


def _splits(B, h, w, cin, cout, dtype, k=3, s=1):
    from centroids_reid_amd import layers as ly, _lib as L
    d, _, _ = ly.conv_desc(B, h, w, cin, cout, k, s, k // 2)
    return int(L.lib().creid_conv2d_wgrad_workspace_bytes(C.byref(d), L._DT[dtype])) // (cout * cin * k * k * 4)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_exact_against_fp64_and_the_tile_kernel(case, dtype, monkeypatch):
    """Operands from {+-1, +-2}: every fp32 partial sum is an integer below 2^24, so the gradient equals the fp64 reference bit for
    bit in the plain and the accumulate form, at every workgroup target, and equals the tile kernel's (CREID_WGRAD_TAPS=0)."""
    from centroids_reid_amd import layers as ly
    cin, cout, h, w, B = case
    gen = torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(case).encode()))
    x = tc.pm12((B, h, w, cin), gen, "cuda").to(dtype)
    dy = tc.pm12((B, h, w, cout), gen, "cuda").to(dtype)
    base = tc.pm12((cout, cin, 3, 3), gen, "cuda") * 3.0
    ref = tc.ref_wgrad(x, dy)
    for target in TARGETS:
        _target(monkeypatch, target)
        monkeypatch.setenv("CREID_WGRAD_TAPS", "1")
        assert _splits(B, h, w, cin, cout, dtype) == tc.taps_splits(B * h * w, cin, cout, target and int(target))[0]
        n0 = _launches()
        got = ly.conv2d_wgrad(x, dy, 3, 1, 1)
        acc = ly.conv2d_wgrad(x, dy, 3, 1, 1, out=base.clone(), accumulate=True)
        torch.cuda.synchronize()
        assert _launches() == n0 + 2
        assert torch.equal(got.double(), ref), (target, int((got.double() != ref).sum()))
        assert torch.equal(acc.double(), ref + base.double()), target
    monkeypatch.setenv("CREID_WGRAD_TAPS", "0")
    n0 = _launches()
    tile = ly.conv2d_wgrad(x, dy, 3, 1, 1)
    torch.cuda.synchronize()
    assert _launches() == n0
    assert torch.equal(tile, got)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_continuous_operands_stay_inside_the_fp32_summation_bound(case, dtype, monkeypatch):
    """Random-normal operands against fp64 of the same rounded operands:
    |got - ref| <= ((M + splits - 1) // splits + 64 + splits) 2^-24 ref(|x|, |dy|) elementwise (fp32 accumulation of the exact
    products in any order within a split, then the splits in any order), the split count read back from the workspace size."""
    from centroids_reid_amd import layers as ly
    cin, cout, h, w, B = case
    gen = torch.Generator(device="cuda").manual_seed(zlib.crc32(repr((case, "normal")).encode()))
    x = torch.randn((B, h, w, cin), generator=gen, device="cuda").to(dtype)
    dy = torch.randn((B, h, w, cout), generator=gen, device="cuda").to(dtype)
    ref, mag = tc.ref_wgrad(x, dy), tc.ref_wgrad(x.abs(), dy.abs())
    M = B * h * w
    for target in TARGETS:
        _target(monkeypatch, target)
        monkeypatch.setenv("CREID_WGRAD_TAPS", "1")
        splits = _splits(B, h, w, cin, cout, dtype)
        n0 = _launches()
        got = ly.conv2d_wgrad(x, dy, 3, 1, 1)
        torch.cuda.synchronize()
        assert _launches() == n0 + 1
        err, bound = (got.double() - ref).abs(), ((M + splits - 1) // splits + 64 + splits) * U * mag
        print(f"{_ids(case)} target {target} splits {splits}: max err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (target, int((err > bound).sum()), float((err / bound).max()))


# (cin, cout, k, stride, B, H, W, dtype)
NOT_COVERED = [(128, 128, 3, 2, 2, 16, 16, torch.bfloat16), (64, 256, 1, 1, 2, 16, 8, torch.bfloat16),
               (64, 64, 3, 1, 2, 16, 8, torch.float32), (64, 64, 3, 1, 2, 8, 4, torch.bfloat16)]


@pytest.mark.gpu
def test_routing(monkeypatch):
    """The launch counter advances once per covered launch with the switch on; not with the switch off, and not for a stride-2
    3 x 3, a 1 x 1, fp32 or a feature map the k-step does not tile -- those give the same bits under either switch value."""
    from centroids_reid_amd import layers as ly
    rng = np.random.default_rng(7)

    def operands(B, H, W, cin, cout, k, s, dtype):
        p = k // 2
        oh, ow = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        x = torch.from_numpy(rng.standard_normal((B, H, W, cin)).astype(np.float32)).to(dtype).cuda()
        dy = torch.from_numpy(rng.standard_normal((B, oh, ow, cout)).astype(np.float32)).to(dtype).cuda()
        return x, dy

    for dtype in DTYPES:
        x, dy = operands(3, 16, 8, 128, 64, 3, 1, dtype)
        monkeypatch.setenv("CREID_WGRAD_TAPS", "1")
        n0 = _launches()
        for i in range(3):
            ly.conv2d_wgrad(x, dy, 3, 1, 1)
            assert _launches() == n0 + i + 1
        monkeypatch.setenv("CREID_WGRAD_TAPS", "0")
        ly.conv2d_wgrad(x, dy, 3, 1, 1)
        assert _launches() == n0 + 3
    for cin, cout, k, s, B, H, W, dtype in NOT_COVERED:
        x, dy = operands(B, H, W, cin, cout, k, s, dtype)
        n0 = _launches()
        outs = []
        for sw in ("1", "0"):
            monkeypatch.setenv("CREID_WGRAD_TAPS", sw)
            outs.append(ly.conv2d_wgrad(x, dy, k, s, k // 2))
        torch.cuda.synchronize()
        assert _launches() == n0, (cin, cout, k, s)
        assert torch.equal(outs[0], outs[1])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("bn_c,bn_rows", [(256, 64), (64, 1024), (1000, 7)])
def test_carried_finalize_has_the_bits_of_the_stand_alone_launch(bn_c, bn_rows, dtype, monkeypatch):
    """creid_conv2d_wgrad_partials_bnfin on a covered shape: with the switch on the finalize rides in the kernel's first
    workgroups; with it off the tile kernel carries it or its own launch follows.  bn_sums, dgamma and dbeta equal bit for bit;
    so does the weight gradient summed from the partial planes (small-integer operands: exact, equal to fp64)."""
    from centroids_reid_amd import layers as ly, _lib as L
    lib = L.lib()
    B, h, w, cin, cout = 3, 16, 8, 256, 256
    gen = torch.Generator(device="cuda").manual_seed(bn_c + bn_rows)
    x = tc.pm12((B, h, w, cin), gen, "cuda").to(dtype)
    dy = tc.pm12((B, h, w, cout), gen, "cuda").to(dtype)
    part = torch.randn((bn_rows, 2, bn_c), generator=gen, device="cuda")
    mean = torch.randn(bn_c, generator=gen, device="cuda")
    invstd = torch.rand(bn_c, generator=gen, device="cuda") + 0.5
    gamma = torch.randn(bn_c, generator=gen, device="cuda")
    g0, b0 = torch.randn(bn_c, generator=gen, device="cuda"), torch.randn(bn_c, generator=gen, device="cuda")
    d, _, _ = ly.conv_desc(B, h, w, cin, cout, 3, 1, 1)
    res = []
    for sw in ("1", "0"):
        monkeypatch.setenv("CREID_WGRAD_TAPS", sw)
        nbytes = int(lib.creid_conv2d_wgrad_workspace_bytes(C.byref(d), L._DT[dtype]))
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        sums = torch.full((3, bn_c), float("nan"), device="cuda")
        dgam, dbet = g0.clone(), b0.clone()
        n0 = _launches()
        L.check(lib.creid_conv2d_wgrad_partials_bnfin(C.byref(d), L.ptr(x), L.ptr(dy), L.ptr(ws), nbytes, L._DT[dtype], L.ptr(part),
                                                      bn_rows, bn_c, 4096, L.ptr(mean), L.ptr(invstd), L.ptr(gamma), L.ptr(sums),
                                                      L.ptr(dgam), L.ptr(dbet), L.stream()), "conv2d_wgrad_partials_bnfin")
        dw = torch.zeros((cout, cin, 3, 3), device="cuda")
        L.check(lib.creid_conv2d_wgrad_reduce_job(C.byref(d), L.ptr(dw), 0, L.ptr(ws), nbytes, L._DT[dtype], L.stream()),
                "conv2d_wgrad_reduce_job")
        torch.cuda.synchronize()
        assert _launches() == n0 + (1 if sw == "1" else 0)
        res.append((sums, dgam, dbet, dw))
    for a, b, name in zip(res[0], res[1], ("bn_sums", "dgamma", "dbeta", "dw")):
        assert not bool(torch.isnan(a).any()), name
        assert torch.equal(a, b), name
    assert torch.equal(res[0][3].double(), tc.ref_wgrad(x, dy))


@pytest.mark.gpu
def test_backward_pass_differs_only_in_the_covered_weight_gradients(monkeypatch):
    """One forward + backward of ResNet50 (bf16, 4 x 128 x 64: the smallest configuration of tests/test_backbone_gpu.py) with the
    switch on and off.  The weight gradient feeds nothing else in the backward pass: every parameter gradient is bit-identical --
    the BatchNorm gradients included, whose finalizes the fused launches now carry -- except the weights of the covered 3 x 3
    layers (layer1 at 32 x 16, layer2 at 16 x 8), and those lie inside the summation bound against fp64 of the launch's own
    operands, recorded at the engine's weight-gradient call."""
    from oracle import backbone_oracle as bo
    from centroids_reid_amd import backbone as bb
    x = bo.synthetic_images(4, 128, 64, seed=31).cuda()
    coef = torch.from_numpy(np.random.default_rng(9).standard_normal((4, 2048)).astype(np.float32)).cuda()
    sd = bo.make_state_dict("resnet50", 1, seed=1234)
    runs = []
    for sw in ("1", "0"):
        monkeypatch.setenv("CREID_WGRAD_TAPS", sw)
        net = bb.build_backbone("resnet50", 1)
        net.load_state_dict(sd, strict=False)
        net = net.cuda()
        eng = bb.BackboneEngine(net, torch.bfloat16)
        seen = {}
        inner = eng._wgrad

        def record(u, a_in, dy, B, H, W, *, fin=None, inner=inner, seen=seen):
            if u.k == 3 and u.stride == 1 and tc.covers(u.cin, u.cout, 3, 1, 1, H, W, H, W, B * H * W):
                seen[id(u.conv.weight)] = (a_in.detach().clone().view(B, H, W, u.cin), dy.detach().clone().view(B, H, W, u.cout))
            return inner(u, a_in, dy, B, H, W, fin=fin)

        eng._wgrad = record
        n0 = _launches()
        eng.forward(x, training=True)
        eng.backward(coef)
        torch.cuda.synchronize()
        assert not eng._wred_pending and not eng._bn_sums     # (_bn_sums: the carried finalizes issued and not yet consumed)
        names = {id(p): n for n, p in net.named_parameters()}
        runs.append((_launches() - n0, {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None},
                     {names[k]: v for k, v in seen.items()}))
    (n_on, g_on, ops_on), (n_off, g_off, ops_off) = runs
    assert n_on == len(ops_on) == 6 and n_off == 0, (n_on, len(ops_on), n_off)          # layer1: 3 blocks, layer2: blocks 1-3
    assert set(g_on) == set(g_off) and len(g_on) > 150
    for n in g_on:
        if n not in ops_on:
            assert torch.equal(g_on[n], g_off[n]), n
    for n, (a_in, dy) in ops_on.items():
        assert torch.equal(a_in, ops_off[n][0]) and torch.equal(dy, ops_off[n][1]), n    # same operands either way
        B, H, W, cin = a_in.shape
        cout = dy.shape[3]
        ref, mag = tc.ref_wgrad(a_in, dy), tc.ref_wgrad(a_in.abs(), dy.abs())
        M = B * H * W
        for sw, g in (("1", g_on[n]), ("0", g_off[n])):
            monkeypatch.setenv("CREID_WGRAD_TAPS", sw)
            splits = _splits(B, H, W, cin, cout, torch.bfloat16)
            bound = ((M + splits - 1) // splits + 64 + splits) * U * mag
            err = (g.double() - ref).abs()
            assert bool((err <= bound).all()), (n, sw, float((err / bound).max()))
