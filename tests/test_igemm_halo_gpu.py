"""The resident-halo form of the producer/consumer convolution kernel (csrc/conv_igemm.hip igemm_bf16_halo_kernel) on the GPU:
bit-identical to the tile kernel it replaces (CREID_IGEMM_HALO=0) with continuous operands, exact against an fp64 reference with
small-integer operands (so the two cannot be wrong together), not taken by geometries it does not cover, and invisible in a
whole training step.  creid_igemm_halo_launches proves which path ran.  The N tile and ring depth of a case are fixed by
registering a launch plan of kind 0 (producer/consumer kernel) for its GEMM shape, as the tuner does."""
import numpy as np
import pytest
import torch

import test_igemm_halo_cpu as hc

DTYPES = [torch.bfloat16, torch.float16]
SUMSQ_REL = 130 * 2.0 ** -24       # sums of squares of a 128-pixel tile once partial sums pass 2^24 (tests/test_plan_sweep_gpu.py)


def _launches():
    from centroids_reid_amd import _lib as L
    return int(L.lib().creid_igemm_halo_launches())


class _Plans:
    """plans (N tile, ring depth, kernel 0) for the forward and the data-gradient GEMM of one case; the shipped file on exit"""
    def __init__(self, M, c, bn, ns):
        self.keys = [(1, M, c, 9 * c, d) for d in (2, 3)]          # 4th slot: transposed | stride << 1
        self.word = (bn, ns, 0)

    def __enter__(self):
        from centroids_reid_amd import _lib as L
        L.lib().creid_tune_clear()
        for k in self.keys:
            assert L.lib().creid_tune_set(*k, *self.word) == 0

    def __exit__(self, *exc):
        from centroids_reid_amd import _lib as L
        L.lib().creid_tune_clear()
        L.load_tuned_plans()


def _forms(x, dy, res, add, krsc, crsk, ss, hw):
    """the five launch forms; outputs in a fixed order"""
    from centroids_reid_amd import layers as ly
    y, part = ly.conv2d_fwd(x, krsc, 1, 1, with_stats=True)
    return {"fwd": y, "fwd_stats": part,
            "aff_res_relu": ly.conv2d_fwd_affine(x, krsc, 1, 1, ss, res, True),
            "aff_plain": ly.conv2d_fwd_affine(x, krsc, 1, 1, ss, None, False),
            "dgrad": ly.conv2d_dgrad(dy, crsk, hw, 1, 1),
            "dgrad_add": ly.conv2d_dgrad(dy, crsk, hw, 1, 1, add_src=add)}


def _ids(c):
    return f"c{c[0]}_B{c[1]}_{c[2]}x{c[3]}_bn{c[4]}_ns{c[5]}"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", hc.CASES, ids=_ids)
def test_halo_kernel_is_bit_identical_to_the_tile_kernel(case, dtype, monkeypatch):
    """Random-normal operands: every output of the five forms equal bit for bit with the switch on and off; the launch counter
    advances once per launch under CREID_IGEMM_HALO=1 and not at all under =0.  (CREID_C64_3X3=0: layer1's own forward kernel
    would take the 64-channel statistics and plain-affine forms ahead of both.)"""
    from centroids_reid_amd import layers as ly
    c, B, H, W, bn, ns = case
    rng = np.random.default_rng(c + B + H + W + bn)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dtype).cuda()
    x, dy, res, add = t(B, H, W, c), t(B, H, W, c), t(B, H, W, c), t(B, H, W, c)
    w = torch.from_numpy((rng.standard_normal((c, c, 3, 3)) / (3.0 * c ** 0.5)).astype(np.float32)).cuda()
    krsc, crsk = ly.weight_prep(w, dtype)
    ss = torch.from_numpy(np.stack([rng.uniform(0.5, 1.5, c), rng.standard_normal(c) * 0.3]).astype(np.float32)).cuda()
    monkeypatch.setenv("CREID_C64_3X3", "0")
    with _Plans(B * H * W, c, bn, ns):
        monkeypatch.setenv("CREID_IGEMM_HALO", "0")
        n0 = _launches()
        base = _forms(x, dy, res, add, krsc, crsk, ss, (H, W))
        n1 = _launches()
        monkeypatch.setenv("CREID_IGEMM_HALO", "1")
        new = _forms(x, dy, res, add, krsc, crsk, ss, (H, W))
        n2 = _launches()
    torch.cuda.synchronize()
    assert n1 == n0, "CREID_IGEMM_HALO=0 must restore the tile kernel"
    assert n2 - n1 == 5, "every form runs the halo kernel"
    for k in base:
        assert torch.equal(new[k], base[k]), k
    assert bool(torch.isfinite(new["fwd"].float()).all()) and float(new["fwd"].float().abs().max()) > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", hc.CASES, ids=_ids)
def test_halo_kernel_is_exact_with_small_integer_operands(case, dtype, monkeypatch):
    """Operands from {+-1, +-2}: every fp32 accumulator is an exact integer (< 4 * 2304), so each output is the one correctly
    rounded value of the fp64 tap-by-tap reference.  tests/test_igemm_halo_cpu.py shows that a wrong border changes >= 90 % of the
    border outputs of these operands."""
    from centroids_reid_amd import layers as ly
    c, B, H, W, bn, ns = case
    gen = torch.Generator().manual_seed(c * 7 + B + H + W + bn)
    x8, dy8, res8, add8 = (hc.pm12((B, H, W, c), gen) for _ in range(4))
    w8 = hc.pm12((c, c, 3, 3), gen)
    ss = torch.stack([torch.randint(1, 5, (c,), generator=gen) * 0.5, torch.randint(-8, 9, (c,), generator=gen) * 0.25]).float()
    x, dy, res, add = (v.to(dtype).cuda() for v in (x8, dy8, res8, add8))
    krsc, crsk = ly.weight_prep(w8.cuda(), dtype)
    monkeypatch.setenv("CREID_C64_3X3", "0")
    monkeypatch.setenv("CREID_IGEMM_HALO", "1")
    with _Plans(B * H * W, c, bn, ns):
        n0 = _launches()
        got = _forms(x, dy, res, add, krsc, crsk, ss.cuda(), (H, W))
        assert _launches() - n0 == 5
    torch.cuda.synchronize()
    rd = lambda v: v.float().to(dtype).double()
    y = hc.ref_conv3x3(x8, w8, 0)
    dx = hc.ref_conv3x3(dy8, w8, 1)
    v = y * ss[0].double() + ss[1].double()                        # exact: dyadic scale / shift
    exp = {"fwd": rd(y), "aff_res_relu": rd(torch.relu(rd(v) + res8.double())), "aff_plain": rd(v),
           "dgrad": rd(dx), "dgrad_add": rd(rd(dx) + add8.double())}
    for k, e in exp.items():
        g = got[k].double().cpu()
        bad = g != e
        assert not bool(bad.any()), (k, int(bad.sum()), bad.nonzero()[:4].tolist())
    tiles = y.reshape(-1, 128, c)
    part = got["fwd_stats"].double().cpu()
    assert torch.equal(part[:, 0], tiles.sum(1)), "column sums of the accumulators"
    t2 = (tiles * tiles).sum(1)
    assert bool(((part[:, 1] - t2).abs() <= SUMSQ_REL * t2).all()), "column sums of squares"


# (cin, cout, k, stride, B, H, W): what the halo kernel does not cover runs as before
INELIGIBLE = [(128, 128, 3, 2, 2, 16, 16), (512, 512, 3, 1, 1, 16, 8), (64, 64, 3, 1, 1, 80, 80), (64, 256, 1, 1, 2, 16, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", INELIGIBLE, ids=["stride2", "c512", "80x80", "1x1"])
def test_ineligible_geometries_keep_their_kernels(case, monkeypatch):
    from centroids_reid_amd import layers as ly
    cin, cout, k, s, B, H, W = case
    p = k // 2
    oh, ow = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    rng = np.random.default_rng(sum(case))
    x = torch.from_numpy(rng.standard_normal((B, H, W, cin)).astype(np.float32)).to(torch.bfloat16).cuda()
    dy = torch.from_numpy(rng.standard_normal((B, oh, ow, cout)).astype(np.float32)).to(torch.bfloat16).cuda()
    w = torch.from_numpy((rng.standard_normal((cout, cin, k, k)) / (k * cin ** 0.5)).astype(np.float32)).cuda()
    krsc, crsk = ly.weight_prep(w, torch.bfloat16)
    monkeypatch.setenv("CREID_C64_3X3", "0")
    outs = []
    n0 = _launches()
    for sw in ("1", "0"):
        monkeypatch.setenv("CREID_IGEMM_HALO", sw)
        y, part = ly.conv2d_fwd(x, krsc, s, p, with_stats=True)
        outs.append((y, part, ly.conv2d_dgrad(dy, crsk, (H, W), s, p)))
    torch.cuda.synchronize()
    assert _launches() == n0
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_training_step_is_bit_identical_with_and_without_the_halo_kernel(monkeypatch):
    """One whole training step of the benchmark model (ResNet50, bf16, P2 x K4 at 256 x 128): loss, logged distances, every
    parameter gradient and every BatchNorm statistic equal bit for bit with the switch on and off -- this covers the launches that
    carry the fused BatchNorm-backward column sums, the masked adds and the piggy-backed weight-gradient reductions."""
    from centroids_reid_amd import ops
    from centroids_reid_amd.bench_train import make_model, synthetic_batch
    # the classifier GEMMs of the heads split K over fp32 atomics by default (order-dependent last bits, run to run): their
    # single-pass form, so that two steps can be compared bit for bit at all
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    batch = synthetic_batch(2, 4, 256, 128, 0)
    res = []
    for sw in ("1", "0"):
        monkeypatch.setenv("CREID_IGEMM_HALO", sw)
        torch.manual_seed(1234)
        model = make_model()
        n0 = _launches()
        out = model.forward_backward(batch, 0)
        torch.cuda.synchronize()
        res.append((_launches() - n0, out,
                    {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None},
                    {n: b.detach().clone() for n, b in model.named_buffers()}))
        del model
    (n_on, out_on, g_on, b_on), (n_off, out_off, g_off, b_off) = res
    # layer1: 3 data gradients (its forward stays on conv3x3_c64_kernel); layer2: 3 + 3 (block 0's conv2 is stride 2);
    # layer3: 5 + 5; layer4's conv2 of blocks 1, 2 has 512 channels
    assert n_on == 19 and n_off == 0, (n_on, n_off)
    assert torch.equal(out_on["loss"], out_off["loss"])
    for k in out_on["other"]:
        assert torch.equal(torch.as_tensor(out_on["other"][k]), torch.as_tensor(out_off["other"][k])), k
    assert set(g_on) == set(g_off) and len(g_on) > 150
    for n in g_on:
        assert torch.equal(g_on[n], g_off[n]), n
    assert set(b_on) == set(b_off) and any(n.endswith("running_var") for n in b_on)
    for n in b_on:
        assert torch.equal(b_on[n], b_off[n]), n
