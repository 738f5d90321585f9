"""CPU: what the exact-integer convolution checks (tests/conv_exact.py) see that a tolerance does not, on a torch emulation of a
16-bit 3 x 3 convolution (fp32 accumulation tap by tap, one RNE rounding to bf16), and the helper's plan-key derivation against
bench_train.conv_plan_keys.

Mutants, each at one border output pixel of one odd-sized image (3 images of 7 x 5, 64 -> 64 channels: M = 105, one partial tile):
  * one PRODUCT of one tap dropped (one 16-bit element of the gathered row read as zero).  With the Gaussian operands and the
    tolerance expression of test_backbone_gpu.py::test_conv_fwd_dgrad_wgrad (rtol 3e-2, atol 3e-2 sqrt(K) 0.05 = 0.036 at
    K = 576; one product has a standard deviation of 1 / 24 = 0.042) the mutant PASSES at the seed used here -- asserted, so the
    test documents the gap; 15 of the seeds 0..39 pass, the others leave the tolerance in at most 40 of the 64 output channels;
  * one whole TAP dropped (all 64 products).  Its standard deviation is sqrt(64 / 576) = 1/3 of an output's, nine times the
    tolerance: the old expression REJECTS it (48 .. 60 of the 64 output channels of the pixel fall outside, at every seed 0..39)
    -- asserted as such; a whole-tap slip at one pixel is therefore not a gap of the old test, a single-element slip is;
  * the last row of the partial tile computed from the pixel index wrapped past M (the first row of the first image).
With the integer operands ({-2..2}) the exact comparison reports every one of them: a dropped product changes a result by the
product itself, an integer >= 1 unless an operand is 0 (the element dropped here is checked to be non-zero)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_exact as ce
from centroids_reid_amd.bench_train import PLAN_WORKLOADS, conv_plan_keys

BF = torch.bfloat16
B, H, W, CIN, COUT, K = 3, 7, 5, 64, 64, 576
PIXEL = (1, 0, 2)                 # image 1, top border row, column 2: its row index in the [M, C] view is 35 + 2 = 37
TAP = (1, 1)                      # the centre tap: never padding, so dropping it always drops real products
SEED = 4


def test_plan_keys_reproduce_conv_plan_keys():
    """the helper's default keys are bench_train.conv_plan_keys's, on every geometry of PLAN_WORKLOADS and both last strides"""
    n = 0
    for (Hh, Ww), batches in PLAN_WORKLOADS.items():
        for Bb in batches:
            for ls in (1, 2):
                for shape, keys in conv_plan_keys(Bb, Hh, Ww, ls):
                    assert ce.plan_keys(Bb, *shape) == keys, (Bb, shape)
                    n += 1
    assert n > 1000
    # and the production collisions tests/test_conv_edge_sweep_gpu.py builds on are in the shipped file
    assert ce.plan_keys(64, 512, 512, 3, 1, 16, 8)["fwd"] in ce.PLANS


def test_c64_coverage_mirror():
    """launch_conv3x3_c64's two tilings (conv_stream.hip)"""
    for hw in ((8, 16), (8, 48), (4, 32), (2, 64), (16, 80), (64, 32), (80, 80)):
        assert ce.c64_covers(*hw), hw
    for hw in ((12, 16), (8, 24), (3, 32), (16, 8), (7, 5), (1, 1), (1, 64)):
        assert not ce.c64_covers(*hw), hw


# ------------------------------------------------------------------------------------ the emulated kernel and its mutants
def conv16(x, w, drop=None, wrap_last=False, dtype=BF):
    """3 x 3, stride 1, pad 1 over NHWC x and OIHW w as the 16-bit kernels compute it: products of the stored operands summed in
    fp32 tap by tap, one rounding.  drop = (channels c0:c1 of TAP at PIXEL are read as zero); wrap_last: row M - 1 of the [M, C]
    view gathers the pixel with index M wrapped to 0."""
    Bn, Hh, Ww, cin = x.shape
    xp = F.pad(x.float(), (0, 0, 1, 1, 1, 1))
    y = torch.zeros(Bn, Hh, Ww, w.shape[0])
    for r in range(3):
        for c in range(3):
            src = xp[:, r:r + Hh, c:c + Ww, :].clone()
            if drop is not None and (r, c) == TAP:
                src[PIXEL][drop[0]:drop[1]] = 0
            y += (src.reshape(-1, cin) @ w.float()[:, :, r, c].t()).view(y.shape)
    if wrap_last:
        y.view(-1, w.shape[0])[-1] = y.view(-1, w.shape[0])[0]
    return y.to(dtype)


def _gauss(seed):
    """the operands of test_conv_fwd_dgrad_wgrad: standard normal x, w / sqrt(K), rounded to bf16; reference in fp64"""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((B, H, W, CIN)).astype(np.float32)).to(BF)
    w = torch.from_numpy((rng.standard_normal((COUT, CIN, 3, 3)) / np.sqrt(K)).astype(np.float32)).to(BF)
    return x, w, ce.ref_fwd(x, w, 1, 1, 0, B)


def _ints(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (B, H, W, CIN), generator=g, dtype=torch.int8)
    w = torch.randint(-2, 3, (COUT, CIN, 3, 3), generator=g, dtype=torch.int8)
    return x, w, ce.ref_fwd(x, w, 1, 1, 0, B)


def _old_tolerance_violations(got, ref):
    """numpy.testing.assert_allclose(got, ref, rtol, atol) of test_conv_fwd_dgrad_wgrad's bf16 forward: |got - ref| <= atol +
    rtol |ref| with (rtol, atol) = (3e-2, 3e-2 sqrt(K) 0.05); the number of elements outside"""
    rt, at = 3e-2, 3e-2 * np.sqrt(K) * 0.05
    return int(((got.double() - ref).abs() > at + rt * ref.abs()).sum())


def _exact_mismatches(got, ref, dtype=BF):
    """Sweep.compare on the [M, C] view against the correctly rounded reference -> (count, first (row, col, got, expected))"""
    sw, state = ce.Sweep(dtype, False), {}
    sw.compare("fwd", "cpu", None, got.reshape(-1, COUT), ce._rd(ref, dtype).reshape(-1, COUT), 0, state)
    return state["fwd"][:2] if state else (0, None)


def test_unmutated_emulation_passes_both_checks():
    x, w, ref = _gauss(SEED)
    assert _old_tolerance_violations(conv16(x, w), ref) == 0
    for dtype in (BF, torch.float16):
        x, w, ref = _ints(SEED)
        assert _exact_mismatches(conv16(x, w, dtype=dtype), ref, dtype) == (0, None)


def test_dropped_product_passes_the_old_tolerance_and_fails_the_exact_comparison():
    x, w, ref = _gauss(SEED)
    mutant = conv16(x, w, drop=(0, 1))
    assert not torch.equal(mutant, conv16(x, w)), "the mutation must change the output"
    assert _old_tolerance_violations(mutant, ref) == 0, "the gap: the old tolerance accepts a dropped product at a border pixel"
    x, w, ref = _ints(SEED)
    assert int(x[PIXEL][0]) != 0
    n, first = _exact_mismatches(conv16(x, w, drop=(0, 1)), ref)
    # every output channel whose weight at (channel 0, centre tap) is non-zero is off by |x w| >= 1
    assert n == int((w[:, 0, 1, 1] != 0).sum()) and n >= 40, n
    assert first[0] == (PIXEL[0] * H + PIXEL[1]) * W + PIXEL[2], first


def test_dropped_tap_fails_both_checks():
    """a whole tap is 1/3 of an output's standard deviation: the old expression rejects it too, at most of the 64 channels"""
    for seed in (SEED, 0, 1):
        x, w, ref = _gauss(seed)
        assert _old_tolerance_violations(conv16(x, w, drop=(0, CIN)), ref) >= 40
    x, w, ref = _ints(SEED)
    n, first = _exact_mismatches(conv16(x, w, drop=(0, CIN)), ref)
    assert n >= 56 and first[0] == 37, (n, first)


def test_wrapped_last_row_of_a_partial_tile_fails_the_exact_comparison():
    """M = 105: row 104 gathered from pixel index 105 wrapped to 0.  The exact comparison sees the row; so do the zero-padded
    statistics of the partial tile (conv_exact.run_geometry), whose column sums change by the difference of the two rows."""
    x, w, ref = _ints(SEED)
    assert (B * H * W) % 128 == 105
    mutant = conv16(x, w, wrap_last=True)
    n, first = _exact_mismatches(mutant, ref)
    assert n >= 56 and first[0] == B * H * W - 1, (n, first)
    pad = lambda t: F.pad(t.reshape(-1, COUT).double(), (0, 0, 0, 23)).view(-1, 128, COUT).sum(1)
    assert not torch.equal(pad(mutant), pad(ref))
    assert torch.equal(pad(conv16(x, w)), pad(ref))


@pytest.mark.parametrize("seed", range(3))
def test_old_tolerance_gap_is_not_a_single_seed(seed):
    """The dropped product stays small at every seed: never more than 40 of the pixel's 64 outputs leave the old tolerance, and
    the other 6656 outputs of the tensor never do -- while the exact comparison counts every non-zero weight."""
    x, w, ref = _gauss(seed)
    assert _old_tolerance_violations(conv16(x, w, drop=(0, 1)), ref) <= 40
    x, w, ref = _ints(seed)
    n, _ = _exact_mismatches(conv16(x, w, drop=(0, 1)), ref)
    assert n == (int((w[:, 0, 1, 1] != 0).sum()) if int(x[PIXEL][0]) != 0 else 0)
