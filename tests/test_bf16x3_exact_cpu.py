"""CPU: the operand grid and the three-term fp64 references of tests/x3_exact.py, which tests/test_bf16x3_exact_gpu.py holds the
bf16x3 kernels to bit for bit -- the grid's promises, the references against torch's own fp64 convolution and gradients, what a
misplaced or missing low-order plane does to the reference, and which kernel instantiations the GPU file's case tables run."""
import pytest
import torch
import torch.nn.functional as F

import test_bf16x3_exact_gpu as gpu_file
import x3_exact as xe


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_grid_promises():
    """On 1e6 elements: hi is an integer in {-1, 0, 1}, lo a multiple of 2^-11 of at most 3 units, hi + lo == x exactly, and lo
    is busy: non-zero in at least 40 % of the elements (the construction gives 4/7; with lo == 0 everywhere this would be the
    integer test again)."""
    x = xe.grid_operands((1000, 1000), _gen(1))
    hi, lo = xe.split(x)
    assert torch.equal(hi, hi.round()) and float(hi.abs().max()) == 1.0
    assert torch.equal(hi + lo, x)
    units = lo / xe.LO_UNIT
    assert torch.equal(units, units.round()) and float(units.abs().max()) == 3.0
    assert not bool(lo[hi == 0].any())
    busy = float((lo != 0).float().mean())
    print(f"lo != 0 in {100 * busy:.1f} % of the elements")
    assert busy >= 0.40
    thin = xe.grid_operands((1000, 1000), _gen(2), density=0.25)
    assert 0.15 < float((thin != 0).float().mean()) < 0.19          # 2/3 * 1/4
    th, tl = xe.split(thin)
    assert torch.equal(th + tl, thin) and torch.equal(th, th.round())


@pytest.mark.parametrize("case", [(2, 9, 7, 8, 6, 3, 1), (2, 10, 8, 8, 6, 3, 2), (3, 8, 6, 4, 8, 1, 2), (2, 5, 5, 4, 4, 1, 1)])
def test_references_match_torch_conv(case):
    """Each three-term reference against the sum of torch's fp64 conv2d / conv2d_input / conv2d_weight on the operand pairs
    (lo, hi), (hi, lo), (hi, hi); grid operands, so every fp64 sum is exact and the comparison is equality.  Odd sizes and
    stride 2 included (the cases of test_plan_sweep_gpu.py::test_reference_matches_torch_conv)."""
    B, H, W, cin, cout, k, s = case
    p = k // 2
    oh, ow = xe.out_hw(H, W, k, s, p)
    g = _gen(sum(case))
    x, w, dy = xe.grid_operands((B, H, W, cin), g), xe.grid_operands((cout, cin, k, k), g), xe.grid_operands((B, oh, ow, cout), g)

    def nchw(t):
        return t.permute(0, 3, 1, 2).double()

    xs, ws, dys = xe.split(x), xe.split(w), xe.split(dy)
    fwd = sum(F.conv2d(nchw(xs[i]), ws[j].double(), stride=s, padding=p) for i, j in xe.TERMS)
    dgr = sum(torch.nn.grad.conv2d_input((B, cin, H, W), ws[j].double(), nchw(dys[i]), stride=s, padding=p) for i, j in xe.TERMS)
    wgr = sum(torch.nn.grad.conv2d_weight(nchw(xs[j]), w.shape, nchw(dys[i]), stride=s, padding=p) for i, j in xe.TERMS)
    assert torch.equal(xe.ref_fwd_x3(x, w, s, p), fwd.permute(0, 2, 3, 1))
    assert torch.equal(xe.ref_dgrad_x3(dy, w, s, p, H, W), dgr.permute(0, 2, 3, 1))
    assert torch.equal(xe.ref_wgrad_x3(x, dy, k, s, p), wgr)
    # the margin is the same computation on absolute values
    assert torch.equal(xe.exactness_margin(xe.ref_fwd_x3, x, w, s, p) / xe.MARGIN_SCALE,
                       sum(F.conv2d(nchw(xs[i]).abs(), ws[j].double().abs(), stride=s, padding=p) for i, j in xe.TERMS).permute(0, 2, 3, 1))


def test_deepest_reduction_is_exact_in_any_order():
    """K = 4608 (the network's deepest reduction): the margin is below 1, the reference is fp32-representable, and fp32
    emulations in two k orders, summing the three terms k-step by k-step as the kernel does, equal it bit for bit; the full
    product x w (with lo * lo) is a different number almost everywhere."""
    g = _gen(3)
    x, w = xe.grid_operands((1, 8, 8, 512), g), xe.grid_operands((64, 512, 3, 3), g)
    ref = xe.ref_fwd_x3(x, w, 1, 1).reshape(64, 64)
    margin = float(xe.exactness_margin(xe.ref_fwd_x3, x, w, 1, 1).max())
    print(f"K = 4608: worst margin {margin:.3f}")
    assert margin < 1 and xe.is_fp32(ref)
    # im2col, then 16-deep k-steps in fp32, forwards and backwards
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    cols = torch.cat([xp[:, r:r + 8, c:c + 8, :].reshape(64, 512) for r in range(3) for c in range(3)], 1)
    wk = w.permute(0, 2, 3, 1).reshape(64, 4608)
    (ah, al), (bh, bl) = xe.split(cols), xe.split(wk)
    for order in (range(0, 4608, 16), reversed(range(0, 4608, 16))):
        acc = torch.zeros(64, 64)
        for k0 in order:
            ks = slice(k0, k0 + 16)
            acc = acc + al[:, ks] @ bh[:, ks].t()
            acc = acc + ah[:, ks] @ bl[:, ks].t()
            acc = acc + ah[:, ks] @ bh[:, ks].t()
        assert torch.equal(acc.double(), ref)
    full = cols.double() @ wk.double().t()
    assert float((full != ref).float().mean()) > 0.9


def test_reference_sees_every_plane():
    """One K = 576 case (3 x 3, 64 channels): each way a kernel could lose or misplace a low-order plane changes more than 90 % of
    the reference's outputs, so equality with the reference excludes it."""
    g = _gen(4)
    s, p = 1, 1
    x, w = xe.grid_operands((2, 16, 8, 64), g), xe.grid_operands((64, 64, 3, 3), g)
    xs, ws = xe.split(x), xe.split(w)

    def conv(a, b):
        return xe.conv_fwd64(a, b, s, p)

    ref = xe.three_terms(conv, xs, ws)
    assert torch.equal(ref, xe.ref_fwd_x3(x, w, s, p))
    w_krsc_lo = ws[1].permute(0, 2, 3, 1)                           # the k axis as the kernel walks it: (tap, channel)
    shifted = torch.roll(w_krsc_lo.reshape(64, 576), 8, 1).view(64, 3, 3, 64).permute(0, 3, 1, 2)
    mutants = {
        "drop lo*hi": xe.three_terms(conv, xs, ws, ((0, 1), (0, 0))),
        "drop hi*lo": xe.three_terms(conv, xs, ws, ((1, 0), (0, 0))),
        "weight planes swapped": xe.three_terms(conv, xs, (ws[1], ws[0])),
        "weight lo plane one 8-element chunk along k": xe.three_terms(conv, xs, (ws[0], shifted)),
        "activation lo plane one 8-element chunk along k": xe.three_terms(conv, (xs[0], torch.roll(xs[1], 8, 3)), ws),
    }
    for name, got in mutants.items():
        changed = float((got != ref).float().mean())
        print(f"{name}: {100 * changed:.1f} % of the outputs change")
        assert changed > 0.90, (name, changed)


def _fwd_bn(case):
    B, H, W, cin, cout, k, s = case[:7]
    oh, ow = xe.out_hw(H, W, k, s, k // 2)
    return xe.x3_bn(B * oh * ow, cout)


def _dgrad_bn(case):
    B, H, W, cin = case[:4]
    return xe.x3_bn(B * H * W, cin)


def test_case_tables_reach_every_instantiation():
    """Through the mirrors of launch_igemm_x3's tile rule and plan_wgrad's fp32 tile choice: the GPU file's tables run
    igemm_x3_kernel<64> and <128> under statistics, under the affine epilogue and as the data gradient, and all four
    wgrad_x3_kernel<TM, TN>; and the cases meant to sit on either side of the <128> threshold do."""
    assert {_fwd_bn(c) for c in gpu_file.FWD_STATS_CASES} == {64, 128}
    assert {_fwd_bn(c) for c in gpu_file.FWD_AFFINE_CASES} == {64, 128}
    assert {_dgrad_bn(c) for c in gpu_file.DGRAD_CASES} == {64, 128}
    tiles = {xe.wgrad_tile(c[4], c[3] * c[5] * c[5]) for c in gpu_file.WGRAD_CASES}
    assert tiles == {(64, 64), (128, 64), (64, 128), (128, 128)}
    assert _fwd_bn((16, 64, 32, 64, 256, 1, 1)) == 128 and _fwd_bn((255, 16, 8, 64, 256, 1, 1)) == 64
    assert _fwd_bn((2, 181, 181, 64, 128, 3, 1)) == 128
    for c in ((16, 64, 32, 256, 64, 1, 1), (16, 64, 32, 256, 128, 3, 2), (3, 105, 104, 256, 512, 1, 2)):
        assert c in gpu_file.DGRAD_CASES and _dgrad_bn(c) == 128
    for c in ((16, 64, 32, 64, 256, 1, 1), (2, 181, 181, 64, 128, 3, 1)):
        assert c in gpu_file.FWD_STATS_CASES and c in gpu_file.FWD_AFFINE_CASES
    # the mirrors themselves at the rule's edges
    assert xe.x3_bn(128 * 512, 128) == 128 and xe.x3_bn(128 * 511, 128) == 64 and xe.x3_bn(128 * 510 + 1, 128) == 64
    assert xe.x3_bn(128 * 4096, 64) == 64 and xe.x3_bn(128 * 4096, 192) == 64
