"""CPU: (1) the stem's layout contract -- tests/stem_exact.py's fp64 model of the packed GEMM the kernels implement (xpad
[B, H + 8, W + 6, 4], w_stem [64][8][32] with k = r * 32 + s * 4 + c) equals F.conv2d(stride = 2, padding = 3) and the helper's
reference (conv_exact.ref_fwd) EXACTLY over the shapes of tests/test_stem_exact_gpu.py and reads nothing outside the padded
image, so the reference and the documented contract agree before any kernel is judged; (2) what the stem entry points refuse
before any launch (the library loads without a GPU): odd H or W, null pointers, and the size limit of stem_check_shape
(csrc/conv_common.hpp; include/creid.h)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import conv_exact as ce
import stem_exact as se

FUSED_B = [(1, 8, 128), (2, 16, 128), (3, 24, 128), (1, 8, 320), (2, 16, 320)]


def _ints(gen, shape, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int8)


@pytest.mark.parametrize("B,H,W", se.GROUP_A + FUSED_B, ids=lambda v: str(v))
def test_packed_gemm_model_is_the_convolution(B, H, W):
    gen = torch.Generator().manual_seed(B * 100003 + H * 1009 + W)
    x8, w8 = _ints(gen, (B, 3, H, W)), _ints(gen, (64, 3, 7, 7))
    xpad, w_stem = se.ref_xpad(x8), se.ref_w_stem(w8)
    assert tuple(xpad.shape) == (B, H + 8, W + 6, 4) and tuple(w_stem.shape) == (64, 8, 32)
    # the padding is zeros, the 4th channel is zero, the image sits at (3, 3)
    assert torch.equal(xpad[:, 3:3 + H, 3:3 + W, :3], x8.double().permute(0, 2, 3, 1))
    assert float(xpad.abs().sum()) == float(x8.double().abs().sum())
    w4 = w_stem.view(64, 8, 8, 4)
    assert not w4[:, 7].any() and not w4[:, :, 7].any() and not w4[:, :, :, 3].any()
    y, max_row, max_col = se.packed_gemm(xpad, w_stem, B, H, W)
    # the last output pixel's last tap: row 2 (H/2 - 1) + 7 = H + 5 of H + 8, column W + 5 of W + 6 (the last one)
    assert (max_row, max_col) == (H + 5, W + 5) and max_row < H + 8 and max_col < W + 6
    want = F.conv2d(x8.double(), w8.double(), stride=2, padding=3).permute(0, 2, 3, 1)
    assert torch.equal(y, want)
    assert torch.equal(ce.ref_fwd(x8.permute(0, 2, 3, 1).contiguous(), w8, 2, se.PAD, 0, B), want)
    assert float(want.abs().max()) <= 4 * 147


def test_reference_weight_gradient_is_the_stems():
    """conv_exact.ref_wgrad(k = 7, s = 2, p = 3) is autograd's gradient of F.conv2d(stride = 2, padding = 3) in fp64, exactly
    (integer operands), and equals the packed GEMM's A^T dy read back through the k = r * 32 + s * 4 + c packing"""
    B, H, W = 3, 14, 10
    gen = torch.Generator().manual_seed(7)
    x8, dy8 = _ints(gen, (B, 3, H, W)), _ints(gen, (B, H // 2, W // 2, 64))
    w = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
    (F.conv2d(x8.double(), w, stride=2, padding=3) * dy8.double().permute(0, 3, 1, 2)).sum().backward()
    ref = ce.ref_wgrad(x8.permute(0, 2, 3, 1).contiguous(), dy8, 7, 2, se.PAD)
    assert torch.equal(ref, w.grad) and float(ref.abs().max()) <= 4 * B * (H // 2) * (W // 2)
    # d(packed_gemm)/d(w_stem): linear in w_stem, so one-hot rows of the identity give the A matrix
    xpad = se.ref_xpad(x8)
    eye = torch.eye(256, dtype=torch.float64)
    a = torch.cat([se.packed_gemm(xpad, eye[k0:k0 + 64].reshape(64, 8, 32), B, H, W)[0].reshape(-1, 64) for k0 in range(0, 256, 64)], 1)
    dws = (dy8.double().reshape(-1, 64).t() @ a).view(64, 8, 8, 4)                   # [o][r][s][c]
    assert torch.equal(dws[:, :7, :7, :3].permute(0, 3, 1, 2), ref)


# ------------------------------------------------------------------------------------ refusals before any launch
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from centroids_reid_amd import _lib as L
    return L.lib()


class _Host:
    """small host buffers for the non-null pointers: a refused call returns before it reads or launches anything"""
    def __init__(self):
        self.bufs = [(C.c_float * 64)() for _ in range(7)]
        self.xpad, self.w, self.y, self.ss, self.dy, self.dw, self.ws = [C.cast(b, C.c_void_p) for b in self.bufs]


USES = {"fwd": ("xpad", "w", "y"), "affine": ("xpad", "w", "y", "ss"), "pool": ("xpad", "w", "y", "ss"),
        "wgrad": ("xpad", "dy", "dw", "ws")}


def _stem_calls(lib, B, H, W, dt, h, null=None):
    """return codes of the three forwards and the weight gradient; `null`: name of the pointer passed as NULL -- then only the
    calls that take that pointer are made (the others would launch, and there is no GPU here)"""
    p = {n: (None if n == null else getattr(h, n)) for n in ("xpad", "w", "y", "ss", "dy", "dw", "ws")}
    calls = {
        "fwd": lambda: lib.creid_stem_conv_fwd(B, H, W, p["xpad"], p["w"], p["y"], None, dt, None),
        "affine": lambda: lib.creid_stem_conv_fwd_affine(B, H, W, p["xpad"], p["w"], p["y"], p["ss"], 1, dt, None),
        "pool": lambda: lib.creid_stem_conv_pool_fwd_affine(B, H, W, p["xpad"], p["w"], p["y"], p["ss"], 1, dt, None),
        "wgrad": lambda: lib.creid_stem_conv_wgrad(B, H, W, p["xpad"], p["dy"], p["dw"], 0, p["ws"], 256, dt, None),
    }
    return {k: fn() for k, fn in calls.items() if null is None or null in USES[k]}


@pytest.mark.parametrize("dt", [0, 1, 2], ids=["fp32", "bf16", "f16"])
@pytest.mark.parametrize("H,W", [(7, 8), (8, 7), (1, 1), (129, 128), (128, 319)])
def test_odd_extents_are_refused(lib, H, W, dt):
    rcs = _stem_calls(lib, 2, H, W, dt, _Host())
    if dt == 0:
        assert rcs.pop("pool") == se.E_DTYPE                 # (the one-launch stem is 16-bit only, whatever the shape)
    assert set(rcs.values()) == {se.E_SHAPE}, rcs
    assert lib.creid_stem_conv_wgrad_workspace_bytes(2, H, W, dt) == 0


@pytest.mark.parametrize("null", ["xpad", "w", "y", "ss", "dy", "dw", "ws"])
def test_null_pointers_are_refused(lib, null):
    # (8 x 128: a shape all four calls accept, so the refusal is the pointer's)
    rcs = _stem_calls(lib, 1, 8, 128, 1, _Host(), null=null)
    assert rcs and set(rcs.values()) == {se.E_ARG}, rcs


@pytest.mark.parametrize("B,H,W", [(0, 8, 128), (-1, 8, 128), (1, 0, 128), (1, 8, -2)])
def test_non_positive_extents_are_refused(lib, B, H, W):
    assert set(_stem_calls(lib, B, H, W, 1, _Host()).values()) == {se.E_ARG}
    assert lib.creid_stem_conv_wgrad_workspace_bytes(B, H, W, 1) == 0


# B * (H/2) * (W/2) >= 2^24: the first sizes past the limit, in each factor; sizes whose products would wrap 32 or 64 bits
TOO_LARGE = [(1 << 24, 2, 2), (1 << 12, 128, 128), (1, 1 << 13, 1 << 13), (4, 8, 1 << 23), (1 << 18, 16, 16), (1 << 32, 2, 2),
             (1 << 40, 1 << 40, 1 << 40), (1, 2, 1 << 62), (3, 1 << 33, 1 << 33), ((1 << 63) - 1, 2, 2)]


@pytest.mark.parametrize("dt", [0, 1, 2], ids=["fp32", "bf16", "f16"])
@pytest.mark.parametrize("B,H,W", TOO_LARGE, ids=lambda v: hex(v))
def test_sizes_past_the_row_limit_are_refused(lib, B, H, W, dt):
    """fast_divmod decomposes a GEMM row with fp32 reciprocals, exact below 2^24 only, and stem_geom narrows the row count to
    int: the stem calls refuse what check_desc refuses for every other convolution, before any launch"""
    assert B * (H // 2) * (W // 2) >= 1 << 24
    rcs = _stem_calls(lib, B, H, W, dt, _Host())
    if dt == 0:
        assert rcs.pop("pool") == se.E_DTYPE
    assert set(rcs.values()) == {se.E_SHAPE}, rcs
    assert lib.creid_stem_conv_wgrad_workspace_bytes(B, H, W, dt) == 0


def test_the_largest_row_count_is_planned():
    """just inside the limit the workspace query answers (a host-side plan, nothing launched), and the padded image's pixel
    count -- which the kernels index in int -- stays below 2^31 for EVERY accepted shape: at most 80 x the row count (H = W = 2), and
    80 * 2^24 < 2^31"""
    import __graft_entry__ as ge
    ge.build()
    from centroids_reid_amd import _lib as L
    for B, H, W in [((1 << 24) - 1, 2, 2), ((1 << 12) - 1, 128, 128), (1, 2, (1 << 25) - 2)]:
        assert B * (H // 2) * (W // 2) < 1 << 24 and B * (H + 8) * (W + 6) < 1 << 31
        for dt in (0, 1, 2):
            nb = L.lib().creid_stem_conv_wgrad_workspace_bytes(B, H, W, dt)
            assert nb >= 64 * 256 * 4 and nb % (64 * 256 * 4) == 0
    assert max((h + 8) * (w + 6) / ((h // 2) * (w // 2)) for h in range(2, 64, 2) for w in range(2, 64, 2)) == 80.0
