"""Operands and references that pin the bf16x3 convolutions (csrc/conv_x3.hip, wgrad_x3_kernel) bit for bit WITH the low-order
planes busy.  Pure torch, no GPU needed to import; used by tests/test_bf16x3_exact_cpu.py and tests/test_bf16x3_exact_gpu.py.

The grid: an element is a + b 2^-11 with a in {-1, 0, 1}, b in {-3..3} and b = 0 where a = 0.  3 * 2^-11 is below half a bf16 ulp
in both binades next to +-1, so the kernels' split gives hi = bf16(x) = a and lo = bf16(x - hi) = b 2^-11, both exact, and
hi + lo == x.  Each of the three terms lo_a hi_w, hi_a lo_w, hi_a hi_w is a multiple of 2^-11; while the sum of their absolute
values stays below 2^24 * 2^-11 = 8192 every fp32 partial sum is exact in any order, so the three-term result is ONE number
whatever the tile, split or k order -- and it differs from the full product (which has lo_a lo_w too) almost everywhere, so the
reference is the three-term value in fp64, never conv(x, w)."""
import torch
import torch.nn.functional as F

LO_UNIT = 2.0 ** -11
MARGIN_SCALE = 2.0 ** 11 / 2.0 ** 24
# (plane of the first operand, plane of the second), 0 = hi, 1 = lo: the kernels' lo*hi + hi*lo + hi*hi
TERMS = ((1, 0), (0, 1), (0, 0))


def grid_operands(shape, gen, density=1.0):
    """fp32 tensor of grid elements on gen's device; density < 1 zeroes elements at random (for reductions too long to stay
    below the exactness limit with dense operands)."""
    dev = gen.device
    a = torch.randint(-1, 2, shape, generator=gen, device=dev)
    b = torch.randint(-3, 4, shape, generator=gen, device=dev) * (a != 0)
    x = a.float() + b.float() * LO_UNIT
    if density < 1.0:
        x = x * (torch.rand(shape, generator=gen, device=dev) < density)
    return x


def split(t):
    """(hi, lo) as fp32: torch's own bf16 rounding (tests/probes/bf16x3_emul.py)"""
    hi = t.to(torch.bfloat16).float()
    return hi, (t - hi).to(torch.bfloat16).float()


def out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


# ------------------------------------------------------------------------------------ fp64 convolutions, tap by tap (NHWC)
def _taps(k, s, oh, ow):
    for r in range(k):
        for c in range(k):
            yield r, c, (slice(r, r + s * (oh - 1) + 1, s), slice(c, c + s * (ow - 1) + 1, s))


def conv_fwd64(x, w, s, p):
    """conv2d(x NHWC, w OIHW) -> [B, oh, ow, cout] fp64"""
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    xp = F.pad(x.double(), (0, 0, p, p, p, p))
    oh, ow = (xp.shape[1] - k) // s + 1, (xp.shape[2] - k) // s + 1
    y = torch.zeros(x.shape[0] * oh * ow, cout, dtype=torch.float64, device=x.device)
    wd = w.double()
    for r, c, (sr, sc) in _taps(k, s, oh, ow):
        y += xp[:, sr, sc, :].reshape(-1, cin) @ wd[:, :, r, c].t()
    return y.view(x.shape[0], oh, ow, cout)


def conv_dgrad64(dy, w, s, p, H, W):
    """dx [B, H, W, cin] of the same convolution: the transposed scatter of every tap, fp64"""
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    n, oh, ow = dy.shape[0], dy.shape[1], dy.shape[2]
    dxp = torch.zeros(n, H + 2 * p, W + 2 * p, cin, dtype=torch.float64, device=dy.device)
    g = dy.double().reshape(-1, cout)
    wd = w.double()
    for r, c, (sr, sc) in _taps(k, s, oh, ow):
        dxp[:, sr, sc, :] += (g @ wd[:, :, r, c]).view(n, oh, ow, cin)
    return dxp[:, p:p + H, p:p + W, :]


def conv_wgrad64(dy, x, k, s, p):
    """dw OIHW fp64 (first operand dy, as in wgrad_x3_kernel's A tile)"""
    cin, oh, ow, cout = x.shape[3], dy.shape[1], dy.shape[2], dy.shape[3]
    dw = torch.zeros(cout, cin, k, k, dtype=torch.float64, device=x.device)
    xp = F.pad(x.double(), (0, 0, p, p, p, p))
    g = dy.double().reshape(-1, cout).t()
    for r, c, (sr, sc) in _taps(k, s, oh, ow):
        dw[:, :, r, c] = g @ xp[:, sr, sc, :].reshape(-1, cin)
    return dw


# ------------------------------------------------------------------------------------ the three-term references
def three_terms(conv, a_planes, b_planes, terms=TERMS):
    """sum over `terms` of conv(a_planes[i], b_planes[j]); planes are (hi, lo)"""
    out = None
    for i, j in terms:
        t = conv(a_planes[i], b_planes[j])
        out = t if out is None else out + t
    return out


def _planes(t, absolute):
    hi, lo = split(t)
    return (hi.abs(), lo.abs()) if absolute else (hi, lo)


def ref_fwd_x3(x, w, s, p, absolute=False):
    """x NHWC fp32, w OIHW fp32 -> [B, oh, ow, cout] fp64: lo_x hi_w + hi_x lo_w + hi_x hi_w"""
    return three_terms(lambda a, b: conv_fwd64(a, b, s, p), _planes(x, absolute), _planes(w, absolute))


def ref_dgrad_x3(dy, w, s, p, H, W, absolute=False):
    """dy NHWC fp32, w OIHW fp32 -> dx [B, H, W, cin] fp64"""
    return three_terms(lambda a, b: conv_dgrad64(a, b, s, p, H, W), _planes(dy, absolute), _planes(w, absolute))


def ref_wgrad_x3(x, dy, k, s, p, absolute=False):
    """x, dy NHWC fp32, both split -> dw OIHW fp64"""
    return three_terms(lambda a, b: conv_wgrad64(a, b, k, s, p), _planes(dy, absolute), _planes(x, absolute))


def exactness_margin(ref, *args):
    """ref (one of the three references above) on absolute values, as a fraction of the limit below which every fp32 partial sum
    of multiples of 2^-11 is exact: < 1 for every output is the condition on the INPUTS under which kernel and reference can be
    compared bit for bit.  A case that fails it is thinned with grid_operands' density, never compared more loosely."""
    return ref(*args, absolute=True) * MARGIN_SCALE


def is_fp32(t):
    """every fp64 value representable in fp32"""
    return bool((t.float().double() == t).all())


def mismatch(got, ref):
    """None where got == ref as values (+0 == -0) over the whole tensor, else the count and the first mismatch as
    (row, column, got, expected) of the [rows, last dim] view"""
    bad = got.double() != ref.double()
    n = int(bad.sum())
    if n == 0:
        return None
    i = int(bad.reshape(-1).nonzero()[0])
    r, c = divmod(i, ref.shape[-1])
    return f"{n} of {ref.numel()} mismatch, first at (row, col, got, expected) " \
           f"({r}, {c}, {float(got.reshape(-1)[i])!r}, {float(ref.reshape(-1)[i])!r})"


# ------------------------------------------------------------------------------------ mirrors of the launch rules
def x3_bn(M, N):
    """launch_igemm_x3's N tile (conv_x3.hip): which igemm_x3_kernel<BN> a launch of M rows x N columns runs.  Forward: M = B oh ow,
    N = cout; data gradient: M = B H W, N = cin."""
    return 128 if N % 128 == 0 and -(-M // 128) * (N // 128) >= 512 else 64


def wgrad_tile(cout, K):
    """plan_wgrad's fp32 tile (conv_wgrad.hip): which wgrad_x3_kernel<TM, TN> a layer runs"""
    return 128 if cout % 128 == 0 else 64, 128 if K % 128 == 0 else 64
