"""float64 reference, error bounds and input generators for the kernels of csrc/elementwise.hip: BatchNorm statistics, finalize,
apply (+ residual, + dual residual, + ReLU and its mask bits), backward; max-pool 3x3 s2 p1 with its argmax taps; global average
pool; NHWC -> NCHW; IBN.  Plain torch / numpy float64 on the CPU; nothing of the package is imported, nothing outside tests/ read.

Comparison in two layers (tests/test_ew_edges_gpu.py):
  1. what the device derives from column sums -- mean, invstd, (scale, shift), running statistics, the backward's (A, B, Cc),
     dgamma, dbeta -- against the float64 value, within a bound that follows from the summation the kernels perform;
  2. every element-wise result against the float64 evaluation WITH THE DEVICE'S OWN PUBLISHED COEFFICIENTS, within the two or
     three fp32 roundings of the apply expression plus half an ulp of the storage type.  The slack layer 1 is entitled to can
     then not hide an error of the apply kernels (a thread on another channel's coefficients is off by O(1), not by 1e-6).
Every bound is a function of the data and of the operation count; gam(k, u) = k u / (1 - k u) is the usual bound on the relative
error of k successive roundings of unit roundoff u (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1).

NaN and infinite inputs are out of scope everywhere in this file."""
import math

import numpy as np
import torch

F64 = torch.float64
KINDS = ("bf16", "f16", "fp32")
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "fp32": torch.float32}
UNIT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "fp32": 2.0 ** -24}          # unit roundoff = half an ulp of 1.0 = 2^-(significand bits)
U32 = UNIT["fp32"]
_PREC = {"bf16": 8, "f16": 11, "fp32": 24}                                 # significand bits, hidden one included
_EMIN = {"bf16": -125, "f16": -13, "fp32": -125}                           # frexp exponent of the smallest normal number
TINY = {k: 2.0 ** (_EMIN[k] - _PREC[k] - 1) for k in KINDS}                # half the spacing of the subnormals
VEC = {"bf16": 8, "f16": 8, "fp32": 4}                                     # elements per 16-byte chunk
ROWS = 128                                                                 # rows per statistics block


def t64(a):
    return a.to(F64) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a), dtype=F64)


def round_to(x, kind):
    """float64 -> the nearest value of the storage type (ties to even, gradual underflow), returned as float64.  One rounding:
    a float64 -> fp32 -> bf16 cast would round twice."""
    x = t64(x)
    _, e = torch.frexp(x)
    q = torch.ldexp(torch.ones_like(x), torch.clamp(e, min=_EMIN[kind]) - _PREC[kind])
    return torch.round(x / q) * q                  # x / q is exact (a power of two); torch.round is half-to-even


def to_storage(x, kind):
    """float64 values that are representable in the storage type -> a tensor of that type (exact)."""
    return t64(x).to(TORCH_DT[kind])


def gam(k, u=U32):
    return k * u / (1.0 - k * u)


# ------------------------------------------------------------------------------------------------ column sums
def lanes(C, kind):
    """(cw, nrl) of the column-pass kernels: cw 16-byte chunk lanes x nrl row lanes of a 256-thread workgroup."""
    cpr = C // VEC[kind]
    cw = min(cpr, 32)
    return cw, 256 // cw


def gamma_cols(C, kind, rows_in_block=ROWS):
    """Relative error of one block's column sum, |dS| <= gamma * sum |terms|.  Within a block of R <= 128 rows a row lane adds
    its ceil(R / nrl) terms one after the other in fp32 (one rounding per term: the add, or the fma of the squares), then the
    lane partials are added one after the other: min(nrl, R) of them are not exact zeros (adding 0.0f rounds nothing).  One more
    rounding covers the conversion of the float64 total.  The blocks are added in float64 (2^-53 per add: nothing next to this)."""
    _, nrl = lanes(C, kind)
    R = min(rows_in_block, ROWS)
    return gam(math.ceil(R / nrl) + min(nrl, R) + 1)


def stat_bounds(sum_abs, sum_sq, mean, var, count, eps, g):
    """Bounds on the device's mean / biased variance / invstd given |dS1| <= g sum|x| and |dS2| <= g sum x^2 (g = gamma_cols):
       mean_d = S1 / n in float64               -> |d mean_d| <= g sum|x| / n                  (dm; the fp32 copy adds U32 |mean|)
       var = S2 / n - mean_d^2 in float64       -> |d var| <= g sum x^2 / n + 2 |mean| dm + dm^2
    sum x^2 / n = mean^2 + var: the variance bound grows with (mean / std)^2 -- the contract of a one-pass E[x^2] - mean^2.
       invstd = (var + eps)^(-1/2), fp32        -> relative (1 - rho)^(-1/2) - 1 with rho = d var / (var + eps), plus U32;
    rho >= 1 leaves invstd unbounded (inf).  Clamping a negative variance to 0 only moves it towards the true one."""
    dm = g * sum_abs / count
    dvar = g * sum_sq / count + 2 * mean.abs() * dm + dm * dm
    rho = dvar / (var + eps)
    inv = 1.0 / torch.sqrt(var + eps)
    rel = torch.where(rho < 1, 1.0 / torch.sqrt(torch.clamp(1 - rho, min=1e-300)) - 1, torch.full_like(rho, float("inf")))
    return dict(mean=dm + U32 * mean.abs(), var=dvar, invstd=inv * (rel + U32 * (1 + rel)), mean_d=dm)


# ------------------------------------------------------------------------------------------------ BatchNorm forward
def bn_stats(x):
    """Two-pass mean and biased variance over the rows of x [M, C] (float64)."""
    x = t64(x)
    mean = x.mean(0)
    return mean, ((x - mean) ** 2).mean(0)


def unbiased(var, count):
    """The running statistic takes var * n / (n - 1); one sample has no unbiased estimate and stays as it is."""
    return var * count / (count - 1) if count > 1 else var.clone()


def invstd_of(var, eps):
    return 1.0 / torch.sqrt(var + eps)


def scale_shift(mean, invstd, gamma, beta):
    sc = invstd * gamma
    return sc, beta - mean * sc


def running_update(run, new, momentum):
    return (1.0 - momentum) * run + momentum * new


def bn_forward_ref(x, gamma, beta, rmean, rvar, momentum, eps):
    """Everything the training finalize publishes, in float64, plus the sums the bounds need."""
    x = t64(x)
    M = x.shape[0]
    mean, var = bn_stats(x)
    inv = invstd_of(var, eps)
    sc, sh = scale_shift(mean, inv, t64(gamma), t64(beta))
    return dict(mean=mean, var=var, invstd=inv, sc=sc, sh=sh, rmean=running_update(t64(rmean), mean, momentum),
                rvar=running_update(t64(rvar), unbiased(var, M), momentum), sum_abs=x.abs().sum(0), sum_sq=(x * x).sum(0), count=M)


def bn_forward_bounds(ref, gamma, beta, rmean, rvar, momentum, eps, g):
    """Bounds on mean, invstd, scale, shift and the running statistics of the device.
       sc = invstd * gamma (one fp32 rounding)                         d sc <= |gamma| d invstd (1 + U32) + U32 |sc|
       sh = beta - mean * sc (two roundings)                           d sh <= |sc| d mean + |mean| d sc + gam(2) (|beta| + |mean sc|)
       run' = (1 - m) * run + m * new: the fp32 (1 - m), two products and the add -> gam(4) on the magnitudes, plus m * d new;
       for the variance d new = d var * n / (n - 1), and the fp32 copy of it (U32)."""
    n = ref["count"]
    b = stat_bounds(ref["sum_abs"], ref["sum_sq"], ref["mean"], ref["var"], n, eps, g)
    gamma, beta = t64(gamma), t64(beta)
    dsc = gamma.abs() * b["invstd"] * (1 + U32) + U32 * ref["sc"].abs()
    dsh = ref["sc"].abs() * b["mean"] + ref["mean"].abs() * dsc + gam(2) * (beta.abs() + (ref["mean"] * ref["sc"]).abs())
    unb = unbiased(ref["var"], n)
    dunb = (b["var"] * n / (n - 1) if n > 1 else b["var"]) + U32 * unb.abs()
    drm = momentum * b["mean"] + gam(4) * (((1 - momentum) * t64(rmean)).abs() + (momentum * ref["mean"]).abs())
    drv = momentum * dunb + gam(4) * (((1 - momentum) * t64(rvar)).abs() + (momentum * unb).abs())
    return dict(mean=b["mean"], invstd=b["invstd"], sc=dsc, sh=dsh, rmean=drm, rvar=drv, var=b["var"])


def bn_apply(x, sc, sh, res=None, res_sc=None, res_sh=None, relu=True):
    """z = x * sc + sh (+ res, or + res * res_sc + res_sh: the dual form), y = max(z, 0) if relu.  Returns (y, z, mag) with
    mag = |x sc| + |sh| + |res term| (+ |res_sh|): what the fp32 roundings of the device's expression scale with."""
    x = t64(x)
    z = x * sc + sh
    mag = (x * sc).abs() + sh.abs()
    if res is not None:
        r = t64(res)
        if res_sc is not None:
            mag = mag + (r * res_sc).abs() + res_sh.abs()
            r = r * res_sc + res_sh
        else:
            mag = mag + r.abs()
        z = z + r
    return (torch.clamp(z, min=0) if relu else z), z, mag


def apply_bound(y, mag, kind, n_round):
    """|y_device - y| for an fp32 expression of n_round roundings on operands of total magnitude mag, stored in `kind`: the
    fp32 error gam(n_round) * mag, plus half an ulp of the stored value (none for fp32 storage: the expression's last rounding
    is the stored one), plus half a subnormal spacing where the storage type underflows gradually."""
    e32 = gam(n_round) * mag
    if kind == "fp32":
        return e32 + TINY[kind]
    return e32 + UNIT[kind] * (y.abs() + e32) + TINY[kind]


def relu_bits(y):
    """bit k of byte i = (y.flat[8 i + k] > 0)."""
    return np.packbits((np.asarray(y).reshape(-1) > 0), bitorder="little")


def bits_to_mask(bits, shape):
    return torch.from_numpy(np.unpackbits(np.asarray(bits, np.uint8), bitorder="little")[: int(np.prod(shape))].reshape(shape).astype(bool))


# ------------------------------------------------------------------------------------------------ BatchNorm backward
def bn_backward_sums(x, g, mask, mean, invstd):
    """dy = g * mask (mask None: no ReLU); S1 = sum dy, S2 = sum dy * xhat with xhat = (x - mean) * invstd, and the sums of
    magnitudes the bounds need."""
    x, dy = t64(x), t64(g)
    if mask is not None:
        dy = dy * mask.to(F64)
    t = dy * ((x - mean) * invstd)
    return dict(dy=dy, s1=dy.sum(0), s2=t.sum(0), a1=dy.abs().sum(0), a2=t.abs().sum(0), count=x.shape[0])


def bn_backward_coef(s1, s2, mean, invstd, gamma, count):
    """dx = k1 (dy - S1 / n - xhat S2 / n) = A dy + B x + Cc with k1 = gamma * invstd."""
    k1 = gamma * invstd
    return k1, -k1 * invstd * s2 / count, -k1 * s1 / count + k1 * invstd * (s2 / count) * mean


def bn_backward_bounds(s, mean, invstd, gamma, g):
    """Bounds on the device's column sums and coefficient rows, mean / invstd being the device's own fp32 values.
       S1: |d| <= g a1.  S2: each term carries the two fp32 roundings of xhat before the fma -> (g + gam(2) (1 + g)) a2.
       dbeta = acc + (float) S1, dgamma = acc + (float) S2: the conversion and the add, U32 each on the result's magnitude.
       A = gamma * invstd: one rounding.
       a_i = (float) S_i * (float)(1 / n): three roundings;  B = -(k1 * invstd) * a2: k1, two products, a2 -> gam(6) |B|
       Cc = -k1 * a1 + ((k1 * invstd) * a2) * mean: gam(6) on the first term (k1, a1, product, the add), gam(8) on the second,
       plus the propagated dS1, dS2."""
    n = s["count"]
    gamma = t64(gamma)
    d1 = g * s["a1"]
    d2 = (g + gam(2) * (1 + g)) * s["a2"]
    A, B, Cc = bn_backward_coef(s["s1"], s["s2"], mean, invstd, gamma, n)
    k1 = (gamma * invstd).abs()
    t1, t2 = (k1 * s["s1"] / n).abs(), (k1 * invstd * s["s2"] / n * mean).abs()
    return dict(s1=d1, s2=d2, A=U32 * A.abs(), B=k1 * invstd.abs() / n * d2 + gam(6) * B.abs(),
                Cc=k1 / n * d1 + k1 * (invstd * mean).abs() / n * d2 + gam(6) * t1 + gam(8) * t2)


def acc_bound(dS, S, out):
    """acc + (float) S in fp32."""
    return dS + U32 * S.abs() + U32 * out.abs()


def bn_dx(x, dy, A, B, Cc):
    """dx and the magnitude of the device's two fma: fmaf(A, dy, fmaf(B, x, Cc))."""
    x, dy = t64(x), t64(dy)
    return A * dy + B * x + Cc, (A * dy).abs() + (B * x).abs() + Cc.abs()


# ------------------------------------------------------------------------------------------------ max-pool 3x3 s2 p1, NHWC
def maxpool_fwd(x):
    """x [B, H, W, C] (even H, W) -> (values [B, H/2, W/2, C], tap codes r * 3 + s uint8): the FIRST maximum in scan order (r
    outer, s inner) over the in-bounds taps only -- padding never wins, not even over an all-negative window."""
    x = t64(x)
    B, H, W, C = x.shape
    OH, OW = H // 2, W // 2
    xp = torch.full((B, H + 2, W + 2, C), float("-inf"), dtype=F64)
    xp[:, 1:H + 1, 1:W + 1] = x
    best = torch.full((B, OH, OW, C), float("-inf"), dtype=F64)
    tap = torch.zeros((B, OH, OW, C), dtype=torch.uint8)
    for r in range(3):
        for s in range(3):
            v = xp[:, r:r + 2 * OH:2, s:s + 2 * OW:2]
            win = v > best
            best = torch.where(win, v, best)
            tap = torch.where(win, torch.full_like(tap, r * 3 + s), tap)
    return best, tap


def maxpool_bwd(dy, tap, H, W, kind):
    """Scatter of dy by tap code; dy on the grid k / 16 makes every sum exact, the result is its one rounding to storage."""
    dy = t64(dy)
    B, OH, OW, C = dy.shape
    dxp = torch.zeros((B, H + 2, W + 2, C), dtype=F64)
    for r in range(3):
        for s in range(3):
            dxp[:, r:r + 2 * OH:2, s:s + 2 * OW:2] += dy * (tap == r * 3 + s).to(F64)
    assert float(dxp[:, 0].abs().sum() + dxp[:, :, 0].abs().sum()) == 0.0, "a tap code points into the padding"
    return round_to(dxp[:, 1:H + 1, 1:W + 1], kind)


def pool_grad(shape, seed):
    """Gradients on the grid k / 16, |k| <= 128: representable in bf16, every sum of up to four exact in fp32."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(-128, 129, size=shape).astype(np.float64) / 16.0)


# ------------------------------------------------------------------------------------------------ pooling and layout
def gap_fwd(x):
    """x [B, HW, C] -> (mean over HW, sum |x| / HW)."""
    x = t64(x)
    return x.mean(1), x.abs().mean(1)


def gap_fwd_bound(mean_abs, HW):
    """Eight row lanes add ceil(HW / 8) terms each, eight partials are added, one division: (ceil(HW / 8) + 8) roundings at
    most, each relative to a partial sum of magnitudes <= sum |x|."""
    return (math.ceil(HW / 8) + 8) * U32 * mean_abs


def gap_bwd(dfeat, HW, kind):
    """dx[b, p, c] = store(dfeat[b, c] * (1.0f / HW)): ONE fp32 product with the fp32 reciprocal, emulated exactly."""
    inv = np.float32(1.0) / np.float32(HW)
    prod = (np.asarray(dfeat, np.float32) * inv).astype(np.float32)
    v = round_to(torch.from_numpy(prod.astype(np.float64)), kind)
    return v[:, None, :].expand(-1, HW, -1).contiguous()


def nhwc_to_nchw(x):
    """[B, HW, C] -> [B, C, HW] fp32."""
    return t64(x).permute(0, 2, 1).contiguous().float()


# ------------------------------------------------------------------------------------------------ IBN
def ibn_forward_ref(x, c_in, in_w, in_b, bn_w, bn_b, rmean, rvar, momentum, eps, training=True):
    """x [B, HW, C]: channels < c_in use per-image statistics (always), the rest batch statistics (training) or the running ones
    (eval).  Every output per (image, channel): mean / var / invstd / sc / sh [B, C]; running statistics of the BatchNorm half."""
    x = t64(x)
    B, HW, C = x.shape
    mean_i, var_i = x.mean(1), ((x - x.mean(1, keepdim=True)) ** 2).mean(1)
    xb = x.reshape(B * HW, C)
    mean_b, var_b = bn_stats(xb)
    rm, rv = t64(rmean), t64(rvar)
    if not training:
        mean_bn, var_bn = rm, rv
    else:
        mean_bn, var_bn = mean_b[c_in:], var_b[c_in:]
    mean = torch.cat([mean_i[:, :c_in], mean_bn.expand(B, -1)], 1)
    var = torch.cat([var_i[:, :c_in], var_bn.expand(B, -1)], 1)
    w, b = torch.cat([t64(in_w), t64(bn_w)]), torch.cat([t64(in_b), t64(bn_b)])
    inv = invstd_of(var, eps)
    sc, sh = scale_shift(mean, inv, w, b)
    sa_i, sq_i = x.abs().sum(1), (x * x).sum(1)
    sum_abs = torch.cat([sa_i[:, :c_in], xb.abs().sum(0)[c_in:].expand(B, -1)], 1)
    sum_sq = torch.cat([sq_i[:, :c_in], (xb * xb).sum(0)[c_in:].expand(B, -1)], 1)
    count = torch.cat([torch.full((c_in,), float(HW), dtype=F64), torch.full((C - c_in,), float(B * HW), dtype=F64)])
    out = dict(mean=mean, var=var, invstd=inv, sc=sc, sh=sh, sum_abs=sum_abs, sum_sq=sum_sq, count=count, w=w, b=b)
    if training:
        nb = B * HW
        out["rmean"] = running_update(rm, mean_b[c_in:], momentum)
        out["rvar"] = running_update(rv, unbiased(var_b[c_in:], nb), momentum)
    return out


def ibn_forward_bounds(ref, c_in, rmean, rvar, momentum, eps, g, training=True):
    """As bn_forward_bounds, per (image, channel).  Eval mode reads the BatchNorm half from the running statistics: the mean is
    exact and invstd = 1.0f / sqrtf(rv + eps) is three fp32 operations: the add (U32, halved by the root), sqrtf and the division
    within one ulp (2 U32) each -> gam(5)."""
    b = stat_bounds(ref["sum_abs"], ref["sum_sq"], ref["mean"], ref["var"], ref["count"], eps, g)
    dmean, dinv = b["mean"].clone(), b["invstd"].clone()
    if not training:
        dmean[:, c_in:] = 0.0
        dinv[:, c_in:] = gam(5) * ref["invstd"][:, c_in:]
    dsc = ref["w"].abs() * dinv * (1 + U32) + U32 * ref["sc"].abs()
    dsh = ref["sc"].abs() * dmean + ref["mean"].abs() * dsc + gam(2) * (ref["b"].abs() + (ref["mean"] * ref["sc"]).abs())
    out = dict(mean=dmean, invstd=dinv, sc=dsc, sh=dsh)
    if training:
        n = float(ref["count"][-1])
        mean_b, var_b = ref["mean"][0, c_in:], ref["var"][0, c_in:]
        unb = unbiased(var_b, n)
        dunb = (b["var"][0, c_in:] * n / (n - 1) if n > 1 else b["var"][0, c_in:]) + U32 * unb.abs()
        out["rmean"] = momentum * dmean[0, c_in:] + gam(4) * (((1 - momentum) * t64(rmean)).abs() + (momentum * mean_b).abs())
        out["rvar"] = momentum * dunb + gam(4) * (((1 - momentum) * t64(rvar)).abs() + (momentum * unb).abs())
    return out


def ibn_backward_ref(x, g, mask, mean, invstd, c_in, w):
    """Backward given the mask and the (device's) per-(image, channel) mean / invstd [B, C]: per-image sums on the InstanceNorm
    channels, batch sums on the rest; returns coefficient rows [B, C] and the four parameter gradients with their magnitudes."""
    x, dy = t64(x), t64(g)
    B, HW, C = x.shape
    if mask is not None:
        dy = dy * mask.to(F64)
    t = dy * ((x - mean[:, None, :]) * invstd[:, None, :])
    s1_i, s2_i, a1_i, a2_i = dy.sum(1), t.sum(1), dy.abs().sum(1), t.abs().sum(1)

    def mix(per_img):                    # [B, C]: per image below c_in, the batch total above
        return torch.cat([per_img[:, :c_in], per_img[:, c_in:].sum(0).expand(B, -1)], 1)
    s1, s2, a1, a2 = mix(s1_i), mix(s2_i), mix(a1_i), mix(a2_i)
    count = torch.cat([torch.full((c_in,), float(HW), dtype=F64), torch.full((C - c_in,), float(B * HW), dtype=F64)])
    A, Bc, Cc = bn_backward_coef(s1, s2, mean, invstd, w, count)
    return dict(dy=dy, s1=s1, s2=s2, a1=a1, a2=a2, count=count, A=A, B=Bc, Cc=Cc,
                d_in_w=s2_i[:, :c_in].sum(0), d_in_b=s1_i[:, :c_in].sum(0), d_bn_w=s2[0, c_in:], d_bn_b=s1[0, c_in:],
                abs_in_w=s2_i[:, :c_in].abs().sum(0), abs_in_b=s1_i[:, :c_in].abs().sum(0))


def ibn_in_grad_bound(dS_img, abs_img_sum, out, B):
    """d(in_w, in_b) += sum over images of (float) per-image sums: 64 image lanes of ceil(B / 64) fp32 adds, min(64, B) lane
    partials, the conversion and the accumulating add -> gam(ceil(B / 64) + min(64, B) + 2) on sum |per-image sum|, plus the
    per-image sums' own errors."""
    return dS_img + gam(math.ceil(B / 64) + min(64, B) + 2) * abs_img_sum + U32 * out.abs()


# ------------------------------------------------------------------------------------------------ the comparator
class Ratios:
    """err / bound, the largest per family; check() is the one assertion every comparison of the sweep goes through."""

    def __init__(self):
        self.worst = {}
        self.cases = {}

    def check(self, family, what, got, ref, bound):
        got, ref, bound = t64(got), t64(ref), t64(bound)
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        bound = bound.expand_as(ref)
        assert math.isfinite(float(bound.max())) and not bool(torch.isnan(bound.sum())), \
            f"{what}: the bound is not finite (ill-conditioned case: choose another input)"
        err = (got - ref).abs_()
        assert math.isfinite(float(err.sum())), f"{what}: non-finite values"
        ratio = err / bound
        ratio[err == 0] = 0.0                         # (0 / 0 where a bound is exactly zero and met)
        worst = float(ratio.max()) if ratio.numel() else 0.0
        self.worst[family] = max(self.worst.get(family, 0.0), worst)
        if not worst <= 1.0:
            i = int(torch.argmax(ratio.reshape(-1)))
            n_bad = int((ratio > 1).sum())
            raise AssertionError(f"{what}: {n_bad} of {ratio.numel()} outside the bound; worst at flat index {i}: got "
                                 f"{float(got.reshape(-1)[i])!r}, reference {float(ref.reshape(-1)[i])!r}, bound "
                                 f"{float(bound.reshape(-1)[i]):.3e}, ratio {worst:.3g}")
        return worst

    def exact(self, family, what, got, ref):
        got, ref = t64(got), t64(ref)
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        bad = got != ref
        self.worst.setdefault(family, 0.0)
        if bool(bad.any()):
            i = int(torch.nonzero(bad.reshape(-1))[0])
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} differ; first at flat index {i}: got "
                                 f"{float(got.reshape(-1)[i])!r}, reference {float(ref.reshape(-1)[i])!r}")

    def count(self, family):
        self.cases[family] = self.cases.get(family, 0) + 1


# ------------------------------------------------------------------------------------------------ input generators
def _f32(a):
    return torch.from_numpy(np.asarray(a, np.float32).astype(np.float64))


def _randn(rng, shape):
    """Standard normal draws in fp32 from a torch generator seeded by the numpy one (numpy draws millions of values on one thread
    in more time than the whole float64 reference takes)."""
    gen = torch.Generator().manual_seed(int(rng.integers(0, 2 ** 31)))
    return torch.randn(shape, generator=gen, dtype=torch.float32)


def _store32(t32, kind):
    """An fp32 tensor -> the nearest values of the storage type, as float64 (one rounding: the source IS fp32; much cheaper
    than round_to on millions of elements)."""
    return t32.to(TORCH_DT[kind]).to(F64)


def bn_inputs(M, C, kind, seed, ratio=0.5, res_mode="none", relu=True, const_channel=None, momentum=0.1, eps=1e-5):
    """x [M, C] with mean / std = ratio per channel (signs alternate), values of the storage type; gamma, beta, running
    statistics fp32; residual (plain) or raw second input with its own gamma / beta (dual); g the incoming gradient.
    const_channel: that channel is the constant 0.125 (variance 0; every partial sum exact) and its beta is +-0.5.

    With relu, every pre-activation z is kept away from zero by more than the device can be off: the element-wise bound
    (apply_bound with three roundings) plus what the statistic bounds allow the coefficients to move, |x| d sc + d sh (+ the
    same for a dual residual), twice over.  The margin is evaluated as per-channel coefficients of |x|, |res| and 1 (an upper
    bound of the sum above; a handful of passes over the tensor instead of dozens).  Offenders are moved (x + 0.25, re-rounded)
    and the statistics recomputed until none is left, so the float64 mask and the device's agree by construction.  A channel
    with x == mean throughout (the constant channel; M == 1) is exempt from the statistic slack: z = beta up to the roundings
    of sh alone, whatever invstd the device arrives at; there the residual is moved instead.

    The float64 statistics of the final inputs are kept (d['ref'], d['ref2']) for the checks to reuse."""
    rng = np.random.default_rng(seed)
    sign = torch.from_numpy(np.where(np.arange(C) % 2 == 0, 1.0, -1.0).astype(np.float32))
    x = _store32(_randn(rng, (M, C)) + np.float32(ratio) * sign, kind)
    gamma = _f32(1 + 0.2 * rng.standard_normal(C))
    beta = _f32(0.2 * rng.standard_normal(C))
    rmean, rvar = _f32(0.3 * rng.standard_normal(C)), _f32(1 + 0.3 * rng.random(C))
    g = _store32(_randn(rng, (M, C)), kind)
    d = dict(M=M, C=C, kind=kind, gamma=gamma, beta=beta, rmean=rmean, rvar=rvar, g=g, res=None, gamma2=None, beta2=None,
             relu=relu, res_mode=res_mode, momentum=momentum, eps=eps)
    if const_channel is not None:
        x[:, const_channel] = 0.125
        beta[const_channel] = 0.5 if const_channel % 2 == 0 else -0.5
    if res_mode != "none":
        d["res"] = _store32(_randn(rng, (M, C)) * np.float32(1.3) + np.float32(0.4), kind)
    if res_mode == "dual":
        d["gamma2"], d["beta2"] = _f32(1 + 0.2 * rng.standard_normal(C)), _f32(0.2 * rng.standard_normal(C))
    gcol = gamma_cols(C, kind, M)
    free = torch.ones(C, dtype=F64)                   # 0: x == mean in the whole channel (constant channel, or M == 1)
    if const_channel is not None:
        free[const_channel] = 0.0
    if M == 1:
        free[:] = 0.0
    us = 0.0 if kind == "fp32" else UNIT[kind]
    e3 = gam(3) * (1 + us)
    zero, one = torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64)

    def side(t):
        a2 = (d["gamma2"], d["beta2"], zero, one, momentum, eps)
        r2 = bn_forward_ref(t, *a2)
        return r2, bn_forward_bounds(r2, *a2, gcol)
    r = dual = None
    for _ in range(20):
        r = bn_forward_ref(x, gamma, beta, rmean, rvar, momentum, eps)
        if res_mode == "dual" and dual is None:
            dual = side(d["res"])
        if not relu:
            break
        b = bn_forward_bounds(r, gamma, beta, rmean, rvar, momentum, eps, gcol)
        # margin <= kx |x| + kr |res| + k0 + us |z|  (apply_bound(z, mag, kind, 3) + slack, with |y| <= |z|)
        kx = e3 * r["sc"].abs() + free * b["sc"]
        k0 = e3 * r["sh"].abs() + free * b["sh"] + TINY[kind]
        z = x * r["sc"] + r["sh"]
        m = x.abs() * kx
        if res_mode == "plain":
            z += d["res"]
            m += d["res"].abs() * e3
        elif res_mode == "dual":
            z += d["res"] * dual[0]["sc"] + dual[0]["sh"]
            m += d["res"].abs() * (e3 * dual[0]["sc"].abs() + free * dual[1]["sc"])
            k0 = k0 + e3 * dual[0]["sh"].abs() + free * dual[1]["sh"]
        m += k0
        z = z.abs_().mul_(1 - 2 * us)
        if not bool((z <= 2 * m).any()):
            break
        bad = z <= 4 * m                              # move a wider band than the one tested: fewer rounds
        pinned = bad & (free == 0)                    # x must stay: move the residual there
        if bool(pinned.any()):
            assert d["res"] is not None, "a pinned channel's beta is too close to zero: choose another seed"
            d["res"][pinned] = round_to(d["res"][pinned] + 0.25, kind)
            dual = None
        move = bad & (free != 0)
        x[move] = round_to(x[move] + 0.25, kind)
    else:
        raise AssertionError("no input with every pre-activation clear of zero found")
    d["x"], d["ref"], d["ref2"] = x, r, (dual[0] if dual is not None else None)
    return d


def ibn_inputs(B, HW, C, c_in, kind, seed, relu=True, training=True, momentum=0.1, eps=1e-5):
    """As bn_inputs for the IBN layer: x [B, HW, C], per-image offsets so the images' statistics differ."""
    rng = np.random.default_rng(seed)
    off = torch.from_numpy(0.5 * rng.standard_normal((B, 1, C)))
    x = round_to(_randn(rng, (B, HW, C)).to(F64) * (0.7 + torch.from_numpy(rng.random((B, 1, C)))) + off, kind)
    half = C - c_in
    p = dict(in_w=_f32(1 + 0.2 * rng.standard_normal(c_in)), in_b=_f32(0.2 * rng.standard_normal(c_in)),
             bn_w=_f32(1 + 0.2 * rng.standard_normal(half)), bn_b=_f32(0.2 * rng.standard_normal(half)),
             rmean=_f32(0.3 * rng.standard_normal(half)), rvar=_f32(1 + 0.3 * rng.random(half)))
    g = _store32(_randn(rng, (B, HW, C)), kind)
    gcol = gamma_cols(C, kind, HW)
    for _ in range(20):
        if not relu:
            break
        r = ibn_forward_ref(x, c_in, p["in_w"], p["in_b"], p["bn_w"], p["bn_b"], p["rmean"], p["rvar"], momentum, eps, training)
        b = ibn_forward_bounds(r, c_in, p["rmean"], p["rvar"], momentum, eps, gcol, training)
        _, z, mag = bn_apply(x, r["sc"][:, None, :], r["sh"][:, None, :], relu=relu)
        # a statistic over ONE sample: x == mean exactly, z = the bias whatever invstd is (as bn_inputs) -- no statistic slack
        free = ((r["count"] > 1) if training else torch.cat([r["count"][:c_in] > 1, torch.ones(half, dtype=torch.bool)]))
        slack = x.abs() * b["sc"][:, None, :] + b["sh"][:, None, :]
        margin = apply_bound(z, mag, kind, 1) + torch.where(free, slack, torch.zeros_like(slack))
        bad = z.abs() <= 2 * margin
        if not bool(bad.any()):
            break
        assert not bool((bad & ~free).any()), "a one-sample channel's bias is too close to zero: choose another seed"
        x[bad] = round_to(x[bad] + 0.25, kind)
    else:
        raise AssertionError("no input with every pre-activation clear of zero found")
    return dict(B=B, HW=HW, C=C, c_in=c_in, kind=kind, x=x, g=g, relu=relu, training=training, momentum=momentum, eps=eps, **p)


def pool_inputs(shape, kind, mode, seed):
    """[B, H, W, C] pool inputs: 'random' continuous; 'relu' post-ReLU with at least half zeros and an all-zero window (the
    first window of image 0 is cleared); 'levels' integers 0..3 (ties everywhere); 'negative' all below zero."""
    rng = np.random.default_rng(seed)
    v = torch.from_numpy(rng.standard_normal(shape))
    if mode == "relu":
        v = torch.clamp(v - 0.2, min=0)
        v[0, :2, :2, :] = 0.0
    elif mode == "levels":
        v = torch.from_numpy(rng.integers(0, 4, size=shape).astype(np.float64))
    elif mode == "negative":
        v = -(v.abs() + 0.01)
    else:
        assert mode == "random"
    return round_to(v, kind)


# ------------------------------------------------------------------------------------------------ the checks of the sweep
# `dev` holds what an implementation produced (CPU tensors): the device in tests/test_ew_edges_gpu.py, an fp32 emulation with
# or without an injected fault in tests/test_ew_ref_cpu.py.  Both go through the same functions.
N_ROUND = {"none": 1, "plain": 2, "dual": 3}        # fp32 roundings of the apply expression: fma (+ add) (+ the residual's fma)


def check_bn_forward(R, d, dev, fam="bn_fwd"):
    """dev: mean, invstd, ss [2, C], rmean, rvar, y [M, C], bits (uint8 or None), ss2 [2, C] (dual).  Statistics against the
    float64 reference; y against the float64 apply with dev's own (scale, shift); the ReLU decision and the mask bits exactly."""
    kind, C, M = d["kind"], d["C"], d["M"]
    gcol = gamma_cols(C, kind, M)
    args = (d["gamma"], d["beta"], d["rmean"], d["rvar"], d["momentum"], d["eps"])
    ref = d.get("ref") or bn_forward_ref(d["x"], *args)
    b = bn_forward_bounds(ref, *args, gcol)
    R.check(fam + "_stats", "mean", dev["mean"], ref["mean"], b["mean"])
    R.check(fam + "_stats", "invstd", dev["invstd"], ref["invstd"], b["invstd"])
    R.check(fam + "_stats", "scale", dev["ss"][0], ref["sc"], b["sc"])
    R.check(fam + "_stats", "shift", dev["ss"][1], ref["sh"], b["sh"])
    R.check(fam + "_stats", "running_mean", dev["rmean"], ref["rmean"], b["rmean"])
    R.check(fam + "_stats", "running_var", dev["rvar"], ref["rvar"], b["rvar"])
    sc2 = sh2 = None
    if d["res_mode"] == "dual":
        z0, o1 = torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64)
        a2 = (d["gamma2"], d["beta2"], z0, o1, d["momentum"], d["eps"])
        ref2 = d.get("ref2") or bn_forward_ref(d["res"], *a2)
        b2 = bn_forward_bounds(ref2, *a2, gcol)
        sc2, sh2 = t64(dev["ss2"][0]), t64(dev["ss2"][1])
        R.check(fam + "_stats", "residual scale", sc2, ref2["sc"], b2["sc"])
        R.check(fam + "_stats", "residual shift", sh2, ref2["sh"], b2["sh"])
    y, z, mag = bn_apply(d["x"], t64(dev["ss"][0]), t64(dev["ss"][1]), d["res"], sc2, sh2, d["relu"])
    R.check(fam + "_apply", "y", dev["y"], y, apply_bound(y, mag, kind, N_ROUND[d["res_mode"]]))
    yd = t64(dev["y"])
    if d["relu"]:
        assert bool(((yd > 0) == (z > 0)).all()), "the ReLU decision differs from the float64 one (inputs keep z clear of zero)"
    if dev.get("bits") is not None:
        got, want = np.asarray(dev["bits"], np.uint8).reshape(-1), relu_bits(yd.numpy())
        assert np.array_equal(got, want), f"mask bits: {int((got != want).sum())} of {want.size} bytes differ from y > 0"
    R.count(fam)


def check_bn_backward(R, d, fwd, dev, dgamma0, dbeta0, fam="bn_bwd"):
    """fwd: the forward's mean, invstd, y; dev: sums [3, C], dgamma, dbeta, dx, gm (or None).  The mask is y > 0 of the forward
    under test.  Coefficient rows and parameter gradients against float64 (with fwd's mean / invstd); dx against the float64
    expression with dev's own rows; gm exactly."""
    kind, C, M = d["kind"], d["C"], d["M"]
    gcol = gamma_cols(C, kind, M)
    mask = (t64(fwd["y"]) > 0) if d["relu"] else None
    mean, inv = t64(fwd["mean"]), t64(fwd["invstd"])
    s = bn_backward_sums(d["x"], d["g"], mask, mean, inv)
    b = bn_backward_bounds(s, mean, inv, d["gamma"], gcol)
    A, B, Cc = bn_backward_coef(s["s1"], s["s2"], mean, inv, d["gamma"], M)
    R.check(fam + "_sums", "A", dev["sums"][0], A, b["A"])
    R.check(fam + "_sums", "B", dev["sums"][1], B, b["B"])
    R.check(fam + "_sums", "Cc", dev["sums"][2], Cc, b["Cc"])
    dg, db = t64(dgamma0) + s["s2"], t64(dbeta0) + s["s1"]
    R.check(fam + "_sums", "dgamma", dev["dgamma"], dg, acc_bound(b["s2"], s["s2"], dg))
    R.check(fam + "_sums", "dbeta", dev["dbeta"], db, acc_bound(b["s1"], s["s1"], db))
    dx, mag = bn_dx(d["x"], s["dy"], t64(dev["sums"][0]), t64(dev["sums"][1]), t64(dev["sums"][2]))
    R.check(fam + "_apply", "dx", dev["dx"], dx, apply_bound(dx, mag, kind, 2))
    if dev.get("gm") is not None:
        R.exact(fam + "_apply", "gm_out", dev["gm"], s["dy"])
    R.count(fam)


def check_pool(R, x, dev_y, dev_tap, dy, dev_dx, kind, fam="pool"):
    ry, rt = maxpool_fwd(x)
    R.exact(fam, "pooled values", dev_y, ry)
    R.exact(fam, "tap codes", dev_tap, rt)
    if dev_dx is not None:
        R.exact(fam, "dx", dev_dx, maxpool_bwd(dy, rt, x.shape[1], x.shape[2], kind))
    R.count(fam)


def check_ibn_forward(R, d, dev, fam="ibn_fwd"):
    """dev: mean, invstd [B, C], ss [B, 2, C], rmean, rvar, y [B, HW, C], bits."""
    kind, C, c_in = d["kind"], d["C"], d["c_in"]
    gcol = gamma_cols(C, kind, d["HW"])
    ref = ibn_forward_ref(d["x"], c_in, d["in_w"], d["in_b"], d["bn_w"], d["bn_b"], d["rmean"], d["rvar"], d["momentum"], d["eps"],
                          d["training"])
    b = ibn_forward_bounds(ref, c_in, d["rmean"], d["rvar"], d["momentum"], d["eps"], gcol, d["training"])
    R.check(fam + "_stats", "mean", dev["mean"], ref["mean"], b["mean"])
    R.check(fam + "_stats", "invstd", dev["invstd"], ref["invstd"], b["invstd"])
    R.check(fam + "_stats", "scale", dev["ss"][:, 0], ref["sc"], b["sc"])
    R.check(fam + "_stats", "shift", dev["ss"][:, 1], ref["sh"], b["sh"])
    if d["training"]:
        R.check(fam + "_stats", "running_mean", dev["rmean"], ref["rmean"], b["rmean"])
        R.check(fam + "_stats", "running_var", dev["rvar"], ref["rvar"], b["rvar"])
    else:
        R.exact(fam + "_stats", "running_mean (eval: untouched)", dev["rmean"], d["rmean"])
        R.exact(fam + "_stats", "running_var (eval: untouched)", dev["rvar"], d["rvar"])
    y, z, mag = bn_apply(d["x"], t64(dev["ss"][:, 0])[:, None, :], t64(dev["ss"][:, 1])[:, None, :], relu=d["relu"])
    R.check(fam + "_apply", "y", dev["y"], y, apply_bound(y, mag, kind, 1))
    yd = t64(dev["y"])
    if d["relu"]:
        assert bool(((yd > 0) == (z > 0)).all()), "the ReLU decision differs from the float64 one (inputs keep z clear of zero)"
    if dev.get("bits") is not None:
        got, want = np.asarray(dev["bits"], np.uint8).reshape(-1), relu_bits(yd.numpy())
        assert np.array_equal(got, want), f"mask bits: {int((got != want).sum())} of {want.size} bytes differ from y > 0"
    R.count(fam)


def check_ibn_backward(R, d, fwd, dev, acc0, fam="ibn_bwd"):
    """dev: coef [B, 3, C], dx, d_in_w, d_in_b, d_bn_w, d_bn_b; acc0: the four accumulators' start values (same order)."""
    kind, C, c_in, B, HW = d["kind"], d["C"], d["c_in"], d["B"], d["HW"]
    gcol = gamma_cols(C, kind, HW)
    mask = (t64(fwd["y"]) > 0) if d["relu"] else None
    mean, inv = t64(fwd["mean"]), t64(fwd["invstd"])
    w = torch.cat([d["in_w"], d["bn_w"]])
    s = ibn_backward_ref(d["x"], d["g"], mask, mean, inv, c_in, w)
    b = bn_backward_bounds(s, mean, inv, w, gcol)
    R.check(fam + "_sums", "A", dev["coef"][:, 0], s["A"], b["A"])
    R.check(fam + "_sums", "B", dev["coef"][:, 1], s["B"], b["B"])
    R.check(fam + "_sums", "Cc", dev["coef"][:, 2], s["Cc"], b["Cc"])
    ref = [t64(acc0[0]) + s["d_in_w"], t64(acc0[1]) + s["d_in_b"], t64(acc0[2]) + s["d_bn_w"], t64(acc0[3]) + s["d_bn_b"]]
    R.check(fam + "_sums", "d_in_w", dev["d_in_w"], ref[0], ibn_in_grad_bound(b["s2"][:, :c_in].sum(0), s["abs_in_w"], ref[0], B))
    R.check(fam + "_sums", "d_in_b", dev["d_in_b"], ref[1], ibn_in_grad_bound(b["s1"][:, :c_in].sum(0), s["abs_in_b"], ref[1], B))
    R.check(fam + "_sums", "d_bn_w", dev["d_bn_w"], ref[2], acc_bound(b["s2"][0, c_in:], s["d_bn_w"], ref[2]))
    R.check(fam + "_sums", "d_bn_b", dev["d_bn_b"], ref[3], acc_bound(b["s1"][0, c_in:], s["d_bn_b"], ref[3]))
    cf = t64(dev["coef"])
    dx, mag = bn_dx(d["x"], s["dy"], cf[:, 0][:, None, :], cf[:, 1][:, None, :], cf[:, 2][:, None, :])
    R.check(fam + "_apply", "dx", dev["dx"], dx, apply_bound(dx, mag, kind, 2))
    R.count(fam)


# ------------------------------------------------------------------------------------------------ the shapes of the sweep
# (M, C, storage kinds, what it reaches)
BN_SHAPES = [
    (1, 8, KINDS, "count == 1"),
    (2, 8, KINDS, ""),
    (127, 8, KINDS, ""),
    (129, 24, KINDS, "cw = 3 / 6: a surplus row lane"),
    (300, 40, KINDS, "cw = 5 / 10"),
    (1000, 72, KINDS, "cw = 9 / 18"),
    (389, 320, KINDS, "two column groups, the second one partial"),
    (24711, 16, KINDS, "194 partial rows: the unrolled finalize loop of CW = 16 plus its tail"),
    (65537, 8, KINDS, "513 partial rows: the CW = 4 finalize"),
    (98437, 8, KINDS, "770 partial rows: the unrolled loop of CW = 4"),
    (65537, 64, ("bf16", "f16"), "past the grid cap, two chunks per thread, power-of-two C"),
    (131073, 32, ("fp32",), "past the grid cap, two chunks per thread, power-of-two C"),
    (120000, 40, ("bf16", "f16"), "past the cap with 5 chunks per row"),
    (60000, 40, ("fp32",), "past the cap with 10 chunks per row"),
    (70000, 72, ("bf16", "f16"), "past the cap with 9 chunks per row"),
]
RATIO_SHAPES = [(300, 40), (1000, 72), (389, 320)]        # mean / std = 16 and 256 run on these
FIN_APPLY_CASES = [(1, 64, 0), (33, 64, 1), (1000, 128, 0), (32768, 64, 0), (131072, 64, 0)]      # (M, C, row_blocks)
POOL_SHAPES = [(1, 2, 2, 8), (2, 4, 6, 8), (3, 16, 8, 24), (2, 10, 14, 64), (1, 6, 4, 264)]
POOL_MODES = ("random", "relu", "levels", "negative")
GAP_SHAPES = [(1, 1, 8), (2, 7, 24), (2, 9, 264), (3, 128, 2048)]
IBN_SHAPES = [(1, 1, 16, 8), (5, 129, 16, 8), (3, 60, 64, 32), (17, 643, 64, 32), (2, 257, 256, 128)]


# ------------------------------------------------------------------------------------------------ grid arithmetic
def ew_blocks_cap(total_threads_needed, mult, cap, fixed=True):
    """Integer mirror of ew_blocks_cap (csrc/elementwise.hip): workgroups of 256 threads, at most `cap`, rounded up so that
    blocks * 256 is a multiple of `mult`.  fixed=False: the rule before it covered a mult that is no power of two."""
    b = min((total_threads_needed + 255) // 256, cap)
    b = max(b, 1)
    q = mult // math.gcd(mult, 256) if fixed else (mult // 256 if mult > 256 else 1)
    return (b + q - 1) // q * q


def drifted_chunks(total, cpr, blocks):
    """Chunks a grid-stride apply kernel handles with another channel chunk's coefficients: thread gtid keeps the coefficients of
    chunk gtid % cpr and visits i = gtid, gtid + nthreads, ...; chunk i belongs to channel chunk i % cpr."""
    i = np.arange(total, dtype=np.int64)
    n = blocks * 256
    return int((((i % n) % cpr) != (i % cpr)).sum())
