"""Per-layer audit of the eval-mode forward against fp64: the references and bounds shared by tests/test_eval_audit_gpu.py (one real
BackboneEngine.forward(x, False, True) + the eval-mode BNNeck, every launch on its own recorded operands) and
tests/test_eval_audit_cpu.py (torch emulations of the same kernels, with the mutations the audit must flag).

Everything here is plain torch in float64 on whatever device the operands live on; nothing calls the project's kernels.  The
comparison itself is layer_audit.Audit.check: |got - ref| <= 1/2 ulp_out(|ref| + b) + b element-wise, the bias and relative-L2
bars of its docstring.  What this file adds is the reference and the first-order bound `b` of each eval-mode launch, derived from
the arithmetic of the kernel it judges (u = 2^-24):

* fold constants (bn_fold_multi_kernel, elementwise.hip; -ffp-contract=off, IEEE division and square root): four fp32 operations
  make the scale, is = 1 / sqrtf(var + eps), sc = is * gamma: the add rounds once (u, halved by the square root), the square
  root, the division and the product once each: <= 3.5 u |sc|, taken as FOLD_U = 4 u.  The shift beta - mean * sc rounds the
  product (u |mean sc|) and the difference (u |sh| <= u |beta| + u |mean sc|) and inherits the scale's error through the mean:
  u |beta| + 2 u |mean sc| + |mean| dsc.  eps is the fp32 value the table carries.
* folded convolution (conv -> fma(acc, sc, sh) -> (+ residual) -> (ReLU) -> one rounding; the fold constants are the device's own,
  as stored): the fp32 accumulator is within K u (|x| |w|) of the fp64 sum (K products per output; bf16x3 adds 2^-16 (|x| |w|)),
  scaled by |sc|, plus layer_audit.affine_bound (3 u per term of the fma and of the fp32 residual add).  The 16-bit epilogues round
  the fma result to the storage type FIRST (the C tile is staged through LDS as 16-bit words), then add the residual in fp32 and
  round again (add_chunk, conv_epilogue.hpp): with a residual on a 16-bit output the bound gains 1/2 ulp_16(|affine| + b) for the
  first rounding and 2 u (|affine| + |residual|) for the fp32 add.  The final rounding is Audit.check's own half ulp.  ReLU is
  1-Lipschitz: the bound of the pre-activation holds for the activation.
* statistics partials of the pair kernel: a [2][64] (sum, sum of squares) row per 128-row tile of the fp32 accumulators:
  sum_rows e + (R + 2) u sum |y| and sum (2 |y| e + e^2) + (R + 2) u sum y^2 (the numerators of layer_audit.stats_bound).
* eval-mode IBN (ibn_finalize_kernel with training = 0): InstanceNorm half = per-image statistics, fp64 over fp32 per-128-row
  partials: layer_audit.stats_bound with count = HW; BatchNorm half = the running mean as it is (exact) and 1 / sqrtf(var + eps)
  (add, square root, division: 2.5 u, taken as 3 u); the applied output is fma(x, sc, sh) with sc = invstd * gamma,
  sh = beta - mean * sc in fp32: layer_audit.affine_bound with the |mean sc| term.
* GAP (gap_fwd_kernel: fp32 sums of HW values, one division): HW u mean|a| + u |ref|, the training audit's bar.
* eval-mode BNNeck (bn1d_fwd_body): y = (x - mean) * invstd * gamma + beta in fp32, invstd = 1 / sqrtf(var + eps): the difference
  (u), invstd (2.5 u), two products (2 u) reach t = (x - mean) invstd gamma: 5.5 u |t|, taken as 6 u |t|, + u |y| for the add.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import layer_audit as la

U = la.U
F32 = torch.float32
FOLD_U = 4.0


def eps32(eps):
    """the fp32 value of eps the kernels receive"""
    return float(np.float32(eps))


# ------------------------------------------------------------------------------------------- fold constants
def fold_reference(gamma, beta, mean, var, eps):
    """fp64 (scale, shift) of an eval-mode BatchNorm and their bounds; gamma / beta None = 1 / 0 (the table's null entries)"""
    var, mean = var.double(), mean.double()
    g = torch.ones_like(var) if gamma is None else gamma.detach().double()
    b = torch.zeros_like(var) if beta is None else beta.detach().double()
    sc = g / torch.sqrt(var + eps32(eps))
    sh = b - mean * sc
    dsc = FOLD_U * U * sc.abs()
    dsh = U * b.abs() + 2 * U * (mean * sc).abs() + mean.abs() * dsc
    return sc, sh, dsc, dsh


def check_fold(au, layer, fold, gamma, beta, mean, var, eps):
    """fold = the device's fp32 [2][C]"""
    sc, sh, dsc, dsh = fold_reference(gamma, beta, mean, var, eps)
    au.check(layer, "fold scale", fold[0], sc, dsc, F32, sigma=dsc, bias=False)
    au.check(layer, "fold shift", fold[1], sh, dsh, F32, sigma=dsh, bias=False)


# ------------------------------------------------------------------------------------------- folded convolution
def conv_reference(x, w, stride, pad, x3=False):
    """fp64 convolution of the stored operands x [B, H, W, cin], w [cout, cin, k, k] -> (ref [M, cout], accumulator bound e,
    statistical accumulator error sigma)"""
    cout = w.shape[0]
    K = w.shape[1] * w.shape[2] * w.shape[3]
    ref = la.conv_fwd(x, w, stride, pad).reshape(-1, cout)
    mag = la.conv_fwd(x.double().abs(), w.double().abs(), stride, pad).reshape(-1, cout)
    split = la.SPLIT * mag if x3 else 0.0
    return ref, K * U * mag + split, math.sqrt(K) * U * mag + split


def folded_reference(conv, e, sig, fold, relu, residual, dt):
    """the folded epilogue on the fp64 convolution `conv` [M, C] -> (ref, bound, sigma, pre-activation reference)"""
    sc, sh = fold[0].double(), fold[1].double()
    y = conv * sc + sh
    b = sc.abs() * e + la.affine_bound(conv, sc, sh, [])
    s = sc.abs() * sig + U * y.abs()
    pre = y
    if residual is not None:
        r = residual.double().reshape(y.shape)
        if dt != F32:
            first = la.half_ulp(y.abs() + b, dt)              # the affine result is rounded to the storage type before the add
            b = b + first + 2 * U * (y.abs() + r.abs())
            s = s + first * (2.0 / math.sqrt(12.0))
        else:
            b = b + 3 * U * r.abs()
        pre = y + r
    return (pre.clamp_min(0.0) if relu else pre), b, s, pre


def check_folded_conv(au, layer, op, got, x, w, stride, pad, fold, relu, residual, dt, x3=False):
    """one creid_conv2d_fwd_affine_nhwc-style output `got` [M, cout] of stored operands; returns the fp64 reference"""
    conv, e, sig = conv_reference(x, w, stride, pad, x3)
    ref, b, s, pre = folded_reference(conv, e, sig, fold, relu, residual, dt)
    au.check(layer, op, got, ref, b, dt, sigma=s, rel_bar=2e-5 if x3 else None)
    if x3:
        # the x3 layer bar max |err| <= 1e-4 rms, against the rms of the pre-activation reference: ReLU zeroes half of the reference
        # without touching the error of the other half
        m = float((got.double().reshape(ref.shape) - ref).abs().max()) / max(float(pre.norm()) / math.sqrt(pre.numel()), 1e-300)
        au.max_rms.append((layer, op, m))
        au.exact(layer, "x3 max <= 1e-4 rms [" + op + "]", m <= 1e-4, f"max err {m:.3e} rms(ref)")
    return ref


# ------------------------------------------------------------------------------------------- statistics partials
def check_tile_partials(au, layer, part, conv, e, rows_per_tile=128):
    """part [tiles][2][C] of the fp32 accumulators whose fp64 value is conv [tiles * rows_per_tile, C]"""
    Cc = conv.shape[1]
    y3, e3 = conv.view(-1, rows_per_tile, Cc), e.view(-1, rows_per_tile, Cc)
    ay = y3.abs()
    d1 = e3.sum(1) + (rows_per_tile + 2) * U * ay.sum(1)
    d2 = 2.0 * (ay * e3).sum(1) + (e3 * e3).sum(1) + (rows_per_tile + 2) * U * (y3 * y3).sum(1)
    p = part.view(-1, 2, Cc)
    au.check(layer, "tile sums", p[:, 0], y3.sum(1), d1, F32, sigma=d1, bias=False)
    au.check(layer, "tile sums of squares", p[:, 1], (y3 * y3).sum(1), d2, F32, sigma=d2, bias=False)


# ------------------------------------------------------------------------------------------- eval-mode IBN
def check_eval_ibn(au, layer, x_raw, a_out, mean, invstd, conv, e, B, HW, half, in_w, in_b, bn_w, bn_b, rmean, rvar, eps, ready, dt,
                   relu=True):
    """creid_ibn_fwd_mask with training = 0.  x_raw [B HW, C] the stored conv output, a_out the applied output, mean / invstd the
    [B, C] the kernel reports; conv / e: the fp64 convolution and its accumulator bound (used when the statistics partials came
    ready from the producing launch: they are sums of its fp32 accumulators); otherwise the kernel sums the stored tensor
    (ibn_col_stats_kernel: one fp32 partial per 128 rows of an image, the last one shorter)."""
    Cc = x_raw.shape[-1]
    tile = 128
    if ready:
        ref, err = conv.reshape(-1, Cc), e.reshape(-1, Cc)
    else:
        ref = x_raw.double().reshape(-1, Cc)
        err = torch.zeros_like(ref)
    r3, e3 = ref.view(B, HW, Cc), err.view(B, HW, Cc)
    rows = []
    for n in range(B):
        m_ref, _, i_ref = la.batch_stats(r3[n, :, :half], eps32(eps))
        dm, dinv, _, _ = la.stats_bound(r3[n, :, :half], e3[n, :, :half], eps32(eps), tile, count=HW)
        rows.append((m_ref, i_ref, dm, dinv))
    st = [torch.stack([t[i] for t in rows]) for i in range(4)]
    au.check(layer, "IN mean", mean[:, :half], st[0], st[2], F32, bias=False, sigma=st[2])
    au.check(layer, "IN invstd", invstd[:, :half], st[1], st[3], F32, bias=False, sigma=st[3])
    au.exact(layer, "BN-half mean = running_mean", torch.equal(mean[:, half:], rmean.reshape(1, -1).expand(B, Cc - half)))
    i_bn = (1.0 / torch.sqrt(rvar.double() + eps32(eps))).reshape(1, -1).expand(B, Cc - half)
    au.check(layer, "BN-half invstd", invstd[:, half:], i_bn, 3 * U * i_bn, F32, bias=False, sigma=3 * U * i_bn)
    x = x_raw.double().view(B, HW, Cc)
    sc = torch.cat([invstd[:, :half].double() * in_w.detach().double(), invstd[:, half:].double() * bn_w.detach().double()], 1)
    beta = torch.cat([in_b.detach().double().expand(B, half), bn_b.detach().double().expand(B, Cc - half)], 1)
    msc = mean.double() * sc
    sh = beta - msc
    y = x * sc.unsqueeze(1) + sh.unsqueeze(1)
    b = la.affine_bound(x, sc.unsqueeze(1), sh.unsqueeze(1), [msc.unsqueeze(1)])
    au.check(layer, "IBN apply", a_out, y.clamp_min(0.0) if relu else y, b, dt, sigma=b)


# ------------------------------------------------------------------------------------------- pooled features, embedding
def check_gap(au, feat, a, B, HW):
    """creid_gap_fwd of the stored activation a [B HW, C]"""
    av = a.double().view(B, HW, -1)
    ref = av.mean(1)
    au.check("gap", "gap fwd", feat, ref, HW * U * av.abs().mean(1) + U * ref.abs(), F32, bias=False,
             sigma=math.sqrt(HW) * U * av.abs().mean(1))


def check_bnneck(au, emb, feat, weight, bias, rmean, rvar, eps):
    """creid_bn1d_fwd on running statistics"""
    g = torch.ones_like(rvar).double() if weight is None else weight.detach().double()
    be = torch.zeros_like(rvar).double() if bias is None else bias.detach().double()
    t = (feat.double() - rmean.double()) / torch.sqrt(rvar.double() + eps32(eps)) * g
    ref = t + be
    b = 6 * U * t.abs() + U * ref.abs()
    au.check("bnneck", "embedding", emb, ref, b, F32, bias=False, sigma=b)
