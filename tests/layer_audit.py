"""Per-layer audit of a training step against fp64: reference operations and the comparison rule shared by
tests/test_layer_audit_gpu.py (a real step of the engine, every layer on its own recorded operands) and
tests/test_layer_audit_cpu.py (torch emulations of the kernels, with mutations the audit must catch).

Everything here is plain torch in float64 on whatever device the operands live on; nothing calls the project's kernels.

The comparison (Audit.check) applies three checks to one output tensor, given its fp64 reference `ref` and a first-order bound
`b` of the error the fp32 evaluation may add before the final rounding to the output type:

* element-wise: |got - ref| <= 1/2 ulp_out(|ref| + b) + b (the fp32 evaluation, then ONE round-to-nearest into the output type);
* bias (16-bit outputs only): the mean signed error in output ulps, and the same with the sign of ref folded in (truncation
  toward zero is -1/2 ulp there), over the elements where the final rounding dominates (statistical accumulation error
  sigma <= ulp / 8).  RNE errors are uniform on [-1/2, 1/2] ulp with standard deviation 1/sqrt(12) ~ 0.29 ulp: the bar is
  BIAS_FLOOR + 6 sigma_mean, sigma_mean = sqrt(1/12 + (sigma / ulp)^2) / sqrt(n).  BIAS_FLOOR = 0.01 ulp covers the non-uniform
  density of values inside one ulp (relative variation <= 2^-7 over a bf16 ulp: ~2^-7 / 12 = 6.5e-4 ulp of bias);
* relative L2: ||got - ref|| <= REL_L2_MARGIN * sqrt(sum(ulp_out(ref)^2 / 12 + sigma^2)) / ||ref||, sigma = the statistical
  accumulation error the caller passes (sqrt(K) u mag for a K-term fp32 sum).  The expectation of the squared error of an
  unbiased rounding is ulp^2 / 12; truncation makes it ulp^2 / 3 (2x the RMS), so REL_L2_MARGIN = 1.5 sits between the two.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24                 # unit roundoff of fp32
SPLIT = 2.0 ** -16             # bf16x3: hi + lo represents an fp32 operand to 2^-18 relative, x 2 operands, + the dropped lo*lo
BIAS_FLOOR = 0.01
REL_L2_MARGIN = 1.5
_FMT = {torch.bfloat16: (7, -126), torch.float16: (10, -14), torch.float32: (23, -126)}


def half_ulp(v, dt):
    """half an ulp of `dt` at |v| (fp64 tensor), with the subnormal spacing below the smallest normal"""
    mant, emin = _FMT[dt]
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** emin)))
    return torch.exp2(e - mant - 1)


def ulp(v, dt):
    return 2.0 * half_ulp(v, dt)


# ------------------------------------------------------------------------------------------- fp64 reference operations
def _taps(k, s, oh, ow):
    for r in range(k):
        for c in range(k):
            yield r, c, (slice(r, r + s * (oh - 1) + 1, s), slice(c, c + s * (ow - 1) + 1, s))


def conv_fwd(x, w, s, p):
    """conv2d of x [B, H, W, Cin] (NHWC, any dtype) with w [Cout, Cin, k, k] in fp64 -> [B, OH, OW, Cout]"""
    k, cout, cin = w.shape[2], w.shape[0], w.shape[1]
    xp = F.pad(x.double(), (0, 0, p, p, p, p))
    B = xp.shape[0]
    oh, ow = (xp.shape[1] - k) // s + 1, (xp.shape[2] - k) // s + 1
    y = torch.zeros(B * oh * ow, cout, dtype=torch.float64, device=x.device)
    wd = w.double()
    for r, c, (sr, sc) in _taps(k, s, oh, ow):
        y += xp[:, sr, sc, :].reshape(-1, cin) @ wd[:, :, r, c].t()
    return y.view(B, oh, ow, cout)


def conv_dgrad(dy, w, s, p, H, W):
    """input gradient of the same convolution: dy [B, OH, OW, Cout] -> [B, H, W, Cin], fp64"""
    k, cout, cin = w.shape[2], w.shape[0], w.shape[1]
    B, oh, ow = dy.shape[0], dy.shape[1], dy.shape[2]
    dxp = torch.zeros(B, H + 2 * p + s, W + 2 * p + s, cin, dtype=torch.float64, device=dy.device)
    g = dy.double().reshape(-1, cout)
    wd = w.double()
    for r, c, (sr, sc) in _taps(k, s, oh, ow):
        dxp[:, sr, sc, :] += (g @ wd[:, :, r, c]).view(B, oh, ow, cin)
    return dxp[:, p:p + H, p:p + W, :]


def conv_wgrad(x, dy, k, s, p):
    """weight gradient [Cout, Cin, k, k] of x [B, H, W, Cin], dy [B, OH, OW, Cout], fp64"""
    cin, cout = x.shape[3], dy.shape[3]
    oh, ow = dy.shape[1], dy.shape[2]
    xp = F.pad(x.double(), (0, 0, p, p, p, p))
    g = dy.double().reshape(-1, cout).t()
    dw = torch.zeros(cout, cin, k, k, dtype=torch.float64, device=x.device)
    for r, c, (sr, sc) in _taps(k, s, oh, ow):
        dw[:, :, r, c] = g @ xp[:, sr, sc, :].reshape(-1, cin)
    return dw


def unpack_bits(mask, M, C):
    """ReLU bits (bit k of byte i = element 8 i + k of the row-major [M, C] tensor) -> bool [M, C]"""
    m = mask.reshape(-1).to(torch.int32)
    bits = torch.stack([(m >> k) & 1 for k in range(8)], dim=1).reshape(-1)
    return bits[:M * C].view(M, C).bool()


def batch_stats(y, eps):
    """per-channel batch mean, biased variance and invstd of fp64 y [M, C] (the statistics of the unrounded conv output)"""
    mean = y.mean(0)
    var = (y * y).mean(0) - mean * mean
    return mean, var, 1.0 / torch.sqrt(var + eps)


def stats_bound(y, e, eps, rows_per_tile=128, count=None):
    """first-order bounds of the batch (mean, invstd) of y [M, C]: the values the kernel sums are each off by <= e from y (the
    conv epilogue sums its fp32 accumulators, K u mag from the fp64 conv output; 0 where the kernel reads the stored tensor the
    reference reads too), one fp32 (sum, sumsq) partial per `rows_per_tile` rows (<= (R + 2) u of the summed magnitudes), fp64
    over the partials, one fp32 rounding of the result.  Returns (dmean, dinvstd, var, dvar) per channel."""
    count = count or y.shape[0]
    ay = y.abs()
    dmean = (e.sum(0) + (rows_per_tile + 2) * U * ay.sum(0)) / count
    dE2 = (2.0 * (ay * e).sum(0) + (e * e).sum(0) + (rows_per_tile + 2) * U * (y * y).sum(0)) / count
    mean = y.sum(0) / count
    var = ((y * y).sum(0) / count - mean * mean).clamp_min(0.0)
    dvar = dE2 + 2.0 * mean.abs() * dmean + dmean * dmean
    invstd = 1.0 / torch.sqrt(var + eps)
    dinv = invstd * (0.5 * dvar / (var + eps) * 1.01 + 2 * U)    # first order in dvar / var, + the fp32 rounding
    return dmean + U * mean.abs(), dinv, var, dvar


def affine_bound(x, sc, sh, terms):
    """fp32 evaluation of fma(x, sc, sh) (+ residual terms) with sc = gamma * invstd, sh = beta - mean * sc in fp32: every
    rounding <= u |its result|; three roundings reach each product term.  `terms` = extra |addends| (residual, second BN)."""
    b = 3 * U * ((x * sc).abs() + sh.abs() + (x * sc + sh).abs())
    for t in terms:
        b = b + 3 * U * t.abs()
    return b


def maxpool3x3s2(y):
    """3 x 3 stride 2 pad 1 max-pool of NHWC y (fp64) -> (values, first-max tap r * 3 + s), taps in window order"""
    B, H, W, Cc = y.shape
    yp = F.pad(y, (0, 0, 1, 1, 1, 1), value=-math.inf)
    OH, OW = H // 2, W // 2
    taps = torch.stack([yp[:, r:r + 2 * OH:2, s:s + 2 * OW:2, :] for r in range(3) for s in range(3)], 0)
    v = taps.max(0).values
    tap = torch.arange(9, device=y.device).view(9, 1, 1, 1, 1)
    i = torch.where(taps == v.unsqueeze(0), tap, torch.full_like(tap, 9)).min(0).values      # the first maximal tap
    return v, i, taps


def maxpool3x3s2_bwd(g, idx, H, W):
    """scatter of g [B, OH, OW, C] through the window taps idx (0..8) -> [B, H, W, C], fp64"""
    B, OH, OW, Cc = g.shape
    out = torch.zeros(B, H + 2, W + 2, Cc, dtype=torch.float64, device=g.device)
    gd = g.double()
    idx = idx.long()
    for r in range(3):
        for s in range(3):
            sel = (idx == r * 3 + s)
            out[:, r:r + 2 * OH:2, s:s + 2 * OW:2, :] += torch.where(sel, gd, torch.zeros((), dtype=torch.float64, device=g.device))
    return out[:, 1:H + 1, 1:W + 1, :]


def bn_bwd(x, dy, mean, invstd, gamma, groups=None):
    """BatchNorm backward in fp64 on the operands the kernel read: x [M, C] (stored), dy [M, C] (masked incoming gradient),
    mean / invstd [C] or, with `groups` = (G, rows per group), [G, C] per-group statistics (InstanceNorm: one group per image).
    Returns dx, sum(dy), sum(dy xhat) (summed per group when grouped), and the bound inputs (a1, a2, xhat)."""
    x, dy = x.double(), dy.double()
    M, Cc = x.shape
    G, R = groups if groups is not None else (1, M)
    xv, dv = x.view(G, R, Cc), dy.view(G, R, Cc)
    mu, isd = mean.double().view(G, 1, Cc), invstd.double().view(G, 1, Cc)
    xhat = (xv - mu) * isd
    s1, s2 = dv.sum(1), (dv * xhat).sum(1)
    a1, a2 = (s1 / R).unsqueeze(1), (s2 / R).unsqueeze(1)
    g = gamma.double().view(1, 1, Cc)
    dx = g * isd * (dv - a1 - xhat * a2)
    return dx.view(M, Cc), s1, s2, (a1, a2, xhat, mu, isd, g)


def bn_bwd_bound(x, dy, parts, R, rows_per_tile=128):
    """first-order bound of the kernel's dx = k1 dy + (-k1 is a2) x + (-k1 a1 + k1 is a2 mu) (bn_fin.hpp: fp32 coefficients from
    fp64 sums over fp32 per-tile partials) and of its two sums.  Every route sums the STORED incoming gradient the reference
    reads (the fused data-gradient epilogue, the heads' part3, reduce2 and the BatchNorm / IBN kernels' own partials all read
    the packed 16-bit values), so the partial sums carry only their fp32 rounding: (R + 2) u sum |dy| and, with xhat = (x - mu)
    is in fp32 (2 u) and one fma, (R + 6) u sum |dy xhat|."""
    a1, a2, xhat, mu, isd, g = parts
    Cc = x.shape[1]
    G = mu.shape[0]
    xv, dv = x.double().view(G, -1, Cc), dy.double().view(G, -1, Cc)
    ds1 = (rows_per_tile + 2) * U * dv.abs().sum(1)
    ds2 = (rows_per_tile + 6) * U * (dv * xhat).abs().sum(1)
    k1 = (g * isd).abs()
    b = 4 * U * k1 * (dv.abs() + a1.abs() + (isd * a2).abs() * (xv.abs() + mu.abs())) \
        + k1 * (ds1.unsqueeze(1) / R + (xv - mu).abs() * isd * ds2.unsqueeze(1) / R)
    return b.view(x.shape), ds1, ds2


# ------------------------------------------------------------------------------------------- comparison
class Audit:
    """Collects one row per (layer, op) check and the failures; `table()` prints the per-layer summary."""

    def __init__(self, tag):
        self.tag, self.rows, self.failures, self.max_rms = tag, [], [], []

    def check(self, layer, op, got, ref, b, dt, sigma=None, bias=True, rel_bar=None, max_rms=None, report_max_rms=False):
        """max_rms: assert max |err| <= max_rms rms(ref); report_max_rms: only record that ratio (self.max_rms).  A non-finite
        output is a failure: nothing is skipped."""
        got, ref = got.double().reshape(-1), ref.double().reshape(-1)
        b = (b if torch.is_tensor(b) else torch.full_like(ref, float(b))).double().reshape(-1).expand_as(ref)
        n_bad = int((~torch.isfinite(got)).sum())
        if n_bad:
            msg = f"{n_bad} non-finite outputs"
            self.rows.append((layer, op, float("inf"), float("nan"), float("inf"), 0.0, msg))
            self.failures.append(f"{self.tag} {layer} {op}: {msg}")
            return
        err = got - ref
        bound = half_ulp(ref.abs() + b, dt) + b
        ratio = float((err.abs() / bound).max()) if err.numel() else 0.0
        sig = torch.zeros_like(ref) if sigma is None else (sigma if torch.is_tensor(sigma) else torch.full_like(ref, float(sigma)))
        sig = sig.double().reshape(-1).expand_as(ref)
        nref = float(ref.norm())
        rel = float(err.norm()) / max(nref, 1e-300)
        if rel_bar is None:
            u2 = ulp(ref, dt) ** 2 / 12.0
            rel_bar = REL_L2_MARGIN * math.sqrt(float((u2 + sig * sig).sum())) / max(nref, 1e-300)
        bias_v = mag_bias = bias_bar = float("nan")
        notes = []
        if bias and dt != torch.float32:
            u_ref = ulp(ref, dt)
            sel = (ref != 0) & (sig <= u_ref / 8)
            n = int(sel.sum())
            if n:
                e_ulp = err[sel] / u_ref[sel]
                bias_v = float(e_ulp.mean())
                mag_bias = float((e_ulp * torch.sign(ref[sel])).mean())
                s_rel = float(torch.sqrt(1.0 / 12 + ((sig[sel] / u_ref[sel]) ** 2).mean()))
                bias_bar = BIAS_FLOOR + 6 * s_rel / math.sqrt(n)
                if max(abs(bias_v), abs(mag_bias)) > bias_bar:
                    notes.append(f"bias {bias_v:+.4f} / {mag_bias:+.4f} ulp > {bias_bar:.4f}")
        if ratio > 1.0:
            notes.append(f"max err / bound {ratio:.3g} ({int((err.abs() > bound).sum())} elements)")
        if rel > rel_bar:
            notes.append(f"rel-L2 {rel:.3e} > {rel_bar:.3e}")
        if max_rms is not None or report_max_rms:
            m = float(err.abs().max()) / max(nref / math.sqrt(max(ref.numel(), 1)), 1e-300)
            self.max_rms.append((layer, op, m))
            if max_rms is not None and m > max_rms:
                notes.append(f"max err {m:.3e} rms(ref) > {max_rms:g} rms(ref)")
        self.rows.append((layer, op, ratio, mag_bias, rel, rel_bar, "; ".join(notes)))
        if notes:
            self.failures.append(f"{self.tag} {layer} {op}: " + "; ".join(notes))

    def exact(self, layer, op, ok, detail=""):
        """a check that must hold exactly (ReLU bits, argmax taps, masked copies)"""
        self.rows.append((layer, op, 0.0 if ok else float("inf"), float("nan"), 0.0, 0.0, "" if ok else f"mismatch {detail}"))
        if not ok:
            self.failures.append(f"{self.tag} {layer} {op}: mismatch {detail}")

    def relu_bits(self, layer, bits, a_out, ref, dt):
        """ReLU bits written with an activation must equal act > 0 exactly.  f16 only: a positive fp32 value below 2^-25 (half
        the smallest f16 subnormal) rounds to 0 after its bit was set; such elements (ref <= 2^-24) are counted, not failed."""
        M, Cc = a_out.shape[0] if a_out.dim() == 2 else a_out.numel() // a_out.shape[-1], a_out.shape[-1]
        got = unpack_bits(bits, M, Cc)
        act = a_out.reshape(M, Cc)
        bad = got != (act > 0)
        tiny = got & (act == 0) & (ref.reshape(M, Cc) <= 2.0 ** -24) if dt == torch.float16 else torch.zeros_like(bad)
        n_bad, n_tiny = int(bad.sum()), int((bad & tiny).sum())
        self.exact(layer, "relu bits", n_bad == n_tiny, f"{n_bad - n_tiny} bits differ from act > 0")
        if n_tiny:
            self.note(layer, "relu bits", f"{n_tiny} f16 values below 2^-25 rounded to 0 after their bit was set")
        return n_bad - n_tiny

    def note(self, layer, op, text):
        self.rows.append((layer, op, float("nan"), float("nan"), float("nan"), float("nan"), text))

    def failing_layers(self):
        return {f[len(self.tag) + 1:].split(" ")[0] for f in self.failures}

    def op_summary(self):
        """one line per kind of check (route tags in [...] dropped): worst bound ratio, worst |bias|, worst rel-L2 / bar"""
        per = {}
        for layer, op, ratio, mb, rel, bar, note in self.rows:
            d = per.setdefault(op.split(" [")[0], [0.0, 0.0, 0.0, 0])
            if ratio == ratio:
                d[0] = max(d[0], ratio)
            if mb == mb:
                d[1] = max(d[1], abs(mb))
            if rel == rel and bar == bar and bar > 0:
                d[2] = max(d[2], rel / bar)
            d[3] += 1
        return "\n".join(f"[{self.tag}] op {op:<34} n {n:>3}  max err/bound {r:.3g}  |bias| {b:.4f}  rel/bar {q:.3f}"
                         for op, (r, b, q, n) in per.items())

    def table(self):
        """one line per layer: worst bound ratio, worst |bias| (ulp, sign of ref folded in), worst rel-L2 / its bar"""
        per = {}
        for layer, op, ratio, mb, rel, bar, note in self.rows:
            d = per.setdefault(layer, [0.0, 0.0, 0.0, 0.0, 0, []])
            if ratio == ratio:
                d[0] = max(d[0], ratio)
            if mb == mb:
                d[1] = max(d[1], abs(mb))
            if rel == rel and bar == bar and bar > 0:
                if rel / bar >= d[3]:
                    d[2], d[3] = rel, rel / bar
            d[4] += 1
            if note:
                d[5].append(f"{op}: {note}")
        lines = [f"[{self.tag}] {'layer':<22} {'checks':>6} {'max err/bound':>13} {'|bias| ulp':>10} {'rel-L2':>10} {'rel/bar':>8}"]
        for layer, (r, mb, rel, rb, n, notes) in per.items():
            lines.append(f"[{self.tag}] {layer:<22} {n:>6} {r:>13.3g} {mb:>10.4f} {rel:>10.3e} {rb:>8.3f}"
                         + (("  " + " | ".join(notes)) if notes else ""))
        return "\n".join(lines)
