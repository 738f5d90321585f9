"""float64 references, error bounds, fp32 step models and input generators for what csrc/heads.hip runs after the heads -- Adam
(creid_adam_step, _dev, _dev_amp), the centers' SGD step, the f16 loss scaler (scale, unscale-and-check, update) -- and for the
general-distance surface: row normalisation, the cosine triplet, mining on a given matrix, clamp + sqrt, per-segment row means.
Plain numpy / torch on the CPU; nothing of the package is imported, nothing outside tests/ is read.

Adam is compared in two layers (tests/test_opt_edges_gpu.py), as tests/ew_ref.py does for BatchNorm:
  1. the bias corrections the device publishes, hyper[2] = bc1 = 1 - b1^t and hyper[3] = bc2s = sqrt(1 - b2^t), against float64.
     They come out of an fp32 powf: with a relative error of k_pow u on b^t, 1 - b^t is off by (k_pow u b^t + u) / (1 - b^t)
     relatively -- a 1000-fold amplification at t = 1, b2 = 0.999.  K_POW is measured (profiles/opt_edges.md), not derived.
  2. every element of p, m, v against the float64 evaluation WITH THE CORRECTIONS THE STEP USED (the published ones; for the
     host-scalar entry point the host's own powf, recomputed here through the same libm), within bounds that follow from the
     kernel's operation sequence.  The slack of layer 1 can then not hide an element-wise error.
gam(k) = k u / (1 - k u), u = 2^-24; TINY = 2^-150 is half the spacing of the fp32 subnormals (one rounding that underflows).

Bit-exact expectations (no contraction, no fast-math, correctly rounded division and square root): amp_scale fl(x s),
amp_unscale_check fl(g inv), sgd_scaled g' = fl(g gmul), p' = fl(p - fl(lr g')), clamp_sqrt fl(sqrt(max(d, lo))), gather_mean_rows
a sequential fp32 sum in list order and one division.

Scope.  Generators spread magnitudes from 1e-20 to 1e3 with exact zeros (p = g = m = v = 0 included: v' = 0, the denominator
is eps alone) and values whose squares underflow; they stay clear of overflow.  Outside the non-finite GRADIENT values that the
unscale-and-check tests place on purpose, NaN and infinite inputs are out of scope.  One known difference is recorded here and
not tested: clamp_sqrt maps NaN to sqrt(lo) (fmaxf returns the other operand) where torch.clamp keeps NaN."""
import ctypes
import ctypes.util
import math

import numpy as np
import torch

import ew_ref as er
import heads_audit as ha

f32, f64 = np.float32, np.float64
F64 = torch.float64
U32 = 2.0 ** -24
TINY = 2.0 ** -150
gam = er.gam
Ratios = er.Ratios

ADAM_TRIP = 4096 * 1024          # elements one grid-stride trip covers: adam_kernel, adam_dev_kernel, amp_unscale_check_kernel
EW_TRIP = 4096 * 256             # sgd_scaled_kernel, clamp_sqrt_kernel
SCALE_TRIP = 1024 * 256          # amp_scale_kernel
# relative error of the fp32 powf behind the bias corrections, in units of u: twice the largest value the measured corrections
# imply (device 0.435, from bc2s at step 20, over steps 1..64, 100, 500, 1000, 2000, 5000, 10000, 20000; host libm 0.222;
# profiles/opt_edges.md) -- neither math library ships a documented ulp bound with the toolchain.  One factor of two for the
# inputs not tried.
K_POW = 0.87


def n32(a):
    return np.ascontiguousarray(np.asarray(a, f32))


def as64(a):
    return np.asarray(a, f32).astype(f64)


def fma32(a, b, c):
    """fmaf emulated as the float64 product-plus-addend rounded to fp32 (differs from a real fma only within 2^-29 ulp of a tie)"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


# ------------------------------------------------------------------------------------------------ bias corrections
_libm = None


def powf32(b, t):
    """the host's powf(float, float): what creid_adam_step calls, and the stand-in for the device's in the fp32 model"""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.powf.restype, _libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    return f32(_libm.powf(float(f32(b)), float(f32(t))))


def bias_corr32(b1, b2, t):
    """(bc1, bc2s) as the kernels and creid_adam_step compute them: 1.0f - powf(b1, t), sqrtf(1.0f - powf(b2, t))"""
    return f32(1) - powf32(b1, t), np.sqrt(f32(1) - powf32(b2, t))


def bias_corr64(b1, b2, t):
    b1, b2 = float(f32(b1)), float(f32(b2))
    return 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)


def pow_bar(b, t, k_pow=None):
    """relative bound on 1.0f - powf(b, t): (k_pow u b^t + u) / (1 - b^t); TINY for a power that underflows"""
    k_pow = K_POW if k_pow is None else k_pow
    b = float(f32(b))
    return (k_pow * U32 * b ** t + U32 + TINY) / (1.0 - b ** t)


def bc_bars(b1, b2, t, k_pow=None):
    """relative bounds on (bc1, bc2s); the root halves the error (sqrt(1 +- r) within r / 2 (1 + r)) and rounds once more"""
    r1, r2 = pow_bar(b1, t, k_pow), pow_bar(b2, t, k_pow)
    return r1, 0.5 * r2 * (1 + r2) + U32 * (1 + r2)


def implied_k_pow(got, b, t, root=False):
    """the smallest k_pow under which pow_bar admits the correction `got` (bc1, or bc2s with root=True)"""
    b = float(f32(b))
    bc = 1.0 - b ** t
    ref = math.sqrt(bc) if root else bc
    rel = abs(float(got) - ref) / ref
    if root:
        rel = max(0.0, 2.0 * (rel - U32))
    if b ** t < 1e-40:
        return 0.0
    return max(0.0, (rel * bc - U32 * bc) / (U32 * b ** t))


def check_bias_corr(R, fam, what, bc1, bc2s, b1, b2, t):
    r1, r2 = bias_corr64(b1, b2, t)
    q1, q2 = bc_bars(b1, b2, t)
    R.check(fam, f"{what}: bc1 at step {t}", [float(bc1)], [r1], [q1 * r1])
    R.check(fam, f"{what}: bc2s at step {t}", [float(bc2s)], [r2], [q2 * r2])


# ------------------------------------------------------------------------------------------------ Adam: float64 and bounds
def hyper_params(lr=3.5e-5, b1=0.9, b2=0.999, eps=1e-8, wd=5e-4, gscale=1.0):
    """the scalars as the ABI receives them: fp32 values, held as Python floats"""
    return {k: float(f32(v)) for k, v in dict(lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, gscale=gscale).items()}


def adam64(p, g, m, v, hp, bc1, bc2s):
    """One step in float64 on the fp32 operands, and the bounds on the kernel's fp32 evaluation of it:
         t  = fl(g gscale); gg = fma(wd, p, t)                      2 roundings on mag = |wd p| + |g gscale|
         m' = fl(fl(b1 m) + fl(fl(1 - b1) gg))                      |dm| <= gam(5) (|b1 m| + (1 - b1) mag)        (= gam(5) |m'| without cancellation)
         v' = fl(fl(b2 v) + fl(fl(fl(1 - b2) gg) gg))               |dv| <= gam(8) (b2 v + (1 - b2) mag^2)        (= gam(8) v')
         den = fl(fl(sqrtf(v') / bc2s) + eps)                        d sqrt <= min(dv / sqrt(v'), sqrt(dv)); three more roundings
         p' = fl(p - fl(fl(lr / bc1) fl(m' / den)))                  |dp| <= u |p'| + |D| (d den / den + gam(3)) + ss dm / den
       with D = ss m' / den the update: the bar on p scales with the update, not with p.  TINY per operation that can underflow."""
    p, g, m, v = as64(p), as64(g), as64(m), as64(v)
    lr, b1, b2, eps, wd, gs = (hp[k] for k in ("lr", "b1", "b2", "eps", "wd", "gscale"))
    bc1, bc2s = float(bc1), float(bc2s)
    t = g * gs
    gg = wd * p + t
    mag = np.abs(wd * p) + np.abs(t)
    m2 = b1 * m + (1 - b1) * gg
    v2 = b2 * v + (1 - b2) * gg * gg
    bm = gam(5) * (np.abs(b1 * m) + (1 - b1) * mag) + 2 * TINY
    bv = gam(8) * (b2 * v + (1 - b2) * mag * mag) + 3 * TINY
    root = np.sqrt(v2)
    den = root / bc2s + eps
    ss = lr / bc1
    delta = ss * m2 / den
    dsq = np.minimum(bv / np.maximum(root, 1e-300), np.sqrt(bv))
    dden = dsq / bc2s * (1 + gam(2)) + gam(3) * den
    lo = np.maximum(den - dden, eps * (1 - U32))      # (the device's denominator is never below fl(0 + eps): a root is not negative;
    #                                                    where wd p and g gscale cancel, dv is large against v' and den - dden is not)
    bdelta = np.abs(delta) * (dden / lo) + ss * bm / lo * (1 + gam(3)) + gam(3) * np.abs(delta) + TINY
    p2 = p - delta
    return dict(p=p2, m=m2, v=v2, delta=delta, bp=bdelta + U32 * (np.abs(p2) + bdelta) + TINY, bm=bm, bv=bv)


def check_adam(R, fam, what, inp, hp, bc1, bc2s, dev):
    """dev: p, m, v after the step; inp: (p, g, m, v) before it; bc1 / bc2s: the corrections the step used"""
    ref = adam64(*inp, hp, bc1, bc2s)
    R.check(fam + "_m", f"{what}: m", dev["m"], ref["m"], ref["bm"])
    R.check(fam + "_v", f"{what}: v", dev["v"], ref["v"], ref["bv"])
    R.check(fam + "_p", f"{what}: p", dev["p"], ref["p"], ref["bp"])
    R.count(fam)


# ------------------------------------------------------------------------------------------------ Adam: the fp32 model
def adam_blocks(n, cap_blocks=4096):
    return max(1, min((n // 4 + 255) // 256, cap_blocks))


def adam_model(p, g, m, v, hp, bc1, bc2s, host=False, cap_blocks=4096, mut=None):
    """adam_kernel (host=True: float4 body plus a scalar tail) / adam_dev_kernel (n % 4 == 0) in numpy fp32, operation by
    operation, on a grid of at most cap_blocks workgroups of 256 threads x float4.  mut: one injected fault (MUTANTS)."""
    p, g, m, v = (n32(a).copy() for a in (p, g, m, v))
    n = p.size
    full = n // 4 * 4
    trip = adam_blocks(n, cap_blocks) * 1024
    todo = np.zeros(n, bool)
    todo[:full] = True
    if mut == "second trip skipped":
        todo[trip:] = False
    if host and mut != "scalar tail skipped" and not (mut == "second trip skipped" and full >= trip):
        todo[full:] = True
    lr, b1, b2, eps, wd, gs = (f32(hp[k]) for k in ("lr", "b1", "b2", "eps", "wd", "gscale"))
    bc1, bc2s = f32(bc1), f32(bc2s)
    vin = v
    if mut == "lane k reads lane k+1's v":
        vin = v.copy()
        vin[:full] = np.roll(v[:full].reshape(-1, 4), -1, axis=1).reshape(-1)
    with np.errstate(all="ignore"):
        if mut == "weight decay dropped":
            gg = g * gs
        elif mut == "gscale applied after the decay":
            gg = fma32(wd, p, g) * gs
        else:
            gg = fma32(wd, p, g * gs)
        m2 = b1 * m + (f32(1) - b1) * gg
        v2 = b2 * vin + (f32(1) - b2) * gg * gg
        if mut == "bc2 used without the square root":
            bc2s = bc2s * bc2s
        den = np.sqrt(v2 + eps) / bc2s if mut == "eps added inside the square root" else np.sqrt(v2) / bc2s + eps
        p2 = p - (lr / bc1) * (m2 / den)
    if mut == "m left un-updated":
        m2 = m
    return dict(p=np.where(todo, p2, p).astype(f32), m=np.where(todo, m2, m).astype(f32), v=np.where(todo, v2, v).astype(f32))


def adam_dev_model(p, g, m, v, hyper, hp, skip=None, cap_blocks=4096, mut=None):
    """creid_adam_step_dev(_amp): the step counter and the corrections live in `hyper` (float[8]: lr, step, bc1, bc2s, ticket);
    a set skip flag leaves everything as it is, the counter included.  Returns (dev dict, hyper after the call)."""
    hyper = n32(hyper).copy()
    if skip:
        return dict(p=n32(p).copy(), m=n32(m).copy(), v=n32(v).copy()), hyper
    step = hyper[1] + f32(1)
    bc1, bc2s = bias_corr32(hp["b1"], hp["b2"], step)
    if mut == "bc1 taken at step - 1":
        bc1 = f32(1) - powf32(hp["b1"], step - f32(1))
    out = adam_model(p, g, m, v, dict(hp, lr=float(hyper[0])), bc1, bc2s, cap_blocks=cap_blocks, mut=mut) if n32(p).size else \
        dict(p=n32(p).copy(), m=n32(m).copy(), v=n32(v).copy())
    hyper[1:4] = (step, bc1, bc2s)
    return out, hyper


def judge_adam_dev(R, fam, what, inp, hp, hyper0, dev, hyper1):
    """One creid_adam_step_dev(_amp) call that was not skipped: the counter advanced by one, lr and the three spare floats
    untouched, the ticket back at int32 0, the published corrections within pow_bar of float64 (layer 1), p / m / v within their
    bounds of the float64 step evaluated with the published corrections (layer 2)."""
    h0, h1 = n32(hyper0), n32(hyper1)
    t = int(h0[1]) + 1
    assert float(h1[1]) == t, f"{what}: hyper[1] {float(h0[1])} -> {float(h1[1])}, expected {t}"
    assert h1.view(np.int32)[4] == 0, f"{what}: the ticket in hyper[4] is {int(h1.view(np.int32)[4])}, not 0"
    assert same_bits(h1[[0, 5, 6, 7]], h0[[0, 5, 6, 7]]), f"{what}: hyper[0] / hyper[5..7] changed"
    check_bias_corr(R, fam + "_bc", what, h1[2], h1[3], hp["b1"], hp["b2"], t)
    if n32(inp[0]).size:
        check_adam(R, fam, what, inp, dict(hp, lr=float(h0[0])), h1[2], h1[3], dev)


# ------------------------------------------------------------------------------------------------ SGD, the loss scaler
def sgd_expect(p, g, lr, gmul):
    """sgd_scaled_kernel: (p', g') bit for bit"""
    g2 = n32(g) * f32(gmul)
    return n32(p) - f32(lr) * g2, g2


def scale_expect(x, s):
    return n32(x) * f32(s)


def clamp_sqrt_expect(d, lo):
    return np.sqrt(np.maximum(n32(d), f32(lo)))


def unscale_model(g, inv, cap_blocks=4096, mut=None):
    """amp_unscale_check_kernel: (g', raised) -- g' = fl(g inv) over every float4, `raised` iff any element of g' is not finite"""
    g = n32(g)
    n = g.size
    assert n % 4 == 0
    with np.errstate(all="ignore"):
        out = g * f32(inv)
    seen = np.ones(n, bool)
    if mut == "second trip skipped":
        seen[adam_blocks(n, cap_blocks) * 1024:] = False
        out = np.where(seen, out, g)
    if mut == "blind to the last float4":
        seen[n - 4:] = False
    if mut == "blind to NaN":
        bad = np.isinf(out)
    elif mut == "blind to -inf":
        bad = np.isnan(out) | (out == np.inf)
    else:
        bad = ~np.isfinite(out)
    return out.astype(f32), bool((bad & seen).any())


def same_bits(a, b):
    a, b = n32(a), n32(b)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def exact_bits(R, fam, what, got, want):
    """bit for bit, the sign of zero included (Ratios.exact compares values: -0.0 == 0.0 there)"""
    got, want = n32(got), n32(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    R.worst.setdefault(fam, 0.0)
    if bad.any():
        i = int(np.nonzero(bad.reshape(-1))[0][0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ in their bits; first at flat index {i}: got "
                             f"{float(got.reshape(-1)[i])!r}, expected {float(want.reshape(-1)[i])!r}")


def sensitive_past(cap, n, *arrays):
    """the elements from index `cap` on (reached in the second grid-stride trip only) get values of order 1: a kernel that
    skipped the trip could not leave them right by leaving them alone"""
    for k, a in enumerate(arrays):
        if n > cap:
            a[cap:] = (f32(1.5) + f32(0.25) * np.arange(n - cap, dtype=f32)) * f32(-1 if k % 2 else 1)


def check_unscale(what, g, inv, flags0, dev_g, dev_flags):
    """The unscaled buffer bit for bit (a NaN stays a NaN, whichever), bit 0 of flags[0] raised iff a result is not finite and
    never cleared, flags[1] and flags[2] untouched."""
    want, raised = unscale_model(g, inv)
    got = n32(dev_g)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
    diff = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not diff.any(), f"{what}: {int(diff.sum())} of {got.size} elements are not fl(g * inv); first at {int(np.nonzero(diff)[0][0])}"
    f0, f1 = [int(x) for x in flags0], [int(x) for x in dev_flags]
    assert f1 == [f0[0] | int(raised), f0[1], f0[2]], f"{what}: flags {f0} -> {f1}, non-finite present: {raised}"


def amp_update_model(state, flags, growth, backoff, interval, mut=None):
    """amp_update_kernel as plain Python: (state', flags').  state = {scale, 1 / scale}; flags = {found_inf, clean steps in a
    row, steps skipped in total}"""
    s = f32(state[0])
    f = [int(x) for x in flags]
    if f[0]:
        s = f32(s * f32(backoff))
        if mut != "flags[1] not reset on overflow":
            f[1] = 0
        f[2] += 1
    else:
        f[1] += 1
        if f[1] >= interval:
            s = f32(s * f32(growth))
            f[1] = 0
    if mut != "no clamp":
        s = f32(min(max(s, f32(1)), f32(16777216.0)))
    return [s, f32(1) / s], [0, f[1], f[2]]


# (name, scale0, flags0, growth, backoff, interval, found_inf per call)
AMP_SEQUENCES = [
    ("overflow at scale 1: stays 1, the skip count rises", 1.0, [0, 0, 5], 2.0, 0.5, 2000, [1, 1, 0, 1]),
    ("growth at 2^24: stays 2^24", 16777216.0, [0, 0, 0], 2.0, 0.5, 2, [0, 0, 0, 0]),
    ("interval 1: grows at every clean call", 1024.0, [0, 0, 0], 2.0, 0.5, 1, [0, 0, 1, 0]),
    ("an overflow one short of growth resets the tracker", 65536.0, [0, 0, 0], 2.0, 0.5, 3, [0, 0, 1, 0, 0, 0]),
    ("backoff 0.3: 1 / scale is a real rounding", 65536.0, [0, 7, 0], 2.0, 0.3, 2000, [1, 1, 0, 1, 1]),
    ("growth 1.7 from a tracker restored one short", 1000.0, [0, 1999, 2], 1.7, 0.3, 2000, [0, 0, 1]),
]


def run_amp_sequence(seq, update):
    """Walk one AMP_SEQUENCES row: `update(state, flags, growth, backoff, interval)` -> (state', flags') is the implementation
    under test; every call must leave what amp_update_model leaves and state[1] == fl(1 / state[0])."""
    name, s0, flags, growth, backoff, interval, found = seq
    state = [f32(s0), f32(1) / f32(s0)]
    flags = list(flags)
    for i, fi in enumerate(found):
        flags[0] = fi
        want_s, want_f = amp_update_model(state, flags, growth, backoff, interval)
        got_s, got_f = update(state, flags, growth, backoff, interval)
        got_s, got_f = [f32(x) for x in got_s], [int(x) for x in got_f]
        assert got_s[0] == want_s[0] and got_f == want_f, f"{name}: call {i}: got {got_s} {got_f}, want {want_s} {want_f}"
        assert got_s[1] == f32(1) / got_s[0], f"{name}: call {i}: state[1] {got_s[1]!r} is not fl(1 / {got_s[0]!r})"
        state, flags = got_s, got_f


# ------------------------------------------------------------------------------------------------ generators
def wild(n, seed, nonneg=False):
    """magnitudes log-uniform over 1e-20 .. 1e3 (the squares of the lower third underflow, gradually or to zero), random signs,
    one element in sixteen an exact zero"""
    rng = np.random.default_rng(seed)
    x = (10.0 ** rng.uniform(-20.0, 3.0, n)).astype(f32)
    if not nonneg:
        x *= np.where(rng.random(n) < 0.5, f32(-1), f32(1))
    x[rng.random(n) < 1.0 / 16] = 0
    return x


def adam_inputs(n, seed):
    """(p, g, m, v): one half of the elements like a network's (p ~ N(0, 1), g, m ~ 1e-2 N(0, 1), v ~ 1e-4 chi^2), the other half
    wild(); the first float4 is p = g = m = v = 0 and the second p != 0, g = m = v = 0"""
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)

    def randn():
        return torch.randn(n, generator=gen, dtype=torch.float32).numpy()
    net = rng.random(n) < 0.5
    p = np.where(net, randn(), wild(n, seed + 1))
    g = np.where(net, f32(1e-2) * randn(), wild(n, seed + 2))
    m = np.where(net, f32(1e-2) * randn(), wild(n, seed + 3))
    v = np.where(net, f32(1e-4) * randn() ** 2, wild(n, seed + 4, nonneg=True))
    for a in (p, g, m, v):
        a[:min(n, 4)] = 0
    for a in (g, m, v):
        a[4:min(n, 8)] = 0
    return tuple(n32(a) for a in (p, g, m, v))


def finite_gradients(n, seed):
    """all-finite gradients for the unscale-and-check kernel, +-3e38 and zeros among them"""
    g = wild(n, seed)
    if n >= 8:
        g[1], g[n - 2] = 3e38, -3e38
    return g


NONFINITE = (np.inf, -np.inf, np.nan)


# ------------------------------------------------------------------------------------------------ per-segment row means
def gather_mean_expect(emb, order, offsets):
    """gather_mean_rows_kernel bit for bit: per segment a sequential fp32 sum of the listed rows, then one division"""
    emb = n32(emb)
    out = np.zeros((len(offsets) - 1, emb.shape[1]), f32)
    for s in range(len(offsets) - 1):
        acc = np.zeros(emb.shape[1], f32)
        for j in range(int(offsets[s]), int(offsets[s + 1])):
            acc = acc + emb[int(order[j])]
        out[s] = acc / f32(int(offsets[s + 1]) - int(offsets[s]))
    return out


def gather_inputs(D, seed, lengths=(1, 2, 7, 300)):
    """emb [320, D]; segments of the given lengths over a non-monotone order in which row 5 is used by the first two segments
    that are long enough"""
    rng = np.random.default_rng(seed)
    rows = 320
    emb = rng.standard_normal((rows, D)).astype(f32) * f32(3) + f32(0.5)
    order, offsets, used = [], [0], 0
    for ln in lengths:
        seg = rng.permutation(rows)[:ln]
        if ln >= 2 and used < 2:
            seg[ln // 2] = 5
            used += 1
        order += [int(r) for r in seg]
        offsets.append(len(order))
    return emb, np.asarray(order, np.int64), np.asarray(offsets, np.int64)


# ------------------------------------------------------------------------------------------------ row normalisation
def t64(a):
    return er.t64(a)


def rownorm64(x, mode, eps):
    """y = x / clamp(|x|, min=eps) (mode 0) or x / (|x| + eps) (mode 1); returns (y, norm) in float64; differentiable"""
    x = t64(x)
    n = torch.linalg.vector_norm(x, dim=1)
    den = n.clamp(min=eps) if mode == 0 else n + eps
    return x / den[:, None], n


def chain256(D):
    """roundings of a block_sum_256 reduction over D terms: a thread's fma chain of ceil(D / 256), six levels of the wave sum,
    two of the four-wave sum"""
    return math.ceil(D / 256) + 8


def rownorm_norm_bound(x):
    """|norm_d - norm|: the sum of squares is off by gam(chain) S + D TINY (squares that underflow), the root by
    min(dS / sqrt(S), sqrt(dS)) and its own rounding"""
    x = t64(x)
    D = x.shape[1]
    S = (x * x).sum(1)
    dS = gam(chain256(D)) * S + D * TINY
    return torch.minimum(dS / torch.sqrt(S).clamp_min(1e-300), torch.sqrt(dS)) + U32 * torch.sqrt(S) + TINY


def rownorm_y_with(x, norm_d, mode, eps):
    """y with the DEVICE'S norm and the bound of the remaining roundings: one division (mode 0: max is exact), the add and the
    division (mode 1)"""
    x, nd = t64(x), t64(norm_d)
    den = torch.clamp(nd, min=eps) if mode == 0 else nd + eps
    y = x / den[:, None]
    return y, gam(1 if mode == 0 else 2) * y.abs() + TINY


def rownorm_bwd_with(x, norm_d, dy, mode, eps):
    """rownorm_bwd_kernel's closed form in float64 on the operands it reads (x, the stored norm, dy), dx = a dy - b x:
         mode 0: n > eps: a = 1 / n, b = (x.dy) / n^3;  else a = 1 / eps, b = 0           (the clamp passes no gradient)
         mode 1: a = 1 / (n + eps), b = (x.dy) / (n (n + eps)^2) for n > 0, else 0
       x.dy is a block_sum_256 reduction; a carries up to two roundings, b up to six on top of the dot's error; the two products
       and the subtraction add one each."""
    x, nd, dy = t64(x), t64(norm_d), t64(dy)
    D = x.shape[1]
    xg = (x * dy).sum(1)
    dxg = gam(chain256(D)) * (x * dy).abs().sum(1) + D * TINY
    if mode == 0:
        big = nd > eps
        a = torch.where(big, 1.0 / nd.clamp_min(1e-300), torch.full_like(nd, 1.0 / eps))
        k = torch.where(big, 1.0 / nd.clamp_min(1e-300) ** 3, torch.zeros_like(nd))
    else:
        den = nd + eps
        a = 1.0 / den
        k = torch.where(nd > 0, 1.0 / (nd.clamp_min(1e-300) * den * den), torch.zeros_like(nd))
    b = xg * k
    dx = a[:, None] * dy - b[:, None] * x
    bound = gam(4) * (a[:, None] * dy).abs() + ((gam(8) * b.abs() + dxg * k * (1 + gam(8)))[:, None]) * x.abs() + 3 * TINY
    return dx, bound


def rownorm_inputs(N, D, seed):
    """Rows of prescribed norms: 1, 30, a norm between the two eps of the sweep (2e-4: above 1e-12, below 1e-3), an exact zero
    row, a row of elements ~2e-23 whose squares underflow (to zero or to a few subnormal ulps).  N = 1 keeps the first only."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((5, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x *= np.array([1.0, 30.0, 2e-4, 0.0, 1.0])[:, None]
    x[4] = 2e-23 * rng.standard_normal(D)
    dy = rng.standard_normal((5, D))
    return n32(x[:N]), n32(dy[:N])


def check_rownorm(R, fam, x, dy, mode, eps, dev):
    """dev: y, norm, dx.  norm against float64; y and dx against float64 WITH the device's norm."""
    eps = float(f32(eps))
    _, n = rownorm64(x, mode, eps)
    R.check(fam + "_norm", f"norm (mode {mode}, eps {eps:g})", dev["norm"], n, rownorm_norm_bound(x))
    y, by = rownorm_y_with(x, dev["norm"], mode, eps)
    R.check(fam + "_y", f"y (mode {mode}, eps {eps:g})", dev["y"], y, by)
    dx, bdx = rownorm_bwd_with(x, dev["norm"], dy, mode, eps)
    R.check(fam + "_dx", f"dx (mode {mode}, eps {eps:g})", dev["dx"], dx, bdx)
    R.count(fam)


def rownorm_model(x, dy, mode, eps, b_order="fixed"):
    """rownorm_fwd_kernel + rownorm_bwd_kernel in numpy fp32 (sums in float64 rounded once: the bounds allow far more).
    b_order='n*den*den': mode 1's b as it was written before the product n (n + eps)^2 was taken apart -- it underflows to
    zero for a norm below ~7e-22 (eps = 1e-12) and b becomes +-inf."""
    x, dy, eps = n32(x), n32(dy), f32(eps)
    with np.errstate(all="ignore"):
        n = np.sqrt((x.astype(f64) ** 2).sum(1).astype(f32))
        den = np.maximum(n, eps) if mode == 0 else n + eps
        y = x / den[:, None]
        xg = (x.astype(f64) * dy.astype(f64)).sum(1).astype(f32)
        if mode == 0:
            a = np.where(n > eps, f32(1) / n, f32(1) / eps)
            b = np.where(n > eps, xg / (n * n * n), f32(0))
        else:
            a = f32(1) / den
            b = np.where(n > 0, xg / (n * den * den) if b_order == "n*den*den" else (xg / n) / (den * den), f32(0))
        dx = a[:, None] * dy - b[:, None] * x
    return dict(y=y.astype(f32), norm=n.astype(f32), dx=dx.astype(f32))


# ------------------------------------------------------------------------------------------------ mining on a given matrix
def mine_expect(dist, labels):
    """hard_example_mining with first-index ties: (dist_ap, dist_an, p_idx, n_idx); the values are copies of matrix entries"""
    dist, labels = n32(dist), np.asarray(labels)
    N = dist.shape[0]
    same = labels[:, None] == labels[None]
    assert bool((~same).any(1).all()), "an anchor without a negative: out of scope (the reference raises)"
    dp = np.where(same, dist, -np.inf)
    dn = np.where(same, np.inf, dist)
    pi, ni = dp.argmax(1), dn.argmin(1)                        # numpy returns the first of equal extrema
    r = np.arange(N)
    return dist[r, pi], dist[r, ni], pi.astype(np.int32), ni.astype(np.int32)


def mine_inputs(N, seed, levels=4):
    """integer-valued distances 0 .. levels - 1 (most rows tie), identities of three rows each (two for N = 2: every row keeps a
    negative)"""
    rng = np.random.default_rng(seed)
    dist = rng.integers(0, levels, (N, N)).astype(f32)
    labels = (np.arange(N) // 3 if N > 3 else np.arange(N) % 2) * 7 % 1000
    return dist, rng.permutation(labels.astype(np.int64)) if N > 3 else labels.astype(np.int64)


# ------------------------------------------------------------------------------------------------ the cosine triplet
def unit_inputs(N, D, seed):
    """Raw rows for creid_rownorm_fwd (mode 0) whose unit images exercise the kinks of |1 - u.v|: row 1 a bit-copy of row 0
    (generic: its dot product with row 0 rounds to, above or below 1), row 2 = -row 0 (antipodal), row 3 the first unit vector
    (u.u == 1 exactly: the clamp is active, no gradient); the rest clustered by identity.  Labels: identities of two or three
    consecutive rows, rows 0 / 1 / 2 share one."""
    rng = np.random.default_rng(seed)
    ident = np.arange(N) // 3 if N > 4 else np.arange(N) // 2
    ident[:min(N, 3)] = 0
    centre = rng.standard_normal((int(ident.max()) + 1, D))
    x = centre[ident] + 0.7 * rng.standard_normal((N, D))
    x = n32(x)
    x[1] = x[0]
    x[2] = -x[0]
    x[3] = 0
    x[3, 0] = 2.5
    if N > 4:
        ident[3] = ident[4]
    labels = (ident * 5 + 11).astype(np.int64)
    assert len(np.unique(labels)) >= 2
    return x, labels


def cos_forward_check(R, fam, xu, labels, mask, margin, dev):
    """dev: dist_mat [N, N], dist_ap, dist_an, p_idx, n_idx, coef [N], out4.  xu: the unit rows the kernel read (fp32).
    dist_mat against float64 within ha.cos_dist_bound; mined indices inside the decision windows of ha.mine64 (equal to the
    float64 first index where decided); dist_ap / dist_an bit-copies of dist_mat at the mined indices; the loss, the means and
    coef against float64 ON THE DEVICE'S OWN dist_ap / dist_an (hinge: coef is 0 or fl(1 / n) exactly, decided by the sign of
    ap - an + margin unless that lies within its two roundings)."""
    margin = float(f32(margin))                              # the kernel receives the margin as fp32
    x = t64(xu)
    N = x.shape[0]
    lab = torch.as_tensor(np.asarray(labels))
    d = ha.cos_dist64(x)
    b = ha.cos_dist_bound(x, d)
    R.check(fam + "_dist", "dist_mat", dev["dist_mat"], d, b)
    mn = ha.mine64(d, b, lab, torch.ones(N, dtype=torch.bool), ha.row_classes(t64(xu)), max(margin, 0.0))
    dm = n32(dev["dist_mat"])
    r = np.arange(N)
    for key, idx in (("p", dev["p_idx"]), ("n", dev["n_idx"])):
        idx = np.asarray(idx).astype(np.int64)
        assert ((idx >= 0) & (idx < N)).all(), f"{key}_idx out of range"
        win, dec, first = mn[key + "_win"].numpy(), mn[key + "_dec"].numpy(), mn[key + "_idx"].numpy()
        assert win[r, idx].all(), f"{key}_idx outside the decision window at anchors {np.nonzero(~win[r, idx])[0]}"
        # a decided anchor: the window is one row or bit-identical rows (bit-equal distances): the FIRST of them, which is the
        # float64 first index
        first_in_win = np.where(win, r[None], N).min(1)
        assert (first_in_win[dec] == first[dec]).all()
        bad = dec & (idx != first_in_win)
        assert not bad.any(), f"{key}_idx differs from the first index at decided anchors {np.nonzero(bad)[0]}"
        got = n32(dev["dist_a" + key])
        assert same_bits(got, dm[r, idx]), f"dist_a{key} is not a copy of dist_mat[a, {key}_idx[a]]"
    ap, an = as64(dev["dist_ap"]), as64(dev["dist_an"])
    on = np.ones(N, bool) if mask is None else np.asarray(mask).astype(bool)
    nm = int(on.sum())
    out4, coef = as64(dev["out4"]), n32(dev["coef"])
    assert out4[3] == nm, ("anchor count", out4[3], nm)
    srnd = gam(math.ceil(N / 256) + 9)
    R.check(fam + "_loss", "mean dist_ap", [out4[1]], [ap[on].sum() / nm], [srnd * ap[on].sum() / nm + TINY])
    R.check(fam + "_loss", "mean dist_an", [out4[2]], [an[on].sum() / nm], [srnd * an[on].sum() / nm + TINY])
    z = ap - an
    if margin >= 0:
        v = z + margin
        slack = gam(2) * (np.abs(z) + margin)
        inv = f32(1) / f32(nm)
        want = np.where(on & (v > 0), inv, f32(0)).astype(f32)
        und = on & (np.abs(v) <= slack)
        ok = (coef == want) | (und & ((coef == 0) | (coef == inv)))
        assert ok.all(), f"coef differs at anchors {np.nonzero(~ok)[0]}"
        act = on & (coef != 0)
        loss = v[act].sum() / nm
        R.check(fam + "_loss", "hinge loss", [out4[0]], [loss], [(srnd + gam(2)) * np.abs(v[act]).sum() / nm + slack[und].sum() / nm + TINY])
    else:
        # log(1 + exp(z)) through log1pf / expf, the logistic coefficient through expf and two divisions.  gam(8) per term ASSUMES
        # at most ~3 ulp from each of the two library calls: no ulp bound of the device's math library is documented or was
        # measured per function (unlike powf); what was measured is the whole expression, 0.29 of this bar at worst
        t = np.logaddexp(0.0, z)
        R.check(fam + "_loss", "soft-margin loss", [out4[0]], [t[on].sum() / nm], [(srnd + gam(8)) * t[on].sum() / nm + TINY])
        want = np.where(on, 1.0 / (1.0 + np.exp(-z)) / nm, 0.0)
        R.check(fam + "_loss", "soft-margin coef", coef, want, gam(8) * np.abs(want) + TINY)
        assert (coef[~on] == 0).all()
    R.count(fam)


def cos_backward_check(R, fam, xu, dev, g, dx0, dev_dx):
    """dx_accum = dx0 + g * gradient, the gradient from ha.triplet_cos_bwd64 on the kernel's own (dist_ap, dist_an, p_idx,
    n_idx, coef); the accumulating add rounds once more"""
    dx, bound = ha.triplet_cos_bwd64(t64(xu), n32(dev["dist_ap"]), n32(dev["dist_an"]), np.asarray(dev["p_idx"]),
                                     np.asarray(dev["n_idx"]), n32(dev["coef"]), float(g))
    ref = t64(dx0) + dx
    R.check(fam + "_dx", "dx", dev_dx, ref, bound + U32 * (ref.abs() + bound) + TINY)
    R.count(fam)


def wave_dot32(u, v):
    """u.v exactly as triplet_mine_body forms it, in its own order: lane l takes the float4 at 4 l, 4 l + 256, ... with four
    sequential fma each, then the six xor-butterfly levels of wave_sum (every lane ends with the same bits).  fp32 [D], D % 4 == 0.
    (fma32's caveat applies: a tie within 2^-29 ulp would round the other way.)"""
    u, v = n32(u), n32(v)
    D = u.size
    chunks = -(-D // 256)
    up, vp = np.zeros(chunks * 256, f32), np.zeros(chunks * 256, f32)
    up[:D], vp[:D] = u, v
    up, vp = up.reshape(chunks, 64, 4), vp.reshape(chunks, 64, 4)
    live = (np.arange(chunks * 256).reshape(chunks, 64, 4)[:, :, 0] < D)
    acc = np.zeros(64, f32)
    for c in range(chunks):
        for k in range(4):
            acc = np.where(live[c], fma32(up[c, :, k], vp[c, :, k], acc), acc)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[lane ^ o]).astype(f32)
    return acc[0]


def cos_dist32(u, v):
    """the fp32 cosine distance of the kernel for one pair, bit for bit: (dot, max(|1 - dot|, 1e-12))"""
    dot = wave_dot32(u, v)
    return dot, np.maximum(np.abs(f32(1) - dot), f32(1e-12))


def cos_model(xu, labels, mask, margin, g, dx0, flip_ties=False):
    """The cosine triplet's forward and backward in numpy fp32 (dot products as fp32 matrix products: another summation order
    than the kernel's, inside the same bounds).  flip_ties: the LAST index of equal extrema -- the fault the windows must see."""
    xu = n32(xu)
    N = xu.shape[0]
    labels = np.asarray(labels)
    dot = xu @ xu.T
    dm = np.maximum(np.abs(f32(1) - dot), f32(1e-12)).astype(f32)
    same = labels[:, None] == labels[None]
    dp, dn = np.where(same, dm, -np.inf), np.where(same, np.inf, dm)
    if flip_ties:
        pi, ni = N - 1 - dp[:, ::-1].argmax(1), N - 1 - dn[:, ::-1].argmin(1)
    else:
        pi, ni = dp.argmax(1), dn.argmin(1)
    r = np.arange(N)
    ap, an = dm[r, pi], dm[r, ni]
    on = np.ones(N, bool) if mask is None else np.asarray(mask).astype(bool)
    nm = f32(on.sum())
    z = ap - an
    if margin >= 0:
        v = z + f32(margin)
        coef = np.where(on & (v > 0), f32(1) / nm, f32(0)).astype(f32)
        loss = f32(v[on & (v > 0)].sum() / nm)
    else:
        coef = np.where(on, (f32(1) / (f32(1) + np.exp(-z))) / nm, f32(0)).astype(f32)
        loss = f32(np.logaddexp(f32(0), z)[on].sum() / nm)
    out4 = np.array([loss, ap[on].sum() / nm, an[on].sum() / nm, nm], f32)
    acc = np.zeros_like(xu)
    for a in range(N):
        if coef[a] == 0:
            continue
        for o, dist, w in ((pi[a], ap[a], -coef[a]), (ni[a], an[a], coef[a])):
            if not dist > f32(1e-12):
                continue
            s = np.sign(f32(1) - f32(xu[a] @ xu[o]))
            acc[a] += w * s * xu[o]
            acc[o] += w * s * xu[a]
    return dict(dist_mat=dm, dist_ap=ap, dist_an=an, p_idx=pi.astype(np.int32), n_idx=ni.astype(np.int32), coef=coef, out4=out4), \
        (n32(dx0) + f32(g) * acc).astype(f32)


# ------------------------------------------------------------------------------------------------ the sizes of the sweep
DEV_SIZES = [0, 4, 1020, 1024, 1028, ADAM_TRIP + 4]                       # n % 4 == 0; the last: one float4 into the second trip
HOST_SIZES = [0, 1, 3, 5, 1025, 1026, 1027, ADAM_TRIP + 1029]             # the last: one workgroup's float4 and a scalar tail, both in trip two
EW_SIZES = [1, 255, 256, 257]                                             # plus one element past each kernel's own cap
PRESET_STEPS = [0, 1, 9, 999, 19999]                                      # hyper[1] before the step, as load_state_dict leaves it

MUTANTS_ADAM = ["bc1 taken at step - 1", "bc2 used without the square root", "weight decay dropped", "gscale applied after the decay",
                "eps added inside the square root", "m left un-updated", "lane k reads lane k+1's v", "second trip skipped",
                "scalar tail skipped"]
MUTANTS_CHECK = ["blind to NaN", "blind to -inf", "blind to the last float4", "second trip skipped"]
MUTANTS_UPDATE = ["flags[1] not reset on overflow", "no clamp"]
