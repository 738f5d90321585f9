"""Reference for generalized-mean pooling with a trainable exponent (creid_gem_fwd / creid_gem_bwd), written from the definition:

    u = max(x, eps),   m = (1/HW) sum_i u_i^p,   y = m^(1/p)                         x [B, HW, C], y [B, C]
    dx_i = dy (1/HW) m^(1/p - 1) u_i^(p - 1)   where x_i >= eps, a true zero below    (the gradient of clamp(min = eps))
    dp   = sum_{b,c} dy y ((sum_i u_i^p ln u_i) / (HW m p) - ln(m) / p^2)

`*_f64`: the definition in float64 (eps^8 = 1e-48 and 65504^8 = 3.4e38 are ordinary doubles: no scaling needed there).
`*_f32`: the same expressions composed in fp32 on the CPU with u^p = exp2(p * log2 u) -- what a straightforward fp32 evaluation
gives.  Its error against float64 is the noise floor the GPU tests take their bounds from: it moves with the inputs (the product
p * log2 u is rounded to fp32, so the error of u^p grows with |p log2 u|; eps^p is subnormal in fp32 from p = 6.3)."""
import torch

F32_MANT, BF16_MANT, F16_MANT = 23, 7, 10


def _f64(x):
    return x.detach().to(torch.float64)


def fwd_f64(x, p, eps=1e-6):
    """y float64 [B, C] and the mean m"""
    u = _f64(x).clamp(min=eps)
    m = u.pow(p).mean(dim=1)
    return m.pow(1.0 / p), m


def dx_f64(x, dy, p, eps=1e-6):
    x = _f64(x)
    HW = x.shape[1]
    u = x.clamp(min=eps)
    _, m = fwd_f64(x, p, eps)
    g = (_f64(dy) / HW * m.pow(1.0 / p - 1.0))[:, None, :] * u.pow(p - 1.0)
    return torch.where(x >= eps, g, torch.zeros_like(g))


def dp_terms_f64(x, dy, p, eps=1e-6):
    """The two terms of dp per (b, c): dy y (sum u^p ln u) / (HW m p)  and  dy y ln(m) / p^2.  dp = (t1 - t2).sum()."""
    x = _f64(x)
    HW = x.shape[1]
    u = x.clamp(min=eps)
    y, m = fwd_f64(x, p, eps)
    t1 = _f64(dy) * y * (u.pow(p) * u.log()).sum(dim=1) / (HW * m * p)
    t2 = _f64(dy) * y * m.log() / (p * p)
    return t1, t2


def dp_f64(x, dy, p, eps=1e-6):
    """(dp, sum of |terms|): the two terms nearly cancel, so an error bound on dp is stated against the second value"""
    t1, t2 = dp_terms_f64(x, dy, p, eps)
    return float((t1 - t2).sum()), float(t1.abs().sum() + t2.abs().sum())


def _pow_f32(u, e):
    return torch.exp2(e * torch.log2(u))


def fwd_f32(x, p, eps=1e-6):
    x = x.detach().to(torch.float32)
    p32 = torch.tensor(p, dtype=torch.float32)
    u = x.clamp(min=eps)
    m = _pow_f32(u, p32).mean(dim=1)
    return torch.exp2(torch.log2(m) / p32), m


def dx_f32(x, dy, p, eps=1e-6):
    x = x.detach().to(torch.float32)
    HW = x.shape[1]
    p32 = torch.tensor(p, dtype=torch.float32)
    u = x.clamp(min=eps)
    _, m = fwd_f32(x, p, eps)
    g = (dy.to(torch.float32) / HW * _pow_f32(m, 1.0 / p32 - 1.0))[:, None, :] * _pow_f32(u, p32 - 1.0)
    return torch.where(x >= eps, g, torch.zeros_like(g))


def rel_err(got, ref):
    """max |got - ref| / |ref| over the elements with ref != 0 (0 where there is none)"""
    ref = _f64(ref)
    nz = ref != 0
    if not bool(nz.any()):
        return 0.0
    return float(((_f64(got) - ref).abs()[nz] / ref.abs()[nz]).max())


def fwd_floor(x, p, eps=1e-6):
    """max relative error of the fp32 composition of y against float64 on these inputs"""
    return rel_err(fwd_f32(x, p, eps)[0], fwd_f64(x, p, eps)[0])


def dx_floor(x, dy, p, eps=1e-6):
    return rel_err(dx_f32(x, dy, p, eps), dx_f64(x, dy, p, eps))


def ulp(ref, mant_bits, min_exp):
    """One unit in the last place of a format with `mant_bits` stored mantissa bits and smallest normal exponent `min_exp`, at the
    binade of each |ref| (float64 in, float64 out)."""
    _, e = torch.frexp(_f64(ref).abs().clamp(min=2.0 ** -200))          # |ref| = f * 2^e, f in [0.5, 1)
    return torch.exp2((e - 1).clamp(min=min_exp).to(torch.float64) - mant_bits)


def ulp_of(dtype, ref):
    if dtype == torch.float32:
        return ulp(ref, F32_MANT, -126)
    if dtype == torch.bfloat16:
        return ulp(ref, BF16_MANT, -126)
    assert dtype == torch.float16
    return ulp(ref, F16_MANT, -14)


def pool_nchw(base_out, p, eps=1e-6):
    """GeM over an NCHW feature map in torch (differentiable in base_out and p, any float dtype): [B, C, H, W] -> [B, C]"""
    return base_out.clamp(min=eps).pow(p).mean(dim=(2, 3)).pow(1.0 / p)


def make_inputs(B, HW, C, dtype, seed):
    """The GPU tests' map, as stored in `dtype`: values up to 30, half of them exact zeros (the ReLU), some below eps = 1e-6, one
    whole-zero channel per image and, in f16, one 65504.  Returns (x in dtype [B, HW, C], dy fp32 [B, C])."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, HW, C), generator=g) * 30.0
    x = torch.where(torch.rand((B, HW, C), generator=g) < 0.5, torch.zeros(()), x)
    x = torch.where(torch.rand((B, HW, C), generator=g) < 0.05, torch.full((), 3e-7), x)
    for b in range(B):
        x[b, :, (3 * b + 2) % C] = 0.0
    if dtype == torch.float16:
        x[0, 0, 1] = 65504.0
    dy = torch.randn((B, C), generator=g)
    return x.to(dtype), dy
