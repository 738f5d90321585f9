"""CPU: the eval-mode audit (tests/eval_audit.py) on torch emulations of the kernels it judges on the GPU -- one bottleneck boundary
(folded conv3 + residual + ReLU, then the pair kernel's second multiply: conv1 + folded bn1 + ReLU on the STORED block output), one
eval-mode IBN layer, the fold constants and GAP.  The emulations compute the way the kernels do: fp32 accumulation, one fp32 fma,
a rounding to the 16-bit storage type, the residual added in fp32, a second rounding (add_chunk, conv_epilogue.hpp); fp32 outputs
round nowhere in between.  The faithful emulation is within the shared bounds for bf16, f16 and fp32, and each mutation a kernel
could plausibly carry is flagged by the same eval_audit.check_* calls that tests/test_eval_audit_gpu.py makes:

  shift built from the batch mean | eps dropped from the fold | sqrt(var) + eps | residual added after the ReLU | ReLU dropped |
  the affine result truncated before the residual add (16-bit) | conv1 of the pair fed with the unrounded block output (16-bit) |
  InstanceNorm half on running statistics | BatchNorm half on instance statistics | statistics that count the zero-padded rows of
  a partial tile | GAP dividing by a padded row count.

None of the eleven is invisible at these sizes (M = 300 rows, 64 -> 256 -> 64 channels; IBN on 2 x 200 and 2 x 256 rows)."""
import math

import pytest
import torch

import eval_audit as ea
import layer_audit as la

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF, F16, F32]
EPS = 1e-5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _fma(a, b, c):
    """one fp32 fma: the exact product-sum (fp64 holds it for fp32 operands up to its own rounding) rounded once"""
    return (a.double() * b.double() + c.double()).float()


def _trunc(v, dt):
    """fp32 -> dt rounded toward zero"""
    r = v.to(dt).double()
    vd = v.double()
    return torch.where(r.abs() > vd.abs(), r - torch.sign(vd) * la.ulp(vd, dt), r).to(dt)


def _mm32(x, w):
    """1 x 1 convolution the kernels' way: products of the stored operands summed in fp32.  x [M, cin], w [cout, cin]"""
    return x.float() @ w.float().t()


def _bn_params(C, g):
    return dict(gamma=0.5 + torch.rand(C, generator=g), beta=0.1 * torch.randn(C, generator=g),
                mean=0.1 * torch.randn(C, generator=g), var=0.5 + torch.rand(C, generator=g))


def _fold_emul(p, eps=EPS, mut=None, batch_mean=None):
    """bn_fold_multi_kernel: is = 1 / sqrtf(var + eps); sc = is * gamma; sh = beta - mean * sc, every operation in fp32"""
    e = torch.tensor(eps, dtype=F32)
    if mut == "no_eps":
        inv = 1.0 / torch.sqrt(p["var"])
    elif mut == "eps_outside":
        inv = 1.0 / (torch.sqrt(p["var"]) + e)
    else:
        inv = 1.0 / torch.sqrt(p["var"] + e)
    sc = inv * p["gamma"]
    mu = batch_mean if mut == "batch_mean" else p["mean"]
    return torch.stack([sc, p["beta"] - mu * sc])


def _audit_fold(fold, p):
    au = la.Audit("cpu")
    ea.check_fold(au, "bn", fold, p["gamma"], p["beta"], p["mean"], p["var"], EPS)
    return au


@pytest.mark.parametrize("C", [64, 257])
def test_fold_passes_and_its_mutations_are_flagged(C):
    p = _bn_params(C, _gen(C))
    assert not _audit_fold(_fold_emul(p), p).failures
    batch_mean = p["mean"] + 0.05 * torch.randn(C, generator=_gen(1))
    assert any("fold shift" in f for f in _audit_fold(_fold_emul(p, mut="batch_mean", batch_mean=batch_mean), p).failures)
    assert any("fold scale" in f for f in _audit_fold(_fold_emul(p, mut="no_eps"), p).failures)
    assert any("fold scale" in f for f in _audit_fold(_fold_emul(p, mut="eps_outside"), p).failures)


def test_fold_null_entries_and_extreme_statistics():
    """null gamma / beta (scale 1, shift 0), var from 0 to 1e6, mean up to +-1e3, both eps values: the bound holds for the
    faithful arithmetic everywhere the direct GPU test of creid_bn2d_fold_multi goes"""
    for eps in (1e-5, 1e-3):
        for var in (0.0, 1e-12, 1e-5, 1.0, 1e6):
            for mean in (0.0, 1e-3, -1e-3, 1e3, -1e3):
                g = _gen(3)
                C = 63
                p = dict(gamma=0.5 + torch.rand(C, generator=g), beta=torch.randn(C, generator=g),
                         mean=torch.full((C,), mean) * (0.5 + torch.rand(C, generator=g)),
                         var=torch.full((C,), var) * (0.5 + torch.rand(C, generator=g)))
                au = la.Audit("cpu")
                ea.check_fold(au, "bn", _fold_emul(p, eps), p["gamma"], p["beta"], p["mean"], p["var"], eps)
                q = dict(p, gamma=torch.ones(C), beta=torch.zeros(C))
                ea.check_fold(au, "bn-null", _fold_emul(q, eps), None, None, p["mean"], p["var"], eps)
                assert not au.failures, (eps, var, mean, au.failures)


# ------------------------------------------------------------------------------------------- one bottleneck boundary
def _boundary_case(dt, seed=0, M=300):
    g = _gen(seed)
    a2 = torch.relu(torch.randn(M, 64, generator=g)).to(dt)
    res = torch.relu(torch.randn(M, 256, generator=g)).to(dt)
    w3 = (torch.randn(256, 64, generator=g) / 8.0).to(dt)
    w1 = (torch.randn(64, 256, generator=g) / 16.0).to(dt)
    return a2, res, w3, w1, _fold_emul(_bn_params(256, g)), _fold_emul(_bn_params(64, g))


def _boundary_emul(a2, res, w3, w1, fold3, fold1, dt, mut=None):
    """conv3 + folded bn3 + residual + ReLU -> the stored block output; conv1 of the next block on it + folded bn1 + ReLU"""
    v = _fma(_mm32(a2, w3), fold3[0], fold3[1])
    if dt != F32:
        v = (_trunc(v, dt) if mut == "trunc_affine" else v.to(dt)).float()     # the staged C tile: rounded to the storage type
    if mut == "res_after_relu":
        o32 = torch.relu(v) + res.float()
    else:
        o32 = v + res.float()
        if mut != "no_relu":
            o32 = torch.relu(o32)
    out3 = o32.to(dt)
    src = o32 if mut == "unrounded_operand" else out3
    v1 = torch.relu(_fma(_mm32(src, w1), fold1[0], fold1[1]))
    return out3, v1.to(dt)


def _audit_boundary(out3, out1, a2, res, w3, w1, fold3, fold1, dt):
    """the calls of test_eval_audit_gpu.py's pair check"""
    au = la.Audit("cpu")
    M = a2.shape[0]
    ea.check_folded_conv(au, "c3", "conv3 + residual + ReLU", out3, a2.view(M, 1, 1, 64), w3.double().view(256, 64, 1, 1), 1, 0, fold3,
                         True, res, dt)
    ea.check_folded_conv(au, "c1", "conv1 + ReLU", out1, out3.view(M, 1, 1, 256), w1.double().view(64, 256, 1, 1), 1, 0, fold1, True,
                         None, dt)
    return au


@pytest.mark.parametrize("dt", DTYPES)
def test_boundary_passes(dt):
    case = _boundary_case(dt)
    au = _audit_boundary(*_boundary_emul(*case, dt), *case, dt)
    assert not au.failures, au.failures


# (fp32 outputs are not rounded between the two operations: the last two mutations exist for the 16-bit types only)
_BOUNDARY_MUTATIONS = [(dt, m, "c3") for dt in DTYPES for m in ("res_after_relu", "no_relu")] \
    + [(dt, m, l) for dt in (BF, F16) for m, l in (("trunc_affine", "c3"), ("unrounded_operand", "c1"))]


@pytest.mark.parametrize("dt,mut,layer", _BOUNDARY_MUTATIONS)
def test_boundary_mutations_are_flagged(dt, mut, layer):
    case = _boundary_case(dt, seed=1)
    au = _audit_boundary(*_boundary_emul(*case, dt, mut=mut), *case, dt)
    assert layer in au.failing_layers(), (mut, au.failures)
    if mut == "unrounded_operand":
        assert au.failing_layers() == {"c1"}, au.failures         # the block output itself is the faithful one


def test_single_rounding_bound_would_fail_the_faithful_16bit_epilogue():
    """why the residual bound has its extra terms: against fma -> + residual -> ONE rounding the faithful two-rounding epilogue is
    out of bounds (where the affine result and the residual cancel), so the kernels are held to the arithmetic they have"""
    a2, res, w3, w1, fold3, fold1 = _boundary_case(BF, seed=2)
    res = -_fma(_mm32(a2, w3), fold3[0], fold3[1]).to(BF) * 0.97                # near-cancelling residual
    out3, _ = _boundary_emul(a2, res.to(BF), w3, w1, fold3, fold1, BF)
    conv, e, sig = ea.conv_reference(a2.view(-1, 1, 1, 64), w3.double().view(256, 64, 1, 1), 1, 0)
    ref, b, s, _ = ea.folded_reference(conv, e, sig, fold3, True, res.to(BF), BF)
    au = la.Audit("cpu")
    au.check("c3", "two roundings", out3, ref, b, BF, sigma=s)
    assert not au.failures, au.failures
    y = conv * fold3[0].double() + fold3[1].double()
    one = la.Audit("cpu")
    one.check("c3", "one rounding", out3, ref, fold3[0].double().abs() * e + la.affine_bound(conv, fold3[0].double(), fold3[1].double(),
                                                                                           [res.double()]), BF)
    assert one.failures and y.abs().max() > 0


# ------------------------------------------------------------------------------------------- eval-mode IBN
def _ibn_case(dt, HW, seed=0, B=2, C=64):
    g = _gen(seed)
    a_in = torch.relu(torch.randn(B * HW, 64, generator=g)).to(dt)
    w = (torch.randn(C, 64, generator=g) / 8.0).to(dt)
    acc = _mm32(a_in, w)
    half = C // 2
    par = dict(in_w=0.5 + torch.rand(half, generator=g), in_b=0.1 * torch.randn(half, generator=g),
               bn_w=0.5 + torch.rand(C - half, generator=g), bn_b=0.1 * torch.randn(C - half, generator=g),
               rmean=0.1 * torch.randn(C - half, generator=g), rvar=0.5 + torch.rand(C - half, generator=g))
    return a_in, w, acc, par, B, HW, half


def _ibn_emul(x, acc, par, B, HW, half, dt, ready, mut=None):
    """creid_ibn_fwd_mask, training = 0: fp32 (sum, sumsq) per 128 rows of an image (of the conv's fp32 accumulators when they came
    ready, of the stored tensor otherwise), fp64 over them; BatchNorm half on running statistics; fp32 scale / shift, one fma"""
    C = x.shape[1]
    src = (acc if ready else x.float()).view(B, HW, C)
    e = torch.tensor(EPS, dtype=F32)
    s1 = torch.zeros(B, C, dtype=torch.float64)
    s2 = torch.zeros_like(s1)
    for r0 in range(0, HW, 128):
        blk = src[:, r0:r0 + 128]
        s1 += blk.sum(1).double()
        s2 += (blk * blk).sum(1).double()
    cnt = -(-HW // 128) * 128 if mut == "count_padded" else HW
    m64 = s1 / cnt
    v64 = (s2 / cnt - m64 * m64).clamp_min(0.0)
    mean, invstd = m64.float(), (1.0 / torch.sqrt(v64 + float(e))).float()
    bn_mean = par["rmean"].expand(B, C - half).clone()
    bn_inv = (1.0 / torch.sqrt(par["rvar"] + e)).expand(B, C - half).clone()
    if mut == "in_running":           # InstanceNorm half normalised with (some layer's) running statistics
        mean[:, :half], invstd[:, :half] = bn_mean[:, :half], bn_inv[:, :half]
    if mut != "bn_instance":
        mean[:, half:], invstd[:, half:] = bn_mean, bn_inv
    sc = invstd * torch.cat([par["in_w"], par["bn_w"]])
    sh = torch.cat([par["in_b"], par["bn_b"]]) - mean * sc
    y = torch.relu(_fma(x.float().view(B, HW, C), sc.unsqueeze(1), sh.unsqueeze(1)))
    return y.to(dt).view(B * HW, C), mean, invstd


def _audit_ibn(a_out, mean, invstd, x, a_in, w, par, B, HW, half, dt, ready):
    au = la.Audit("cpu")
    conv, e, _ = ea.conv_reference(a_in.view(B * HW, 1, 1, 64), w.double().view(-1, 64, 1, 1), 1, 0)
    ea.check_eval_ibn(au, "ibn", x, a_out, mean, invstd, conv, e, B, HW, half, par["in_w"], par["in_b"], par["bn_w"], par["bn_b"],
                      par["rmean"], par["rvar"], EPS, ready, dt)
    return au


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("HW,ready", [(256, True), (200, False)])
def test_eval_ibn_passes_and_its_mutations_are_flagged(dt, HW, ready):
    a_in, w, acc, par, B, HW, half = _ibn_case(dt, HW)
    x = acc.to(dt)
    args = (x, a_in, w, par, B, HW, half, dt, ready)
    assert not _audit_ibn(*_ibn_emul(x, acc, par, B, HW, half, dt, ready), *args).failures
    for mut in ("in_running", "bn_instance") + (() if HW % 128 == 0 else ("count_padded",)):
        bad = _audit_ibn(*_ibn_emul(x, acc, par, B, HW, half, dt, ready, mut=mut), *args)
        assert bad.failures, mut
        if mut == "in_running" or mut == "count_padded":
            assert any("IN mean" in f for f in bad.failures) and any("IN invstd" in f for f in bad.failures), bad.failures
        else:
            assert any("BN-half" in f for f in bad.failures), bad.failures


# ------------------------------------------------------------------------------------------- pooled features, embedding
@pytest.mark.parametrize("dt", DTYPES)
def test_gap_and_bnneck_pass_and_a_padded_count_is_flagged(dt):
    g = _gen(9)
    B, HW, C = 3, 91, 128                                     # 13 x 7: the odd map of configuration G
    a = torch.relu(torch.randn(B * HW, C, generator=g)).to(dt)
    s = torch.zeros(B, C)
    for i in range(HW):                                       # fp32 running sums
        s += a.view(B, HW, C)[:, i].float()
    au = la.Audit("cpu")
    ea.check_gap(au, s / HW, a, B, HW)
    p = _bn_params(C, g)
    feat = s / HW
    emb = (feat - p["mean"]) * (1.0 / torch.sqrt(p["var"] + torch.tensor(EPS))) * p["gamma"] + p["beta"]
    ea.check_bnneck(au, emb, feat, p["gamma"], p["beta"], p["mean"], p["var"], EPS)
    assert not au.failures, au.failures
    bad = la.Audit("cpu")
    ea.check_gap(bad, s / (-(-HW // 8) * 8), a, B, HW)        # the eight row lanes' padded count
    assert bad.failures
    bad = la.Audit("cpu")
    ea.check_bnneck(bad, (feat - p["mean"]) * (1.0 / (torch.sqrt(p["var"]) + EPS)) * p["gamma"] + p["beta"], feat, p["gamma"], p["beta"],
                    p["mean"], p["var"], EPS)
    assert bad.failures


def test_tile_partials_pass_and_a_dropped_row_is_flagged():
    """the pair kernel's [tiles][2][64] statistics rows: fp32 sums of its accumulators per 128-row tile"""
    g = _gen(11)
    M = 384
    o = torch.relu(torch.randn(M, 256, generator=g)).to(BF)
    w1 = (torch.randn(64, 256, generator=g) / 16.0).to(BF)
    acc = _mm32(o, w1)
    part = torch.stack([acc.view(3, 128, 64).sum(1), (acc * acc).view(3, 128, 64).sum(1)], 1)
    conv, e, _ = ea.conv_reference(o.view(M, 1, 1, 256), w1.double().view(64, 256, 1, 1), 1, 0)
    au = la.Audit("cpu")
    ea.check_tile_partials(au, "pair", part, conv, e)
    assert not au.failures, au.failures
    acc[200] = 0                                               # a row the sums miss
    bad = la.Audit("cpu")
    ea.check_tile_partials(bad, "pair", torch.stack([acc.view(3, 128, 64).sum(1), (acc * acc).view(3, 128, 64).sum(1)], 1), conv, e)
    assert bad.failures
