"""GPU: every layer op of one production-shape training step against fp64, each on its OWN recorded operands.

One real step runs through CTLModel.forward_backward (creid_ctl_heads_fused writes the backbone's incoming gradient `g` and the
deepest bn3 column sums `part3`, exactly as in bench.py; config F drives the engine with a given feature gradient, which takes the
gap_bwd route).  The engine's methods are wrapped on the instance: `forward` (the pooled features), `backward` (a snapshot of
`saved` -- the engine's SavedStep records --, `g`, `part3`), `_bn_bwd`, `_ibn_bwd`, `_dgrad` (inputs and results cloned right after each call: stream order makes the
clone see exactly what the launch wrote) and `_wgrad` (its operands; weight and BatchNorm-parameter gradients are compared at the
end, when the carried split reductions and finalizes have all run).  The C entry points called during the step are counted
through a proxy of the library handle, so the routes the default knobs select are asserted, not assumed.  Knobs stay at their
defaults: the audit checks what ships.

References are torch float64 on the GPU (tests/layer_audit.py: tap-by-tap convolutions, BatchNorm / InstanceNorm statistics and
backward, max-pool with its taps); nothing here calls the project's kernels.  16-bit operands are taken as stored, convolution
weights are the engine's own w_krsc / w_crsk copies (bf16x3: the fp32 masters; both are checked to be the round-to-nearest-even
copies of the masters), and batch statistics come from the fp64 conv output BEFORE its rounding (the conv epilogues sum their
fp32 accumulators; only creid_ibn_fwd_mask, where H W % 128 != 0, sums the stored tensor, and there the reference reads it too).

Bars (derived in tests/layer_audit.py; Audit.check adds 1/2 ulp of the output type at |ref| + b to every bound b).  "measured" =
the worst over configurations A-F on one MI355X, as a fraction of the bound (profiles/layer_audit.md has the per-layer tables):
* conv forward: b = K 2^-24 (|x| |w|), K = the products per output (test_plan_words_accumulate_in_fp32's rule); bf16x3 adds
  2^-16 (|x| |w|) (hi + lo keeps 2^-18 of each fp32 operand, two operands, the dropped lo * lo term).  Measured 0.999 (16-bit: a
  result exactly half-way, RNE's own bound), 0.112 (fp32), 0.67 (bf16x3).  bf16x3 also keeps the x3 layer bars: rel-L2 <= 2e-5
  (measured 4.7e-6) and max <= 1e-4 rms(ref) (holds);
* data gradient: the same rule, K = cout k^2.  With add_src the 16-bit epilogue rounds the accumulator to the storage type (the
  tile is staged through LDS as 16-bit words), adds add_src in fp32 and rounds again: + 1/2 ulp(|acc|) + 2 u (|acc| + |add|).
  The single-rounding bound failed by up to 298x on every c1 data gradient with add_src (profiles/layer_audit.md).  Measured
  0.999 / 0.152 / 0.694.  bf16x3: rel-L2 <= 2e-5 holds (measured 5.9e-6); max <= 1e-4 rms(ref) does NOT hold for every data
  gradient (layer2.0.downsample: 1.07e-4 and 1.02e-4 in two runs; next 9.8e-5, 9.5e-5): it is recorded, not asserted, and the
  derived element-wise bound is;
* weight gradient: (pixels per split + 64 + splits) 2^-24 (|dy|^T |x|), the split count read back from the workspace size; the
  + 64 is the rounding of a split's length up to whole k-steps of 64 (16-bit) or 16 (fp32) pixels (conv_wgrad.hip plan_wgrad),
  as in test_plan_words_accumulate_in_fp32's code.  Measured 0.0258 (stem 0.0017); bf16x3 rel-L2 <= 2e-5 (measured 1.2e-5),
  max / rms(ref) recorded (measured up to 8.6e-5);
* batch mean / invstd: layer_audit.stats_bound (accumulator error, fp32 per-tile partials, fp64 over the tiles).  Measured 0.072 /
  0.025; running statistics (momentum x those bounds + 3 u of each term): 0.071 / 0.19;
* apply (plain, residual, dual, finalize+apply, the axf side output a2, InstanceNorm): layer_audit.affine_bound, 3 u per term.
  Measured 1.0 (16-bit half-way results), 0.50 (fp32);
* BatchNorm / InstanceNorm backward: layer_audit.bn_bwd_bound (4 u per coefficient term, fp32 per-tile partials of the stored
  gradient).  Measured 1.0 / 0.181; their gamma / beta gradients (the bound of the fp64 sum of those partials): 0.038;
* max-pool forward: the apply bound (measured 1.0); the taps: a window maximum, and the kernel's first maximum where an
  emulation of its fp32 arithmetic reproduces the pooled value (all windows; 41159 tied windows at A, 0 taps off); backward: 3 u
  of the summed |g| of the <= 4 windows that share an input pixel (measured 1.0);
* ReLU bits, the masked gradient copies, the weight copies: exact (0 mismatches; f16: 2 bits over values below 2^-25);
* GAP: HW u mean|a| + 1/2 ulp_fp32 (measured 0.103); gap_bwd (F): u |dfeat / HW| + 1/2 ulp (1.0); the heads' g: one value per
  (image, channel).
Bias and relative-L2 bars: Audit.check's docstring.  Measured: |bias| <= 0.0064 ulp (bar >= 0.01), rel-L2 <= 0.70 of its bar for
16-bit outputs (0.667 = the ulp / sqrt(12) of unbiased rounding under a bar of 1.5x that).
Runtime: the seven configurations take 33 s on one MI355X.
"""
import ctypes as C
import dataclasses
import math
from collections import Counter
from types import SimpleNamespace

import pytest
import torch

import layer_audit as la

pytestmark = pytest.mark.gpu

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
CONFIGS = {        # mode, arch, P, K, H, W, driven by the heads (fused) or by a given feature gradient
    "A": ("bf16", "resnet50", 16, 4, 256, 128, True),
    "B": ("f16", "resnet50", 16, 4, 256, 128, True),
    "C": ("fp32", "resnet50", 16, 4, 256, 128, True),
    "D": ("bf16x3", "resnet50", 16, 4, 256, 128, True),
    "E": ("bf16", "resnet50_ibn_a", 14, 4, 320, 320, True),
    "F-bf16": ("bf16", "resnet50", 1, 3, 96, 80, False),
    "F-fp32": ("fp32", "resnet50", 1, 3, 96, 80, False),
}
MODES = {"bf16": BF, "f16": F16, "fp32": F32, "bf16x3": "bf16x3"}
F16_SCALE = 1024.0     # f16 loss scale for the audited step (the default 2^16 start may overflow a first step; 2^10 does not)


# ------------------------------------------------------------------------------------------- recording
class _LibProxy:
    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        self._calls[name] += 1
        return getattr(self._lib, name)


def _names(eng):
    names = {id(eng.stem): "stem"}
    i = 0
    for li, layer in enumerate((eng.net.layer1, eng.net.layer2, eng.net.layer3, eng.net.layer4), start=1):
        for bi in range(len(layer)):
            b = eng.blocks[i]
            for key, nm in (("c1", "conv1"), ("c2", "conv2"), ("c3", "conv3"), ("ds", "downsample")):
                if b[key] is not None:
                    names[id(b[key])] = f"layer{li}.{bi}.{nm}"
            i += 1
    return names


def _randomise(net, seed):
    """BatchNorm / InstanceNorm affine parameters and running statistics away from (1, 0): a dropped gamma or beta must show"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if hasattr(m, "weight") and hasattr(m, "bias") and m.weight is not None and m.weight.dim() == 1 and m.bias is not None \
                    and m.weight.requires_grad:
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g, device="cuda"))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g, device="cuda"))
            if hasattr(m, "running_mean"):
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g, device="cuda"))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g, device="cuda"))


def record_step(cfg, monkeypatch):
    from centroids_reid_amd import _lib as L
    from centroids_reid_amd.bench_train import make_model, synthetic_batch
    mode, arch, P, K, H, W, fused = CONFIGS[cfg]
    torch.manual_seed(0)                                     # (the holders' initial weights)
    model = make_model(dtype=MODES[mode], arch=arch, K=K)
    eng = model.backbone.engine
    _randomise(eng.net, 11)
    if mode == "f16":
        eng.loss_scaler.state.copy_(torch.tensor([F16_SCALE, 1.0 / F16_SCALE], device="cuda"))
    rec = SimpleNamespace(bn=[], ibn=[], dgrad=[], wgrad=[], calls=Counter(), saved=None, g=None, part3=False, dfeat=None,
                          feat=None, eng=eng, names=_names(eng), mode=mode, arch=arch, B=P * K, H=H, W=W, fused=fused)
    rec.running0 = {id(u): (u.bn.running_mean.clone(), u.bn.running_var.clone()) for u in eng.all_units()}
    real_lib = L.lib()
    monkeypatch.setattr(L, "lib", lambda: _LibProxy(real_lib, rec.calls))
    o_fwd, o_bwd, o_bn, o_ibn, o_dg, o_wg = eng.forward, eng.backward, eng._bn_bwd, eng._ibn_bwd, eng._dgrad, eng._wgrad

    def forward(x, training, want_base_out=False):
        out = o_fwd(x, training, want_base_out)
        rec.feat = out[1].clone()
        return out

    def backward(dfeat, g=None, part3=None):
        sv = eng.saved
        rec.saved = dataclasses.replace(sv, blocks=[dataclasses.replace(b) for b in sv.blocks])
        rec.g = None if g is None else g.clone()
        rec.part3 = part3 is not None
        rec.dfeat = None if dfeat is None else dfeat.clone()
        return o_bwd(dfeat, g=g, part3=part3)

    def bn_bwd(layer, g, *, want_gm=False, part=None, mask=None, reduce2=None):
        u = layer.unit
        route = "ready2" if id(u) in eng._bn_sums else ("ready1" if part is not None else "ready0")
        if route == "ready1" and eng.sched.fin_with_wred and eng._wred_pending:
            route = "fin+wred"
        act, own = (layer.act, layer.bits) if layer.relu else (None, None)      # (no ReLU behind the layer: nothing masks g)
        gc = g.clone()
        dx, gm, part2 = out = o_bn(layer, g, want_gm=want_gm, part=part, mask=mask, reduce2=reduce2)
        assert (gm is not None) == (want_gm and reduce2 is None) and (part2 is not None) == (reduce2 is not None)
        rec.bn.append(dict(u=u, x=layer.x, g=gc, act=act, bits=mask if mask is not None else own, mean=layer.mean,
                           invstd=layer.invstd, M=layer.x.shape[0], route=route, reduce2=reduce2 is not None, dx=dx.clone(),
                           gm=None if gm is None else gm.clone()))
        return out

    def ibn_bwd(layer, g, B, part=None):
        gc = g.clone()
        dx = o_ibn(layer, g, B, part=part)
        rec.ibn.append(dict(u=layer.unit, x=layer.x, g=gc, act=layer.act, bits=layer.bits, mean=layer.mean, invstd=layer.invstd,
                            B=B, HW=layer.hw, ready=part is not None, dx=dx.clone()))
        return dx

    def dgrad(u, dy, B, H_, W_, *, add_src=None, consumer=None, add_src_stride=1, add_mask=None, on_output_grid=False):
        carry = bool(eng._wred_pending) and len(eng._wred_pending) >= (2 if eng.sched.fin_with_wred else 1)
        dyc = dy.clone()
        addc = None if add_src is None else add_src.clone()
        out = o_dg(u, dy, B, H_, W_, add_src=add_src, consumer=consumer, add_src_stride=add_src_stride, add_mask=add_mask,
                   on_output_grid=on_output_grid)
        # bnred: the launch also returned the column sums of the consumer's BatchNorm backward (never without a consumer)
        assert out[1] is None or (consumer is not None and eng.sched.fuse_bn_reduce)
        rec.dgrad.append(dict(u=u, dy=dyc, B=B, H=H_, W=W_, add=addc, stride=add_src_stride, add_mask=add_mask,
                              bnred=out[1] is not None, carry=carry, on_output_grid=on_output_grid, dx=out[0].clone()))
        return out

    def wgrad(u, a_in, dy, B, H_, W_, *, fin=None):
        rec.wgrad.append(dict(u=u, a_in=a_in, dy=dy.clone(), B=B, H=H_, W=W_,
                              bnfin=fin is not None and fin[1] is not None and eng.sched.bnfin_piggyback and eng.sched.wred_piggyback))
        return o_wg(u, a_in, dy, B, H_, W_, fin=fin)

    for n, f in (("forward", forward), ("backward", backward), ("_bn_bwd", bn_bwd), ("_ibn_bwd", ibn_bwd), ("_dgrad", dgrad),
                 ("_wgrad", wgrad)):
        monkeypatch.setattr(eng, n, f)
    if fused:
        x, labels, camid, is_real = synthetic_batch(P, K, H, W, 0)
        rec.x = x
        model.forward_backward((x, labels, camid, is_real), 0)
    else:
        gen = torch.Generator(device="cuda").manual_seed(5)
        x = torch.randn((P * K, 3, H, W), generator=gen, device="cuda")
        rec.x = x
        for p in eng.net.parameters():
            p.grad = None
        _, feat = eng.forward(x, True)
        eng.backward(torch.randn(feat.shape, generator=gen, device="cuda") * 1e-2)
    torch.cuda.synchronize()
    monkeypatch.undo()
    rec.lib = real_lib
    return rec


# ------------------------------------------------------------------------------------------- audit
def _dt_out(rec):
    return rec.eng.dtype                      # activations / gradients: bf16, f16 or fp32 (bf16x3: fp32)


def _fwd_w(rec, u):
    if rec.eng.x3:
        return u.conv.weight.detach().double()
    return u.w_krsc.permute(0, 3, 1, 2).double()


def _bwd_w(rec, u):
    if rec.eng.x3:
        return u.conv.weight.detach().double()
    return u.w_crsk.permute(3, 0, 1, 2).double()


def _mask_of(bits, act, M, Cc):
    if bits is not None:
        return la.unpack_bits(bits, M, Cc)
    if act is not None:
        return act.view(M, Cc) > 0
    return None


def _conv_check(au, rec, name, u, a_in, B, h, w, x_raw):
    x3 = rec.eng.x3
    wt = _fwd_w(rec, u)
    xin = a_in.view(B, h, w, u.cin)
    ref = la.conv_fwd(xin, wt, u.stride, u.pad).reshape(-1, u.cout)
    mag = la.conv_fwd(xin.double().abs(), wt.abs(), u.stride, u.pad).reshape(-1, u.cout)
    K = u.cin * u.k * u.k
    e = K * la.U * mag + (la.SPLIT * mag if x3 else 0.0)
    sig = math.sqrt(K) * la.U * mag + (la.SPLIT * mag if x3 else 0.0)
    au.check(name, "conv fwd", x_raw, ref, e, _dt_out(rec), sigma=sig, rel_bar=2e-5 if x3 else None, max_rms=1e-4 if x3 else None)
    d, _, _ = _desc(B, h, w, u)
    return ref, e, -(-ref.shape[0] // rec.lib.creid_conv2d_bn_partial_rows(C.byref(d)))     # rows per statistics partial


def _stats_check(au, rec, name, bn, ref, e, mean, invstd, rows_per_tile=128):
    M = ref.shape[0]
    m_ref, var_ref, i_ref = la.batch_stats(ref, bn.eps)
    dm, di, _, dvar = la.stats_bound(ref, e, bn.eps, rows_per_tile)
    au.check(name, "batch mean", mean, m_ref, dm, F32, sigma=dm, bias=False)
    au.check(name, "batch invstd", invstd, i_ref, di, F32, sigma=di, bias=False)
    return m_ref, var_ref, dm, dvar


def _running_check(au, rec, name, u, m_ref, var_ref, dm, dvar, M):
    rm0, rv0 = rec.running0[id(u)]
    mom = u.bn.momentum
    rm_ref = (1 - mom) * rm0.double() + mom * m_ref
    unb = var_ref * M / (M - 1)
    rv_ref = (1 - mom) * rv0.double() + mom * unb
    au.check(name, "running_mean", u.bn.running_mean, rm_ref, mom * dm + 3 * la.U * ((1 - mom) * rm0.double().abs() + mom * m_ref.abs()),
             F32, bias=False, sigma=mom * dm + 3 * la.U * rm_ref.abs())
    au.check(name, "running_var", u.bn.running_var, rv_ref, mom * dvar * M / (M - 1) + 3 * la.U * ((1 - mom) * rv0.double().abs() + mom * unb),
             F32, bias=False, sigma=mom * dvar * M / (M - 1) + 3 * la.U * rv_ref.abs())


def _apply_ref(x, mean, invstd, gamma, beta):
    sc = invstd.double() * gamma.detach().double()
    sh = beta.detach().double() - mean.double() * sc
    return x.double() * sc + sh, sc, sh, mean.double() * sc     # (|mean sc|: the rounding of shift = beta - mean sc)


def _apply_check(au, rec, name, layer, relu, residual=None, res_terms=()):
    a_out, x, mean, invstd, bn = layer.act, layer.x, layer.mean, layer.invstd, layer.unit.bn
    M, Cc = x.shape
    y, sc, sh, msc = _apply_ref(x, mean, invstd, bn.weight, bn.bias)
    terms = list(res_terms) + [msc]
    if residual is not None:
        y = y + residual
        terms.append(residual)
    b = la.affine_bound(x.double(), sc, sh, terms)
    ref = y.clamp_min(0.0) if relu else y
    au.check(name, "apply", a_out, ref, b, _dt_out(rec), sigma=b)
    if layer.bits is not None:
        au.relu_bits(name, layer.bits, a_out.view(M, Cc), ref.view(M, Cc), rec.eng.dtype)
    return ref


def _ibn_fwd_check(au, rec, name, layer, ref, e, B):
    """IBN-a bn1: InstanceNorm (per image) on the first `half` channels, BatchNorm on the rest; mean / invstd are [B, C]"""
    u, x_raw, a_out, mean, invstd, HW = layer.unit, layer.x, layer.act, layer.mean, layer.invstd, layer.hw
    ibn, bn = u.ibn, u.bn
    h = ibn.half
    Cc = ref.shape[1]
    if HW % 128 == 0:           # the conv epilogue's per-image 128-row partials of its fp32 accumulators
        rpi, tile = HW // 128, 128
    else:                       # creid_ibn_fwd_mask sums the STORED conv output itself: the reference reads the same values
        rpi = rec.lib.creid_ibn_rows_per_image(HW)
        tile = -(-HW // rpi)
        ref, e = x_raw.double().view(-1, Cc), torch.zeros_like(e)
    r3, e3 = ref.view(B, HW, Cc), e.view(B, HW, Cc)
    mi = []
    for n in range(B):
        m_ref, _, i_ref = la.batch_stats(r3[n, :, :h], ibn.IN.eps)
        dm, dinv, _, _ = la.stats_bound(r3[n, :, :h], e3[n, :, :h], ibn.IN.eps, tile)
        mi.append((m_ref, i_ref, dm, dinv))
    au.check(name, "IN mean", mean[:, :h], torch.stack([t[0] for t in mi]), torch.stack([t[2] for t in mi]), F32, bias=False,
             sigma=torch.stack([t[2] for t in mi]))
    au.check(name, "IN invstd", invstd[:, :h], torch.stack([t[1] for t in mi]), torch.stack([t[3] for t in mi]), F32, bias=False,
             sigma=torch.stack([t[3] for t in mi]))
    m_ref, var_ref, dm, dvar = _stats_check(au, rec, name, bn, ref[:, h:], e[:, h:], mean[0, h:], invstd[0, h:], tile)
    assert torch.equal(mean[:, h:], mean[:1, h:].expand(B, Cc - h)), "IBN BatchNorm half: one mean for every image"
    _running_check(au, rec, name, u, m_ref, var_ref, dm, dvar, ref.shape[0])
    x = x_raw.view(B, HW, Cc).double()
    sc = torch.cat([invstd[:, :h].double() * ibn.IN.weight.detach().double(), invstd[:, h:].double() * bn.weight.detach().double()], 1)
    beta = torch.cat([ibn.IN.bias.detach().double().expand(B, h), bn.bias.detach().double().expand(B, Cc - h)], 1)
    sh = beta - mean.double() * sc
    y = x * sc.unsqueeze(1) + sh.unsqueeze(1)
    b = la.affine_bound(x, sc.unsqueeze(1), sh.unsqueeze(1), [(mean.double() * sc).unsqueeze(1)])
    ref_a = y.clamp_min(0.0)
    au.check(name, "IBN apply", a_out, ref_a, b, _dt_out(rec), sigma=b)
    if layer.bits is not None:
        au.relu_bits(name, layer.bits, a_out.view(B * HW, Cc), ref_a.view(B * HW, Cc), rec.eng.dtype)


def _pool_tie_check(au, rec, x0, mean0, invstd0, bn, idx0, p0, B, H1, W1, dt):
    """tie-breaks of the fused bn1 + max-pool against the kernel's own arithmetic: y = fmaf(x, sc, sh) in fp32 with sc = invstd
    gamma, sh = beta - mean sc (fp32; evaluated with and without a contracted fma), rounded to the stored type, FIRST maximal tap
    (bn_apply_maxpool_kernel, F.max_pool2d's rule).  Where the emulation reproduces the pooled value the taps must agree."""
    sc = invstd0 * bn.weight.detach()
    best = None
    for sh in ((bn.bias.detach().double() - mean0.double() * sc.double()).float(), bn.bias.detach() - mean0 * sc):
        y = (x0.double() * sc.double() + sh.double()).float().to(dt).double().view(B, H1, W1, 64)
        pv, first, taps = la.maxpool3x3s2(y)
        same = pv == p0.view_as(pv).double()
        if best is None or int(same.sum()) > int(best[0].sum()):
            best = (same, first, taps, pv)
    same, first, taps, pv = best
    tied = (taps == pv.unsqueeze(0)).sum(0) >= 2
    diff = same & (first != idx0.view_as(first).long())
    n, n_same, n_tied = same.numel(), int(same.sum()), int((tied & same).sum())
    au.exact("stem", "max-pool tie-break (first max)", int(diff.sum()) == 0 and n_same >= 0.999 * n,
             f"{int(diff.sum())} taps differ, emulation reproduces {n_same} of {n} windows")
    au.note("stem", "max-pool ties", f"{n_tied} tied windows of {n} (emulation reproduces {n_same}), {int(diff.sum())} taps "
            "off the first maximum")
    rec.pool_ties = (n_tied, n, n_same, int(diff.sum()))


def _weight_copies_check(au, rec):
    """the operands the audit takes from the engine: w_krsc / w_crsk must be the masters rounded to nearest even (bf16x3: the hi
    plane bf16(w), the lo plane bf16(w - hi)), transposed"""
    eng = rec.eng
    bad = []
    for u in eng.all_units():
        if u is eng.stem:
            continue
        w = u.conv.weight.detach()
        krsc = w.permute(0, 2, 3, 1)
        if eng.x3:
            hi = krsc.to(BF)
            want = torch.stack([hi, (krsc - hi.float()).to(BF)])
            ok = torch.equal(u.w_krsc.view(torch.int16), want.view(torch.int16))
            if u.w_crsk is not None:
                ok = ok and torch.equal(u.w_crsk.view(torch.int16), want.permute(0, 4, 2, 3, 1).contiguous().view(torch.int16))
        else:
            want = krsc.to(eng.dtype)
            ok = torch.equal(u.w_krsc, want) and torch.equal(u.w_crsk, want.permute(3, 1, 2, 0))
        if not ok:
            bad.append(rec.names[id(u)])
    au.exact("weights", "w_krsc / w_crsk = RNE(master)", not bad, " ".join(bad[:8]))


def audit_forward(au, rec):
    eng, sv = rec.eng, rec.saved
    B, H, W = rec.B, rec.H, rec.W
    dt = eng.dtype
    _weight_copies_check(au, rec)
    # stem: layout pass, 7 x 7 conv, bn1 statistics, apply (+ ReLU) and the 3 x 3 s2 max-pool with its taps
    xpad, bn0, idx0 = sv.stem.xpad, sv.stem.bn, sv.stem.idx
    x0, y0, mean0, invstd0 = bn0.x, bn0.act, bn0.mean, bn0.invstd
    img = xpad[:, 3:3 + H, 3:3 + W, :3]
    au.exact("stem", "image layout", torch.equal(img, rec.x.permute(0, 2, 3, 1).to(dt)))
    st = eng.stem
    wt = st.conv.weight.detach().to(dt).double()
    ref0 = la.conv_fwd(img, wt, 2, 3).reshape(-1, 64)
    mag0 = la.conv_fwd(img.double().abs(), wt.abs(), 2, 3).reshape(-1, 64)
    e0 = 147 * la.U * mag0
    au.check("stem", "conv fwd", x0, ref0, e0, dt, sigma=math.sqrt(147) * la.U * mag0)
    m_ref, var_ref, dm, dvar = _stats_check(au, rec, "stem", st.bn, ref0, e0, mean0, invstd0)
    _running_check(au, rec, "stem", st, m_ref, var_ref, dm, dvar, ref0.shape[0])
    H1, W1 = H // 2, W // 2
    p0 = sv.blocks[0].a_in
    y, sc, sh, msc = _apply_ref(x0, mean0, invstd0, st.bn.weight, st.bn.bias)
    b = la.affine_bound(x0.double(), sc, sh, [msc])
    if eng.net.stem_relu:
        _apply_check(au, rec, "stem", bn0, True)
        pv, pidx, taps = la.maxpool3x3s2(y0.view(B, H1, W1, 64).double())       # pooled values of the stored activation: exact
        au.exact("stem", "max-pool values", torch.equal(p0.view_as(pv).double(), pv))
        au.exact("stem", "max-pool taps (first max)", torch.equal(idx0.view_as(pidx).long(), pidx))
    else:
        yv = y.view(B, H1, W1, 64)
        pv, _, taps = la.maxpool3x3s2(yv)
        bb = la.maxpool3x3s2(b.view(B, H1, W1, 64))[0]
        au.check("stem", "bn1 + max-pool", p0, pv, bb, dt, sigma=bb)
        sel = torch.gather(taps, 0, idx0.view(1, *pv.shape).long()).squeeze(0)
        au.exact("stem", "max-pool tap is a window max", bool((sel >= pv - 2 * bb - 2 * la.half_ulp(pv, dt)).all()))
        _pool_tie_check(au, rec, x0, mean0, invstd0, st.bn, idx0, p0, B, H1, W1, dt)
    # bottlenecks
    for b_u, s in zip(eng.blocks, sv.blocks):
        c1, c2, c3, ds = s.c1, s.c2, s.c3, s.ds
        assert [l.unit for l in (c1, c2, c3)] == [b_u[k] for k in ("c1", "c2", "c3")] and (ds is None) == (b_u["ds"] is None)
        n1, n2, n3 = (rec.names[id(l.unit)] for l in (c1, c2, c3))
        ref1, e1, t1 = _conv_check(au, rec, n1, c1.unit, s.a_in, B, s.hin, s.win, c1.x)
        if c1.unit.ibn is not None:
            _ibn_fwd_check(au, rec, n1, c1, ref1, e1, B)
        else:
            m_ref, var_ref, dm, dvar = _stats_check(au, rec, n1, c1.unit.bn, ref1, e1, c1.mean, c1.invstd, t1)
            _running_check(au, rec, n1, c1.unit, m_ref, var_ref, dm, dvar, ref1.shape[0])
            _apply_check(au, rec, n1, c1, True)
        ref2, e2, t2 = _conv_check(au, rec, n2, c2.unit, c1.act, B, c1.h, c1.w, c2.x)
        m_ref, var_ref, dm, dvar = _stats_check(au, rec, n2, c2.unit.bn, ref2, e2, c2.mean, c2.invstd, t2)
        _running_check(au, rec, n2, c2.unit, m_ref, var_ref, dm, dvar, ref2.shape[0])
        _apply_check(au, rec, n2, c2, True)
        ref3, e3, t3 = _conv_check(au, rec, n3, c3.unit, c2.act, B, c2.h, c2.w, c3.x)
        m_ref, var_ref, dm, dvar = _stats_check(au, rec, n3, c3.unit.bn, ref3, e3, c3.mean, c3.invstd, t3)
        _running_check(au, rec, n3, c3.unit, m_ref, var_ref, dm, dvar, ref3.shape[0])
        if ds is not None:
            nd = rec.names[id(ds.unit)]
            refd, ed, td = _conv_check(au, rec, nd, ds.unit, s.a_in, B, s.hin, s.win, ds.x)
            m_ref, var_ref, dm, dvar = _stats_check(au, rec, nd, ds.unit.bn, refd, ed, ds.mean, ds.invstd, td)
            _running_check(au, rec, nd, ds.unit, m_ref, var_ref, dm, dvar, refd.shape[0])
            assert eng.sched.dual_apply and ds.act is None and not ds.relu
            r, scd, shd, mscd = _apply_ref(ds.x, ds.mean, ds.invstd, ds.unit.bn.weight, ds.unit.bn.bias)   # dual: fp32, unrounded
            res_terms = [ds.x.double() * scd, shd, mscd]
        else:
            r, res_terms = s.a_in.double(), []
        _apply_check(au, rec, n3, c3, True, residual=r, res_terms=res_terms)
    # GAP
    h, w = sv.final
    a = sv.blocks[-1].c3.act.view(B, h * w, -1).double()
    ref = a.mean(1)
    au.check("gap", "gap fwd", rec.feat, ref, h * w * la.U * a.abs().mean(1) + la.U * ref.abs(), F32, bias=False,
             sigma=math.sqrt(h * w) * la.U * a.abs().mean(1))


def audit_backward(au, rec):
    eng, sv = rec.eng, rec.saved
    B = rec.B
    dt = eng.dtype
    x3 = eng.x3
    h, w = sv.final
    grads = {}                   # parameter -> (ref, bound): the BatchNorm / InstanceNorm gamma and beta gradients
    if rec.g is not None:
        gv = rec.g.view(B, h * w, -1)
        au.exact("heads", "g one value per (image, channel)", torch.equal(gv, gv[:, :1].expand_as(gv)))
    else:
        first = rec.bn[0]
        ref = (rec.dfeat.double() / (h * w)).unsqueeze(1).expand(B, h * w, -1).reshape(first["g"].shape)
        au.check("gap", "gap bwd", first["g"], ref, la.U * ref.abs(), dt, sigma=la.U * ref.abs())
    for r in rec.bn:
        u = r["u"]
        name = rec.names[id(u)]
        M, Cc = r["x"].shape
        mask = _mask_of(r["bits"], r["act"], M, Cc)
        dy = r["g"].double() if mask is None else r["g"].double() * mask
        ref, s1, s2, parts = la.bn_bwd(r["x"], dy, r["mean"], r["invstd"], u.bn.weight.detach())
        b, ds1, ds2 = la.bn_bwd_bound(r["x"], dy, parts, M, -(-M // rec.lib.creid_bn2d_bwd_rows(M)))
        tag = r["route"] + (" reduce2" if r["reduce2"] else "") + (" masked-g" if r["bits"] is not None and r["act"] is None else "")
        au.check(name, f"bn bwd dx [{tag}]", r["dx"], ref, b, dt, sigma=b)
        if r["gm"] is not None:
            au.exact(name, "bn bwd masked g", torch.equal(r["gm"].double(), dy))
        grads[u.bn.bias] = (s1.view(-1), ds1.view(-1))
        grads[u.bn.weight] = (s2.view(-1), ds2.view(-1))
        if u is eng.stem:
            # max-pool backward: the stem BatchNorm's incoming gradient is the last data gradient scattered through idx0
            H1, W1 = rec.H // 2, rec.W // 2
            gp = rec.dgrad[-1]["dx"].view(B, H1 // 2, W1 // 2, 64)
            idx0 = sv.stem.idx.view(B, H1 // 2, W1 // 2, 64)
            refp = la.maxpool3x3s2_bwd(gp, idx0, H1, W1)
            bp = 3 * la.U * la.maxpool3x3s2_bwd(gp.abs(), idx0, H1, W1)
            au.check("stem", "max-pool bwd", r["g"], refp.reshape(r["g"].shape), bp, dt, sigma=bp)
            rec.stem_dx = r["dx"]
    for r in rec.ibn:
        u = r["u"]
        name = rec.names[id(u)]
        ibn, bn = u.ibn, u.bn
        hh = ibn.half
        B_, HW = r["B"], r["HW"]
        M, Cc = r["x"].shape
        mask = _mask_of(r["bits"], r["act"], M, Cc)
        dy = r["g"].double() if mask is None else r["g"].double() * mask
        rpi = rec.lib.creid_ibn_rows_per_image(HW)
        tile = -(-HW // rpi)
        xi, di = r["x"][:, :hh].contiguous(), dy[:, :hh].contiguous()
        ref_i, s1i, s2i, pi = la.bn_bwd(xi, di, r["mean"][:, :hh], r["invstd"][:, :hh], ibn.IN.weight.detach(), groups=(B_, HW))
        b_i, d1i, d2i = la.bn_bwd_bound(xi, di, pi, HW, tile)
        xb, db = r["x"][:, hh:].contiguous(), dy[:, hh:].contiguous()
        ref_b, s1b, s2b, pb = la.bn_bwd(xb, db, r["mean"][0, hh:], r["invstd"][0, hh:], bn.weight.detach())
        b_b, d1b, d2b = la.bn_bwd_bound(xb, db, pb, M, tile)
        au.check(name, "IBN bwd dx", r["dx"], torch.cat([ref_i, ref_b], 1), torch.cat([b_i, b_b], 1), dt,
                 sigma=torch.cat([b_i, b_b], 1))
        grads[ibn.IN.bias] = (s1i.sum(0), d1i.sum(0))
        grads[ibn.IN.weight] = (s2i.sum(0), d2i.sum(0))
        grads[bn.bias] = (s1b.view(-1), d1b.view(-1))
        grads[bn.weight] = (s2b.view(-1), d2b.view(-1))
    for r in rec.dgrad:
        u = r["u"]
        name = rec.names[id(u)]
        wt = _bwd_w(rec, u)
        B_, H_, W_ = r["B"], r["H"], r["W"]
        # on_output_grid (the stride-2 1 x 1 downsample): the same weights as a stride-1 1 x 1 convolution over the output grid
        k, stride, pad = (1, 1, 0) if r["on_output_grid"] else (u.k, u.stride, u.pad)
        assert not r["on_output_grid"] or (u.k, u.stride, u.pad) == (1, 2, 0)
        oh, ow = (H_ + 2 * pad - k) // stride + 1, (W_ + 2 * pad - k) // stride + 1
        dy = r["dy"].view(B_, oh, ow, u.cout)
        ref = la.conv_dgrad(dy, wt, stride, pad, H_, W_)
        mag = la.conv_dgrad(dy.double().abs(), wt.abs(), stride, pad, H_, W_)
        add = torch.zeros((), dtype=torch.float64, device=ref.device)
        tags = []
        if r["add"] is not None:
            a = r["add"].double().view(-1, u.cin)
            if r["add_mask"] is not None:
                a = a * la.unpack_bits(r["add_mask"], a.shape[0], u.cin)
                tags.append("add_mask")
            if r["stride"] == 2:
                full = torch.zeros_like(ref)
                full[:, ::2, ::2, :] = a.view(B_, H_ // 2, W_ // 2, u.cin)
                add = full
                tags.append("add_src s2")
            else:
                add = a.view_as(ref)
                tags.append("add_src")
        if r["bnred"]:
            tags.append("bnred")
        if r["carry"]:
            tags.append("carry")
        if r["on_output_grid"]:
            tags.append("s2 shim")
        K = u.cout * k * k
        e = K * la.U * mag + (la.SPLIT * mag if x3 else 0.0)
        sig = math.sqrt(K) * la.U * mag + (la.SPLIT * mag if x3 else 0.0)
        if r["add"] is not None:
            # the 16-bit epilogue rounds the accumulator to the storage type (it is staged through LDS as 16-bit words), THEN
            # adds add_src in fp32 and rounds again: + 1/2 ulp of |acc| (the one-rounding bound failed by up to 298x where acc
            # and add_src cancel; profiles/layer_audit.md)
            first = la.half_ulp(ref.abs() + e, dt) if dt != F32 else 0.0
            e = e + first + 2 * la.U * (ref.abs() + add.abs())
            sig = sig + first * (2.0 / math.sqrt(12.0))
        ref = ref + add
        # bf16x3: the x3 layer bar max <= 1e-4 rms(ref) (set on unit-normal operands) does NOT hold for every production-shape
        # data gradient (measured up to 1.07e-4 on layer2.0.downsample): it is recorded, and the derived element-wise bound
        # (2^-16 |dy| |w| per element, measured <= 0.69 of it) is what is asserted
        au.check(name, "dgrad [" + " ".join(tags) + "]", r["dx"], ref, e, dt, sigma=sig, rel_bar=2e-5 if x3 else None,
                 report_max_rms=x3)
    # weight gradients (final after backward: split reductions carried by later launches)
    for r in rec.wgrad:
        u = r["u"]
        name = rec.names[id(u)]
        B_, H_, W_ = r["B"], r["H"], r["W"]
        oh, ow = (H_ + 2 * u.pad - u.k) // u.stride + 1, (W_ + 2 * u.pad - u.k) // u.stride + 1
        xin = r["a_in"].view(B_, H_, W_, u.cin)
        dy = r["dy"].view(B_, oh, ow, u.cout)
        ref = la.conv_wgrad(xin, dy, u.k, u.stride, u.pad)
        mag = la.conv_wgrad(xin.double().abs(), dy.double().abs(), u.k, u.stride, u.pad)
        d, _, _ = _desc(B_, H_, W_, u)
        nb = rec.lib.creid_conv2d_wgrad_x3_workspace_bytes(C.byref(d)) if x3 else \
            rec.lib.creid_conv2d_wgrad_workspace_bytes(C.byref(d), eng.dt)
        splits = max(1, nb // (u.cout * u.cin * u.k * u.k * 4))
        M = B_ * oh * ow
        per = -(-M // splits) + 64 + splits            # (+ 64: a split's length is rounded up to whole 64- or 16-pixel k-steps)
        e = per * la.U * mag + (la.SPLIT * mag if x3 else 0.0)
        au.check(name, "wgrad" + (" [bnfin carrier]" if r["bnfin"] else ""), u.conv.weight.grad, ref, e, F32, bias=False,
                 sigma=math.sqrt(per) * la.U * mag + (la.SPLIT * mag if x3 else 0.0), rel_bar=2e-5 if x3 else None,
                 report_max_rms=x3)
    st = eng.stem
    H, W = rec.H, rec.W
    img = sv.stem.xpad[:, 3:3 + H, 3:3 + W, :3]
    dy0 = rec.stem_dx.view(B, H // 2, W // 2, 64)
    ref = la.conv_wgrad(img, dy0, 7, 2, 3)
    mag = la.conv_wgrad(img.double().abs(), dy0.double().abs(), 7, 2, 3)
    splits = max(1, rec.lib.creid_stem_conv_wgrad_workspace_bytes(B, H, W, eng.dt) // (64 * 256 * 4))
    per = -(-(B * (H // 2) * (W // 2)) // splits) + 64 + splits
    au.check("stem", "wgrad (creid_stem_conv_wgrad)", st.conv.weight.grad, ref, per * la.U * mag, F32, bias=False,
             sigma=math.sqrt(per) * la.U * mag)
    # BatchNorm / InstanceNorm gamma and beta gradients (one backward per parameter per step, gradients zeroed first)
    pname = {}
    for u in eng.all_units():
        nm = rec.names[id(u)]
        pname[u.bn.weight], pname[u.bn.bias] = nm, nm
        if u.ibn is not None:
            pname[u.ibn.IN.weight], pname[u.ibn.IN.bias] = nm, nm
    for p, (ref, d) in grads.items():
        au.check(pname[p], "dgamma/dbeta", p.grad, ref, d + la.U * ref.abs(), F32, bias=False, sigma=d + la.U * ref.abs())


def _desc(B, H, W, u):
    from centroids_reid_amd import backbone as bb
    return bb._desc(B, H, W, u.cin, u.cout, u.k, u.stride, u.pad)


def expected_routes(rec):
    """C entry points the default knobs must reach in this configuration (backbone.py: the conditions next to each route)"""
    eng = rec.eng
    need = {"creid_stem_conv_fwd", "creid_stem_conv_wgrad", "creid_maxpool3x3s2_bwd"}
    need.add("creid_bn2d_apply_dual_mask")                                      # dual apply (CREID_DUAL_APPLY=1)
    if -(-rec.B * (rec.H // 16) * (rec.W // 16) // 128) <= eng.sched.fin_apply_rows:
        need.add("creid_bn2d_finalize_apply_mask")                              # finalize + apply (CREID_FIN_APPLY=64 rows)
    need.add("creid_bn2d_apply_maxpool3x3s2" if not eng.net.stem_relu else "creid_maxpool3x3s2_fwd")
    if rec.fused:
        need.add("creid_ctl_heads_fused")
    else:
        need.add("creid_gap_bwd")
    if eng.x3_train:
        need |= {"creid_conv2d_dgrad_x3_nhwc", "creid_conv2d_wgrad_x3_nhwc"}
    else:
        need.add("creid_conv2d_wgrad_partials")                                 # split reductions carried (CREID_WRED_PIGGYBACK=1)
    if eng.dtype in (BF, F16):
        need |= {"creid_conv1x1_bnrelu_fwd",                                    # axf: bn2 + ReLU on conv3's operand path
                 "creid_bn2d_bwd_mask_reduce2",                                 # bn3 + downsample BN sums in one pass
                 "creid_conv2d_wgrad_partials_bnfin",                           # CREID_FIN_CARRIER=wgrad
                 "creid_conv2d_wgrad_reduce_job",                               # the layer's last split reduction, flushed
                 "creid_conv2d_dgrad_fused_nhwc"}                               # fused BN reduction / carried split reduction
    if eng.net.arch.endswith("_ibn_a"):
        need |= {"creid_ibn_fwd_mask", "creid_ibn_bwd_mask"}
    return need


def run_audit(rec, tag):
    au = la.Audit(tag)
    with torch.no_grad():
        audit_forward(au, rec)
        audit_backward(au, rec)
    return au


def _check_counts_and_routes(rec):
    eng = rec.eng
    c = rec.calls              # C entry points called during the step (one attribute fetch per launch)
    n_fwd = c["creid_stem_conv_fwd"] + c["creid_conv2d_fwd_nhwc"] + c["creid_conv1x1_bnrelu_fwd"]
    n_wg = c["creid_stem_conv_wgrad"] + c["creid_conv2d_wgrad_partials"] + c["creid_conv2d_wgrad_partials_bnfin"] \
        + c["creid_conv2d_wgrad_x3_nhwc"] + c["creid_conv2d_wgrad_nhwc"]
    n_bn = c["creid_bn2d_bwd_mask"] + c["creid_bn2d_bwd_mask_reduce2"] + c["creid_ibn_bwd_mask"]
    assert (n_fwd, n_wg, n_bn) == (53, 53, 53), (n_fwd, n_wg, n_bn)
    assert len(rec.wgrad) == 52 and eng.stem.conv.weight.grad is not None, len(rec.wgrad)
    assert len(rec.bn) + len(rec.ibn) == 53, (len(rec.bn), len(rec.ibn))
    missing = expected_routes(rec) - set(rec.calls)
    assert not missing, f"routes not taken: {sorted(missing)}"
    if eng.dtype in (BF, F16):
        routes = Counter(r["route"] for r in rec.bn)
        assert routes["ready2"] > 0 and routes["ready1"] > 0, routes                # carried finalize / fused partials
        assert any(r["carry"] for r in rec.dgrad), "no split reduction carried by a data gradient"
        assert any(r["stride"] == 2 for r in rec.dgrad) and any(r["add_mask"] is not None for r in rec.dgrad)
        assert any(r["reduce2"] for r in rec.bn) and any(r["bnfin"] for r in rec.wgrad)
        if rec.fused:
            assert rec.part3, "the heads did not hand over bn3's column sums"
    return sorted(rec.calls)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_layer_audit(cfg, monkeypatch):
    rec = record_step(cfg, monkeypatch)
    routes = _check_counts_and_routes(rec)
    au = run_audit(rec, cfg)
    print("\n" + au.table())
    print(au.op_summary())
    print(f"[{cfg}] C entry points: {' '.join(r[6:] for r in routes)}")
    if au.max_rms:
        worst = sorted(au.max_rms, key=lambda t: -t[2])[:3]
        print(f"[{cfg}] bf16x3 max err / rms(ref), worst: " + ", ".join(f"{l} {o} {m:.3e}" for l, o, m in worst))
    assert not au.failures, f"{len(au.failures)} failure(s):\n" + "\n".join(au.failures[:60])
    if cfg == "F-bf16":
        # the audit can fail: one channel of one recorded conv output x (1 + 2^-7) is named, and nothing else is
        target = "layer1.0.conv1"
        x1 = rec.saved.blocks[0].c1.x
        x1.view(-1, x1.shape[1])[:, 5] *= (1.0 + 2.0 ** -7)
        bad = run_audit(rec, cfg + "-perturbed")
        assert bad.failing_layers() == {target}, bad.failures[:20]
