"""GPU: every launch of one eval-mode forward against fp64, each on its OWN recorded operands, and creid_bn2d_fold_multi directly.

One real BackboneEngine.forward(x, False, True) runs through a CTLModel with the knobs at their defaults, followed by the
eval-mode BNNeck (model.bn); BatchNorm / InstanceNorm parameters and running statistics are randomised away from (1, 0, 0, 1).  The
engine's `fold_bn`, `_conv_fold`, `_conv_bn`, `_ibn_tail` and `_stem_operand` are wrapped on the instance (results cloned right
after each call: stream order makes the clone see what the launch wrote); the launches `_forward_eval_folded` issues inline with
raw pointers (pair, stem, max-pool, GAP, nhwc_to_nchw) are recorded through a proxy of the library handle that also counts every
C entry point, and their tensors are found by data_ptr() among the activations a wrapped `eng._empty` keeps alive for the whole
forward (so no buffer is recycled before it is read).  Routes are asserted from those counts against what the architecture and
the geometry rule of `_forward_eval_folded` give; running statistics and num_batches_tracked must be bit-identical afterwards.

References are torch float64 (tests/layer_audit.py, tests/eval_audit.py); nothing here calls the project's kernels.  Operands are
taken as stored: 16-bit activations as they are, the engine's own w_krsc copies (bf16x3: the fp32 masters; the copies are checked
to be their round-to-nearest-even values), the device's own fold constants in the convolution checks.

Bars (derived in tests/eval_audit.py's docstring from each kernel's arithmetic; Audit.check adds 1/2 ulp of the output type at
|ref| + b to every bound b).  "measured" = the worst over configurations A-H on one MI355X as a fraction of the bound
(profiles/eval_audit.md has the per-layer tables):
* fold constants: 4 u |sc| for the scale (add, square root, division, product: 3.5 u); u |beta| + 2 u |mean sc| + |mean| dsc for
  the shift.  Output fp32.
* stem: fp64 conv -> affine with the device's fold constants (-> ReLU) -> 3 x 3 s2 max-pool -> one rounding; b = |sc| 147 u (|x| |w|)
  + affine_bound, the window maximum of b for the pooled value.  Where two launches ran, the conv + affine output is checked too and
  the pool of the STORED tensor must be exact.  image_to_nhwc4_pad: exact, zero borders and the fourth channel included.
* every folded convolution (plain, ReLU, residual + ReLU, the downsample without ReLU, strides 1 and 2, the BasicBlock's second
  3 x 3): b = |sc| K u (|x| |w|) + affine_bound, bf16x3: + |sc| 2^-16 (|x| |w|).  With a residual on a 16-bit output the epilogue
  rounds the affine result to the storage type, adds the residual in fp32 and rounds again (add_chunk on a packed chunk):
  + 1/2 ulp_16(|affine| + b) + 2 u (|affine| + |residual|).  bf16x3 keeps the x3 layer bars: rel-L2 <= 2e-5 and max <= 1e-4 rms of the
  pre-activation reference.
* pair launches: the block output as a folded conv3 with residual; the conv1 output against fp64 on the STORED block output
  (K = 256), folded bn1 + ReLU; on the statistics route the raw output (K u |x| |w|) and its [tiles][2][64] partials
  (eval_audit.check_tile_partials).
* eval-mode IBN: per-image mean / invstd of the InstanceNorm half against fp64 statistics of the unrounded conv output
  (layer_audit.stats_bound, count = HW) where the partials came ready from the producing launch, of the stored tensor where
  HW % 128 != 0 and the kernel sums it itself; BatchNorm half: the running mean exactly, 1 / sqrtf(var + eps) to 3 u; the applied
  output with affine_bound.
* GAP: HW u mean|a| + u |ref|; creid_nhwc_to_nchw_f32: exact; the embedding (creid_bn1d_fwd on running statistics):
  6 u |(x - mean) invstd gamma| + u |y|.
Bias and relative-L2 bars: Audit.check's docstring.

Measured = ... of the bound (16-bit / fp32 / bf16x3 where they differ): fold scale 0.48, shift 0.49 (direct test: 0.38 / 0.50);
stem 0.994 / 0.034; folded conv 0.998 / 0.069 / 0.25, + ReLU 0.997 / 0.056 / 0.19, + residual + ReLU 0.999 / 0.074 / 0.43 (16-bit:
results exactly half-way, RNE's own bound); pair conv3 0.999, conv1 0.988, raw conv1 0.987, its tile sums 0.0018 / 0.0011; raw conv
feeding IBN 0.998; IN mean 0.0074, IN invstd 0.025, BN-half invstd 0.44, IBN apply 1.0 (half-way results); GAP 0.091; embedding
0.51.  |bias| <= 0.0087 ulp (bar >= 0.01), rel-L2 <= 0.69 of its bar (0.667 = the ulp / sqrt(12) of unbiased rounding under a bar
of 1.5x that); bf16x3: rel-L2 <= 5.6e-6 (bar 2e-5), max <= 3.9e-5 rms (bar 1e-4).  No bound needed a correction: the two-rounding
residual epilogue is in the bound from the start (tests/test_eval_audit_cpu.py shows the one-rounding bound failing on it).
Configuration G: stem_check_shape accepts 100 x 52, so G runs as the issue proposes.
Runtime on one MI355X: 0.8 - 1.4 s per configuration in a process of its own (first launches included), 0.1 - 0.3 s each after the
first one in a shared process (4.2 s for the eight), the three fold tests 0.3 s.
"""
import ctypes as C
import time
from collections import Counter
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import eval_audit as ea
import layer_audit as la

pytestmark = pytest.mark.gpu

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
CONFIGS = {        # mode, arch, B, H, W
    "A": ("bf16", "resnet50", 5, 256, 128),          # fused stem + pool; two pair-affine launches of 80 tiles
    "B": ("f16", "resnet50", 5, 256, 128),           # the same on the f16 MFMA
    "C": ("fp32", "resnet50", 3, 128, 64),           # two-launch stem, no pair, fp32 GEMM
    "D": ("bf16x3", "resnet50", 3, 128, 64),         # conv_x3.hip folded forward
    "E": ("bf16", "resnet50_ibn_a", 3, 64, 64),      # layer1 map 16 x 16: pair-statistics launches, IBN from ready partials
    "F": ("bf16", "resnet50_ibn_a", 2, 96, 80),      # layer1 map 24 x 20 = 480: pair declined, IBN sums the stored tensor
    "G": ("f16", "resnet50", 3, 100, 52),            # H % 8 != 0: 16-bit two-launch stem, pair M = 975, odd maps in layer3 / 4
    "H": ("bf16", "resnet18", 3, 128, 64),           # BasicBlock: residual inside the second 3 x 3's epilogue
}
MODES = {"bf16": BF, "f16": F16, "fp32": F32}


# ------------------------------------------------------------------------------------------- recording
class _LibProxy:
    """counts every C entry point called and hands (arguments, return code) of the hooked ones to the recorder"""

    def __init__(self, lib, rec):
        self._lib, self._rec = lib, rec

    def __getattr__(self, name):
        fn, rec = getattr(self._lib, name), self._rec

        def call(*args):
            rc = fn(*args)
            rec.calls[name] += 1
            hook = rec.hooks.get(name)
            if hook is not None:
                hook(args, rc)
            return rc
        return call


def _addr(a):
    return a.value if isinstance(a, C.c_void_p) else a


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


def _randomise(model, seed):
    """BatchNorm / InstanceNorm affine parameters and running statistics away from (1, 0, 0, 1): a dropped gamma, beta, mean or
    variance must show"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, "weight") and hasattr(m, "bias") and m.weight is not None and m.weight.dim() == 1 and m.bias is not None \
                    and m.weight.requires_grad:
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g, device="cuda"))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g, device="cuda"))
            if hasattr(m, "running_mean"):
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g, device="cuda"))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g, device="cuda"))


def _bn_state(model):
    return {n: b.clone() for n, b in model.named_buffers() if n.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked")}


def record_forward(cfg, monkeypatch):
    from centroids_reid_amd import _lib as L
    from centroids_reid_amd.config import get_cfg_defaults
    from centroids_reid_amd.train_ctl_model import CTLModel
    mode, arch, B, H, W = CONFIGS[cfg]
    torch.manual_seed(0)                                     # (the holders' initial weights)
    c = get_cfg_defaults()
    c.MODEL.PRETRAINED = False
    c.MODEL.NAME = arch
    c.MODEL.BACKBONE_EMB_SIZE = 512 if arch == "resnet18" else 2048
    c.USE_MIXED_PRECISION = mode != "fp32"
    if mode == "bf16x3":                                     # the shipped use of the mode: an fp32 model evaluated in bf16x3
        model = CTLModel(c, num_classes=751, num_query=0, compute_dtype=F32, eval_precision="bf16x3").cuda()
    else:
        model = CTLModel(c, num_classes=751, num_query=0, compute_dtype=MODES[mode]).cuda()
    _randomise(model, 11)
    model.backbone.eval()
    model.bn.eval()
    eng = model.backbone.engine_for(False)
    assert eng.sched.eval_fold and eng.x3 == (mode == "bf16x3")
    rec = SimpleNamespace(eng=eng, model=model, names=_names(eng), mode=mode, arch=arch, B=B, H=H, W=W, calls=Counter(), hooks={},
                          keep=[], by_ptr={}, folds={}, convs=[], raw={}, ibn=[], pairs=[], stem={}, xpad=None, gap=None, nchw=None,
                          ibn_flags=[])
    rec.state0 = _bn_state(model)
    real_lib = L.lib()
    monkeypatch.setattr(L, "lib", lambda: _LibProxy(real_lib, rec))
    o_empty, o_fold, o_cf, o_cb, o_it, o_so = eng._empty, eng.fold_bn, eng._conv_fold, eng._conv_bn, eng._ibn_tail, eng._stem_operand

    def empty(*shape, dtype=None):
        t = o_empty(*shape, dtype=dtype)
        rec.keep.append(t)                                   # alive until the audit is done: no activation is recycled
        rec.by_ptr[t.data_ptr()] = t
        return t

    def fold_bn():
        o_fold()
        rec.folds = {id(u): u.fold.clone() for u in eng.all_units() if u.ibn is None}

    def conv_fold(u, a_in, B_, H_, W_, relu, residual=None):
        out = o_cf(u, a_in, B_, H_, W_, relu, residual)
        rec.convs.append(dict(u=u, a_in=a_in, B=B_, H=H_, W=W_, relu=relu, residual=residual, out=out[0].clone()))
        return out

    def conv_bn(u, a_in, B_, H_, W_, training, relu, residual=None, residual_ss=None, apply=True):
        out = o_cb(u, a_in, B_, H_, W_, training, relu, residual, residual_ss, apply)
        rec.raw[id(u)] = dict(u=u, a_in=a_in, B=B_, H=H_, W=W_, x=out.x.clone())
        return out

    def ibn_tail(u, x, B_, h_, w_, training, relu, part=None):
        out = o_it(u, x, B_, h_, w_, training, relu, part)           # (the SavedLayer of the IBN layer)
        rec.ibn.append(dict(u=u, x=x, B=B_, HW=h_ * w_, training=training, relu=relu, ready=part is not None, a=out.act.clone(),
                            mean=out.mean.clone(), invstd=out.invstd.clone()))
        return out

    def stem_operand(x, B_, H_, W_):
        out = o_so(x, B_, H_, W_)
        rec.xpad = out.clone()
        return out

    for n, f in (("_empty", empty), ("fold_bn", fold_bn), ("_conv_fold", conv_fold), ("_conv_bn", conv_bn), ("_ibn_tail", ibn_tail),
                 ("_stem_operand", stem_operand)):
        monkeypatch.setattr(eng, n, f)

    def t(a):
        return rec.by_ptr[_addr(a)]

    def pair(stats):
        def hook(a, rc):
            assert rc == 0, rc
            # (M, c_mid, c_out, c_next, a2, w3, fold3, residual, out3, w1, fold1 | out1, out1 | partials, dtype, stream)
            p = dict(stats=stats, M=a[0], a2=t(a[4]), w3=_addr(a[5]), res=t(a[7]), out3=t(a[8]).clone(), w1=_addr(a[9]))
            if stats:
                p.update(out1=t(a[10]).clone(), part=t(a[11]).clone())
            else:
                p.update(out1=t(a[11]).clone())
            rec.pairs.append(p)
        return hook

    rec.hooks["creid_bottleneck_c3_c1_fwd_affine"] = pair(False)
    rec.hooks["creid_bottleneck_c3_c1_fwd_stats"] = pair(True)
    rec.hooks["creid_stem_conv_pool_fwd_affine"] = lambda a, rc: rec.stem.update(fused_rc=rc, **({"pooled": t(a[5]).clone()} if rc == 0 else {}))
    rec.hooks["creid_stem_conv_fwd_affine"] = lambda a, rc: rec.stem.update(y0=t(a[5]).clone())
    rec.hooks["creid_maxpool3x3s2_fwd"] = lambda a, rc: rec.stem.update(pooled=t(a[6]).clone(), taps=_addr(a[7]))
    rec.hooks["creid_gap_fwd"] = lambda a, rc: setattr(rec, "gap", dict(a=t(a[0]), B=a[1], HW=a[2], C=a[3]))
    rec.hooks["creid_nhwc_to_nchw_f32"] = lambda a, rc: setattr(rec, "nchw", dict(a=t(a[0]), B=a[1], HW=a[2], C=a[3]))
    rec.hooks["creid_ibn_fwd_mask"] = lambda a, rc: rec.ibn_flags.append(dict(training=a[11], ready=a[17]))

    gen = torch.Generator(device="cuda").manual_seed(5)
    rec.x = torch.randn((B, 3, H, W), generator=gen, device="cuda")
    with torch.no_grad():
        rec.base_out, rec.feat = eng.forward(rec.x, False, True)
        rec.emb = model.bn(rec.feat)
    torch.cuda.synchronize()
    monkeypatch.undo()
    rec.state1 = _bn_state(model)
    return rec


# ------------------------------------------------------------------------------------------- expected routes
def expected_routes(rec):
    """what the default knobs must launch, from the architecture and the geometry rule of _forward_eval_folded"""
    eng = rec.eng
    is16 = eng.dtype in (BF, F16)
    exp = Counter()
    # the one-launch stem exists for 16-bit images 128 or 320 wide whose height is a multiple of 8 (conv_stem.hip); fp32 never asks
    exp["stem_fused_rc"] = None if not is16 else (0 if (rec.W in (128, 320) and rec.H % 8 == 0) else -4)
    h, w = rec.H // 4, rec.W // 4
    ready = []
    prev_pair = False
    for bi, b in enumerate(eng.blocks):
        if eng.basic:
            exp["affine"] += 2 + (b["ds"] is not None)
            continue
        s = b["c2"].stride
        h2, w2 = (h + 2 - 3) // s + 1, (w + 2 - 3) // s + 1
        if b["c1"].ibn is not None:
            ready.append((h * w) % 128 == 0)
            if not prev_pair:
                exp["fwd_raw"] += 1
        elif not prev_pair:
            exp["affine"] += 1
        exp["affine"] += 1 + (b["ds"] is not None)           # conv2, downsample
        nb = eng.blocks[bi + 1] if bi + 1 < len(eng.blocks) else None
        pair = (is16 and nb is not None and nb["ds"] is None and (b["c3"].cin, b["c3"].cout, nb["c1"].cout) == (64, 256, 64)
                and (nb["c1"].ibn is None or (h2 * w2) % 128 == 0))
        if pair:
            exp["pair_stats" if nb["c1"].ibn is not None else "pair_affine"] += 1
        else:
            exp["affine"] += 1                               # conv3
        prev_pair = pair
        h, w = h2, w2
    exp["ibn_ready"] = ready
    return exp


def check_routes(rec):
    c, exp = rec.calls, expected_routes(rec)
    got_ready = [bool(f["ready"]) for f in rec.ibn_flags]
    assert all(f["training"] == 0 for f in rec.ibn_flags)
    assert c["creid_bn2d_fold_multi"] == 1 and c["creid_gap_fwd"] == 1 and c["creid_nhwc_to_nchw_f32"] == 1 and c["creid_bn1d_fwd"] == 1
    assert c["creid_image_to_nhwc4_pad"] == 1
    assert c["creid_bottleneck_c3_c1_fwd_affine"] == exp["pair_affine"], (c["creid_bottleneck_c3_c1_fwd_affine"], exp["pair_affine"])
    assert c["creid_bottleneck_c3_c1_fwd_stats"] == exp["pair_stats"], (c["creid_bottleneck_c3_c1_fwd_stats"], exp["pair_stats"])
    assert c["creid_conv2d_fwd_affine_nhwc"] == exp["affine"], (c["creid_conv2d_fwd_affine_nhwc"], exp["affine"])
    assert c["creid_conv2d_fwd_nhwc"] == exp["fwd_raw"], (c["creid_conv2d_fwd_nhwc"], exp["fwd_raw"])
    assert got_ready == exp["ibn_ready"], (got_ready, exp["ibn_ready"])
    if exp["stem_fused_rc"] is None:
        assert c["creid_stem_conv_pool_fwd_affine"] == 0
    else:
        assert c["creid_stem_conv_pool_fwd_affine"] == 1 and rec.stem["fused_rc"] == exp["stem_fused_rc"], rec.stem.get("fused_rc")
    two = exp["stem_fused_rc"] != 0
    assert c["creid_stem_conv_fwd_affine"] == int(two) and c["creid_maxpool3x3s2_fwd"] == int(two)
    if two:
        assert rec.stem["taps"] is None                      # eval: no argmax taps are written
    # training-mode launches have no place in an eval forward
    for name in ("creid_bn2d_finalize", "creid_bn2d_finalize_apply_mask", "creid_bn2d_apply_mask", "creid_bn2d_apply_dual_mask",
                 "creid_stem_conv_fwd", "creid_gap_fwd_count", "creid_conv1x1_bnrelu_fwd"):
        assert c[name] == 0, name
    return dict(stem_fused_rc=exp["stem_fused_rc"], pair_affine=exp["pair_affine"], pair_stats=exp["pair_stats"], affine=exp["affine"],
                fwd_raw=exp["fwd_raw"], ibn_ready=f"{sum(got_ready)} of {len(got_ready)}")


# ------------------------------------------------------------------------------------------- audit
def _fwd_w(rec, u):
    if rec.eng.x3:
        return u.conv.weight.detach().double()
    return u.w_krsc.permute(0, 3, 1, 2).double()


def _weight_copies_check(au, rec):
    eng = rec.eng
    bad = []
    for u in eng.all_units():
        if u is eng.stem:
            continue
        krsc = u.conv.weight.detach().permute(0, 2, 3, 1)
        if eng.x3:
            hi = krsc.to(BF)
            ok = torch.equal(u.w_krsc.view(torch.int16), torch.stack([hi, (krsc - hi.float()).to(BF)]).view(torch.int16))
        else:
            ok = torch.equal(u.w_krsc, krsc.to(eng.dtype))
        if not ok:
            bad.append(rec.names[id(u)])
    au.exact("weights", "w_krsc = RNE(master)", not bad, " ".join(bad[:8]))


def _conv_op(r):
    u = r["u"]
    op = "folded conv" + (" + residual" if r["residual"] is not None else "") + (" + ReLU" if r["relu"] else "")
    return op + f" [{u.k}x{u.k} s{u.stride}]"


def run_audit(rec, tag):
    au = la.Audit(tag)
    eng, names = rec.eng, rec.names
    dt, x3 = eng.dtype, eng.x3
    B, H, W = rec.B, rec.H, rec.W
    seen = Counter()
    _weight_copies_check(au, rec)
    # fold constants of every plain BatchNorm
    for u in eng.all_units():
        if u.ibn is None:
            ea.check_fold(au, names[id(u)], rec.folds[id(u)], u.bn.weight, u.bn.bias, u.bn.running_mean, u.bn.running_var, u.bn.eps)
    # stem
    want = torch.zeros(B, H + 8, W + 6, 4, dtype=dt, device="cuda")
    want[:, 3:3 + H, 3:3 + W, :3] = rec.x.permute(0, 2, 3, 1).to(dt)
    au.exact("stem", "image_to_nhwc4_pad", torch.equal(rec.xpad, want))
    st = eng.stem
    img = rec.xpad[:, 3:3 + H, 3:3 + W, :3]
    conv, e, sig = ea.conv_reference(img, st.conv.weight.detach().to(dt).double(), 2, 3)
    ref, b, s, _ = ea.folded_reference(conv, e, sig, rec.folds[id(st)], bool(eng.net.stem_relu), None, dt)
    H1, W1 = H // 2, W // 2
    pooled = rec.stem["pooled"]
    pv, pb, ps = (la.maxpool3x3s2(v.view(B, H1, W1, 64))[0] for v in (ref, b, s))
    two = "y0" in rec.stem
    au.check("stem", "conv + bn1 + max-pool [" + ("two launches" if two else "one launch") + "]", pooled, pv, pb, dt, sigma=ps)
    if two:
        au.check("stem", "conv + bn1", rec.stem["y0"], ref, b, dt, sigma=s)
        au.exact("stem", "max-pool of the stored tensor", torch.equal(la.maxpool3x3s2(rec.stem["y0"].view(B, H1, W1, 64).double())[0],
                                                                      pooled.view(B, H1 // 2, W1 // 2, 64).double()))
    seen[id(st)] += 1
    # folded convolutions
    for r in rec.convs:
        u = r["u"]
        ea.check_folded_conv(au, names[id(u)], _conv_op(r), r["out"], r["a_in"].view(r["B"], r["H"], r["W"], u.cin), _fwd_w(rec, u),
                             u.stride, u.pad, rec.folds[id(u)], r["relu"], r["residual"], dt, x3)
        seen[id(u)] += 1
    # pair launches
    by_w = {u.w_krsc.data_ptr(): u for u in eng.all_units() if u is not st}
    pair_raw = {}
    for p in rec.pairs:
        u3, u1, M = by_w[p["w3"]], by_w[p["w1"]], p["M"]
        ea.check_folded_conv(au, names[id(u3)], "pair: conv3 + residual + ReLU", p["out3"], p["a2"].view(M, 1, 1, 64), _fwd_w(rec, u3), 1, 0,
                             rec.folds[id(u3)], True, p["res"], dt)
        seen[id(u3)] += 1
        if not p["stats"]:
            ea.check_folded_conv(au, names[id(u1)], "pair: conv1 + ReLU", p["out1"], p["out3"].view(M, 1, 1, 256), _fwd_w(rec, u1), 1, 0,
                                 rec.folds[id(u1)], True, None, dt)
            seen[id(u1)] += 1
        else:
            conv, e, sig = ea.conv_reference(p["out3"].view(M, 1, 1, 256), _fwd_w(rec, u1), 1, 0)
            au.check(names[id(u1)], "pair: raw conv1", p["out1"], conv, e, dt, sigma=sig)
            ea.check_tile_partials(au, names[id(u1)], p["part"], conv, e)
            pair_raw[id(u1)] = (conv, e, p["out1"])
    # eval-mode IBN
    for r in rec.ibn:
        u = r["u"]
        name = names[id(u)]
        if id(u) in pair_raw:
            conv, e, x_raw = pair_raw[id(u)]
            assert r["ready"]
        else:
            q = rec.raw[id(u)]
            conv, e, sig = ea.conv_reference(q["a_in"].view(q["B"], q["H"], q["W"], u.cin), _fwd_w(rec, u), u.stride, u.pad, x3)
            au.check(name, "conv fwd (raw, IBN)", q["x"], conv, e, dt, sigma=sig)
            x_raw = q["x"]
        au.exact(name, "IBN reads the conv output", torch.equal(r["x"], x_raw))
        ibn, bn = u.ibn, u.bn
        assert ibn.IN.eps == bn.eps and not r["training"] and r["relu"]
        ea.check_eval_ibn(au, name, r["x"], r["a"], r["mean"], r["invstd"], conv, e, r["B"], r["HW"], ibn.half, ibn.IN.weight, ibn.IN.bias,
                          bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, r["ready"], dt)
        seen[id(u)] += 1
    # every convolution of the network exactly once
    missing = [names[id(u)] for u in eng.all_units() if seen[id(u)] != 1]
    au.exact("coverage", "every conv unit audited once", not missing, " ".join(missing[:8]))
    # pooled features, base output, embedding
    g = rec.gap
    ea.check_gap(au, rec.feat, g["a"], g["B"], g["HW"])
    n = rec.nchw
    au.exact("base_out", "nhwc_to_nchw_f32", n["a"] is g["a"] and torch.equal(
        rec.base_out.reshape(n["B"], n["C"], n["HW"]), n["a"].view(n["B"], n["HW"], n["C"]).permute(0, 2, 1).float()))
    nb = rec.model.bn
    ea.check_bnneck(au, rec.emb, rec.feat, nb.weight, nb.bias, nb.running_mean, nb.running_var, nb.eps)
    return au


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_eval_audit(cfg, monkeypatch):
    t0 = time.perf_counter()
    rec = record_forward(cfg, monkeypatch)
    routes = check_routes(rec)
    for k, v in rec.state0.items():
        assert torch.equal(v, rec.state1[k]), f"{k} changed during an eval forward"
    assert rec.eng.saved is None
    with torch.no_grad():
        au = run_audit(rec, cfg)
    torch.cuda.synchronize()
    print("\n" + au.table())
    print(au.op_summary())
    print(f"[{cfg}] routes: " + "  ".join(f"{k}={v}" for k, v in routes.items()))
    if au.max_rms:
        worst = sorted(au.max_rms, key=lambda t: -t[2])[:3]
        print(f"[{cfg}] bf16x3 max err / rms(pre-activation ref), worst: " + ", ".join(f"{l} {o} {m:.3e}" for l, o, m in worst))
    print(f"[{cfg}] {time.perf_counter() - t0:.1f} s")
    assert not au.failures, f"{len(au.failures)} failure(s):\n" + "\n".join(au.failures[:60])


# ------------------------------------------------------------------------------------------- creid_bn2d_fold_multi, directly
WIDTHS = (1, 63, 64, 255, 256, 257, 2048, 4096)                # 4096: two passes of the grid-stride loop (grid.y = 8 x 256 threads)
VARS = (0.0, 1e-12, 1e-5, 1.0, 1e6)
MEANS = (0.0, 1e-3, -1e-3, 1e3, -1e3)
GUARD, SENT = 16, 0x5A5A5A5A


def _fold_table(entries):
    """entries: (C, eps, null gamma, null beta, seed).  The table as BackboneEngine.fold_bn builds it, the outputs in ONE shared
    buffer with GUARD sentinel words before, between and behind the [2][C] blocks."""
    from centroids_reid_amd import _lib as L
    rec = np.zeros(len(entries), dtype=np.dtype([("g", "<u8"), ("b", "<u8"), ("m", "<u8"), ("v", "<u8"), ("o", "<u8"), ("C", "<i4"),
                                                  ("eps", "<f4")]))
    assert L.lib().creid_bn2d_fold_entry_bytes() == rec.dtype.itemsize == 48
    total = GUARD + sum(2 * e[0] + GUARD for e in entries)
    buf = torch.full((total,), SENT, dtype=torch.int32, device="cuda")
    out = buf.view(torch.float32)
    ops, o = [], GUARD
    for i, (Cc, eps, ng, nb, seed) in enumerate(entries):
        g = torch.Generator(device="cuda").manual_seed(seed)
        c = torch.arange(Cc, device="cuda")
        var = torch.tensor(VARS, device="cuda")[(c + i) % 5]                       # every (var, mean) pair within 25 channels
        mean = torch.tensor(MEANS, device="cuda")[(c // 5 + i) % 5]
        gamma = None if ng else (0.5 + torch.rand(Cc, generator=g, device="cuda")) * (1 - 2 * (c % 3 == 0)).float()
        beta = None if nb else torch.randn(Cc, generator=g, device="cuda")
        ops.append((gamma, beta, mean.contiguous(), var.contiguous(), eps, o, Cc))
        rec[i] = (0 if ng else gamma.data_ptr(), 0 if nb else beta.data_ptr(), ops[-1][2].data_ptr(), ops[-1][3].data_ptr(),
                  out.data_ptr() + 4 * o, Cc, eps)
        o += 2 * Cc + GUARD
    tab = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    return tab, buf, out, ops


def _run_fold(entries, tag):
    from centroids_reid_amd import _lib as L
    tab, buf, out, ops = _fold_table(entries)
    L.check(L.lib().creid_bn2d_fold_multi(L.ptr(tab), len(entries), L.stream()), "bn2d_fold_multi")
    torch.cuda.synchronize()
    au = la.Audit(tag)
    owned = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
    for i, (gamma, beta, mean, var, eps, o, Cc) in enumerate(ops):
        ea.check_fold(au, f"entry{i} C={Cc} eps={eps:g}" + (" null-gamma" if gamma is None else "") + (" null-beta" if beta is None else ""),
                      out[o:o + 2 * Cc].view(2, Cc), gamma, beta, mean, var, eps)
        owned[o:o + 2 * Cc] = True
    assert bool((buf[~owned] == SENT).all()), "words outside the entries' [2][C] blocks were written"
    assert int((~owned).sum()) == GUARD * (len(entries) + 1)
    assert not au.failures, f"{len(au.failures)} failure(s):\n" + "\n".join(au.failures[:40])
    return {op: max(r[2] for r in au.rows if r[1] == op) for op in ("fold scale", "fold shift")}


@pytest.mark.parametrize("eps", [1e-5, 1e-3])
def test_fold_multi_single_entry(eps):
    """n_entries = 1 at every width, null gamma / beta entries included"""
    worst = {"fold scale": 0.0, "fold shift": 0.0}
    for k, Cc in enumerate(WIDTHS):
        for ng, nb in ((False, False), (True, False), (False, True), (True, True)) if Cc in (1, 257, 4096) else ((False, False),):
            w = _run_fold([(Cc, eps, ng, nb, 100 + k)], f"fold1 C={Cc}")
            worst = {k_: max(worst[k_], w[k_]) for k_ in worst}
    print(f"\n[fold1 eps={eps:g}] max err / bound: " + ", ".join(f"{k_} {v:.3f}" for k_, v in worst.items()))


def test_fold_multi_sixty_entries():
    """n_entries = 60: every width, both eps values, null gamma / beta entries, neighbours in one buffer"""
    entries = [(WIDTHS[i % 8], (1e-5, 1e-3)[(i // 8) % 2], i % 5 == 3, i % 7 == 2, 200 + i) for i in range(60)]
    assert any(e[2] and e[3] for e in entries)
    w = _run_fold(entries, "fold60")
    print("\n[fold60] max err / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))
