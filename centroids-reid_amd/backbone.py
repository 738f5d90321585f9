"""Stage A host side: ResNet50 / ResNet50-IBN-a on the HIP layer kernels.

`ResNet` / `ResNet_IBN` mirror the module tree of modelling/backbones/resnet.py:90-133 and
resnet_ibn_a.py:77-141 as pure PARAMETER HOLDERS (same attribute names -> same state_dict keys:
conv1.weight, bn1.running_mean, layer1.0.downsample.0.weight, ...; master weights stay fp32 OIHW
like the reference's checkpoints).  The arithmetic is done by `BackboneEngine`, an explicit
forward/backward schedule over NHWC activations that calls the C ABI (implicit-GEMM convs on the
MFMA pipe with BN statistics fused into the epilogue, fused BN+residual+ReLU, transposing-LDS
wgrad); torch only provides memory, the stream and the autograd hook at the module boundary.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os
import weakref

import torch
from torch import nn

from . import _lib as L

LAYERS = (3, 4, 6, 3)
PLANES = (64, 128, 256, 512)


# ----------------------------------------------------------------------------- holders
class Conv2d(nn.Module):
    def __init__(self, cin, cout, k, stride=1, padding=0):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding = cin, cout, k, stride, padding
        w = torch.empty(cout, cin, k, k)
        w.normal_(0, math.sqrt(2.0 / (k * k * cout)))           # resnet.py:156-160 random_init
        self.weight = nn.Parameter(w)


class BatchNorm2d(nn.Module):
    def __init__(self, c, eps=1e-5, momentum=0.1):
        super().__init__()
        self.num_features, self.eps, self.momentum = c, eps, momentum
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, 1)
        self.bn1 = BatchNorm2d(planes)
        self.conv2 = Conv2d(planes, planes, 3, stride, 1)
        self.bn2 = BatchNorm2d(planes)
        self.conv3 = Conv2d(planes, planes * 4, 1)
        self.bn3 = BatchNorm2d(planes * 4)
        self.downsample = downsample
        self.stride = stride


class BasicBlock(nn.Module):
    """modelling/backbones/resnet.py:22-48 (resnet18 / resnet34): conv3x3(stride) - bn - relu - conv3x3 - bn, + residual, relu."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, 3, stride, 1)
        self.bn1 = BatchNorm2d(planes)
        self.conv2 = Conv2d(planes, planes, 3, 1, 1)
        self.bn2 = BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride


class ResNet(nn.Module):
    """Parameter tree of modelling/backbones/resnet.py:90-120 (Bottleneck, layers [3,4,6,3])."""
    arch = "resnet50"
    stem_relu = False            # resnet.py:97,125 -- the stem ReLU is commented out upstream

    def __init__(self, last_stride=2, block=Bottleneck, layers=LAYERS):
        super().__init__()
        self.inplanes = 64
        self.conv1 = Conv2d(3, 64, 7, 2, 3)
        self.bn1 = BatchNorm2d(64)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=last_stride)
        self.out_channels = 512 * block.expansion          # Baseline.in_planes: 2048, or 512 for the BasicBlock networks

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(Conv2d(self.inplanes, planes * block.expansion, 1, stride, 0),
                                       BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes))
        return nn.Sequential(*layers)

    def load_param(self, model_path):
        """resnet.py:135-154: strip 'backbone.base.' / 'base.' prefixes, skip fc/bottleneck/classifier."""
        param_dict = torch.load(model_path, map_location="cpu", weights_only=False)
        if "state_dict" in param_dict:
            param_dict = param_dict["state_dict"]
        own = self.state_dict()
        for i in param_dict:
            if "backbone" in i:
                name = i[14:]
            elif "base" in i:
                name = i[5:]
            else:
                name = i
            if any(t in i for t in ("fc", "bottleneck", "classifier", "transformer")):
                continue
            own[name].copy_(param_dict[i])


class InstanceNorm2d(nn.Module):
    def __init__(self, c, eps=1e-5):
        super().__init__()
        self.num_features, self.eps = c, eps
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))


class IBN(nn.Module):
    """resnet_ibn_a.py:18-32: first half of the channels InstanceNorm2d(affine), second half BatchNorm2d."""

    def __init__(self, planes):
        super().__init__()
        self.half = int(planes / 2)
        self.IN = InstanceNorm2d(self.half)
        self.BN = BatchNorm2d(planes - self.half)


class Bottleneck_IBN(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, ibn=False, stride=1, downsample=None):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, 1)
        self.bn1 = IBN(planes) if ibn else BatchNorm2d(planes)
        self.conv2 = Conv2d(planes, planes, 3, stride, 1)
        self.bn2 = BatchNorm2d(planes)
        self.conv3 = Conv2d(planes, planes * 4, 1)
        self.bn3 = BatchNorm2d(planes * 4)
        self.downsample = downsample
        self.stride = stride


class _UnusedFC(nn.Module):
    """resnet_ibn_a.py:92-93: the IBN backbone carries an unused Linear(2048 -> 1000) in its state_dict."""

    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(cout, cin), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)


class ResNet_IBN(ResNet):
    """Parameter tree of modelling/backbones/resnet_ibn_a.py:77-124 (IBN in bn1 of layer1-3, stem WITH ReLU)."""
    arch = "resnet50_ibn_a"
    stem_relu = True             # resnet_ibn_a.py:129

    def __init__(self, last_stride=2, layers=LAYERS, num_classes=1000):
        nn.Module.__init__(self)
        self.inplanes = 64
        self.conv1 = Conv2d(3, 64, 7, 2, 3)
        self.bn1 = BatchNorm2d(64)
        self.layer1 = self._make_ibn_layer(64, layers[0])
        self.layer2 = self._make_ibn_layer(128, layers[1], stride=2)
        self.layer3 = self._make_ibn_layer(256, layers[2], stride=2)
        self.layer4 = self._make_ibn_layer(512, layers[3], stride=last_stride)
        self.out_channels = 2048
        self.fc = _UnusedFC(512 * 4, num_classes)

    def _make_ibn_layer(self, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * 4:
            downsample = nn.Sequential(Conv2d(self.inplanes, planes * 4, 1, stride, 0), BatchNorm2d(planes * 4))
        ibn = planes != 512                                                       # resnet_ibn_a.py:116-118
        layers = [Bottleneck_IBN(self.inplanes, planes, ibn, stride, downsample)]
        self.inplanes = planes * 4
        for _ in range(1, blocks):
            layers.append(Bottleneck_IBN(self.inplanes, planes, ibn))
        return nn.Sequential(*layers)

    def load_param(self, model_path):
        """resnet_ibn_a.py:143-162."""
        param_dict = torch.load(model_path, map_location="cpu", weights_only=False)
        if "state_dict" in param_dict:
            param_dict = param_dict["state_dict"]
        own = self.state_dict()
        for i in param_dict:
            if any(t in i for t in ("fc", "bottleneck", "reduce_embeddings.weight", "classifier")):
                continue
            own[i[5:] if "base" in i else i].copy_(param_dict[i])


def resnet50_ibn_a(last_stride, **kwargs):
    return ResNet_IBN(last_stride, LAYERS, **kwargs)


# the deeper Bottleneck variants of MODEL.NAME (modelling/baseline.py:73-81, resnet_ibn_a.py:173-181): same kernels, same
# engine, other block counts (the engine walks whatever blocks the parameter tree holds)
ARCH_LAYERS = {"resnet50": (3, 4, 6, 3), "resnet101": (3, 4, 23, 3), "resnet152": (3, 8, 36, 3),
               "resnet50_ibn_a": (3, 4, 6, 3), "resnet101_ibn_a": (3, 4, 23, 3),
               "resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}          # BasicBlock networks (modelling/baseline.py:56-65), round 6


def build_backbone(arch, last_stride):
    if arch not in ARCH_LAYERS:
        raise NotImplementedError(f"MODEL.NAME={arch!r}: the reference's Baseline knows {sorted(ARCH_LAYERS)} (modelling/baseline.py:56-81)")
    layers = ARCH_LAYERS[arch]
    if arch.endswith("_ibn_a"):
        net = ResNet_IBN(last_stride, layers)
    else:
        net = ResNet(last_stride, block=BasicBlock if arch in ("resnet18", "resnet34") else Bottleneck, layers=layers)
    net.arch = arch
    return net


# ----------------------------------------------------------------------------- engine
def _desc(B, H, W, cin, cout, k, stride, pad):
    oh = (H + 2 * pad - k) // stride + 1
    ow = (W + 2 * pad - k) // stride + 1
    return L.ConvDesc(B, H, W, cin, oh, ow, cout, k, k, stride, pad), oh, ow


class _ConvUnit:
    """conv + BN bookkeeping for one (holder conv, holder bn) pair."""
    __slots__ = ("conv", "bn", "ibn", "w_krsc", "w_crsk", "k", "stride", "pad", "cin", "cout", "fold")

    def __init__(self, conv, bn):
        self.ibn = bn if isinstance(bn, IBN) else None
        self.conv, self.bn = conv, (bn.BN if isinstance(bn, IBN) else bn)
        self.k, self.stride, self.pad = conv.kernel_size, conv.stride, conv.padding
        self.cin, self.cout = conv.in_channels, conv.out_channels
        self.w_krsc = self.w_crsk = None
        self.fold = None               # eval mode: BatchNorm as a per-channel affine, float [2][cout] (view of one flat buffer)


@dataclasses.dataclass(slots=True)
class SavedLayer:
    """One convolution + normalisation of a forward, as its helper returns it and as the backward reads it (no temporaries).
    `act`: the normalised output, or None where the layer kept statistics only and its apply rides in another launch (`ss`,
    scale / shift, is set until that launch has read it).  `bits`: the ReLU mask, one bit per element -- it lives nowhere else.
    `relu` = False: no ReLU follows the normalisation, the backward masks by neither `act` nor `bits`."""
    unit: _ConvUnit
    x: torch.Tensor                # raw convolution output [M, cout]
    mean: torch.Tensor
    invstd: torch.Tensor
    h: int
    w: int
    relu: bool
    act: torch.Tensor = None
    bits: torch.Tensor = None
    ss: torch.Tensor = None

    @property
    def hw(self):
        return self.h * self.w


@dataclasses.dataclass(slots=True)
class SavedBlock:
    a_in: torch.Tensor             # the block's input [B hin win, cin]
    hin: int
    win: int
    c1: SavedLayer
    c2: SavedLayer
    c3: SavedLayer = None          # None: BasicBlock
    ds: SavedLayer = None          # None: identity shortcut


@dataclasses.dataclass(slots=True)
class SavedStem:
    xpad: torch.Tensor
    bn: SavedLayer                 # x = conv1's output (x0); act = the full-resolution bn1 output (y0), None when bn1 + max-pool ran fused
    idx: torch.Tensor              # the max-pool's taps


@dataclasses.dataclass(slots=True)
class SavedStep:
    B: int
    H: int
    W: int
    stem: SavedStem
    blocks: list
    final: tuple                   # (h, w) of the last feature map
    gem: tuple = None              # pooling="gem": (the last feature map, what creid_gem_fwd saved)


@dataclasses.dataclass(slots=True)
class WredJob:
    """A weight gradient's split reduction that waits for a launch to ride in."""
    desc: L.ConvDesc
    grad: torch.Tensor
    ws: torch.Tensor
    nbytes: int


@dataclasses.dataclass(frozen=True)
class Schedule:
    """Which launches the engine issues and in which order, decided once per engine by resolve_schedule()."""
    # training forward writes each ReLU's mask as bits (1 byte per 8 channels); the BatchNorm backward and the fused
    # data-gradient epilogue read that instead of re-reading the activation (CREID_RELU_BITMASK=0: read the activation)
    relu_bitmask: bool
    stem_fuse_pool: bool           # CREID_STEM_FUSE: bn1 + maxpool in one pass (38 vs 51 us)
    stem_pool_fused: bool          # CREID_STEM_POOL, eval: conv1 + bn1 + maxpool in one launch
    pair_fused: bool               # CREID_PAIR_FUSE, eval, layer1: conv3 of block i + conv1 of block i + 1
    # CREID_STEM_FUSE_BWD: the backward counterpart (max-pool gradient gathered inside the BN backward passes) is correct but
    # slower: the gather is VALU-bound and runs twice (146 vs 116 us, tools/debug/stem_tail_probe.py) -- off by default
    stem_fuse_pool_bwd: bool
    drop_gm: bool                  # CREID_DROP_GM, A/B knob: 0 = bn3's backward still writes the masked copy
    fuse_bn_reduce: bool           # CREID_FUSE_BN_REDUCE: BatchNorm-backward column sums in the data-gradient epilogue (16-bit, DMA)
    # eval-mode forward: BatchNorm (running statistics = constants) folded into the producing convolution's epilogue --
    # one launch per conv instead of conv -> finalize -> apply (CREID_EVAL_FOLD=0: the three-launch schedule).  The folded epilogue
    # of the 16-bit types lives in the LDS-DMA kernels only: with CREID_IGEMM_DMA=0 a bf16 forward takes the three-launch schedule
    # instead of failing.  bf16x3 exists as the folded forward only: no statistics / apply schedule
    eval_fold: bool
    # training forward: bn2 + ReLU applied inside conv3's operand path (creid_conv1x1_bnrelu_fwd) for the bottlenecks whose
    # width (conv3's input channels, 64 or 128) is listed in CREID_C3_AXF -- the stand-alone apply pass of bn2 disappears; "" = never.
    # Measured (profiles/r06_bn_apply_in_conv3.md): layer2 (128) gains ~8 us per block, layer1 (64) loses ~3 us per block
    c3_axf: frozenset
    ds_reduce2: bool               # CREID_DS_REDUCE2: bn3's backward apply also sums the downsample BatchNorm's columns
    dual_apply: bool               # CREID_DUAL_APPLY, A/B knob: 0 = separate downsample-BN apply launch
    # training forward: BatchNorm finalize + apply as ONE launch on layers with at most CREID_FIN_APPLY statistic rows (M <= 8192
    # by default: 24 launches less per B = 64 step at the same step time -- captured and eager --, bit-identical:
    # profiles/r05_fin_apply.md; 0 = never); CREID_FIN_APPLY_RB = row blocks of that launch (0 = library rule)
    fin_apply_rows: int
    fin_apply_rb: int
    # weight-gradient split reductions ride in the first workgroups of the NEXT data-gradient launch
    # (creid_conv2d_dgrad_fused_nhwc) instead of 53 stand-alone 5-25 us launches; CREID_WRED_PIGGYBACK=0: round-1 path.
    # (bf16x3 weight gradients: partial tiles + the fp32 split reduction in one call, creid_conv2d_wgrad_x3_nhwc)
    wred_piggyback: bool
    # CREID_FIN_CARRIER, where a BatchNorm-backward finalize goes between the data gradient that produced its column sums and
    # the apply that needs them: "wgrad" (the first workgroups of a weight-gradient launch) | "wred" (finalize and the pending split
    # reduction share one launch; launch order wgrad -> dgrad) | "none" (own launch).  16-bit engines with carried reductions only
    bnfin_piggyback: bool
    fin_with_wred: bool
    wgrad_first: bool              # launch order per convolution: weight gradient, then data gradient (every carrier but "wgrad")
    heads_bnred: bool              # CREID_HEADS_BNRED: creid_ctl_heads_fused produces the deepest bn3's backward column sums


# schedule switches that no longer exist, with the value that still passes (what retired each: docs/history/)
RETIRED_SWITCHES = (("CREID_WGRAD_STREAM", "0"), ("CREID_REDUCE_STREAM", "0"), ("CREID_EVAL_DS_SIDE", "0"), ("CREID_WPREP_SIDE", "0"),
                    ("CREID_BN_APPLY_DRY", "0"), ("CREID_WGRAD_FIRST", "0"), ("CREID_CARRIER_MAX_MB", "1e9"),
                    ("CREID_BNFIN_PIGGYBACK", "1"))


def resolve_schedule(dtype, mode=None, trainable=False, env=os.environ):
    """The Schedule of an engine with activation type `dtype` in compute mode `mode` (None or "bf16x3"): every environment
    switch is read here, once, and every rule that ties two of them together is applied here."""
    for name, default in RETIRED_SWITCHES:
        if env.get(name, default) != default:
            raise L.CreidError(f"{name}={env[name]} selects a schedule that was retired (docs/history/backbone_schedule_switches.md "
                               "has the measurement that retired it): unset it")

    def on(name, default="1"):
        return env.get(name, default) == "1"

    x3 = mode == "bf16x3"
    is16 = dtype in (torch.bfloat16, torch.float16)
    dma = on("CREID_IGEMM_DMA")
    if dtype == torch.float16 and not dma:
        raise L.CreidError("compute dtype float16 needs the LDS-DMA convolution kernels: unset CREID_IGEMM_DMA=0 "
                           "(the register-staged fallback kernels exist for bfloat16 and float32 only)")
    wred_piggyback = on("CREID_WRED_PIGGYBACK") and not (x3 and trainable)
    carrier = env.get("CREID_FIN_CARRIER", "wgrad") if wred_piggyback and is16 else "none"
    return Schedule(
        relu_bitmask=is16 and on("CREID_RELU_BITMASK"),
        stem_fuse_pool=on("CREID_STEM_FUSE"),
        stem_pool_fused=on("CREID_STEM_POOL"),
        pair_fused=on("CREID_PAIR_FUSE"),
        stem_fuse_pool_bwd=on("CREID_STEM_FUSE_BWD", "0"),
        drop_gm=on("CREID_DROP_GM"),
        fuse_bn_reduce=is16 and on("CREID_FUSE_BN_REDUCE") and dma,
        eval_fold=x3 or (on("CREID_EVAL_FOLD") and (dtype == torch.float32 or dma)),
        c3_axf=frozenset(int(v) for v in env.get("CREID_C3_AXF", "64,128").split(",") if v.strip()),
        ds_reduce2=on("CREID_DS_REDUCE2"),
        dual_apply=on("CREID_DUAL_APPLY"),
        fin_apply_rows=int(env.get("CREID_FIN_APPLY", "64")),
        fin_apply_rb=int(env.get("CREID_FIN_APPLY_RB", "64")),
        wred_piggyback=wred_piggyback,
        bnfin_piggyback=carrier == "wgrad",
        fin_with_wred=carrier == "wred",
        wgrad_first=carrier != "wgrad",
        heads_bnred=on("CREID_HEADS_BNRED"))


POOLINGS = ("avg", "gem")


class BackboneEngine:
    """Explicit forward / backward schedule for one backbone instance.

    dtype: a torch dtype (the activation and MFMA input type), or the string "bf16x3" -- the eval-mode forward with fp32
    activations whose convolutions run three bf16 MFMAs per product on split operands (fp32-grade embeddings on the bf16 matrix
    pipe, csrc/conv_x3.hip).  By default that mode has no training forward / backward; trainable=True adds them: the fp32
    engine's training schedule with the forward, data-gradient and weight-gradient launches of the 52 non-stem convolutions
    on the bf16x3 entry points (every activation, BatchNorm, IBN and the stem stay exact fp32)."""

    def __init__(self, net: ResNet, dtype=torch.bfloat16, trainable=False, pooling="avg", gem=None):
        """pooling: "avg" (the reference's global average pool) or "gem" -- generalized-mean pooling (csrc/gem_pool.hip) in
        every forward of this engine and its backward; `gem` is then the module that owns the exponent (`gem.p`, a [1] fp32
        parameter read on the device at every launch) and `gem.eps`."""
        self.net = net
        if pooling not in POOLINGS:
            raise ValueError(f"pooling must be one of {POOLINGS}, got {pooling!r}")
        if (pooling == "gem") != (gem is not None):
            raise ValueError("pooling='gem' needs the module that owns the exponent (gem=...), pooling='avg' takes none")
        self.pooling, self.gem = pooling, gem
        self.mode = dtype if isinstance(dtype, str) else None
        if self.mode is not None and self.mode not in L.EVAL_PRECISIONS:
            raise ValueError(f"unknown compute mode {dtype!r} (a torch dtype or one of {L.EVAL_PRECISIONS})")
        self.x3 = self.mode == "bf16x3"
        if trainable and not self.x3:
            raise ValueError("trainable=True selects the training form of a string compute mode; torch dtypes always train")
        self.x3_train = self.x3 and trainable
        if self.x3_train and isinstance(net.layer1[0], BasicBlock):
            raise L.CreidError(f"compute mode bf16x3 trains the Bottleneck networks only ({getattr(net, 'arch', 'resnet18/34')} is a "
                               "BasicBlock network): train it with bfloat16, float16 or float32")
        if self.x3:
            dtype = torch.float32          # activations and every non-convolution launch stay fp32
        self.dtype = dtype
        self.dt = L._DT[dtype]
        self.conv_dt = L.BF16X3 if self.x3 else self.dt     # dtype code of the forward convolutions and their weight copies
        # tests and tools select another schedule with dataclasses.replace(eng.sched, field=value): the raw field, no re-resolution
        self.sched = resolve_schedule(dtype, self.mode, trainable)
        # engines of the same network share a weight-change flag: an optimiser step announced to the training engine also
        # makes an eval-mode engine (Baseline eval_precision) re-derive its copies
        net.__dict__.setdefault("_creid_engines", weakref.WeakSet()).add(self)
        self.units = []
        self.stem = _ConvUnit(net.conv1, net.bn1)
        self.blocks = []
        # BasicBlock networks (resnet18 / resnet34, round 6): two 3 x 3 convolutions per block, no c3 -- the same kernels on a
        # plain schedule (_forward_basic / _backward_basic: none of the bottleneck-specific carriers and fusions)
        self.basic = isinstance(net.layer1[0], BasicBlock)
        self.cout = int(getattr(net, "out_channels", 2048))
        for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
            for blk in layer:
                u = dict(c1=_ConvUnit(blk.conv1, blk.bn1), c2=_ConvUnit(blk.conv2, blk.bn2),
                         c3=None if self.basic else _ConvUnit(blk.conv3, blk.bn3),
                         ds=_ConvUnit(blk.downsample[0], blk.downsample[1]) if blk.downsample is not None else None)
                self.blocks.append(u)
        self.weights_dirty = True      # set by writers torch cannot see (our ctypes optimiser kernels)
        self._wsig = None              # (data_ptr, _version) of every conv weight at the last prep_weights()
        self._wprep_key = None
        # nn.Module.load_state_dict copies through `param.copy_` under no_grad (bumps _version), but a post-hook makes
        # the refresh independent of how a loader writes
        net.register_load_state_dict_post_hook(lambda *_a: setattr(self, "weights_dirty", True))
        self._ws = None
        self._keep = []                # replaced workspaces, kept until backward() ends
        self.loss_scaler = None        # f16 training: solver.LossScaler; backward() multiplies the incoming head gradient by its scale
        self._bn_sums = {}             # id(unit) -> coefficient tensor whose finalize has already been issued
        self._wred_pending = []        # FIFO of WredJob
        self._wred_ws = [None, None, None]
        self._wred_flip = 0
        self.on_group_done = None
        self._group_first, o = {}, 0             # index of each layer's FIRST block -> layer number
        for k, layer in enumerate((net.layer1, net.layer2, net.layer3, net.layer4), start=1):
            self._group_first[o] = k
            o += len(layer)
        self.saved = None              # SavedStep: what a training forward leaves for backward(), which drops it (so does an eval forward)
        self._pending_steps = None     # device counter of training forwards not yet folded into num_batches_tracked
        self._fold_key = None

    # ---- helpers
    @property
    def weights_dirty(self):
        return self._weights_dirty

    @weights_dirty.setter
    def weights_dirty(self, v):
        self._weights_dirty = v
        if v:
            for e in list(self.net.__dict__.get("_creid_engines", ())):
                e._weights_dirty = True

    @property
    def device(self):
        return self.net.conv1.weight.device

    def _empty(self, *shape, dtype=None):
        return torch.empty(shape, dtype=dtype or self.dtype, device=self.device)

    def _relu_bits(self, a):           # the buffer for the ReLU mask of `a`, one bit per element; None where the schedule keeps no bits
        return torch.empty(a.numel() // 8, dtype=torch.uint8, device=self.device) if self.sched.relu_bitmask else None

    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._keep.append(self._ws)
            self._ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=self.device)
        return self._ws

    def all_units(self):
        yield self.stem
        for b in self.blocks:
            for k in ("c1", "c2", "c3", "ds"):
                if b[k] is not None:
                    yield b[k]

    def prep_weights(self):
        """fp32 OIHW master weights -> compute-dtype [O][r][s][I] and [I][r][s][O] copies (ONE launch for all
        52 non-stem convolutions through a device descriptor table, rebuilt only if a pointer moved)."""
        import numpy as np
        lib, st = L.lib(), L.stream()
        units = [u for u in self.all_units() if u is not self.stem]
        for u in units:
            if u.w_krsc is None and self.x3:
                u.w_krsc = self._empty(2, u.cout, u.k, u.k, u.cin, dtype=torch.bfloat16)   # hi plane, lo plane
                if self.x3_train:                                                          # the data gradient's copy
                    u.w_crsk = self._empty(2, u.cin, u.k, u.k, u.cout, dtype=torch.bfloat16)
            elif u.w_krsc is None:
                u.w_krsc = self._empty(u.cout, u.k, u.k, u.cin)
                u.w_crsk = self._empty(u.cin, u.k, u.k, u.cout)
        if self.stem.w_krsc is None:
            self.stem.w_krsc = self._empty(64, 8, 32)
        key = tuple(u.conv.weight.data_ptr() for u in units)
        if self._wprep_key != key:
            rec = np.zeros(len(units), dtype=np.dtype([("w", "<u8"), ("krsc", "<u8"), ("crsk", "<u8"), ("O", "<i4"),
                                                        ("I", "<i4"), ("kh", "<i4"), ("kw", "<i4"), ("start", "<i8")]))
            assert lib.creid_weight_prep_entry_bytes() == rec.dtype.itemsize == 48
            start, tiles, tstart = 0, 0, np.zeros(len(units), np.int32)
            for i, u in enumerate(units):
                rec[i] = (u.conv.weight.data_ptr(), u.w_krsc.data_ptr(), 0 if u.w_crsk is None else u.w_crsk.data_ptr(), u.cout,
                          u.cin, u.k, u.k, start)
                start += u.cout * u.cin * u.k * u.k
                tstart[i] = tiles
                tiles += ((u.cout + 31) // 32) * ((u.cin + 31) // 32)
            self._wprep_tab = torch.from_numpy(rec.view(np.uint8).copy()).to(self.device)
            self._wprep_tiles = torch.from_numpy(tstart).to(self.device)
            self._wprep_total = tiles
            self._wprep_key = key
        L.check(lib.creid_stem_weight_prep(L.ptr(self.stem.conv.weight), self.dt, L.ptr(self.stem.w_krsc), st),
                "stem_weight_prep")
        if self.x3_train:              # both two-plane copies (forward and data gradient) in one launch
            L.check(lib.creid_weight_prep_x3_train_multi(L.ptr(self._wprep_tab), L.ptr(self._wprep_tiles), len(units),
                                                         self._wprep_total, st), "weight_prep_x3_train_multi")
        else:
            L.check(lib.creid_weight_prep_multi(L.ptr(self._wprep_tab), L.ptr(self._wprep_tiles), len(units), self._wprep_total,
                                                self.conv_dt, st), "weight_prep_multi")
        self.weights_dirty = False
        self._wsig = self._weight_signature()

    def _weight_signature(self):
        """Changes whenever torch-visible code rewrites or re-homes a convolution weight after the compute-dtype
        copies were made (load_state_dict, an external / PL optimiser, EMA, broadcast, .to()): in-place ops bump
        `_version`, re-homing changes `data_ptr`.  Writers torch cannot see set `weights_dirty` themselves."""
        return tuple((u.conv.weight.data_ptr(), u.conv.weight._version) for u in self.all_units())

    def fold_counters(self):
        """Fold the pending step count into every BatchNorm2d.num_batches_tracked (before a state_dict)."""
        if self._pending_steps is None:
            return
        for u in self.all_units():
            u.bn.num_batches_tracked += self._pending_steps.to(u.bn.num_batches_tracked.device)
        self._pending_steps.zero_()

    def fold_bn(self):
        """Eval mode: (scale, shift) of every plain BatchNorm2d from its running statistics, ONE launch over a device
        table (rebuilt only if a tensor moved); always re-evaluated, so statistics updated by a training step or a
        load_state_dict are picked up without any dirty tracking."""
        import numpy as np
        lib, st = L.lib(), L.stream()
        units = [u for u in self.all_units() if u.ibn is None]
        key = tuple((u.bn.weight.data_ptr(), u.bn.bias.data_ptr(), u.bn.running_mean.data_ptr(),
                     u.bn.running_var.data_ptr()) for u in units)
        if self._fold_key != key:
            total = sum(2 * u.cout for u in units)
            self._fold_buf = torch.empty(total, dtype=torch.float32, device=self.device)
            rec = np.zeros(len(units), dtype=np.dtype([("g", "<u8"), ("b", "<u8"), ("m", "<u8"), ("v", "<u8"), ("o", "<u8"),
                                                       ("C", "<i4"), ("eps", "<f4")]))
            assert lib.creid_bn2d_fold_entry_bytes() == rec.dtype.itemsize == 48
            o = 0
            for i, u in enumerate(units):
                u.fold = self._fold_buf[o:o + 2 * u.cout].view(2, u.cout)
                rec[i] = (u.bn.weight.data_ptr(), u.bn.bias.data_ptr(), u.bn.running_mean.data_ptr(),
                          u.bn.running_var.data_ptr(), u.fold.data_ptr(), u.cout, u.bn.eps)
                o += 2 * u.cout
            self._fold_tab = torch.from_numpy(rec.view(np.uint8).copy()).to(self.device)
            self._fold_n = len(units)
            self._fold_key = key
        L.check(lib.creid_bn2d_fold_multi(L.ptr(self._fold_tab), self._fold_n, st), "bn2d_fold_multi")

    # ---- layer steps
    def _conv_fold(self, u, a_in, B, H, W, relu, residual=None):
        """Eval mode: conv -> folded BatchNorm -> (+residual) -> (ReLU) in one launch.  Returns (a_out, oh, ow)."""
        lib, st = L.lib(), L.stream()
        d, oh, ow = _desc(B, H, W, u.cin, u.cout, u.k, u.stride, u.pad)
        a = self._empty(B * oh * ow, u.cout)
        L.check(lib.creid_conv2d_fwd_affine_nhwc(C.byref(d), L.ptr(a_in), L.ptr(u.w_krsc), L.ptr(a), L.ptr(u.fold),
                                                 L.ptr(residual), 1 if relu else 0, self.conv_dt, st), "conv2d_fwd_affine")
        return a, oh, ow

    def _stem_operand(self, x, B, H, W):
        """The stem convolution's operand: zero-padded NHWC4 [B, H + 8, W + 6, 4] in the compute dtype.  An fp32 NCHW batch
        goes through the layout pass; a transforms.StemOperand (the device-side input transforms wrote that layout directly)
        is used as it is."""
        if not isinstance(x, torch.Tensor):
            assert x.xpad.dtype == self.dtype and tuple(x.xpad.shape) == (B, H + 8, W + 6, 4), "stem operand of another dtype / shape"
            return x.xpad
        xpad = self._empty(B, H + 8, W + 6, 4)
        L.check(L.lib().creid_image_to_nhwc4_pad(L.ptr(x), B, H, W, self.dt, L.ptr(xpad), L.stream()), "image_pad")
        return xpad

    def _forward_eval_folded(self, x_nchw, want_base_out):
        """validation_step / inference forward (modelling/bases.py:169-177, inference/inference_utils.py:104-113): 53
        convolutions with their BatchNorm folded in + pad, max-pool, GAP -- no statistics, no separate normalisation
        passes.  IBN blocks (resnet_ibn_a.py:27-32) keep their own pass: InstanceNorm needs per-image statistics."""
        lib, st = L.lib(), L.stream()
        B, _, H, W = x_nchw.shape
        self.fold_bn()
        xpad = self._stem_operand(x_nchw, B, H, W)
        H1, W1 = H // 2, W // 2
        H2, W2 = H1 // 2, W1 // 2
        a = self._empty(B * H2 * W2, 64)
        rc = -4
        if self.sched.stem_pool_fused and self.dtype != torch.float32:
            # conv1 + folded bn1 (+ ReLU) + max-pool in one launch: the full-resolution tensor is never written (conv_stem.hip)
            rc = lib.creid_stem_conv_pool_fwd_affine(B, H, W, L.ptr(xpad), L.ptr(self.stem.w_krsc), L.ptr(a), L.ptr(self.stem.fold),
                                                     1 if self.net.stem_relu else 0, self.dt, st)
            if rc != -4:
                L.check(rc, "stem_conv_pool_fwd_affine")
        if rc == -4:                                     # image size outside the fused kernel's tiles (or fp32): two launches
            y0 = self._empty(B * H1 * W1, 64)
            L.check(lib.creid_stem_conv_fwd_affine(B, H, W, L.ptr(xpad), L.ptr(self.stem.w_krsc), L.ptr(y0), L.ptr(self.stem.fold),
                                                   1 if self.net.stem_relu else 0, self.dt, st), "stem_conv_fwd_affine")
            L.check(lib.creid_maxpool3x3s2_fwd(L.ptr(y0), B, H1, W1, 64, self.dt, L.ptr(a), None, st), "maxpool_fwd")   # no argmax taps
            del y0
        del xpad
        h, w = H2, W2
        a1_next = None                    # conv1 output of the CURRENT block when the previous block's conv3 launch produced it
        for bi, b in enumerate(self.blocks):
            a_in, hin, win = a, h, w
            if self.basic:                # resnet.py:33-48: two folded 3 x 3 convolutions, the residual added in the second one's epilogue
                a1, h1, w1 = self._conv_fold(b["c1"], a_in, B, hin, win, True)
                r = a_in if b["ds"] is None else self._conv_fold(b["ds"], a_in, B, hin, win, False)[0]
                a, h, w = self._conv_fold(b["c2"], a1, B, h1, w1, True, residual=r)
                continue
            if a1_next is not None:
                a1, h1, w1, a1_next = a1_next, hin, win, None
            elif b["c1"].ibn is not None:
                c1 = self._conv_bn(b["c1"], a_in, B, hin, win, False, True)
                a1, h1, w1 = c1.act, c1.h, c1.w
            else:
                a1, h1, w1 = self._conv_fold(b["c1"], a_in, B, hin, win, True)
            a2, h2, w2 = self._conv_fold(b["c2"], a1, B, h1, w1, True)
            r = a_in if b["ds"] is None else self._conv_fold(b["ds"], a_in, B, hin, win, False)[0]
            nb =self.blocks[bi + 1] if bi + 1 < len(self.blocks) else None
            pair = (self.sched.pair_fused and nb is not None and nb["ds"] is None and self.dtype != torch.float32
                    and (b["c3"].cin, b["c3"].cout, nb["c1"].cout) == (64, 256, 64) and nb["c1"].stride == 1)
            if pair and nb["c1"].ibn is not None:
                pair = (h2 * w2) % 128 == 0              # the statistics partials must be per-image row blocks
            if pair:
                # conv3 + bn3 + residual + ReLU of this block AND conv1 (+ bn1 + ReLU, or the statistics an IBN layer needs) of the
                # next one in one launch: the block output is written (it is the next residual) but never read back by conv1
                # (conv_pair.hip; layer1 only)
                M3 = B * h2 * w2
                a = self._empty(M3, 256)
                x1 = self._empty(M3, 64)
                if nb["c1"].ibn is None:
                    L.check(lib.creid_bottleneck_c3_c1_fwd_affine(M3, 64, 256, 64, L.ptr(a2), L.ptr(b["c3"].w_krsc), L.ptr(b["c3"].fold),
                                                                  L.ptr(r), L.ptr(a), L.ptr(nb["c1"].w_krsc), L.ptr(nb["c1"].fold),
                                                                  L.ptr(x1), self.dt, st), "bottleneck_c3_c1_fwd_affine")
                    a1_next = x1
                else:
                    part = self._empty((M3 // 128) * 2, 64, dtype=torch.float32)
                    L.check(lib.creid_bottleneck_c3_c1_fwd_stats(M3, 64, 256, 64, L.ptr(a2), L.ptr(b["c3"].w_krsc), L.ptr(b["c3"].fold),
                                                                 L.ptr(r), L.ptr(a), L.ptr(nb["c1"].w_krsc), L.ptr(x1), L.ptr(part),
                                                                 self.dt, st), "bottleneck_c3_c1_fwd_stats")
                    a1_next = self._ibn_tail(nb["c1"], x1, B, h2, w2, False, True, part).act
                h, w = h2, w2
            else:
                a, h, w = self._conv_fold(b["c3"], a2, B, h2, w2, True, residual=r)
        feat = self._empty(B, self.cout, dtype=torch.float32)
        if self.gem is not None:
            self._gem_fwd(a, B, h * w, feat, False)
        else:
            L.check(lib.creid_gap_fwd(L.ptr(a), B, h * w, self.cout, self.dt, L.ptr(feat), st), "gap_fwd")
        self.saved = None
        base_out = None
        if want_base_out:
            base_out = self._empty(B, self.cout, h, w, dtype=torch.float32)
            L.check(lib.creid_nhwc_to_nchw_f32(L.ptr(a), B, h * w, self.cout, self.dt, L.ptr(base_out), st), "nhwc_to_nchw")
        return base_out, feat

    def _conv_bn(self, u, a_in, B, H, W, training, relu, residual=None, residual_ss=None, apply=True):
        """conv -> BN(batch or running stats) -> (+residual) -> (ReLU).  Returns the SavedLayer.
        apply=False: statistics only, the layer has `ss` and no `act` (the downsample branch: its normalisation
        happens inside the block's bn3 pass, which takes the raw tensor as `residual` and that pair as `residual_ss`)."""
        lib, st = L.lib(), L.stream()
        d, oh, ow = _desc(B, H, W, u.cin, u.cout, u.k, u.stride, u.pad)
        x = self._empty(B * oh * ow, u.cout)
        # the conv epilogue's per-128-row (sum, sumsq) partials are per-image row blocks when HW % 128 == 0:
        # IBN then needs no statistics pass of its own (InstanceNorm uses instance statistics in eval too)
        stats = training if u.ibn is None else (oh * ow) % 128 == 0
        rows = lib.creid_conv2d_bn_partial_rows(C.byref(d)) if stats else 0
        part = self._empty(rows * 2, u.cout, dtype=torch.float32) if stats else None
        L.check(lib.creid_conv2d_fwd_nhwc(C.byref(d), L.ptr(a_in), L.ptr(u.w_krsc), L.ptr(x), L.ptr(part), self.conv_dt, st),
                "conv2d_fwd")
        if u.ibn is not None:
            return self._ibn_tail(u, x, B, oh, ow, training, relu, part)
        return self._bn_tail(u, x, part, rows, oh, ow, training, relu, residual, residual_ss, apply)

    def _conv3_axf(self, u, c2, B, residual, residual_ss):
        """conv3 of a bottleneck on conv2's RAW output (c2: its statistics-only layer): bn2 + ReLU on the operand path, the
        normalised tensor and its ReLU bits as side outputs (what the backward reads: they complete c2), then bn3 as usual."""
        lib, st = L.lib(), L.stream()
        d, oh, ow = _desc(B, c2.h, c2.w, u.cin, u.cout, 1, 1, 0)
        M = B * oh * ow
        x = self._empty(M, u.cout)
        rows = lib.creid_conv2d_bn_partial_rows(C.byref(d))
        part = self._empty(rows * 2, u.cout, dtype=torch.float32)
        a_in = self._empty(M, u.cin)
        mask = torch.empty(M * u.cin // 8, dtype=torch.uint8, device=self.device)
        L.check(lib.creid_conv1x1_bnrelu_fwd(L.ptr(c2.x), L.ptr(c2.ss), L.ptr(u.w_krsc), M, u.cin, u.cout, L.ptr(x), L.ptr(part),
                                             L.ptr(a_in), L.ptr(mask), self.dt, st), "conv1x1_bnrelu_fwd")
        c2.act, c2.bits, c2.ss = a_in, mask, None
        return self._bn_tail(u, x, part, rows, oh, ow, True, True, residual, residual_ss, True)

    def _ibn_tail(self, u, x, B, h, w, training, relu, part=None):
        lib, st = L.lib(), L.stream()
        ibn, bn = u.ibn, u.bn
        HW = h * w
        rpi = lib.creid_ibn_rows_per_image(HW)
        ready = 1 if part is not None else 0
        if part is None:
            part = self._empty(B * rpi * 2, u.cout, dtype=torch.float32)
        mean = self._empty(B, u.cout, dtype=torch.float32)
        invstd = self._empty(B, u.cout, dtype=torch.float32)
        ss = self._empty(B * 2, u.cout, dtype=torch.float32)
        a = self._empty(B * HW, u.cout)
        mask = self._relu_bits(a) if training and relu else None
        L.check(lib.creid_ibn_fwd_mask(L.ptr(x), B, HW, u.cout, ibn.half, L.ptr(ibn.IN.weight), L.ptr(ibn.IN.bias),
                                       L.ptr(bn.weight), L.ptr(bn.bias), L.ptr(bn.running_mean), L.ptr(bn.running_var),
                                       1 if training else 0, bn.momentum, bn.eps, 1 if relu else 0, self.dt, L.ptr(part), ready,
                                       L.ptr(mean), L.ptr(invstd), L.ptr(ss), L.ptr(a), L.ptr(mask), st), "ibn_fwd")
        return SavedLayer(u, x, mean, invstd, h, w, relu, act=a, bits=mask)

    def _ibn_bwd(self, layer, g, B, part=None):
        lib, st = L.lib(), L.stream()
        u, ibn, bn, HW = layer.unit, layer.unit.ibn, layer.unit.bn, layer.hw
        rpi = lib.creid_ibn_rows_per_image(HW)
        ready = 1 if part is not None else 0
        if part is None:
            part = self._empty(B * rpi * 2, u.cout, dtype=torch.float32)
        coef = self._empty(B * 3, u.cout, dtype=torch.float32)
        per_img = self._empty(B * 2, ibn.half, dtype=torch.float32)
        dx = self._empty(B * HW, u.cout)
        L.check(lib.creid_ibn_bwd_mask(L.ptr(layer.x), L.ptr(g), L.ptr(layer.act), L.ptr(layer.bits), L.ptr(layer.mean),
                                       L.ptr(layer.invstd), B, HW, u.cout, ibn.half, L.ptr(ibn.IN.weight), L.ptr(bn.weight), self.dt,
                                       L.ptr(part), ready, L.ptr(coef), L.ptr(per_img), L.ptr(self._grad_of(ibn.IN.weight)),
                                       L.ptr(self._grad_of(ibn.IN.bias)), L.ptr(self._grad_of(bn.weight)),
                                       L.ptr(self._grad_of(bn.bias)), L.ptr(dx), st), "ibn_bwd")
        return dx

    def _bn_tail(self, u, x, part, rows, h, w, training, relu, residual, residual_ss=None, apply=True):
        lib, st = L.lib(), L.stream()
        bn, M = u.bn, x.shape[0]
        mean = self._empty(u.cout, dtype=torch.float32)
        invstd = self._empty(u.cout, dtype=torch.float32)
        ss = self._empty(2, u.cout, dtype=torch.float32)
        sched = self.sched
        if (sched.fin_apply_rows and training and apply and residual_ss is None and rows <= sched.fin_apply_rows
                and u.cout % (32 if self.dtype == torch.float32 else 64) == 0):
            # finalize + apply in ONE launch (CREID_FIN_APPLY=<max statistic rows>; profiles/r05_fin_apply.md)
            a = self._empty(M, u.cout)
            mask = self._relu_bits(a) if relu else None
            L.check(lib.creid_bn2d_finalize_apply_mask(L.ptr(part), rows, u.cout, M, L.ptr(bn.running_mean), L.ptr(bn.running_var),
                                                       bn.momentum, bn.eps, L.ptr(bn.weight), L.ptr(bn.bias), L.ptr(mean), L.ptr(invstd),
                                                       L.ptr(ss), L.ptr(x), L.ptr(residual), 1 if relu else 0, self.dt, L.ptr(a),
                                                       L.ptr(mask), sched.fin_apply_rb, st), "bn2d_finalize_apply")
            return SavedLayer(u, x, mean, invstd, h, w, relu, act=a, bits=mask)
        L.check(lib.creid_bn2d_finalize(L.ptr(part), rows, u.cout, M, L.ptr(bn.running_mean), L.ptr(bn.running_var),
                                        1 if training else 0, bn.momentum, bn.eps, L.ptr(bn.weight), L.ptr(bn.bias),
                                        L.ptr(mean), L.ptr(invstd), L.ptr(ss), st), "bn2d_finalize")
        if not apply:
            return SavedLayer(u, x, mean, invstd, h, w, relu, ss=ss)
        a = self._empty(M, u.cout)
        mask = self._relu_bits(a) if training and relu else None
        if residual_ss is not None:
            L.check(lib.creid_bn2d_apply_dual_mask(L.ptr(x), L.ptr(ss), L.ptr(residual), L.ptr(residual_ss), 1 if relu else 0, M,
                                                   u.cout, self.dt, L.ptr(a), L.ptr(mask), st), "bn2d_apply_dual")
        else:
            L.check(lib.creid_bn2d_apply_mask(L.ptr(x), L.ptr(ss), L.ptr(residual), 1 if relu else 0, M, u.cout, self.dt,
                                              L.ptr(a), L.ptr(mask), st), "bn2d_apply")
        return SavedLayer(u, x, mean, invstd, h, w, relu, act=a, bits=mask)      # the bits travel to _bn_bwd / _dgrad with it

    def _gem_fwd(self, a, B, hw, feat, training):
        """Generalized-mean pool of the final map a [B hw, C] into feat; training: also the step counter (as creid_gap_fwd_count)
        and the saved per-(b, c) quantities, which are returned."""
        p = self.gem.p
        if not (p.is_cuda and p.dtype == torch.float32 and p.numel() == 1):
            raise L.CreidError("the GeM exponent must be one fp32 value on the GPU (move the model with .cuda())")
        stats = self._empty(3, B, self.cout, dtype=torch.float32) if training else None
        L.check(L.lib().creid_gem_fwd(L.ptr(a), B, hw, self.cout, self.dt, L.ptr(p), self.gem.eps, L.ptr(feat), L.ptr(stats),
                                      L.ptr(self._pending_steps) if training else None, L.stream()), "gem_fwd")
        return stats

    # ---- forward
    def forward(self, x_nchw, training: bool, want_base_out: bool = False):
        """x_nchw: fp32 [B, 3, H, W] on the GPU, or a transforms.StemOperand (same batch, already in the stem's layout)."""
        if isinstance(x_nchw, torch.Tensor):
            L.require_gpu(x_nchw)
            assert x_nchw.dtype == torch.float32 and x_nchw.dim() == 4 and x_nchw.shape[1] == 3
        else:
            L.require_gpu(x_nchw.xpad)
        if training and self.x3 and not self.x3_train:
            raise L.CreidError("compute mode bf16x3 is an eval-mode forward only (validation / inference): train with bfloat16, "
                               "float16 or float32 and pass eval_precision='bf16x3' to Baseline / CTLModel, or train in the mode "
                               "with compute_dtype='bf16x3' (BackboneEngine(net, 'bf16x3', trainable=True))")
        if self.weights_dirty or self._wsig != self._weight_signature():
            # (training steps replayed from a hipGraph re-derive the 16-bit weight copies every step: the optimiser has just
            # rewritten the masters)
            self.prep_weights()
        lib, st, sched = L.lib(), L.stream(), self.sched
        B, _, H, W = x_nchw.shape
        if not training and sched.eval_fold:
            return self._forward_eval_folded(x_nchw, want_base_out)
        # (f16 -- the reference's precision=16, utils/misc.py:111 -- trains like bf16; its gradients need the dynamic loss scale
        # that ModelBase.configure_optimizers attaches as `loss_scaler`: solver.LossScaler)
        if training and self._pending_steps is None:
            # ONE device counter per step instead of 53 per-layer `num_batches_tracked += 1`; the increment itself rides in the
            # forward's last launch (creid_gap_fwd_count)
            self._pending_steps = torch.zeros((), dtype=torch.long, device=self.device)
        # stem
        xpad = self._stem_operand(x_nchw, B, H, W)
        H1, W1 = H // 2, W // 2
        M0 = B * H1 * W1
        x0 = self._empty(M0, 64)
        rows = (M0 + 127) // 128 if training else 0
        part = self._empty(rows * 2, 64, dtype=torch.float32) if training else None
        L.check(lib.creid_stem_conv_fwd(B, H, W, L.ptr(xpad), L.ptr(self.stem.w_krsc), L.ptr(x0), L.ptr(part), self.dt, st),
                "stem_conv_fwd")
        H2, W2 = H1 // 2, W1 // 2
        p0 = self._empty(B * H2 * W2, 64)
        idx0 = self._empty(B * H2 * W2, 64, dtype=torch.uint8)
        if sched.stem_fuse_pool and not self.net.stem_relu:
            # bn1 + maxpool in one pass over the raw conv output: the normalised 64-channel full-resolution tensor is read
            # by nothing else (no stem ReLU -> the backward needs no mask of it either) and is never written
            bn0 = self._bn_tail(self.stem, x0, part, rows, H1, W1, training, False, None, apply=False)
            L.check(lib.creid_bn2d_apply_maxpool3x3s2(L.ptr(x0), L.ptr(bn0.ss), 0, B, H1, W1, 64, self.dt, L.ptr(p0), L.ptr(idx0),
                                                      st), "bn2d_apply_maxpool")
            bn0.ss = None
        else:
            bn0 = self._bn_tail(self.stem, x0, part, rows, H1, W1, training, self.net.stem_relu, None)
            L.check(lib.creid_maxpool3x3s2_fwd(L.ptr(bn0.act), B, H1, W1, 64, self.dt, L.ptr(p0), L.ptr(idx0), st), "maxpool_fwd")
        a, h, w = p0, H2, W2
        blocks, gem = [], None
        for b in self.blocks:
            # BasicBlock (resnet.py:33-48): conv1 - bn1 - relu - conv2 - bn2 (+ residual) - relu; a bottleneck has conv3 - bn3 behind
            # conv2 - bn2 - relu and adds the residual there.  `last`: the convolution whose normalisation takes the residual
            s = SavedBlock(a, h, w, c1=self._conv_bn(b["c1"], a, B, h, w, training, True), c2=None)
            last = b["c2"] if self.basic else b["c3"]
            axf = (not self.basic and training and self.dtype != torch.float32 and sched.relu_bitmask and last.k == 1
                   and last.stride == 1 and last.cin in sched.c3_axf and last.cin in (64, 128) and b["c2"].ibn is None)
            if not self.basic:   # axf: conv2 + statistics only, bn2's (scale, shift) go to conv3, which normalises its operand itself
                s.c2 = self._conv_bn(b["c2"], s.c1.act, B, s.c1.h, s.c1.w, training, True, apply=not axf)
            r, rss = s.a_in, None
            if b["ds"] is not None:
                # downsample branch, dual apply: conv + statistics only; its normalisation rides in the apply pass of `last` (one
                # launch and the write + read of the normalised branch tensor less per downsample block)
                s.ds = self._conv_bn(b["ds"], s.a_in, B, s.hin, s.win, training, False, apply=not (self.basic or sched.dual_apply))
                r, rss = (s.ds.x if s.ds.act is None else s.ds.act), s.ds.ss
                s.ds.act = s.ds.ss = None        # the backward reads neither: they live as long as this block's forward
            if self.basic:
                out = s.c2 = self._conv_bn(last, s.c1.act, B, s.c1.h, s.c1.w, training, True, residual=r, residual_ss=rss)
            elif axf:
                out = s.c3 = self._conv3_axf(last, s.c2, B, r, rss)
            else:
                out = s.c3 = self._conv_bn(last, s.c2.act, B, s.c2.h, s.c2.w, training, True, residual=r, residual_ss=rss)
            a, h, w = out.act, out.h, out.w
            if training:
                blocks.append(s)
            del s                                # (an eval forward keeps no block alive into the next one's launches)
        feat = self._empty(B, self.cout, dtype=torch.float32)
        if self.gem is not None:
            # the final map itself is kept for the backward (with the average pool nothing reads it after this launch when the
            # ReLU masks travel as bits), next to the per-(b, c) quantities the forward saves
            gem = (a, self._gem_fwd(a, B, h * w, feat, training))
        elif training:
            L.check(lib.creid_gap_fwd_count(L.ptr(a), B, h * w, self.cout, self.dt, L.ptr(feat), L.ptr(self._pending_steps), st), "gap_fwd")
        else:
            L.check(lib.creid_gap_fwd(L.ptr(a), B, h * w, self.cout, self.dt, L.ptr(feat), st), "gap_fwd")
        self.saved = SavedStep(B, H, W, SavedStem(xpad, bn0, idx0), blocks, (h, w), gem) if training else None
        base_out = None
        if want_base_out:
            base_out = self._empty(B, self.cout, h, w, dtype=torch.float32)
            L.check(lib.creid_nhwc_to_nchw_f32(L.ptr(a), B, h * w, self.cout, self.dt, L.ptr(base_out), st), "nhwc_to_nchw")
        return base_out, feat

    # ---- backward
    def _grad_of(self, p):
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        return p.grad

    def _bn_bwd(self, layer, g, *, want_gm=False, part=None, mask=None, reduce2=None):
        """BN backward of `layer`; `part` = column-reduction partials already produced by a fused dgrad epilogue; `mask` = ReLU
        bits to apply to g (default: the layer's own).  reduce2 = the SavedLayer of a second BatchNorm backward over the same
        masked gradient (the downsample branch's): the apply pass also produces its column sums.  Returns (dx, gm, part2): gm the
        masked copy of g with want_gm, part2 those column sums with reduce2, None otherwise."""
        lib, st = L.lib(), L.stream()
        u, bn, x, mean, invstd, M = layer.unit, layer.unit.bn, layer.x, layer.mean, layer.invstd, layer.x.shape[0]
        act, bits = (layer.act, layer.bits) if layer.relu else (None, None)
        rows = lib.creid_bn2d_bwd_rows(M)
        ready = 1 if part is not None else 0
        sums = self._bn_sums.pop(id(u), None)
        if sums is not None:
            ready = 2                      # finalize already issued (it rode in a weight-gradient launch): apply only
        else:
            part = part if part is not None else self._empty(rows * 2, u.cout, dtype=torch.float32)
            sums = self._empty(3, u.cout, dtype=torch.float32)
        dx = self._empty(M, u.cout)
        gm = self._empty(M, u.cout) if want_gm else None
        dgam = self._grad_of(bn.weight) if bn.weight.requires_grad else None
        dbet = self._grad_of(bn.bias) if bn.bias.requires_grad else None
        if ready == 1 and self.sched.fin_with_wred and self._wred_pending:
            # the finalize and the oldest pending split reduction in ONE launch, then apply only
            job = self._wred_pending.pop(0)
            L.check(lib.creid_bn2d_bwd_finalize_wred(L.ptr(part), rows, u.cout, M, L.ptr(mean), L.ptr(invstd), L.ptr(bn.weight),
                                                     L.ptr(sums), L.ptr(dgam), L.ptr(dbet), C.byref(job.desc), L.ptr(job.grad), 1,
                                                     L.ptr(job.ws), job.nbytes, self.dt, st), "bn2d_bwd_finalize_wred")
            ready = 2
        mask = bits if mask is None else mask
        if reduce2 is not None:
            part2 = self._empty(rows * 2, u.cout, dtype=torch.float32)
            L.check(lib.creid_bn2d_bwd_mask_reduce2(L.ptr(x), L.ptr(g), L.ptr(mask), L.ptr(mean), L.ptr(invstd), L.ptr(bn.weight), M,
                                                    u.cout, self.dt, L.ptr(part), ready, L.ptr(sums), L.ptr(dgam), L.ptr(dbet),
                                                    L.ptr(dx), L.ptr(reduce2.x), L.ptr(reduce2.mean), L.ptr(reduce2.invstd),
                                                    L.ptr(part2), st), "bn2d_bwd_reduce2")
            return dx, None, part2
        L.check(lib.creid_bn2d_bwd_mask(L.ptr(x), L.ptr(g), L.ptr(act), L.ptr(mask), L.ptr(mean), L.ptr(invstd),
                                        L.ptr(bn.weight), M, u.cout, self.dt, L.ptr(part), ready, L.ptr(sums), L.ptr(dgam),
                                        L.ptr(dbet), L.ptr(dx), L.ptr(gm), st), "bn2d_bwd")
        return dx, gm, None

    def _wgrad(self, u, a_in, dy, B, H, W, *, fin=None):
        """Weight gradient.  fin = (SavedLayer, partials) of a BatchNorm whose backward finalize should ride in this launch
        (ignored -- the BatchNorm backward then runs its own finalize -- where the carrier does not apply)."""
        if not u.conv.weight.requires_grad:
            return
        lib, st = L.lib(), L.stream()
        d, _, _ = _desc(B, H, W, u.cin, u.cout, u.k, u.stride, u.pad)
        if self.x3_train:
            nbytes = lib.creid_conv2d_wgrad_x3_workspace_bytes(C.byref(d))
            ws = self._workspace(nbytes)
            L.check(lib.creid_conv2d_wgrad_x3_nhwc(C.byref(d), L.ptr(a_in), L.ptr(dy), L.ptr(self._grad_of(u.conv.weight)), 1,
                                                   L.ptr(ws), nbytes, st), "conv2d_wgrad_x3")
            return
        nbytes = lib.creid_conv2d_wgrad_workspace_bytes(C.byref(d), self.dt)
        gw = self._grad_of(u.conv.weight)
        if self.sched.wred_piggyback:
            # partial tiles now; the sum over the splits is carried by the next data-gradient launch.  At most two
            # jobs are ever pending (c1 and the downsample branch), so three rotating workspaces never collide.
            k = self._wred_flip = (self._wred_flip + 1) % 3
            if self._wred_ws[k] is None or self._wred_ws[k].numel() < nbytes:
                self._keep.append(self._wred_ws[k])
                self._wred_ws[k] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=self.device)
            ws = self._wred_ws[k]
            if fin is not None and self.sched.bnfin_piggyback and fin[1] is not None:
                fl, fpart = fin
                fu, fbn, fM = fl.unit, fl.unit.bn, fl.x.shape[0]
                sums = self._empty(3, fu.cout, dtype=torch.float32)
                dgam = self._grad_of(fbn.weight) if fbn.weight.requires_grad else None
                dbet = self._grad_of(fbn.bias) if fbn.bias.requires_grad else None
                L.check(lib.creid_conv2d_wgrad_partials_bnfin(C.byref(d), L.ptr(a_in), L.ptr(dy), L.ptr(ws), nbytes, self.dt,
                                                              L.ptr(fpart), lib.creid_bn2d_bwd_rows(fM), fu.cout, fM,
                                                              L.ptr(fl.mean), L.ptr(fl.invstd), L.ptr(fbn.weight), L.ptr(sums),
                                                              L.ptr(dgam), L.ptr(dbet), st), "conv2d_wgrad_partials_bnfin")
                self._bn_sums[id(fu)] = sums
            else:
                L.check(lib.creid_conv2d_wgrad_partials(C.byref(d), L.ptr(a_in), L.ptr(dy), L.ptr(ws), nbytes, self.dt, st),
                        "conv2d_wgrad_partials")
            self._wred_pending.append(WredJob(d, gw, ws, nbytes))
            assert len(self._wred_pending) <= 3
            return
        ws = self._workspace(nbytes)
        L.check(lib.creid_conv2d_wgrad_nhwc(C.byref(d), L.ptr(a_in), L.ptr(dy), L.ptr(gw), 1, L.ptr(ws), nbytes, self.dt, st),
                "conv2d_wgrad")

    def _dgrad(self, u, dy, B, H, W, *, add_src=None, consumer=None, add_src_stride=1, add_mask=None, on_output_grid=False):
        """Data gradient, returns (dx, part).  consumer = the SavedLayer of the normalisation that consumes the result: its
        backward column reduction is fused into the epilogue (16-bit) and the partials are returned as `part` (else None); IBN has
        per-(image, channel) statistics and is fused only where the 128-row tiles do not straddle images.  on_output_grid (a
        stride-2 1 x 1 convolution): the gradient on the even input pixels only, as the plain 1 x 1 GEMM over the output grid H x W."""
        lib, st = L.lib(), L.stream()
        d, _, _ = _desc(B, H, W, u.cin, u.cout, 1, 1, 0) if on_output_grid else _desc(B, H, W, u.cin, u.cout, u.k, u.stride, u.pad)
        M = B * H * W
        dx = self._empty(M, u.cin)
        if self.x3_train:                  # (the fp32 schedule: no fused BatchNorm reduction, no mask, stride-1 add_src)
            assert add_src_stride == 1 and add_mask is None
            L.check(lib.creid_conv2d_dgrad_x3_nhwc(C.byref(d), L.ptr(dy), L.ptr(u.w_crsk), L.ptr(dx), L.ptr(add_src), st),
                    "conv2d_dgrad_x3")
            return dx, None
        per_image = consumer is not None and consumer.unit.ibn is not None
        fuse_bn = consumer is not None and self.sched.fuse_bn_reduce and not (per_image and consumer.hw % 128 != 0)
        carry = len(self._wred_pending) >= (2 if self.sched.fin_with_wred else 1)   # "wred" mode keeps one job for the finalize launch
        if carry or fuse_bn or add_mask is not None:
            job = self._wred_pending.pop(0) if carry else WredJob(None, None, None, 0)
            x = act = bits = mean = invstd = part = None
            if fuse_bn:
                x, act, bits, mean, invstd = consumer.x, consumer.act, consumer.bits, consumer.mean, consumer.invstd
                part = self._empty(lib.creid_bn2d_bwd_rows(M) * 2, u.cin, dtype=torch.float32)
            L.check(lib.creid_conv2d_dgrad_fused_nhwc(C.byref(d), L.ptr(dy), L.ptr(u.w_crsk), L.ptr(dx), L.ptr(add_src),
                                                      add_src_stride, L.ptr(add_mask), L.ptr(x), L.ptr(act), L.ptr(bits),
                                                      L.ptr(mean), L.ptr(invstd), L.ptr(part), consumer.hw if per_image and fuse_bn else 0,
                                                      C.byref(job.desc) if carry else None, L.ptr(job.grad), 1,
                                                      L.ptr(job.ws), job.nbytes, self.dt, st), "conv2d_dgrad_fused")
            return dx, part
        L.check(lib.creid_conv2d_dgrad_nhwc(C.byref(d), L.ptr(dy), L.ptr(u.w_crsk), L.ptr(dx), L.ptr(add_src), self.dt, st),
                "conv2d_dgrad")
        return dx, None

    def first_bn_bwd_operands(self):
        """What creid_ctl_heads_fused needs to produce the column sums of the FIRST BatchNorm backward (the last bottleneck's bn3)
        while it writes g: (x3, ReLU bits of the block output, mean, invstd, partial-rows buffer), or None when that reduction
        keeps its own launch (fp32 engine, no mask bits, 128-row tiles that straddle images in the general case are fine)."""
        sv, sched = self.saved, self.sched
        if self.basic or sv is None or not (sched.heads_bnred and sched.fuse_bn_reduce and sched.drop_gm and sched.relu_bitmask):
            return None
        c3 = sv.blocks[-1].c3
        if c3.bits is None or c3.unit.cout % 256 != 0:
            return None
        part = self._empty(L.lib().creid_bn2d_bwd_rows(c3.x.shape[0]) * 2, c3.unit.cout, dtype=torch.float32)
        return c3.x, c3.bits, c3.mean, c3.invstd, part

    def backward(self, dfeat: torch.Tensor, g: torch.Tensor = None, part3: torch.Tensor = None):
        """Accumulates parameter gradients into `.grad` (fp32, reference layouts).  `self.on_group_done(k)`, if set,
        is called after the last kernel of layer k (4, 3, 2, 1) has been enqueued -- every gradient of that layer is
        then final in stream order (the data-parallel bucketed all-reduce hangs on it, parallel.py).
        g (optional, [B * h * w, 2048] in the compute dtype): the gradient of the final feature map, already pooled back and (f16)
        loss-scaled -- the last launch of creid_ctl_heads_fused writes it; `dfeat` is ignored then.  part3 (optional): the column
        sums of the deepest bn3 backward, produced by that same launch."""
        sv = self.saved
        assert sv is not None, "backward() needs a training-mode forward first"
        lib, st, sched = L.lib(), L.stream(), self.sched
        self._bn_sums.clear()
        B, (h, w) = sv.B, sv.final
        if g is None:
            dfeat = dfeat.contiguous().float()
            if self.loss_scaler is not None and self.dtype == torch.float16:
                dfeat = self.loss_scaler.scale_(dfeat)        # every f16 gradient tensor / backbone parameter gradient below is scaled
            g = self._empty(B * h * w, self.cout)
            if self.gem is not None:
                a_fin, stats = sv.gem
                p = self.gem.p
                # p.grad is final after this call, before any gradient of layer 4: the data-parallel bucket that closes with
                # layer 4 (it runs to the end of the flat buffer, `gap.p` sits behind layer 4 in it) carries it
                dp = self._grad_of(p) if p.requires_grad else None
                parts = None
                if dp is not None:
                    parts = self._empty(lib.creid_gem_bwd_partials(B, self.cout, self.dt), dtype=torch.float32)
                L.check(lib.creid_gem_bwd(L.ptr(a_fin), L.ptr(dfeat), L.ptr(stats), B, h * w, self.cout, self.dt, L.ptr(p),
                                          self.gem.eps, L.ptr(g), L.ptr(dp), L.ptr(parts), st), "gem_bwd")
            else:
                L.check(lib.creid_gap_bwd(L.ptr(dfeat), B, h * w, self.cout, self.dt, L.ptr(g), st), "gap_bwd")
        elif self.gem is not None:
            raise L.CreidError("a pooled-back gradient g comes from creid_ctl_heads_fused, which applies the average pool's "
                               "backward: with pooling='gem' hand backward() the feature gradient dfeat")
        else:
            assert g.dtype == self.dtype and tuple(g.shape) == (B * h * w, self.cout) and g.is_contiguous()
        g = self._backward_basic(sv.blocks, g, B) if self.basic else self._backward_bottleneck(sv.blocks, g, part3, B)
        # stem
        H, W, xpad, bn0, idx0 = sv.H, sv.W, sv.stem.xpad, sv.stem.bn, sv.stem.idx
        H1, W1 = bn0.h, bn0.w
        if sched.stem_fuse_pool_bwd and not self.net.stem_relu:
            # the max-pool gradient is gathered inside the BatchNorm backward passes, the full-resolution dy0 is never written
            bn, M0 = self.stem.bn, B * H1 * W1
            part0 = self._empty(lib.creid_bn2d_bwd_rows(M0) * 2, 64, dtype=torch.float32)
            sums0 = self._empty(3, 64, dtype=torch.float32)
            dx0 = self._empty(M0, 64)
            dgam = self._grad_of(bn.weight) if bn.weight.requires_grad else None
            dbet = self._grad_of(bn.bias) if bn.bias.requires_grad else None
            L.check(lib.creid_bn2d_bwd_pooled(L.ptr(bn0.x), L.ptr(g), L.ptr(idx0), B, H1, W1, None, L.ptr(bn0.mean), L.ptr(bn0.invstd),
                                              L.ptr(bn.weight), 64, self.dt, L.ptr(part0), L.ptr(sums0), L.ptr(dgam), L.ptr(dbet),
                                              L.ptr(dx0), st), "bn2d_bwd_pooled")
        else:
            dy0 = self._empty(B * H1 * W1, 64)
            L.check(lib.creid_maxpool3x3s2_bwd(L.ptr(g), L.ptr(idx0), B, H1, W1, 64, self.dt, L.ptr(dy0), st), "maxpool_bwd")
            dx0, _, _ = self._bn_bwd(bn0, dy0)
        if self.stem.conv.weight.requires_grad:
            nbytes = lib.creid_stem_conv_wgrad_workspace_bytes(B, H, W, self.dt)
            ws = self._workspace(nbytes)
            L.check(lib.creid_stem_conv_wgrad(B, H, W, L.ptr(xpad), L.ptr(dx0), L.ptr(self._grad_of(self.stem.conv.weight)), 1,
                                              L.ptr(ws), nbytes, self.dt, st), "stem_conv_wgrad")
        self._flush_wred()
        self._keep.clear()
        self.saved = None

    def _backward_bottleneck(self, blocks, g, part3, B):
        """Backward of the Bottleneck networks, block by block in reverse.  part3: bn3 partials of the CURRENT block, produced by
        the previous (deeper) block -- for the deepest block by the heads' last launch when the caller hands them in
        (first_bn_bwd_operands).  Returns the gradient w.r.t. the max-pool output."""
        sched = self.sched
        for bi in range(len(blocks) - 1, -1, -1):
            s = blocks[bi]
            c1, c2, c3, ds = s.c1, s.c2, s.c3, s.ds
            nxt = blocks[bi - 1].c3 if bi > 0 else None     # bn3 of the block whose output gradient we produce
            # the block's incoming gradient g is masked by the final ReLU on three paths (bn3, the residual add, the
            # downsample BN).  With the mask as bits every consumer applies it itself and the masked copy `gm` is never
            # written; otherwise bn3's backward writes it once.
            m3 = c3.bits if (sched.fuse_bn_reduce and sched.drop_gm) else None
            # downsample blocks: bn3's apply pass also sums the columns the downsample branch's BatchNorm backward needs (same
            # masked gradient, one read of it instead of two and one launch less; CREID_DS_REDUCE2=0: separate launches)
            reduce2 = ds if (m3 is not None and ds is not None and sched.ds_reduce2 and not sched.fin_with_wred) else None
            dx3, gm, ds_part = self._bn_bwd(c3, g, want_gm=m3 is None, part=part3, reduce2=reduce2)
            gm = g if m3 is not None else gm
            da2, p2 = self._conv_bwd(c3.unit, c2.act, dx3, B, c2.h, c2.w, consumer=c2)
            dx2, _, _ = self._bn_bwd(c2, da2, part=p2)
            da1, p1 = self._conv_bwd(c2.unit, c1.act, dx2, B, c1.h, c1.w, consumer=c1)
            dx1 = self._ibn_bwd(c1, da1, B, part=p1) if c1.unit.ibn is not None else self._bn_bwd(c1, da1, part=p1)[0]
            # conv1: the downsample branch's launches lie between its weight gradient (where that comes first) and its data
            # gradient, which adds the shortcut's gradient in its epilogue
            if sched.wgrad_first:
                self._wgrad(c1.unit, s.a_in, dx1, B, s.hin, s.win)
            if ds is not None:
                dxd, _, _ = self._bn_bwd(ds, gm, mask=m3, part=ds_part)
                # stride-2 1x1 downsample: its data gradient lives on the even pixels only -- compute it as a plain 1x1 GEMM
                # over the OUTPUT grid and let the c1 dgrad epilogue scatter-add it
                even = (ds.unit.stride == 2 and ds.unit.k == 1 and nxt is not None and sched.fuse_bn_reduce
                        and s.hin % 2 == 0 and s.win % 2 == 0)
                gh, gw = (ds.h, ds.w) if even else (s.hin, s.win)
                tmp, _ = self._dgrad(ds.unit, dxd, B, gh, gw, on_output_grid=even)       # (also carries a pending split reduction)
                self._wgrad(ds.unit, s.a_in, dxd, B, s.hin, s.win)
                g, part3 = self._dgrad(c1.unit, dx1, B, s.hin, s.win, add_src=tmp, consumer=nxt, add_src_stride=2 if even else 1)
            else:
                g, part3 = self._dgrad(c1.unit, dx1, B, s.hin, s.win, add_src=gm, consumer=nxt, add_mask=m3)
            if not sched.wgrad_first:
                self._wgrad(c1.unit, s.a_in, dx1, B, s.hin, s.win, fin=None if nxt is None else (nxt, part3))
            if self.on_group_done is not None and bi in self._group_first:
                self._flush_wred()                       # the layer's last split reduction: nothing left to carry it
                self.on_group_done(self._group_first[bi])
        return g

    def _conv_bwd(self, u, a_in, dy, B, H, W, *, consumer):
        """Both gradients of one convolution in the schedule's order, returns the data gradient's (dx, part).  Data gradient first:
        it feeds the dependent chain dgrad -> BN finalize -> BN apply -> dgrad; the weight gradient is off that chain and carries
        the finalize of `consumer`'s BatchNorm backward (and gets its own split reduction carried by the NEXT data gradient)."""
        if self.sched.wgrad_first:
            self._wgrad(u, a_in, dy, B, H, W)
        dx, part = self._dgrad(u, dy, B, H, W, consumer=consumer)
        if not self.sched.wgrad_first:
            self._wgrad(u, a_in, dy, B, H, W, fin=None if consumer.unit.ibn is not None else (consumer, part))
        return dx, part

    def _backward_basic(self, blocks, g, B):
        """Backward of the BasicBlock networks (resnet18 / resnet34), block by block in reverse: bn2 backward (it also writes the
        ReLU-masked gradient the shortcut needs), conv2's weight and data gradient, bn1 backward, conv1's weight gradient, the
        downsample branch (BatchNorm backward, weight gradient, data gradient) and conv1's data gradient with the shortcut's
        gradient added in its epilogue.  Plain launches of the same kernels as the bottleneck schedule; split reductions of the
        weight gradients ride in the following data gradients as there.  Returns the gradient w.r.t. the max-pool output."""
        for bi in range(len(blocks) - 1, -1, -1):
            s = blocks[bi]
            c1, c2, ds = s.c1, s.c2, s.ds
            dx2, gm, _ = self._bn_bwd(c2, g, want_gm=True)
            self._wgrad(c2.unit, c1.act, dx2, B, c1.h, c1.w)
            da1, _ = self._dgrad(c2.unit, dx2, B, c1.h, c1.w)
            dx1, _, _ = self._bn_bwd(c1, da1)
            self._wgrad(c1.unit, s.a_in, dx1, B, s.hin, s.win)
            if ds is not None:
                dxd, _, _ = self._bn_bwd(ds, gm)
                self._wgrad(ds.unit, s.a_in, dxd, B, s.hin, s.win)
                short, _ = self._dgrad(ds.unit, dxd, B, s.hin, s.win)
            else:
                short = gm
            g, _ = self._dgrad(c1.unit, dx1, B, s.hin, s.win, add_src=short)
            if self.on_group_done is not None and bi in self._group_first:
                self._flush_wred()
                self.on_group_done(self._group_first[bi])
        return g

    def _flush_wred(self):
        """Split reductions that found no data-gradient launch to ride on (the last one of the backward pass and, with a
        group hook, of every layer group): the same job as the carried form, as its own launch."""
        lib, st = L.lib(), L.stream()
        while self._wred_pending:
            job = self._wred_pending.pop(0)
            L.check(lib.creid_conv2d_wgrad_reduce_job(C.byref(job.desc), L.ptr(job.grad), 1, L.ptr(job.ws), job.nbytes, self.dt, st),
                    "conv2d_wgrad_reduce_job")


class _BackboneFn(torch.autograd.Function):
    """Autograd boundary: the engine's backward writes parameter .grad directly."""

    @staticmethod
    def forward(ctx, x, trigger, engine, want_base_out):
        ctx.engine = engine
        base_out, feat = engine.forward(x, True, want_base_out)
        if base_out is None:
            base_out = feat.new_empty(0)
        ctx.mark_non_differentiable(base_out)
        return base_out, feat

    @staticmethod
    def backward(ctx, _g_base, g_feat):
        ctx.engine.backward(g_feat)
        return None, None, None, None
