"""modelling/baseline.py:44-107 Baseline on the HIP backbone engine.

`Baseline(cfg).forward(x) -> (base_out, global_feat)`; `self.base` holds the backbone parameters
under the reference's names (state_dict keys `base.conv1.weight`, ...).  `compute_dtype` selects the
activation / MFMA input type: torch.bfloat16 (throughput mode; the reference's AMP analogue when
cfg.USE_MIXED_PRECISION) or torch.float32 (parity mode, exact-f32 MFMA).  `eval_precision="bf16x3"` runs the eval-mode forward
(validation, inference) on a second engine over the same fp32 master weights: fp32 activations, convolutions as three bf16
MFMAs per product on split operands -- fp32-grade embeddings at several times the fp32 mode's rate; training keeps
`compute_dtype`.  `compute_dtype="bf16x3"` trains in that mode too: the fp32 mode's schedule with every non-stem convolution
(forward, data gradient, weight gradient) on the split-operand bf16 path; its eval-mode forward is the bf16x3 one.
`pooling="gem"` replaces the global average pool between the final map and the embedding by generalized-mean pooling with one
trainable exponent (`gap.p`, start value `gem_p`; Radenovic et al., TPAMI 2019) in every forward and in the backward; the default
`pooling="avg"` is the reference's mean and adds nothing to the state dict."""
from __future__ import annotations

import torch
from torch import nn

from . import _lib as L
from . import backbone as bb


GEM_P_RANGE = (1.0, 8.0)


class GemPool(nn.Module):
    """Owner of the generalized-mean pool's exponent: y = (mean_hw max(x, eps)^p)^(1/p).  The arithmetic lives in the backbone
    engine (creid_gem_fwd / creid_gem_bwd); this module is the parameter's home in the state dict (`gap.p`, shape [1], fp32)."""

    def __init__(self, p=3.0, eps=1e-6):
        super().__init__()
        if not GEM_P_RANGE[0] <= float(p) <= GEM_P_RANGE[1]:
            raise ValueError(f"gem_p must lie in [{GEM_P_RANGE[0]:g}, {GEM_P_RANGE[1]:g}], got {p!r}")
        if not float(eps) > 0:
            raise ValueError(f"gem_eps must be positive, got {eps!r}")
        self.p = nn.Parameter(torch.full((1,), float(p), dtype=torch.float32))
        self.eps = float(eps)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        # a reference-layout checkpoint has no exponent: it loads (strict too) and p keeps its start value
        n = len(missing_keys)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        if prefix + "p" not in state_dict:
            del missing_keys[n:]

    def extra_repr(self):
        return f"eps={self.eps:g}"


class Baseline(nn.Module):
    in_planes = 2048

    def __init__(self, cfg, compute_dtype=None, eval_precision=None, pooling="avg", gem_p=3.0, gem_eps=1e-6):
        super().__init__()
        if pooling not in bb.POOLINGS:
            raise ValueError(f"pooling must be one of {bb.POOLINGS}, got {pooling!r}")
        self.pooling = pooling
        gap = GemPool(gem_p, gem_eps) if pooling == "gem" else None       # (refused before any weight is built or loaded)
        last_stride = cfg.MODEL.LAST_STRIDE
        model_name = cfg.MODEL.NAME
        self.use_mixed_precision = cfg.USE_MIXED_PRECISION
        # modelling/baseline.py:56-81: resnet50 / 101 / 152 and resnet50_ibn_a / resnet101_ibn_a (Bottleneck networks, in_planes
        # 2048); resnet18 / resnet34 (BasicBlock, in_planes 512; round 6)
        self.base = bb.build_backbone(model_name, last_stride)
        self.in_planes = self.base.out_channels
        if gap is not None:
            self.gap = gap                 # `gap.p`, behind `base.*` in named_parameters(): the reference's name for its pooling
        self.model_name = model_name
        if cfg.MODEL.PRETRAINED and not cfg.MODEL.RESUME_TRAINING and not cfg.TEST.ONLY_TEST:
            self.base.load_param(cfg.MODEL.PRETRAIN_PATH)      # modelling/baseline.py:84-87
            print("Loading pretrained ImageNet model......")
        self.compute_dtype = compute_dtype or (torch.bfloat16 if cfg.USE_MIXED_PRECISION else torch.float32)
        if isinstance(self.compute_dtype, str) and self.compute_dtype not in L.TRAIN_PRECISIONS:
            raise ValueError(f"compute_dtype must be a torch dtype or one of {L.TRAIN_PRECISIONS}, got {self.compute_dtype!r}")
        # base_out = the reference's NCHW fp32 feature map (modelling/baseline.py:91-96).  A stand-alone Baseline returns it like the
        # reference does; ModelBase / CTLModel, which never consume it (`_, features = self.backbone(x)`, modelling/bases.py:171,
        # train_ctl_model.py:44), switch it off and save the 67 MB layout pass per batch.  It is a detached copy: gradients flow
        # through global_feat only.
        self.return_base_out = True
        if eval_precision is not None and eval_precision not in L.EVAL_PRECISIONS:
            raise ValueError(f"eval_precision must be None or one of {L.EVAL_PRECISIONS}, got {eval_precision!r}")
        self.eval_precision = eval_precision
        self._engine = None
        self._eval_engine = None
        self.loss_scaler = None           # f16 training: solver.LossScaler (ModelBase.configure_optimizers attaches it)

    def _engine_matches(self, eng):
        cd = self.compute_dtype
        if isinstance(cd, str):           # a string mode's engine computes in fp32: match on the mode, not on .dtype
            return eng.mode == cd and eng.x3_train
        return eng.mode is None and eng.dtype == cd

    def _pool_args(self):
        return dict(pooling=self.pooling, gem=getattr(self, "gap", None))

    @property
    def engine(self):
        if self._engine is None or not self._engine_matches(self._engine):
            if isinstance(self.compute_dtype, str):
                self._engine = bb.BackboneEngine(self.base, self.compute_dtype, trainable=True, **self._pool_args())
            else:
                self._engine = bb.BackboneEngine(self.base, self.compute_dtype, **self._pool_args())
        self._engine.loss_scaler = self.loss_scaler
        return self._engine

    def engine_for(self, training: bool):
        """The engine a forward in this mode runs on: the eval_precision engine for eval-mode forwards when one is set."""
        if training or self.eval_precision is None or self.eval_precision == self.compute_dtype:
            return self.engine
        if self._eval_engine is None or self._eval_engine.mode != self.eval_precision:
            self._eval_engine = bb.BackboneEngine(self.base, self.eval_precision, **self._pool_args())
        return self._eval_engine

    def state_dict(self, *args, **kwargs):
        if self._engine is not None:
            self._engine.fold_counters()
        return super().state_dict(*args, **kwargs)

    def forward(self, x):
        eng = self.engine_for(self.training)
        if isinstance(x, torch.Tensor):                 # (a transforms.StemOperand passes through: already the stem's layout)
            x = x.contiguous().float()
        if self.training and torch.is_grad_enabled():
            base_out, feat = bb._BackboneFn.apply(x, self.base.conv1.weight, eng, self.return_base_out)
            if base_out.numel() == 0:
                base_out = None
        else:
            base_out, feat = eng.forward(x, self.training, self.return_base_out)
        return base_out, feat

    def load_param(self, trained_path, load_specific=None):
        param_dict = torch.load(trained_path, map_location="cpu", weights_only=False)
        for i in param_dict:
            if load_specific is not None:
                if load_specific in i:
                    self.state_dict()[i].copy_(param_dict[i])
            else:
                if "classifier" in i:
                    continue
                self.state_dict()[i].copy_(param_dict[i])
        self.engine.weights_dirty = True
