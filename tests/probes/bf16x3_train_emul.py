"""Host emulation of bf16x3 TRAINING (compute_dtype="bf16x3"): every non-stem convolution is an autograd function whose forward,
input gradient and weight gradient each compute  lo*hi + hi*lo + hi*hi  in fp32 with x_hi = bf16(x), x_lo = bf16(x - x_hi)
(csrc/conv_x3.hip, csrc/conv_wgrad.hip wgrad_x3_kernel); activations, BatchNorm and the stem stay fp32.  One training-mode
forward / backward of the oracle's network (oracle/backbone_oracle.py) under a fixed random projection of the embeddings, in
fp64 (the yardstick), fp32 and the emulated mode.  Prints the errors the GPU tests bound:
  - aggregate relative L2 of the 53 conv-weight gradients, emulation against fp32 (tests/test_bf16x3_train_gpu.py);
  - the same against fp64 next to fp32's own, and the embeddings' max-abs error.
Not collected by pytest; uses oracle/ as a checker.
    python tests/probes/bf16x3_train_emul.py [arch] [B] [H] [W]      (default resnet50 8 128 64)"""
import os
import sys
import types

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import backbone_oracle as bo   # noqa: E402


def split(t):
    hi = t.to(torch.bfloat16).float()
    return hi, (t - hi).to(torch.bfloat16).float()


def x3(op, a, b):
    """op(a, b) as lo*hi + hi*lo + hi*hi of fp32 operands, in that order."""
    ah, al = split(a)
    bh, bl = split(b)
    return op(al, bh) + op(ah, bl) + op(ah, bh)


class X3Conv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, padding):
        ctx.save_for_backward(x, w)
        ctx.geo = (stride, padding)
        return x3(lambda a, b: F.conv2d(a, b, stride=stride, padding=padding), x, w)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, padding = ctx.geo
        gx = x3(lambda g, ww: torch.nn.grad.conv2d_input(x.shape, ww, g, stride=stride, padding=padding), gy.contiguous(), w)
        gw = x3(lambda g, xx: torch.nn.grad.conv2d_weight(xx, w.shape, g, stride=stride, padding=padding), gy.contiguous(), x)
        return gx, gw, None, None


def _conv_x3(x, w, bias=None, stride=1, padding=0, **kw):
    if x.dtype != torch.float32 or w.shape[1] == 3:          # fp64 / fp32 references and the exact-fp32 stem
        return F.conv2d(x, w, bias, stride=stride, padding=padding, **kw)
    return X3Conv.apply(x, w, stride, padding)


def grads(sd, x, coef, arch, dtype, emulate):
    shim = types.SimpleNamespace(**{k: getattr(F, k) for k in dir(F) if not k.startswith("__")})
    if emulate:
        shim.conv2d = _conv_x3
    saved, bo.F = bo.F, shim
    try:
        params = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()
                  if v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var"))}
        full = {**{k: (v.to(dtype) if v.dtype.is_floating_point else v).clone() for k, v in sd.items()}, **params}
        _, feat = bo.backbone_forward(x.to(dtype), full, arch, 1, training=True)
        (feat * coef.to(dtype)).sum().backward()
    finally:
        bo.F = saved
    return {k: p.grad.double() for k, p in params.items() if p.grad is not None}, feat.detach().double()


def main():
    arch = sys.argv[1] if len(sys.argv) > 1 else "resnet50"
    B, H, W = (int(v) for v in (sys.argv[2:5] if len(sys.argv) > 4 else (8, 128, 64)))
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    x = bo.synthetic_images(B, H, W, seed=43)
    coef = torch.randn((B, 2048), generator=torch.Generator().manual_seed(8))
    sd = bo.make_state_dict(arch, 1, seed=4322)
    g64, f64 = grads(sd, x, coef, arch, torch.float64, False)
    g32, f32 = grads(sd, x, coef, arch, torch.float32, False)
    gx3, fx3 = grads(sd, x, coef, arch, torch.float32, True)
    names = [n for n in g64 if n.endswith("weight") and g64[n].dim() == 4]

    def rel(g, ref):
        num = sum(float((g[n] - ref[n]).pow(2).sum()) for n in names)
        return (num / sum(float(ref[n].pow(2).sum()) for n in names)) ** 0.5
    worst = max((float((gx3[n] - g32[n]).norm() / g32[n].norm()), n) for n in names)
    print(f"{arch} B={B} {H}x{W}, {len(names)} conv weights")
    print(f"  conv-weight gradients, aggregate rel. L2: bf16x3 vs fp32 {rel(gx3, g32):.3e} | vs fp64: bf16x3 {rel(gx3, g64):.3e}, "
          f"fp32 {rel(g32, g64):.3e}")
    print(f"  worst single tensor bf16x3 vs fp32: {worst[0]:.3e} ({worst[1]})")
    print(f"  embeddings max-abs vs fp64: bf16x3 {float((fx3 - f64).abs().max()):.2e}, fp32 {float((f32 - f64).abs().max()):.2e}; "
          f"bf16x3 vs fp32 {float((fx3 - f32).abs().max()):.2e} (|feat| max {float(f64.abs().max()):.2f})")


if __name__ == "__main__":
    main()
