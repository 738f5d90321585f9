"""Host emulation of the bf16x3 eval-mode forward (CREID_BF16X3) against fp32 and f16, on the clustered-identity recipe of
f16_hi_emul.py (ResNet50 256 x 128, 96 ids x 8 images, 192 queries).  Each convolution computes
a_lo * w_hi + a_hi * w_lo + a_hi * w_hi in fp32 with x_hi = bf16(x), x_lo = bf16(x - x_hi); activations stay fp32 in memory
(as csrc/conv_x3.hip stores them).  Not collected by pytest; uses oracle/ as a checker.
    python tests/probes/bf16x3_emul.py [noise ...]      (default 0.6 0.9)"""
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f16_hi_emul as base  # noqa: E402   (the recipe, the fold and the f32 / f16 policies)
from oracle import backbone_oracle as bo, reid_oracle as ro   # noqa: E402


def split(t):
    hi = t.to(torch.bfloat16).float()
    return hi, (t - hi).to(torch.bfloat16).float()


def forward_x3(x, sd):
    def conv(a, name, stride=1, pad=0, bn=None, res=None, relu=True):
        ah, al = split(a)
        wh, wl = split(sd[name + ".weight"])
        y = (F.conv2d(al, wh, stride=stride, padding=pad) + F.conv2d(ah, wl, stride=stride, padding=pad)
             + F.conv2d(ah, wh, stride=stride, padding=pad))
        s, t = base.fold(sd, bn)
        y = y * s + t
        if res is not None:
            y = y + res
        return F.relu(y) if relu else y

    y = F.conv2d(x, sd["conv1.weight"], stride=2, padding=3)       # the stem stays exact fp32 (as in the product)
    s, t = base.fold(sd, "bn1")
    y = F.max_pool2d(y * s + t, 3, 2, 1)
    for pre, _i, _p, st, ds, _ibn in bo.arch_spec("resnet50", 1):
        o = conv(y, pre + ".conv1", bn=pre + ".bn1")
        o = conv(o, pre + ".conv2", st, 1, pre + ".bn2")
        r = conv(y, pre + ".downsample.0", st, 0, pre + ".downsample.1", relu=False) if ds else y
        y = conv(o, pre + ".conv3", bn=pre + ".bn3", res=r)
    return y.mean(dim=(2, 3))


def main():
    noises = [float(a) for a in sys.argv[1:]] or [0.6, 0.9]
    torch.manual_seed(0)
    n_id, nq, ng, H, W = 96, 2, 6, 256, 128
    per = nq + ng
    sd = bo.make_state_dict("resnet50", 1, seed=1234)
    for k in sd:
        if k.endswith(("bn1.weight", "bn2.weight", "bn3.weight", "downsample.1.weight", "running_var")):
            sd[k] = torch.ones_like(sd[k])
        elif k.endswith(("bn1.bias", "bn2.bias", "bn3.bias", "downsample.1.bias", "running_mean")):
            sd[k] = torch.zeros_like(sd[k])
    neck = {"w": torch.ones(2048), "b": torch.zeros(2048), "rm": torch.zeros(2048), "rv": torch.ones(2048)}
    print("| noise | policy | mAP | delta mAP | rel. L2 error of the embeddings: mean / max | rank-1 flips | s |\n|---|---|---|---|---|---|---|")
    for noise in noises:
        gen = torch.Generator().manual_seed(0)
        b = F.interpolate(torch.randn((n_id, 3, H // 16, W // 16), generator=gen), size=(H, W), mode="bilinear", align_corners=False)
        x = b.repeat_interleave(per, 0) + noise * torch.randn((n_id * per, 3, H, W), generator=gen)
        slot = np.tile(np.arange(per), n_id)
        q_rows = np.nonzero(slot < nq)[0]; g_rows = np.nonzero(slot >= nq)[0]
        order = np.concatenate([q_rows, g_rows])
        pids = np.repeat(np.arange(n_id), per)[order]
        cams = np.concatenate([np.zeros(len(q_rows), np.int64), np.ones(len(g_rows), np.int64)])
        s2 = {k: v.clone() for k, v in sd.items()}
        with torch.no_grad():
            for s in range(0, 512, 64):
                _, f = bo.backbone_forward(x[s:s + 64], s2, training=True)
                F.batch_norm(f, neck["rm"], neck["rv"], neck["w"], neck["b"], True, 0.1, 1e-5)
        ref = None
        for pol in ("f32", "f16", "bf16x3"):
            t0 = time.time()
            out = []
            with torch.no_grad():
                for s in range(0, len(x), 64):
                    f = forward_x3(x[s:s + 64], s2) if pol == "bf16x3" else base.forward(x[s:s + 64], s2, pol)
                    out.append(F.batch_norm(f, neck["rm"], neck["rv"], neck["w"], neck["b"], False, 0.1, 1e-5))
            e = torch.cat(out)[torch.as_tensor(order)].contiguous()
            _, mAP, _, _ = ro.r1_map(e, pids, cams, len(q_rows))
            en = F.normalize(e, dim=1)
            top1 = (en[:len(q_rows)] @ en[len(q_rows):].T).argmax(1)
            if ref is None:
                ref = (en, mAP, top1)
            rel = (en - ref[0]).norm(dim=1)
            print(f"| {noise} | {pol} | {mAP:.6f} | {mAP - ref[1]:+.2e} | {rel.mean().item():.2e} / {rel.max().item():.2e} | "
                  f"{int((top1 != ref[2]).sum())} | {time.time() - t0:.0f} |", flush=True)


if __name__ == "__main__":
    main()
