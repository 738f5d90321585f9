"""The device Resize (csrc/resize.hip, creid_resize_u8) measured: its device time beside the augment pass it feeds, its share of
the achievable HBM rate, the host side of feeding un-resized images, and run_inference fed both ways.
    python tools/resize_bench.py --out profiles/device_resize.md
Two batches: 512 x (128 x 64 -> 256 x 128), Market-1501's files at the reference's size, and 128 x (736 x 736 -> 320 x 320), a
2.3 x downscale.  Device times: >= 5 warm-ups, then the two kernels alternated, 30 rounds of 20 launches each between device
events; medians and the spread (max - min) / median over the rounds.  Host times: wall clock around work that ends in a device
synchronise, median of 7.  Images are seeded noise decoded in memory: NO JPEG decode anywhere.  Needs a GPU; no fallback."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from centroids_reid_amd import _lib as L   # noqa: E402
from centroids_reid_amd.transforms import DeviceTransform, RaggedImages   # noqa: E402

try:
    from PIL import Image   # noqa: F401
    HAVE_PIL = True
except ImportError:
    HAVE_PIL = False

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
HBM_ACHIEVABLE = 6.29e12                   # bytes/s, measured float4 copy on the MI355X
CASES = [("512 x (128 x 64 -> 256 x 128)", 512, (128, 64), (256, 128)),
         ("128 x (736 x 736 -> 320 x 320)", 128, (736, 736), (320, 320))]
ROUNDS, PER_ROUND = 30, 20


def images(B, hw, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (*hw, 3), dtype=np.uint8) for _ in range(B)]


def device_rounds(fns):
    """Alternate the launches of `fns`; per function the per-launch milliseconds of every round."""
    for _ in range(5):
        for f in fns:
            f()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(ROUNDS):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(PER_ROUND):
                f()
            b.record()
            b.synchronize()
            out[i].append(a.elapsed_time(b) / PER_ROUND)
    return [np.array(v) for v in out]


def med_spread(v):
    m = float(np.median(v))
    return m, float((v.max() - v.min()) / m)


def wall(fn, reps=7):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def kernel_section(lines):
    lib = L.lib()
    lines += ["## 1, 2. Device time of `creid_resize_u8` beside `creid_augment_u8`, and the share of the HBM rate", "",
              "Per launch, device events; bytes = what the algorithm must move (source pixels + resized pixels for the resize; resized",
              "pixels + the output tensor for the augment pass, test transform).  Share of HBM = bytes / time / 6.29 TB/s (the measured",
              "copy rate).  The working sets (63 MB and 247 MB for the resize) are re-used launch after launch and the first fits in the",
              "256 MiB Infinity Cache, so the shares say how far a kernel is from the rate a streaming pass could reach at most, not that",
              "its bytes came from HBM.", "",
              "| batch | kernel | bytes moved | time (us) | spread | GB/s | share of 6.29 TB/s |", "|---|---|---|---|---|---|---|"]
    for label, B, hw, (H, W) in CASES:
        t = DeviceTransform((H, W), MEAN, STD, is_train=False)
        r = RaggedImages.pack(images(B, hw, 1)).to("cuda")
        words = t.resize_tables(r)
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda")
        nchw = torch.empty((B, 3, H, W), dtype=torch.float32, device="cuda")
        stem = torch.empty((B, H + 8, W + 6, 4), dtype=torch.bfloat16, device="cuda")
        m, s = MEAN, STD

        def k_resize():
            L.check(lib.creid_resize_u8(L.ptr(r.data), r.data.numel(), L.ptr(r.offsets), L.ptr(r.sizes), L.ptr(words), words.numel(),
                                        L.ptr(words), B, H, W, L.ptr(out), L.stream()), "resize")

        def k_aug(lay, dst, dt):
            return lambda: L.check(lib.creid_augment_u8(L.ptr(out), None, B, H, W, 0, *m, *s, *m, lay, L._DT[dt], L.ptr(dst), L.stream()), "aug")
        want = t.resize_batch(r)
        k_resize()
        assert torch.equal(out, want)
        res = device_rounds([k_resize, k_aug(0, nchw, torch.float32), k_aug(1, stem, torch.bfloat16)])
        nb = [r.data.numel() + out.numel(), out.numel() + nchw.numel() * 4, out.numel() + stem.numel() * 2]
        for name, v, n in zip(("creid_resize_u8", "creid_augment_u8 -> fp32 NCHW", "creid_augment_u8 -> bf16 stem operand"), res, nb):
            md, sp = med_spread(v)
            rate = n / (md * 1e-3)
            lines.append(f"| {label} | {name} | {n / 1e6:.1f} MB | {md * 1e3:.1f} | {sp * 100:.0f} % | {rate / 1e9:.0f} | {rate / HBM_ACHIEVABLE * 100:.1f} % |")
        lines.append(f"| {label} | resize / augment (fp32 NCHW) | | {np.median(res[0]) / np.median(res[1]):.2f} x | | | |")
    lines.append("")


def host_section(lines):
    lines += ["## 3. The host side: pack + upload of the un-resized images against resize on the host + upload of the resized batch", "",
              "Wall time of one batch from decoded in-memory images to pixels on the device (synchronised), one process, 16 CPU threads",
              "allowed (the host resize is one `DeviceTransform.resize` = `PIL.Image.resize` call per image, in a loop, as a DataLoader",
              "worker would run it).", "",
              "| batch | path | host wall (ms) | bytes uploaded |", "|---|---|---|---|"]
    for label, B, hw, (H, W) in CASES:
        t = DeviceTransform((H, W), MEAN, STD, is_train=False)
        imgs = images(B, hw, 2)

        def ragged():
            return RaggedImages.pack(imgs).to("cuda")
        r = ragged()
        lines.append(f"| {label} | RaggedImages.pack + upload | {wall(ragged):.2f} | {(r.data.numel() + r.meta.numel() * 8) / 1e6:.1f} MB |")
        lines.append(f"| {label} | ... + resize_batch on the device | {wall(lambda: t.resize_batch(ragged())):.2f} | same |")
        if HAVE_PIL:
            pil = [Image.fromarray(im) for im in imgs]

            def dense():
                return torch.from_numpy(np.stack([t.resize(p) for p in pil])).pin_memory().to("cuda", non_blocking=True)
            lines.append(f"| {label} | DeviceTransform.resize per image + stack + upload | {wall(dense):.2f} | {B * H * W * 3 / 1e6:.1f} MB |")
        else:
            lines.append(f"| {label} | DeviceTransform.resize per image + stack + upload | not measured (no Pillow on this box) | {B * H * W * 3 / 1e6:.1f} MB |")
    lines.append("")


def inference_section(lines):
    from centroids_reid_amd import inference as inf
    from centroids_reid_amd.bench_train import make_model
    torch.manual_seed(0)
    model = make_model(num_classes=16, dtype=torch.bfloat16).eval()
    N, bs, (H, W) = 4096, 128, (256, 128)
    t = DeviceTransform((H, W), MEAN, STD, is_train=False)
    imgs = images(N, (128, 64), 3)
    names = [str(i) for i in range(N)]
    lines += ["## 4. `run_inference` fed both ways", "",
              f"{N} in-memory decoded 128 x 64 images (no JPEG decode), loader batches of {bs}, macro_batch 512, bf16 ResNet-50 at 256 x 128;",
              "wall time of the whole call (host work, uploads, the forward, the download of the embeddings), median of 5.", "",
              "| loader yields | images/s | wall (ms) |", "|---|---|---|"]

    class Ragged:
        def __iter__(self):
            for i in range(0, N, bs):
                yield imgs[i:i + bs], None, names[i:i + bs]                 # packed by run_inference

    same = False
    e_r, _ = inf.run_inference(model, Ragged(), transform=t)
    ms = wall(lambda: inf.run_inference(model, Ragged(), transform=t), reps=5)
    lines.append(f"| lists of un-resized arrays (pack + upload + device Resize) | {N / ms * 1e3:.0f} | {ms:.0f} |")
    if HAVE_PIL:
        pil = [Image.fromarray(im) for im in imgs]

        class Dense:
            def __iter__(self):
                for i in range(0, N, bs):
                    yield torch.from_numpy(np.stack([t.resize(p) for p in pil[i:i + bs]])), None, names[i:i + bs]
        e_d, _ = inf.run_inference(model, Dense(), transform=t)
        assert np.array_equal(e_d, e_r), "the two feeds must give the same embedding bits"
        ms = wall(lambda: inf.run_inference(model, Dense(), transform=t), reps=5)
        lines.append(f"| uint8 batches resized on the host (PIL per image) | {N / ms * 1e3:.0f} | {ms:.0f} |")
        same = True
    else:
        lines.append("| uint8 batches resized on the host (PIL per image) | not measured (no Pillow on this box) | |")
    pre = [t.resize_batch(RaggedImages.pack(imgs[i:i + bs])).cpu() for i in range(0, N, bs)]

    class Pre:
        def __iter__(self):
            for j, i in enumerate(range(0, N, bs)):
                yield pre[j], None, names[i:i + bs]
    ms = wall(lambda: inf.run_inference(model, Pre(), transform=t), reps=5)
    lines.append(f"| uint8 batches resized beforehand, resize NOT timed (the ceiling of the host feed) | {N / ms * 1e3:.0f} | {ms:.0f} |")
    if same:
        lines += ["", "The embeddings of the two feeds are bit-identical (asserted)."]
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/device_resize.md")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/resize_bench.py measures on the GPU; there is no fallback")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lines = ["# The Resize on the device: `creid_resize_u8` measured", "",
             f"One MI355X, one process, one session ({torch.cuda.get_device_name(0)}, torch {torch.__version__}); written by",
             "`tools/resize_bench.py`.  Seeded noise images, decoded in memory: no JPEG decode is part of any number here.", ""]
    kernel_section(lines)
    host_section(lines)
    inference_section(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
