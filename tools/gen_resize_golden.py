"""Record tests/golden/pil_resize.npz: sources and Pillow's own `Image.resize((W, H), Image.BILINEAR)` outputs for the device
Resize (csrc/resize.hip).  Pillow only -- the GPU tests read this file, never Pillow.

    python tools/gen_resize_golden.py

Targets straddle the kernel's 32 x 64 tile (and its 8-row wave slices): 21 x 37 (inside one tile), 32 x 64 (exactly one),
33 x 65 (one sample more on both axes); the production case is Market-1501's 128 x 64 file at the reference's 256 x 128.  Keys:
"<case>/src" uint8 [h, w, 3] and "<case>/out" uint8 [H, W, 3]; case names start with "t<H>x<W>_"."""
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = ((21, 37), (32, 64), (33, 65))


def picture(rng, h, w):
    """Edges, ramps and speckle: coarse random blocks under a per-channel ramp, a twentieth of the pixels pure noise."""
    bh, bw = (h + 6) // 7, (w + 6) // 7
    img = np.kron(rng.integers(0, 256, (bh, bw, 3)), np.ones((7, 7, 1), np.int64))[:h, :w].astype(np.int64)
    ramp = np.add.outer(np.arange(h) * int(rng.integers(0, 4)), np.arange(w) * int(rng.integers(0, 4)))
    img = (img + ramp[:, :, None]) % 256
    noise = rng.integers(0, 256, (h, w, 3))
    return np.where(rng.random((h, w, 1)) < 0.05, noise, img).astype(np.uint8)


def stripes(h, w, rows):
    v = (np.arange(h)[:, None] if rows else np.arange(w)[None, :]) % 2 * 255
    return np.ascontiguousarray(np.broadcast_to(v[:, :, None], (h, w, 3))).astype(np.uint8)


def sources(rng, H, W):
    odd = lambda v: int(v) | 1
    yield "1x1", picture(rng, 1, 1)
    yield "2x3", picture(rng, 2, 3)
    yield "identity", picture(rng, H, W)
    yield "h_equal", picture(rng, H, odd(W * 1.4))
    yield "w_equal", picture(rng, odd(H * 1.4), W)
    yield "up", picture(rng, odd(H / 1.7), odd(W / 1.3))                    # non-integer factors, odd sizes
    yield "down23", picture(rng, odd(H * 2.3), odd(W * 2.3))
    yield "heavy_w", picture(rng, 3, 11 * W + 4)                             # ksize = 25 horizontally
    yield "heavy_h", picture(rng, 11 * H + 4, 5)                             # ksize = 25 vertically
    yield "stripe_rows", stripes(odd(H * 1.5), W + 3, True)                  # rounding and clipping at saturation
    yield "stripe_cols", stripes(H + 3, odd(W * 1.5), False)


def main():
    rng = np.random.default_rng(20240607)
    out = {}

    def add(name, src, H, W):
        out[name + "/src"] = src
        out[name + "/out"] = np.asarray(Image.fromarray(src).resize((W, H), Image.BILINEAR), dtype=np.uint8)
        assert out[name + "/out"].shape == (H, W, 3)
    for H, W in TARGETS:
        for name, src in sources(rng, H, W):
            add(f"t{H}x{W}_{name}", src, H, W)
    add("t256x128_market", picture(rng, 128, 64), 256, 128)
    path = os.path.join(ROOT, "tests", "golden", "pil_resize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out) // 2, "cases")


if __name__ == "__main__":
    main()
