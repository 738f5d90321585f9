"""Input side of the path ("device-side augment would follow"): the reference's per-image transforms
(datasets/transforms/build.py:10-33, datasets/transforms/random_erasing.py:11-55) on the device: the Resize over a ragged uint8
batch, everything after it as ONE pass over the resized uint8 batch.

    ReidTransforms(cfg).build_transforms(is_train) -> DeviceTransform
    t = DeviceTransform(...)
    params = t.draw(B)                       # host: the reference's random draws, same generators, same order per image
    x = t(images_u8, params)                 # device: flip -> pad -> crop -> ToTensor -> Normalize -> RandomErasing, fp32 NCHW
    x = t(images_u8, params, layout="stem")  # or straight into the stem convolution's padded NHWC4 operand (StemOperand)
    r = RaggedImages.pack(decoded_images)    # host: images of ANY size, packed back to back in one page-locked buffer
    x = t(r.to("cuda"), params)              # device: Resize first (creid_resize_u8), then the same pass
    u8 = t.resize_batch(r)                   # or the Resize alone -> uint8 [B, H, W, 3]

The Resize (T.Resize(size) on a PIL image = `Image.resize((W, H), BILINEAR)`) runs on the device too, in `creid_resize_u8`
(csrc/resize.hip), and its result EQUALS Pillow's byte for byte: Pillow's 8-bit resample is fixed-point integer arithmetic
(include/creid.h restates it), the coefficient tables are made here on the host in float64 (`resample_table`) and the kernel
does integer work only.  It precedes every random draw and uses none, so `draw()` is untouched and the same `params` give the
same output for a ragged batch as for the batch resized beforehand.  `DeviceTransform.resize` (host, one PIL image) stays for
callers that resize in their DataLoader workers.  Everything after the Resize is a pure function of (pixels, draws) and runs in
`creid_augment_u8` (csrc/augment.hip).  No CPU fallback: a CPU batch raises like every other entry point."""
from __future__ import annotations

import math
import random as _py_random

import numpy as np
import torch
import torch.utils.data

from . import _lib as L


class StemOperand:
    """A batch already in the stem convolution's operand layout (zero-padded NHWC4 [B, H + 8, W + 6, 4], compute dtype);
    `Baseline.forward` / the backbone engine take it in place of the fp32 NCHW tensor and skip their own layout pass."""

    def __init__(self, xpad: torch.Tensor, B: int, H: int, W: int):
        self.xpad, self.B, self.H, self.W = xpad, B, H, W

    @property
    def shape(self):
        return (self.B, 3, self.H, self.W)

    @property
    def device(self):
        return self.xpad.device


MAX_SOURCE_SIDE, MAX_TARGET_SIDE = 16384, 4096        # the limits of creid_resize_u8 (include/creid.h)
PRECISION_BITS = 22                                    # Pillow's fixed point for 8-bit images
_TABLES: dict = {}


def resample_table(n_in: int, n_out: int) -> np.ndarray:
    """Pillow's bilinear coefficients for one axis resampled from `n_in` to `n_out` samples, as creid_resize_u8 reads them: int32
    [n_out * (2 + ksize)] = {first tap, tap count} per output sample, then `ksize` = 2 ceil(max(n_in / n_out, 1)) + 1 coefficients
    per output sample (22-bit fixed point, zero beyond the tap count).  Everything in float64, as Pillow computes it; cached."""
    key = (int(n_in), int(n_out))
    tab = _TABLES.get(key)
    if tab is not None:
        return tab
    n_in, n_out = key
    if not (1 <= n_in <= MAX_SOURCE_SIDE and 1 <= n_out <= MAX_TARGET_SIDE):
        raise ValueError(f"resize {n_in} -> {n_out}: source sides 1..{MAX_SOURCE_SIDE}, target sides 1..{MAX_TARGET_SIDE}")
    xx = np.arange(n_out, dtype=np.int64)
    if n_in == n_out:                                   # Pillow skips the pass: the identity
        ksize = 3
        first, count = xx, np.ones(n_out, np.int64)
        k = np.zeros((n_out, ksize), np.int64)
        k[:, 0] = 1 << PRECISION_BITS
    else:
        scale = n_in / n_out
        fs = max(scale, 1.0)
        ksize = 2 * int(math.ceil(fs)) + 1
        center = (xx + 0.5) * scale
        first = np.maximum(np.trunc(center - fs + 0.5).astype(np.int64), 0)
        count = np.minimum(np.trunc(center + fs + 0.5).astype(np.int64), n_in) - first
        x = np.arange(ksize, dtype=np.int64)[None, :]
        a = np.abs(((x + first[:, None]) - center[:, None] + 0.5) * (1.0 / fs))
        w = np.where((a < 1.0) & (x < count[:, None]), 1.0 - a, 0.0)
        ww = np.zeros(n_out)
        for i in range(ksize):                          # the running sum in tap order (not numpy's pairwise sum)
            ww = ww + w[:, i]
        w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
        k = np.trunc(w * float(1 << PRECISION_BITS) + 0.5).astype(np.int64)
    tab = np.concatenate([np.stack([first, count], 1).reshape(-1), k.reshape(-1)]).astype(np.int32)
    tab.setflags(write=False)
    if len(_TABLES) > 4096:
        _TABLES.clear()
    _TABLES[key] = tab
    return tab


def _as_hwc_u8(im) -> np.ndarray:
    """One image as a contiguous uint8 [h, w, 3] array: a PIL image (converted to RGB as `DeviceTransform.resize` does), a numpy
    array or a CPU tensor."""
    if isinstance(im, torch.Tensor):
        if im.is_cuda:
            raise ValueError("RaggedImages.pack takes host images (the pack is what gets uploaded)")
        arr = im.numpy()
    elif isinstance(im, np.ndarray):
        arr = im
    elif hasattr(im, "convert"):
        arr = np.asarray(im.convert("RGB"))
    else:
        raise ValueError(f"an image is a uint8 [h, w, 3] array or tensor, or a PIL image; got {type(im).__name__}")
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError(f"an image is uint8 [h, w, 3]; got {arr.dtype} {tuple(arr.shape)}")
    h, w = arr.shape[:2]
    if not (1 <= h <= MAX_SOURCE_SIDE and 1 <= w <= MAX_SOURCE_SIDE):
        raise ValueError(f"image sides must be 1..{MAX_SOURCE_SIDE}; got {(h, w)}")
    return arr


def _host_buffer(n: int, dtype) -> torch.Tensor:
    """Page-locked where there is a device to upload to (torch's caching host allocator hands a block out again only after the
    copies enqueued from it have completed); pageable inside a DataLoader worker, which must not create a device context."""
    pin = torch.cuda.is_available() and torch.utils.data.get_worker_info() is None
    return torch.empty(n, dtype=dtype, pin_memory=pin)


class RaggedImages:
    """A batch of uint8 RGB images of different sizes: `data` uint8 [sum 3 h w], the images packed back to back as HWC (so an image
    starts at ANY byte offset), `meta` int64 [2 B] = the B byte offsets, then the B (h, w) pairs as int32 -- one buffer, so a pack
    goes up in two copies.  Built on the host (`pack`, `cat`), moved with `to(device)`."""

    def __init__(self, data: torch.Tensor, meta: torch.Tensor, sizes_host: np.ndarray):
        self.data, self.meta = data, meta
        self.sizes_host = sizes_host                    # int32 [B, 2] on the host: the resize tables are chosen from it
        self._uploaded = None

    @classmethod
    def _from_arrays(cls, arrays):
        sizes = np.array([a.shape[:2] for a in arrays], dtype=np.int32).reshape(-1, 2)
        nbytes = 3 * sizes[:, 0].astype(np.int64) * sizes[:, 1].astype(np.int64)
        offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
        B = len(arrays)
        data = _host_buffer(int(nbytes.sum()), torch.uint8)
        meta = _host_buffer(2 * B, torch.int64)
        flat = data.numpy()
        for a, o, n in zip(arrays, offsets, nbytes):
            np.copyto(flat[o:o + n].reshape(a.shape), a)
        m = meta.numpy()
        m[:B] = offsets
        m[B:].view(np.int32)[:] = sizes.reshape(-1)
        return cls(data, meta, sizes)

    @classmethod
    def pack(cls, images) -> "RaggedImages":
        """images: a non-empty sequence of uint8 [h, w, 3] arrays / CPU tensors or PIL images (`.convert("RGB")`)."""
        arrays = [_as_hwc_u8(im) for im in images]
        if not arrays:
            raise ValueError("RaggedImages.pack: no images")
        return cls._from_arrays(arrays)

    @classmethod
    def cat(cls, packs) -> "RaggedImages":
        """Join packs (on one device) in order."""
        packs = list(packs)
        if not packs or not all(isinstance(p, RaggedImages) for p in packs):
            raise ValueError("RaggedImages.cat takes a non-empty sequence of RaggedImages")
        if len(packs) == 1:
            return packs[0]
        if any(p.device != packs[0].device for p in packs):
            raise ValueError("RaggedImages.cat: the packs are on different devices")
        sizes = np.concatenate([p.sizes_host for p in packs])
        B = len(sizes)
        nbytes = 3 * sizes[:, 0].astype(np.int64) * sizes[:, 1].astype(np.int64)
        offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
        dev = packs[0].device
        if dev.type == "cpu":
            data = _host_buffer(int(nbytes.sum()), torch.uint8)
            torch.cat([p.data for p in packs], out=data)
        else:
            data = torch.cat([p.data for p in packs])
        meta = _host_buffer(2 * B, torch.int64)
        m = meta.numpy()
        m[:B] = offsets
        m[B:].view(np.int32)[:] = sizes.reshape(-1)
        return cls(data, meta if dev.type == "cpu" else meta.to(dev, non_blocking=True), sizes)

    def __len__(self):
        return len(self.sizes_host)

    @property
    def device(self):
        return self.data.device

    @property
    def is_cuda(self):
        return self.data.is_cuda

    @property
    def offsets(self) -> torch.Tensor:
        return self.meta[:len(self)]

    @property
    def sizes(self) -> torch.Tensor:
        return self.meta[len(self):].view(torch.int32).view(-1, 2)

    def to(self, device) -> "RaggedImages":
        """Upload (non-blocking from the page-locked pack, on the current stream).  The device copy keeps the host pack alive
        and carries the event of its upload: `wait_uploaded()` tells when the host buffers may be rewritten."""
        dev = torch.device(device)
        if dev == self.device or (dev.type == "cuda" and self.is_cuda and dev.index is None):
            return self
        out = RaggedImages(self.data.to(dev, non_blocking=True), self.meta.to(dev, non_blocking=True), self.sizes_host)
        if dev.type == "cuda" and not self.is_cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            out._uploaded = (ev, self)
        return out

    def cuda(self):
        return self.to("cuda")

    def wait_uploaded(self):
        if self._uploaded is not None:
            self._uploaded[0].synchronize()


_TABLE_STAGE: dict = {}


def _upload_tables(words: np.ndarray, device) -> torch.Tensor:
    """int32 device tensor of the batch's table offsets and tables through a reused page-locked staging buffer (the discipline
    of reid_metric._upload_labels: reused only after the event of its previous upload)."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    ent = _TABLE_STAGE.get(key)
    if ent is None or ent[0].numel() < len(words):
        if ent is not None:
            ent[1].synchronize()
        ent = _TABLE_STAGE[key] = (torch.empty(max(len(words), 1 << 14), dtype=torch.int32, pin_memory=True), torch.cuda.Event())
    else:
        ent[1].synchronize()
    stage, ev = ent
    np.copyto(stage.numpy()[:len(words)], words)
    dev = stage[:len(words)].to(device, non_blocking=True)
    ev.record(torch.cuda.current_stream(device))
    return dev


class DeviceTransform:
    def __init__(self, size, mean, std, is_train=True, flip_p=0.5, padding=10, re_prob=0.5, sl=0.02, sh=0.4, r1=0.3):
        self.H, self.W = int(size[0]), int(size[1])
        self.mean = [float(v) for v in mean]
        self.std = [float(v) for v in std]
        self.is_train, self.flip_p, self.padding, self.re_prob = bool(is_train), float(flip_p), int(padding), float(re_prob)
        self.sl, self.sh, self.r1 = sl, sh, r1

    # ---- host: Resize (T.Resize(size) on a PIL image = bilinear resize to (W, H))
    def resize(self, pil_image) -> np.ndarray:
        from PIL import Image
        im = pil_image.convert("RGB")
        if im.size != (self.W, self.H):
            im = im.resize((self.W, self.H), Image.BILINEAR)
        return np.asarray(im, dtype=np.uint8)

    # ---- host: the random draws, in the reference pipeline's order for every image
    def draw(self, B: int, rnd=None, generator: torch.Generator | None = None) -> np.ndarray:
        """int32 [B, 8] = {flip, crop_top, crop_left, erase, x1, y1, h, w}.  Flip and crop come from torch's generator
        (torchvision: `torch.rand(1) < p`, `torch.randint(0, h - th + 1, (1,))`, then the column), the erasing rectangle from
        python's `random` (random_erasing.py:33-47) -- pass `rnd` / `generator` to use private streams."""
        rnd = rnd or _py_random
        out = np.zeros((B, 8), np.int32)
        if not self.is_train:
            return out                                                  # the test transform has no draws
        for b in range(B):
            flip = bool(torch.rand(1, generator=generator) < self.flip_p)
            span_h, span_w = 2 * self.padding + 1, 2 * self.padding + 1
            top = int(torch.randint(0, span_h, (1,), generator=generator).item()) if self.padding else 0
            left = int(torch.randint(0, span_w, (1,), generator=generator).item()) if self.padding else 0
            out[b, :3] = (int(flip), top, left)
            out[b, 3:] = self.draw_erasing(rnd)
        return out

    def draw_erasing(self, rnd):
        """random_erasing.py:31-55: (erase, x1 = first row, y1 = first column, h, w)."""
        H, W = self.H, self.W
        if rnd.uniform(0, 1) >= self.re_prob:
            return 0, 0, 0, 0, 0
        for _ in range(100):
            area = H * W
            target_area = rnd.uniform(self.sl, self.sh) * area
            aspect_ratio = rnd.uniform(self.r1, 1 / self.r1)
            h = int(round(math.sqrt(target_area * aspect_ratio)))
            w = int(round(math.sqrt(target_area / aspect_ratio)))
            if w < W and h < H:
                return 1, rnd.randint(0, H - h), rnd.randint(0, W - w), h, w
        return 0, 0, 0, 0, 0

    # ---- device: Resize
    def resize_tables(self, ragged: "RaggedImages") -> torch.Tensor:
        """The int32 device tensor creid_resize_u8 reads for this pack: [B, 2] table offsets (the image's width table, its height
        table), then one table per distinct (side -> target side) pair of the batch.  One small upload."""
        B, H, W = len(ragged), self.H, self.W
        where, parts, pos = {}, [], 2 * B
        toff = np.empty((B, 2), np.int32)
        for axis, target in ((1, W), (0, H)):
            for n_in in np.unique(ragged.sizes_host[:, axis]):
                tab = resample_table(int(n_in), target)
                where[int(n_in)] = pos
                parts.append(tab)
                pos += len(tab)
            toff[:, 1 - axis] = [where[int(n)] for n in ragged.sizes_host[:, axis]]
            where.clear()
        return _upload_tables(np.concatenate([toff.reshape(-1)] + parts), ragged.device)

    def resize_batch(self, ragged: "RaggedImages") -> torch.Tensor:
        """uint8 [B, H, W, 3] on the device: every image of the pack resized to (H, W) as `resize` does it, byte for byte
        (creid_resize_u8).  A host pack is uploaded first."""
        if not isinstance(ragged, RaggedImages):
            raise ValueError(f"resize_batch takes a RaggedImages, got {type(ragged).__name__}")
        if not torch.cuda.is_available():
            raise L.CreidError("centroids-reid_amd ops need a HIP device (no CPU fallback); resize_batch got a host pack")
        r = ragged if ragged.is_cuda else ragged.to("cuda")
        L.require_gpu(r.data, r.meta)
        B, H, W = len(r), self.H, self.W
        words = self.resize_tables(r)
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=r.device)
        L.check(L.lib().creid_resize_u8(L.ptr(r.data), r.data.numel(), L.ptr(r.offsets), L.ptr(r.sizes), L.ptr(words), words.numel(),
                                        L.ptr(words), B, H, W, L.ptr(out), L.stream()), "resize_u8")
        return out

    # ---- device
    def __call__(self, images_u8, params=None, layout: str = "nchw", dtype=torch.float32):
        """images_u8: uint8 [B, H, W, 3] on the GPU (resized, HWC as PIL yields them), or a RaggedImages of any sizes, which is
        resized first (resize_batch).  params: int32 [B, 8] from draw() (numpy or device tensor); None = the test transform (and,
        in training mode, a fresh draw())."""
        if isinstance(images_u8, RaggedImages):
            images_u8 = self.resize_batch(images_u8)
        L.require_gpu(images_u8)
        assert images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[3] == 3, "uint8 [B, H, W, 3] expected"
        B, H, W, _ = images_u8.shape
        assert (H, W) == (self.H, self.W), f"images must be resized to {(self.H, self.W)} first (DeviceTransform.resize, or pass a RaggedImages)"
        images_u8 = images_u8.contiguous()
        if params is None and self.is_train:
            params = self.draw(B)
        pdev = None
        if params is not None and self.is_train:
            pdev = params if isinstance(params, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(params, dtype=np.int32))
            pdev = pdev.to(device=images_u8.device, dtype=torch.int32).contiguous()
            assert tuple(pdev.shape) == (B, 8)
        if layout == "nchw":
            assert dtype == torch.float32, "the reference tensor is fp32"
            out = torch.empty((B, 3, H, W), dtype=torch.float32, device=images_u8.device)
            lay = 0
        elif layout == "stem":
            out = torch.empty((B, H + 8, W + 6, 4), dtype=dtype, device=images_u8.device)
            lay = 1
        else:
            raise ValueError(f"layout {layout!r}: 'nchw' or 'stem'")
        m, s = self.mean, self.std
        L.check(L.lib().creid_augment_u8(L.ptr(images_u8), L.ptr(pdev), B, H, W, self.padding if self.is_train else 0,
                                         m[0], m[1], m[2], s[0], s[1], s[2], m[0], m[1], m[2], lay, L._DT[dtype], L.ptr(out),
                                         L.stream()), "augment_u8")
        return out if lay == 0 else StemOperand(out, B, H, W)


class ReidTransforms:
    """datasets/transforms/build.py:10-33 (same constructor and `build_transforms(is_train)`); the result works on uint8
    batches (resized, or ragged) on the device instead of on one PIL image in a DataLoader worker."""

    def __init__(self, cfg):
        self.cfg = cfg

    def build_transforms(self, is_train=True) -> DeviceTransform:
        i = self.cfg.INPUT
        return DeviceTransform(i.SIZE_TRAIN if is_train else i.SIZE_TEST, i.PIXEL_MEAN, i.PIXEL_STD, is_train=is_train,
                               flip_p=i.PROB, padding=i.PADDING, re_prob=i.RE_PROB)
