"""Pillow's 8-bit bilinear `Image.resize`, restated in plain Python / numpy for the resize tests.  Written from the arithmetic
alone (two separable passes, horizontal first, 22-bit integer coefficients, the intermediate rounded to uint8) and sharing no
code with the product's table builder (centroids-reid_amd/transforms.py `resample_table`): scalar loops, one output sample at a
time, so that the two can be compared against each other and against Pillow (tests/test_resize_cpu.py)."""
import math

import numpy as np

BITS = 22


def axis_coeffs(n_in, n_out):
    """[(first tap, [integer coefficient per tap])] for every output sample of one axis."""
    scale = float(n_in) / float(n_out)
    fs = scale if scale > 1.0 else 1.0
    support = fs
    inv = 1.0 / fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)              # int() truncates toward zero like a C cast
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > n_in:
            xmax = n_in
        ws, ww = [], 0.0
        for x in range(xmax - xmin):
            a = (x + xmin - center + 0.5) * inv
            if a < 0.0:
                a = -a
            w = 1.0 - a if a < 1.0 else 0.0
            ws.append(w)
            ww += w
        ks = []
        for w in ws:
            if ww != 0.0:
                w = w / ww
            ks.append(int(w * (1 << BITS) + 0.5))
        out.append((xmin, ks))
    return out


def ksize(n_in, n_out):
    return 2 * int(math.ceil(max(float(n_in) / float(n_out), 1.0))) + 1


def _pass(img, n_out):
    """Resample axis 1 of an int64 [rows, n_in, 3] array to n_out samples, rounded and clipped to 0..255."""
    rows, n_in, _ = img.shape
    if n_in == n_out:
        return img
    res = np.empty((rows, n_out, 3), np.int64)
    for xx, (xmin, ks) in enumerate(axis_coeffs(n_in, n_out)):
        acc = np.full((rows, 3), 1 << (BITS - 1), np.int64)
        for x, k in enumerate(ks):
            acc += k * img[:, xmin + x, :]
        res[:, xx, :] = np.clip(acc >> BITS, 0, 255)
    return res


def resize(src, H, W):
    """uint8 [h, w, 3] -> uint8 [H, W, 3] as `Image.fromarray(src).resize((W, H), Image.BILINEAR)`."""
    img = np.asarray(src).astype(np.int64)
    img = _pass(img, W)                                                     # horizontal first
    img = _pass(img.transpose(1, 0, 2), H).transpose(1, 0, 2)               # then vertical, on the uint8-rounded rows
    return np.ascontiguousarray(img).astype(np.uint8)
