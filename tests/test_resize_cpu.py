"""CPU side of the device Resize (csrc/resize.hip, transforms.RaggedImages / DeviceTransform.resize_batch): the arithmetic is
Pillow's, the product's coefficient tables are the restatement's, the ragged pack is laid out as the kernel reads it, and every
bad argument is refused before anything is launched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pil_resample as pr  # noqa: E402

try:
    from PIL import Image
except ImportError:                                     # the golden file then stands in for Pillow
    Image = None


def _golden_cases(golden):
    g = golden("pil_resize")
    return [(n, g[n + "/src"], g[n + "/out"]) for n in sorted({k.split("/")[0] for k in g})]


def _sweep():
    """(n_in, n_out) pairs: the edge sizes, ratios just below / on / above integers, and a seeded random fill."""
    pairs = [(1, 1), (1, 2), (1, 37), (2, 1), (37, 1), (511, 1), (5, 5), (64, 64), (64, 128), (128, 256), (3, 2), (2, 3),
             (511, 21), (16384, 3), (16384, 4096), (1, 4096), (4096, 4095), (4095, 4096)]
    for out in (7, 21, 64):
        for m in (1, 2, 3, 5, 12):
            pairs += [(out * m - 1, out), (out * m, out), (out * m + 1, out), (out, out * m - 1), (out, out * m + 1)]
    rng = np.random.default_rng(11)
    pairs += [(int(a), int(b)) for a, b in zip(rng.integers(1, 900, 160), rng.integers(1, 400, 160))]
    return sorted(set(pairs))


def _restated_table(n_in, n_out):
    ks = pr.ksize(n_in, n_out)
    bounds, coefs = [], []
    for xmin, k in pr.axis_coeffs(n_in, n_out):
        assert len(k) <= ks
        bounds += [xmin, len(k)]
        coefs += k + [0] * (ks - len(k))
    return np.array(bounds + coefs, np.int32)


def test_sweep_is_wide_enough():
    s = _sweep()
    assert len(s) >= 200
    assert any(a == 1 for a, b in s) and any(b == 1 for a, b in s) and any(a == b for a, b in s)


def test_product_tables_equal_the_restatement():
    from centroids_reid_amd.transforms import resample_table
    for n_in, n_out in _sweep():
        tab = resample_table(n_in, n_out)
        assert tab.dtype == np.int32
        if n_in == n_out:                                # the identity table: one tap of weight 1.0 on the sample itself
            want = np.concatenate([np.stack([np.arange(n_out), np.ones(n_out, np.int64)], 1).reshape(-1),
                                   np.tile([1 << 22, 0, 0], n_out)])
            assert np.array_equal(tab, want), (n_in, n_out)
            continue
        assert np.array_equal(tab, _restated_table(n_in, n_out)), (n_in, n_out)
        first, count = tab[:2 * n_out:2], tab[1:2 * n_out:2]
        assert first.min() >= 0 and (first + count).max() <= n_in and count.min() >= 1, (n_in, n_out)   # taps stay inside the image


def test_table_limits():
    from centroids_reid_amd.transforms import resample_table
    for bad in ((0, 4), (4, 0), (16385, 4), (4, 4097)):
        with pytest.raises(ValueError):
            resample_table(*bad)


def test_restatement_equals_pillow_or_its_recording(golden):
    """Against Pillow itself where it imports (one line of pixels per (in, out) pair of the sweep, through both passes), and
    against the recorded Pillow outputs everywhere."""
    for name, src, out in _golden_cases(golden):
        assert np.array_equal(pr.resize(src, out.shape[0], out.shape[1]), out), name
    if Image is None:
        return
    rng = np.random.default_rng(5)
    for n_in, n_out in _sweep():
        if n_in > 2048:
            continue                                      # (the scalar restatement is slow there; the tables above cover them)
        line = rng.integers(0, 256, (2, n_in, 3), dtype=np.uint8)
        line[1, ::2] = 255; line[1, 1::2] = 0
        for src, size in ((line, (n_out, 2)), (np.ascontiguousarray(line.transpose(1, 0, 2)), (2, n_out))):
            want = np.asarray(Image.fromarray(src).resize(size, Image.BILINEAR))
            assert np.array_equal(pr.resize(src, size[1], size[0]), want), (n_in, n_out, size)


def test_golden_file_covers_the_tile_edges(golden):
    cases = _golden_cases(golden)
    targets = {out.shape[:2] for _, _, out in cases}
    assert targets == {(21, 37), (32, 64), (33, 65), (256, 128)}          # inside / exactly / one past the kernel's 32 x 64 tile
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "pil_resize.npz")) < 256 * 1024
    for H, W in ((21, 37), (32, 64), (33, 65)):
        mine = {n.split("_", 1)[1]: s.shape[:2] for n, s, o in cases if o.shape[:2] == (H, W)}
        assert mine["1x1"] == (1, 1) and mine["2x3"] == (2, 3) and mine["identity"] == (H, W)
        assert mine["h_equal"][0] == H and mine["h_equal"][1] != W and mine["w_equal"][1] == W and mine["w_equal"][0] != H
        assert pr.ksize(mine["heavy_w"][1], W) >= 25 and pr.ksize(mine["heavy_h"][0], H) >= 25
        assert {"up", "down23", "stripe_rows", "stripe_cols"} <= set(mine)


def test_ragged_pack_cat_len():
    from centroids_reid_amd.transforms import RaggedImages
    rng = np.random.default_rng(0)
    shapes = [(3, 5), (1, 1), (7, 3), (2, 9)]                              # odd byte counts: 45, 3, 63, 54
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    r = RaggedImages.pack([imgs[0], torch.from_numpy(imgs[1]), imgs[2][:, :, :]])
    assert len(r) == 3 and r.data.dtype == torch.uint8 and r.data.numel() == 45 + 3 + 63
    assert r.offsets.tolist() == [0, 45, 48] and r.offsets.dtype == torch.int64
    assert r.sizes.tolist() == [[3, 5], [1, 1], [7, 3]] and r.sizes.dtype == torch.int32
    flat = r.data.numpy()
    for i, o in enumerate(r.offsets.tolist()):
        assert np.array_equal(flat[o:o + imgs[i].size].reshape(imgs[i].shape), imgs[i])
    r2 = RaggedImages.pack([np.asfortranarray(imgs[3])])                  # a non-contiguous image is packed as HWC all the same
    both = RaggedImages.cat([r, r2])
    assert len(both) == 4 and both.offsets.tolist() == [0, 45, 48, 111] and both.sizes.tolist() == [list(s) for s in shapes]
    assert np.array_equal(both.data.numpy()[111:].reshape(2, 9, 3), imgs[3])
    assert np.array_equal(both.data.numpy()[:111], flat)
    assert RaggedImages.cat([r]) is r
    if Image is not None:
        p = RaggedImages.pack([Image.fromarray(imgs[0]), Image.fromarray(imgs[2][:, :, 0])])     # mode "L" -> RGB
        assert p.sizes.tolist() == [[3, 5], [7, 3]]
        assert np.array_equal(p.data.numpy()[:45].reshape(3, 5, 3), imgs[0])
        assert np.array_equal(p.data.numpy()[45:].reshape(7, 3, 3), np.repeat(imgs[2][:, :, :1], 3, 2))


def test_ragged_pack_refuses_what_is_not_an_image():
    from centroids_reid_amd.transforms import RaggedImages
    for bad in ([], [np.zeros((4, 4, 3), np.float32)], [np.zeros((4, 4), np.uint8)], [np.zeros((4, 4, 4), np.uint8)],
                [np.zeros((0, 4, 3), np.uint8)], [torch.zeros((3, 4, 4), dtype=torch.uint8)], ["a.jpg"]):
        with pytest.raises(ValueError):
            RaggedImages.pack(bad)
    with pytest.raises(ValueError):
        RaggedImages.cat([])
    with pytest.raises(ValueError):
        RaggedImages.cat([np.zeros((4, 4, 3), np.uint8)])


def test_no_cpu_fallback():
    from centroids_reid_amd import _lib as L
    from centroids_reid_amd.transforms import DeviceTransform, RaggedImages
    t = DeviceTransform((8, 8), [0.5] * 3, [0.25] * 3, is_train=False)
    with pytest.raises(ValueError):
        t.resize_batch(torch.zeros((1, 4, 5, 3), dtype=torch.uint8))      # a dense batch is not a pack
    with pytest.raises(L.CreidError):
        t(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))                   # a CPU batch, as before
    if not torch.cuda.is_available():                                     # (with a device a host pack is simply uploaded)
        r = RaggedImages.pack([np.zeros((4, 5, 3), np.uint8)])
        with pytest.raises(L.CreidError):
            t.resize_batch(r)
        with pytest.raises(L.CreidError):
            t(r)


def test_abi_argument_checks_launch_nothing():
    """creid_resize_u8 refuses null pointers, empty or oversized targets and the batch bound of creid_augment_u8 with
    CREID_E_ARG (-1) before it launches: the calls below pass on a machine with no device (the pointers are never followed)."""
    import __graft_entry__ as ge
    ge.build()
    from centroids_reid_amd import _lib as L
    f = L.lib().creid_resize_u8
    buf = (C.c_int64 * 8)()
    p = C.c_void_p(C.addressof(buf))
    good = dict(src=p, src_bytes=64, off=p, size=p, tab=p, tab_len=16, toff=p, B=1, H=8, W=8, out=p)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["src"], a["src_bytes"], a["off"], a["size"], a["tab"], a["tab_len"], a["toff"], a["B"], a["H"], a["W"], a["out"], None)
    for name in ("src", "off", "size", "tab", "toff", "out"):
        assert call(**{name: None}) == -1, name
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(B=-1), dict(H=4097), dict(W=4097), dict(src_bytes=0), dict(tab_len=0),
               dict(B=1 << 31), dict(B=(1 << 40) // (264 * 134) + 1, H=256, W=128)):
        assert call(**kw) == -1, kw
