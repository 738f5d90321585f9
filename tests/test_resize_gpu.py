"""GPU: the device Resize (creid_resize_u8, csrc/resize.hip) EQUALS Pillow -- every byte of every recorded case
(tests/golden/pil_resize.npz, written by tools/gen_resize_golden.py from Pillow alone) -- wherever an image sits in a ragged
batch, and a ragged batch goes through the augment pass and through run_inference with the bits of the pre-resized batch."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pil_resample as pr  # noqa: E402

pytestmark = pytest.mark.gpu
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
_CACHE = {}


def _cases(golden):
    """{(H, W): [(name, src, pillow_out)]}, loaded once."""
    if "cases" not in _CACHE:
        g = golden("pil_resize")
        by = {}
        for n in sorted({k.split("/")[0] for k in g}):
            out = g[n + "/out"]
            by.setdefault(out.shape[:2], []).append((n, g[n + "/src"], out))
        _CACHE["cases"] = by
    return _CACHE["cases"]


def _transform(size, is_train=False, **kw):
    from centroids_reid_amd.transforms import DeviceTransform
    return DeviceTransform(size, MEAN, STD, is_train=is_train, **kw)


@pytest.mark.parametrize("size", [(21, 37), (32, 64), (33, 65)])
def test_small_cases_equal_pillow_as_one_ragged_batch(golden, size):
    from centroids_reid_amd.transforms import RaggedImages
    cases = _cases(golden)[size]
    assert len(cases) == 11
    r = RaggedImages.pack([src for _, src, _ in cases])
    assert any(o % 2 for o in r.offsets.tolist()) and len({s.shape[:2] for _, s, _ in cases}) == len(cases)   # odd offsets, all sizes differ
    got = _transform(size).resize_batch(r.to("cuda"))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(cases), *size, 3) and got.is_cuda
    got = got.cpu().numpy()
    for i, (name, _, want) in enumerate(cases):
        assert np.array_equal(got[i], want), (name, int((got[i] != want).sum()))


def test_production_case_equals_pillow(golden):
    from centroids_reid_amd.transforms import RaggedImages
    (name, src, want), = _cases(golden)[(256, 128)]
    assert src.shape == (128, 64, 3)
    got = _transform((256, 128)).resize_batch(RaggedImages.pack([src] * 3)).cpu().numpy()     # a host pack is uploaded by the call
    for b in range(3):
        assert np.array_equal(got[b], want), b


def test_batch_position_does_not_matter(golden):
    """The same image first, second and last in a batch, between images of other sizes: a wrong byte offset or table index shows."""
    from centroids_reid_amd.transforms import RaggedImages
    cases = {n.split("_", 1)[1]: (s, o) for n, s, o in _cases(golden)[(33, 65)]}
    probe, want = cases["down23"]
    others = [cases[k][0] for k in ("2x3", "up", "heavy_w", "stripe_cols", "identity")]
    batch = [probe, probe, others[0], others[1], others[2], others[3], others[4], probe]
    got = _transform((33, 65)).resize_batch(RaggedImages.pack(batch).cuda()).cpu().numpy()
    for pos in (0, 1, len(batch) - 1):
        assert np.array_equal(got[pos], want), pos
    assert np.array_equal(got[6], cases["identity"][1])


@pytest.mark.parametrize("size", [(21, 37), (33, 65)])
def test_ragged_batch_through_the_augment_equals_the_resized_batch(golden, size):
    from centroids_reid_amd.transforms import RaggedImages
    cases = _cases(golden)[size]
    B = len(cases)
    t = _transform(size, is_train=True, padding=3)
    params = t.draw(B, rnd=random.Random(2), generator=torch.Generator().manual_seed(3))
    assert params[:, 0].any() and params[:, 3].any()                      # some flips, some erased blocks
    ragged = RaggedImages.pack([s for _, s, _ in cases]).to("cuda")
    dense = torch.from_numpy(np.stack([o for _, _, o in cases])).cuda()
    assert torch.equal(t(ragged, params), t(dense, params))
    for dt in (torch.float32, torch.bfloat16):
        a, b = t(ragged, params, layout="stem", dtype=dt), t(dense, params, layout="stem", dtype=dt)
        assert a.xpad.dtype == dt and a.shape == b.shape and torch.equal(a.xpad, b.xpad), dt
    te = _transform(size)
    assert torch.equal(te(ragged), te(dense))


def test_run_inference_on_ragged_batches_equals_the_resized_batches():
    """Loader batches of un-resized images (a RaggedImages, a plain list of arrays) embed to the bits of the same images resized
    beforehand (the restatement is Pillow, tests/test_resize_cpu.py), and two ragged loader batches share ONE forward."""
    from centroids_reid_amd import inference as inf
    from centroids_reid_amd.bench_train import make_model
    from centroids_reid_amd.transforms import RaggedImages
    torch.manual_seed(3)
    model = make_model(num_classes=16, dtype=torch.bfloat16).eval()
    rng = np.random.default_rng(9)
    shapes = [(128, 64), (97, 45), (301, 133), (64, 32), (128, 51), (203, 64), (33, 77)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    dense = torch.from_numpy(np.stack([pr.resize(im, 128, 64) for im in imgs]))
    names = [f"img_{i}.jpg" for i in range(len(imgs))]
    t = _transform((128, 64))
    calls = []
    hook = model.backbone.register_forward_hook(lambda *a: calls.append(1))
    try:
        e_dense, p_dense = inf.run_inference(model, [(dense[:4], None, names[:4]), (dense[4:], None, names[4:])], transform=t)
        assert len(calls) == 1
        ragged_loader = [(RaggedImages.pack(imgs[:4]), None, names[:4]), (imgs[4:], None, names[4:])]
        del calls[:]
        e_ragged, p_ragged = inf.run_inference(model, ragged_loader, transform=t)
        assert len(calls) == 1                                            # macro-batched: RaggedImages.cat, one forward
        del calls[:]
        e_each, _ = inf.run_inference(model, ragged_loader, transform=t, macro_batch=0)
        assert len(calls) == 2
        del calls[:]
        e_mixed, p_mixed = inf.run_inference(model, [ragged_loader[0], (dense[4:], None, names[4:])], transform=t)
        assert len(calls) == 2                                            # a ragged batch, then a dense one: flushed apart
    finally:
        hook.remove()
    assert list(p_ragged) == names == list(p_dense) == list(p_mixed)
    assert e_dense.shape == (7, 2048) and np.isfinite(e_dense).all() and np.abs(e_dense).max() > 0
    for e in (e_ragged, e_each, e_mixed):
        assert np.array_equal(e.view(np.uint32), e_dense.view(np.uint32))
