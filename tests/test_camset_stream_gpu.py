"""GPU: the camera-aware centroid validation on the device.  The centroid index (csrc/centroid_index.hip) against the reference's
grouping loop array for array, and the camera-set streamed evaluation (creid_stream_plan_camsets + creid_stream_poslist*_camsets
+ the unchanged count / finalize) against the materialised camera-set evaluation of the same dtype."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _holder(nq):
    from centroids_reid_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.MODEL.USE_CENTROIDS = True
    cfg.MODEL.KEEP_CAMID_CENTROIDS = True
    cfg.num_query = nq
    return SimpleNamespace(hparams=cfg, trainer=SimpleNamespace(logger=None, current_epoch=0))


# ------------------------------------------------------------------ the centroid index
def _index_labels():
    """nq = 60, ng = 3000, pids 3 k + 5.  The camera of gallery row j is camids[j] (modelling/bases.py:214), so the cameras of
    the special pids are set at full-vector index j = gallery row, and the special rows lie at j >= nq, clear of the queries'."""
    rng = np.random.default_rng(5)
    nq, ng = 60, 3000
    pid = lambda k: 3 * k + 5
    pids = pid(rng.integers(0, 40, nq + ng))
    camids = rng.integers(0, 6, nq + ng)
    free = rng.permutation(np.arange(nq, ng))                            # gallery rows (= camera slots) the cases may take
    taken = [0]

    def rows(count):
        r = np.sort(free[taken[0]:taken[0] + count]); taken[0] += count
        return r

    def gallery(k, count, cams):
        r = rows(count)
        pids[nq + r] = pid(k)
        camids[r] = cams if np.ndim(cams) else np.full(count, cams)
        return r

    def query(i, k, cam):
        pids[i], camids[i] = pid(k), cam

    gallery(40, 9, rng.integers(0, 4, 9))                                # a gallery pid with no query
    query(0, 41, 2)                                                      # a query pid with no gallery row (inside the range)
    query(1, 200, 1); pids[2] = 2                                        # ... above and below the gallery's range
    gallery(42, 11, 3); query(3, 42, 3)                                  # every row on the query's camera: nothing emitted
    gallery(43, 14, rng.integers(0, 2, 14)); query(4, 43, 7); query(5, 43, 9); query(6, 43, 0)   # cameras 7, 9 collapse
    gallery(44, 12, np.array([0, 62, 5] * 4)); query(7, 44, 0); query(8, 44, 62)                  # cameras 0 and 62
    gallery(45, 70, rng.integers(0, 5, 70)); query(9, 45, 1); query(10, 45, 9)                    # beyond one wave
    gallery(46, 1100, rng.integers(0, 6, 1100)); query(11, 46, 0); query(12, 46, 3); query(13, 46, 40)   # beyond 1024
    return pids, camids, nq, ng


def _host_arrays(pids, camids, nq):
    from centroids_reid_amd.bases import _camera_centroids_host
    groups, labels, cams = _camera_centroids_host(pids, camids, nq)
    order = np.concatenate(groups).astype(np.int64) + nq
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    masks = np.array([sum(1 << int(c) for c in s) for s in cams], np.int64)
    return order, offsets, np.asarray(labels, np.int64), masks, cams


def test_device_centroid_index_equals_host_loop(monkeypatch):
    from centroids_reid_amd import bases
    pids, camids, nq, ng = _index_labels()
    order, offsets, labels, masks, cam_lists = _host_arrays(pids, camids, nq)
    # the label set holds every case it is meant to hold
    lens = np.diff(offsets)
    assert not (labels == 3 * 40 + 5).any() and not (labels == 3 * 42 + 5).any()
    assert (labels == 3 * 43 + 5).sum() == 2 and (labels == 3 * 44 + 5).sum() == 2
    assert (masks[labels == 3 * 44 + 5] >> 62).any() and (masks & 1).any()
    assert lens[labels == 3 * 45 + 5].max() == 70 and lens[labels == 3 * 46 + 5].max() == 1100
    assert (lens[labels == 3 * 46 + 5] > 64).all() and (labels == 3 * 46 + 5).sum() == 3

    runs = [bases.camera_centroid_index(pids, camids, nq, "cuda") for _ in range(2)]
    assert runs[0] is not None
    for got in runs:
        for g, want in zip(got, (order, offsets, labels, masks)):
            assert g.dtype == torch.int64 and g.is_cuda
            np.testing.assert_array_equal(g.cpu().numpy(), want)

    # the centroids: the device index against the host loop through the same public call, bit for bit
    rng = np.random.default_rng(6)
    emb = torch.from_numpy(rng.standard_normal((nq + ng, 64)).astype(np.float32)).cuda()
    h = _holder(nq)
    e_dev, l_dev, c_dev = bases.ModelBase.validation_create_centroids(h, emb, pids, camids, respect_camids=True)
    monkeypatch.setattr(bases, "camera_centroid_index", lambda *a, **k: None)
    e_host, l_host, c_host = bases.ModelBase.validation_create_centroids(h, emb, pids, camids, respect_camids=True)
    assert torch.equal(e_dev, e_host)
    np.testing.assert_array_equal(l_dev, l_host)
    assert l_dev.dtype == l_host.dtype
    assert isinstance(c_dev, list) and list(c_dev) == c_host and c_host[nq:] == cam_lists
    assert all(type(c) is int for s in c_dev[nq:] for c in s)
    np.testing.assert_array_equal(c_dev.masks.cpu().numpy(), masks)
    np.testing.assert_array_equal(c_dev.q_cams, camids[:nq])


def test_centroid_index_leaves_other_label_sets_to_the_host_loop():
    from centroids_reid_amd import bases
    rng = np.random.default_rng(8)
    nq, ng = 10, 90
    pids = rng.integers(0, 7, nq + ng); camids = rng.integers(0, 4, nq + ng)
    far = pids.copy(); far[nq] += 1 << 40
    assert bases.camera_centroid_index(far, camids, nq, "cuda") is None          # range beyond the dense counting sort
    for bad in (63, -1):
        c = camids.copy(); c[ng - 1] = bad
        assert bases.camera_centroid_index(pids, c, nq, "cuda") is None          # a camera a 63-bit mask cannot hold
    c = camids.copy(); c[ng:] = 99                                               # never read as a camera (:214): taken
    assert bases.camera_centroid_index(pids, c, nq, "cuda") is not None
    emb = torch.from_numpy(rng.standard_normal((nq + ng, 32)).astype(np.float32)).cuda()
    c = camids.copy(); c[0] = 70
    e, l, cams = bases.ModelBase.validation_create_centroids(_holder(nq), emb, pids, c, respect_camids=True)
    assert not hasattr(cams, "masks") and e.shape[0] == len(l) == len(cams)      # as before this index existed


# ------------------------------------------------------------------ recorded golden, streamed
def test_val_centroids_camera_sets_golden_streamed(golden):
    from centroids_reid_amd.bases import ModelBase
    from centroids_reid_amd.reid_metric import CameraSets, R1_mAP
    g = golden("eval_camsets")
    nq = int(g["num_query"])
    emb, labels, camsets = ModelBase.validation_create_centroids(
        _holder(nq), torch.from_numpy(g["feats"]).cuda(), g["pids"], g["camids"], respect_camids=True)
    assert isinstance(camsets, CameraSets)
    metric = R1_mAP(num_query=nq, streamed=True)
    cmc, mAP, topk = metric.compute(emb, labels, camsets, respect_camids=True)
    assert "distmat" not in metric.last and "indices" not in metric.last
    assert metric.last["plan"].camsets
    assert abs(mAP - float(g["mAP"])) < 1e-12
    np.testing.assert_allclose(cmc, g["cmc"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(topk, g["topk"], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(metric.last["single_performance"][:, 0], g["single"][:, 0])
    np.testing.assert_allclose(metric.last["single_performance"][:, 2], g["single"][:, 2], rtol=0, atol=1e-12)
    # the same lists without the carrier (masks rebuilt on the host and uploaded): the same numbers
    cmc2, mAP2, topk2 = R1_mAP(num_query=nq, streamed=True).compute(emb, labels, list(camsets), respect_camids=True)
    assert mAP2 == mAP
    np.testing.assert_array_equal(cmc2, cmc)


# ------------------------------------------------------------------ a generic camera-set gallery
_CASE = {}


def _generic_case(D):
    """nq = 130, ng = 1999, 38 pids, sets of 1-4 of 8 cameras; small-integer features (exact in every dtype: ties are real and
    resolve by gallery index).  Query 0: every same-pid entry removed; query 1: 150 positives (general path); query 2: 128."""
    if D in _CASE:
        return _CASE[D]
    rng = np.random.default_rng(31 + D)
    nq, ng = 130, 1999
    qp = rng.integers(0, 37, nq); gp = rng.integers(0, 35, ng)
    qc = rng.integers(0, 8, nq)
    gsets = [sorted(set(rng.integers(0, 8, rng.integers(1, 5)).tolist())) for _ in range(ng)]
    spot = rng.permutation(ng)
    a, b, c, d = spot[:30], spot[30:180], spot[180:308], spot[308:330]
    qp[0], qc[0] = 35, 5
    for j in a:                                                          # pid 35: camera 5 in every set
        gp[j] = 35; gsets[j] = sorted(set(gsets[j]) | {5})
    qp[1], qc[1] = 36, 7
    for j in b:                                                          # pid 36: 150 entries without camera 7
        gp[j] = 36; gsets[j] = sorted(set(gsets[j]) - {7}) or [0]
    qp[2], qc[2] = 37, 6
    for j in c:                                                          # pid 37: 128 entries without camera 6 ...
        gp[j] = 37; gsets[j] = sorted(set(gsets[j]) - {6}) or [1]
    for j in d:                                                          # ... and 22 with it
        gp[j] = 37; gsets[j] = sorted(set(gsets[j]) | {6})
    f = rng.integers(-3, 4, (nq + ng, D)).astype(np.float32)
    f[nq + b[:40]] = f[1]                                                # ties at distance 0, among positives and beyond
    f[nq + spot[400:440]] = f[1]
    f[nq + c[:10]] = f[nq + c[10:20]]
    pids = np.concatenate([qp, gp])
    camsets = [[int(x)] for x in qc] + gsets
    _CASE[D] = (torch.from_numpy(f), pids, camsets, nq)
    return _CASE[D]


def _materialised(f, pids, camsets, nq, dtype):
    from centroids_reid_amd import reid_metric as rm
    mat = rm.R1_mAP(num_query=nq, feat_norm=False, compute_dtype=dtype)
    cmc, mAP, topk = mat.compute(f, pids, camsets, respect_camids=True)
    assert "distmat" in mat.last
    _, _, _, _, valid, ap, first = rm.eval_func_device(mat.last["indices"], pids[:nq], pids[nq:], camsets[:nq], camsets[nq:],
                                                       camsets=True)
    return (cmc, mAP, topk), valid.cpu().numpy(), ap.cpu().numpy(), first.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "f16"])
@pytest.mark.parametrize("D", [64, 40])
def test_streamed_camsets_equal_materialised(D, dtype):
    from centroids_reid_amd import reid_metric as rm
    f, pids, camsets, nq = _generic_case(D)
    f = f.cuda()
    (cmc_m, mAP_m, topk_m), valid_m, ap_m, first_m = _materialised(f, pids, camsets, nq, dtype)
    st = rm.R1_mAP(num_query=nq, feat_norm=False, compute_dtype=dtype, streamed=True)
    cmc, mAP, topk = st.compute(f, pids, camsets, respect_camids=True)
    assert "distmat" not in st.last
    plan = st.last["plan"]
    assert plan.camsets and plan.n_pos[0] == 0 and plan.n_pos[1] == 150 and plan.n_pos[2] == 128
    assert 1 in plan.overflow and 2 not in plan.overflow and plan.cap == 128
    valid, ap, first = (st.last[k].cpu().numpy() for k in ("valid", "ap", "first"))
    assert valid[0] == 0 and valid[1] == 1 and valid[2] == 1
    np.testing.assert_array_equal(valid, valid_m)
    ok = valid_m == 1
    np.testing.assert_array_equal(first[ok], first_m[ok])
    np.testing.assert_allclose(ap[ok], ap_m[ok], rtol=0, atol=1e-12)
    assert abs(mAP - mAP_m) < 1e-12
    np.testing.assert_array_equal(cmc, cmc_m)
    np.testing.assert_allclose(topk, topk_m, rtol=0, atol=1e-12)
    # a second evaluation of the shape speculates on the first one's capacity and must agree with it
    cmc2, mAP2, _ = st.compute(f, pids, camsets, respect_camids=True)
    assert mAP2 == mAP
    np.testing.assert_array_equal(cmc2, cmc)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "f16"])
def test_compute_chunked_camsets_equals_compute(dtype):
    from centroids_reid_amd import _lib as L
    from centroids_reid_amd import reid_metric as rm
    f, pids, camsets, nq = _generic_case(64)
    f = f.cuda()
    a = rm.R1_mAP(num_query=nq, feat_norm=False, compute_dtype=dtype, streamed=True)
    cmc, mAP, topk = a.compute(f, pids, camsets, respect_camids=True)
    b = rm.R1_mAP(num_query=nq, feat_norm=False, compute_dtype=dtype)
    cmc2, mAP2, topk2 = b.compute_chunked(f, pids, camsets, respect_camids=True)
    assert mAP2 == mAP and "distmat" not in b.last
    np.testing.assert_array_equal(cmc2, cmc)
    np.testing.assert_array_equal(topk2, topk)
    for k in ("valid", "ap", "first"):
        assert torch.equal(a.last[k], b.last[k])
    with pytest.raises(L.CreidError, match="respect_camids"):
        rm.R1_mAP(num_query=nq, dist_func="cosine").compute_chunked(f, pids, camsets, respect_camids=True)


@pytest.mark.parametrize("offset", [0, -977, 10_000_000])
def test_device_plan_camsets_equals_host_plan(offset):
    from centroids_reid_amd import reid_metric as rm
    _, pids, camsets, nq = _generic_case(64)
    pids = pids + offset
    pids[3] = pids[nq:].max() + 3                                        # above the gallery's range
    pids[4] = pids[nq:].min() - 2                                        # below it
    ng = len(pids) - nq
    qc, masks = rm._camset_split(camsets, nq)
    cams = np.concatenate([qc, masks])
    dev = rm.StreamPlan.on_device(pids, cams, nq, "cuda", camsets=True).finish()
    dev2 = rm.StreamPlan.on_device(pids, qc, nq, "cuda", camsets=True, g_cam_masks=torch.from_numpy(masks).cuda()).finish()
    host = rm.StreamPlan(pids[:nq], pids[nq:], qc, masks, "cuda", camsets=True)
    hs = host.q_slot.cpu().numpy()
    hc, ho = host.csr_off.cpu().numpy(), host.g_order.cpu().numpy()
    for d in (dev, dev2):
        assert d.camsets and d.cap == host.cap
        np.testing.assert_array_equal(d.overflow, host.overflow)
        np.testing.assert_array_equal(d.n_pos, host.n_pos)
        ds = d.q_slot[:nq].cpu().numpy()
        np.testing.assert_array_equal(ds < 0, hs < 0)
        dc, do = d.csr_off.cpu().numpy(), d.g_order.cpu().numpy()
        assert sorted(do.tolist()) == list(range(ng))
        for qi in range(nq):
            if hs[qi] < 0:
                continue
            x = np.sort(do[dc[ds[qi]]:dc[ds[qi] + 1]]); y = np.sort(ho[hc[hs[qi]]:hc[hs[qi] + 1]])
            np.testing.assert_array_equal(x, y)
    assert (host.n_pos > 128).any() and (host.n_pos == 128).any() and (hs < 0).sum() >= 2


def test_streamed_camsets_refuse_cameras_outside_0_62():
    from centroids_reid_amd import _lib as L
    from centroids_reid_amd import reid_metric as rm
    f = torch.zeros(5, 8).cuda()
    st = rm.R1_mAP(num_query=2, streamed=True)
    with pytest.raises(L.CreidError, match="0..62"):
        st.compute(f, [0, 1, 0, 1, 2], [[63], [0], [0], [1], [2]], respect_camids=True)
    with pytest.raises(L.CreidError, match="0..62"):
        st.compute(f, [0, 1, 0, 1, 2], [[0], [1], [0], [1, 63], [2]], respect_camids=True)
