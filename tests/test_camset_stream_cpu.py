"""CPU: the host side of the camera-set streamed evaluation.  The host StreamPlan(camsets=True) against a brute-force count
written from utils/eval_reid.py:51-55, and the closed form the device centroid index implements (csrc/centroid_index.hip)
against the reference's grouping loop (modelling/bases.py:205-236, kept as bases._camera_centroids_host)."""
import numpy as np
import pytest


def _brute_n_pos(qp, gp, qc, gsets):
    """utils/eval_reid.py:51-55: an entry is removed iff it has the query's pid and the query's camera is in its set; the
    positives are the same-pid entries that are kept."""
    out = np.zeros(len(qp), np.int64)
    for i in range(len(qp)):
        for j in range(len(gp)):
            if gp[j] == qp[i] and qc[i] not in gsets[j]:
                out[i] += 1
    return out


def _masks(gsets):
    return np.array([sum(1 << c for c in s) for s in gsets], np.int64)


@pytest.mark.parametrize("seed,nq,ng,npid,ncam", [(0, 40, 300, 12, 8), (1, 25, 900, 3, 63), (2, 7, 64, 70, 2)])
def test_host_plan_camsets_counts_match_brute_force(seed, nq, ng, npid, ncam):
    from centroids_reid_amd import reid_metric as rm
    rng = np.random.default_rng(seed)
    qp = rng.integers(0, npid + 2, nq)                                   # some query pids have no gallery entry
    gp = rng.integers(0, npid, ng)
    qc = rng.integers(0, ncam, nq)
    gsets = [sorted(set(rng.integers(0, ncam, rng.integers(1, 5)).tolist())) for _ in range(ng)]
    plan = rm.StreamPlan(qp, gp, qc, _masks(gsets), "cpu", camsets=True)
    want = _brute_n_pos(qp, gp, qc, gsets)
    np.testing.assert_array_equal(plan.n_pos, want)
    np.testing.assert_array_equal(plan.overflow, np.nonzero(want > 128)[0])
    small = want[want <= 128]
    cap = 2
    while cap < max(int(small.max(initial=1)), 1):
        cap *= 2
    assert plan.cap == cap
    if seed == 1:
        assert len(plan.overflow) > 0 and (want == 0).any()              # the case has general-path rows and empty lists
    # the plain form on the same labels counts something else (cameras as ids, not as sets): the keyword matters
    plain = rm.StreamPlan(qp, gp, qc, _masks(gsets), "cpu")
    assert plain.camsets is False and plan.camsets is True
    assert (plain.n_pos != plan.n_pos).any()


def test_host_plan_camsets_refuses_query_cameras_outside_0_62():
    from centroids_reid_amd import _lib as L
    from centroids_reid_amd import reid_metric as rm
    for bad in (63, -1):
        with pytest.raises(L.CreidError, match="0..62"):
            rm.StreamPlan([0, 1], [0, 1, 1], [0, bad], [1, 2, 4], "cpu", camsets=True)


def _closed_form(pids, camids, nq):
    """Section "Semantics" of the device index, in numpy: (order, offsets, labels, masks)."""
    pids, camids = np.asarray(pids), np.asarray(camids)
    lq, lg = pids[:nq], pids[nq:]
    ng = len(lg)
    cam_g = camids[:ng]                                                  # the :214 quirk: gallery-relative index, full vector
    cam_q = camids[:nq]
    order, offsets, labels, masks = [], [0], [], []
    for u in np.unique(lg):
        rows = np.nonzero(lg == u)[0]                                    # ascending gallery index
        gmask = 0
        for c in cam_g[rows]:
            gmask |= 1 << int(c)
        qmask = 0
        for c in cam_q[lq == u]:
            qmask |= 1 << int(c)
        collapsed = False
        for cur in range(63):
            if not (qmask >> cur) & 1:
                continue
            if (gmask >> cur) & 1:
                used = gmask & ~(1 << cur)
                if used == 0:
                    continue
                members = rows[cam_g[rows] != cur]
            else:
                if collapsed:
                    continue
                collapsed = True
                used, members = gmask, rows
            order.extend((members + nq).tolist()); offsets.append(len(order)); labels.append(int(u)); masks.append(used)
    return (np.asarray(order, np.int64), np.asarray(offsets, np.int64), np.asarray(labels, np.int64),
            np.asarray(masks, np.int64))


def _host_loop_arrays(pids, camids, nq):
    from centroids_reid_amd.bases import _camera_centroids_host
    groups, labels, cams = _camera_centroids_host(pids, camids, nq)
    order = np.concatenate(groups).astype(np.int64) + nq if groups else np.zeros(0, np.int64)
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    return order, offsets, np.asarray(labels, np.int64), _masks(cams)


def test_closed_form_equals_reference_grouping_loop():
    rng = np.random.default_rng(2024)
    total = 0
    for t in range(300):
        nq = int(rng.integers(1, 40))
        ng = int(rng.integers(1, 120))
        npid = int(rng.integers(1, 12))
        ncam = int(rng.integers(1, 7))
        pids = rng.integers(0, npid, nq + ng) * 3 + 5
        camids = rng.integers(0, ncam, nq + ng)
        if t % 5 == 0:
            camids[rng.integers(0, nq + ng, 3)] = 62
        got = _closed_form(pids, camids, nq)
        want = _host_loop_arrays(pids, camids, nq)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
        total += len(got[2])
    assert total > 2000                                                  # centroids compared


def test_mask_camera_lists_round_trip():
    from centroids_reid_amd.bases import _mask_camera_lists
    sets = [[0], [62], [0, 5, 62], [1, 2, 3], list(range(63))]
    out = _mask_camera_lists(_masks(sets))
    assert out == sets and all(type(c) is int for s in out for c in s)
    assert _mask_camera_lists(np.zeros(0, np.int64)) == []
