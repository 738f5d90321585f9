"""Host side of the ranked lists under the evaluation protocol: the refusals that need no device, JunkFilter.from_labels on
every label form R1_mAP.compute accepts, and the numpy reference of tests/ranked_ref.py against a literal per-query loop."""
import numpy as np
import pytest
import torch

import ranked_ref as R


def _rm():
    from centroids_reid_amd import reid_metric as rm
    return rm


@pytest.mark.parametrize("bad", [0, -1, 1025, 10.0, "10", True, [10]])
def test_ranked_topk_is_an_int_from_1_to_1024(bad):
    rm = _rm()
    from centroids_reid_amd._lib import CreidError
    with pytest.raises(CreidError, match="ranked_topk"):
        rm.R1_mAP(num_query=4, ranked_topk=bad)
    for streamed in (False, True):
        with pytest.raises(CreidError, match="ranked_topk"):
            rm.R1_mAP(num_query=4, streamed=streamed, ranked_topk=bad)


def test_ranked_topk_accepted_values():
    rm = _rm()
    assert rm.R1_mAP(num_query=4).ranked_topk is None
    for ok in (1, 10, 1024, np.int64(7)):
        m = rm.R1_mAP(num_query=4, streamed=True, prefilter=torch.bfloat16, ranked_topk=ok)      # allowed with prefilter=
        assert m.ranked_topk == int(ok) and isinstance(m.ranked_topk, int)


def test_topk_stream_refuses_junk_with_prefilter():
    """Decided before anything touches a device: CPU tensors get this far."""
    rm = _rm()
    from centroids_reid_amd._lib import CreidError
    q, g = torch.zeros((2, 8)), torch.zeros((5, 8))
    junk = rm.JunkFilter([0, 1], [0, 0], [0, 1, 2, 3, 4], [0, 0, 1, 1, 2])
    with pytest.raises(CreidError, match="prefilter"):
        rm.topk_stream(q, g, 2, junk=junk, prefilter=torch.bfloat16)
    with pytest.raises(CreidError, match="JunkFilter"):
        rm.topk_stream(q, g, 2, junk=(0, 1))


def test_junk_filter_from_labels_forms():
    rm = _rm()
    from centroids_reid_amd._lib import CreidError
    nq = 3
    pids = [5, 6, 7, 5, 5, 6, 9]
    cams = [0, 1, 2, 0, 1, 1, 2]
    want = dict(q_pids=[5, 6, 7], q_cams=[0, 1, 2], g_pids=[5, 5, 6, 9], g_cams=[0, 1, 1, 2])
    for p, c in ((pids, cams), (np.asarray(pids), np.asarray(cams, np.int32)), (torch.tensor(pids), torch.tensor(cams))):
        j = rm.JunkFilter.from_labels(p, c, nq, "cpu")
        assert not j.camsets
        for key, v in want.items():
            t = getattr(j, key)
            assert t.dtype == torch.int64 and t.device.type == "cpu" and t.tolist() == v
    # camera sets: a list of camera lists, and the carrier that already holds masks and query cameras
    lists = [[0], [1], [2], [0, 3], [1], [1, 2, 62], [5]]
    masks = [0b1001, 0b10, (1 << 62) | 0b110, 1 << 5]
    j = rm.JunkFilter.from_labels(np.asarray(pids), lists, nq, "cpu", respect_camids=True)
    assert j.camsets and j.q_cams.tolist() == [0, 1, 2] and j.g_cams.tolist() == masks and j.g_pids.tolist() == [5, 5, 6, 9]

    class NoWalk(rm.CameraSets):
        def __getitem__(self, i):
            raise AssertionError("the lists of a CameraSets are not walked")

        def __iter__(self):
            raise AssertionError("the lists of a CameraSets are not walked")
    carrier = NoWalk(lists, torch.tensor(masks), np.asarray([0, 1, 2]))
    j2 = rm.JunkFilter.from_labels(pids, carrier, nq, "cpu", respect_camids=True)
    assert j2.camsets and j2.q_cams.tolist() == [0, 1, 2] and j2.g_cams.tolist() == masks
    with pytest.raises(CreidError, match="0..62"):
        rm.JunkFilter.from_labels(pids, [[0], [1], [2], [63], [1], [1], [5]], nq, "cpu", respect_camids=True)
    with pytest.raises(CreidError, match="0..62"):
        rm.JunkFilter.from_labels(pids, [[0], [63], [2], [3], [1], [1], [5]], nq, "cpu", respect_camids=True)
    with pytest.raises(CreidError, match="one pid and one camera"):
        rm.JunkFilter([0, 1], [0], [0, 1], [0, 1])
    # the helpers the device routes use
    sub = j.rows(slice(1, 3))
    assert sub.q_pids.tolist() == [6, 7] and sub.g_cams.tolist() == masks and sub.camsets
    sub = j.rows(torch.tensor([2, 0]))
    assert sub.q_cams.tolist() == [2, 0]
    assert j.gallery_slice(2, 2).g_pids.tolist() == [5, 6]
    assert j.matched(torch.tensor([[0, 2, -1], [2, -1, -1], [3, 0, 1]])).tolist() == [[True, False, False], [True, False, False],
                                                                                  [False, False, False]]


def _literal(dist, q_pids, q_cams, g_pids, g_cams, k, camsets):
    """utils/visrank.py:193-232 as written: walk the ranked row, skip invalid entries, stop after k."""
    m, n = dist.shape
    out = []
    for i in range(m):
        order = sorted(range(n), key=lambda j: (dist[i, j], j))
        row = []
        for j in order:
            if camsets:
                invalid = g_pids[j] == q_pids[i] and (g_cams[j] >> q_cams[i]) & 1
            else:
                invalid = g_pids[j] == q_pids[i] and g_cams[j] == q_cams[i]
            if not invalid:
                row.append((j, dist[i, j], g_pids[j] == q_pids[i]))
                if len(row) == k:
                    break
        out.append(row)
    return out


@pytest.mark.parametrize("camsets", [False, True], ids=["ids", "camsets"])
def test_ranked_ref_against_a_literal_loop(camsets):
    """6 x 20, hand-made: query 0 has junk at its ranks 1 and 2, query 1 ties (ordered by index) with the junk one in the
    middle, query 2 has no gallery entry of its pid, query 3 has only 7 non-junk entries (two of them matches), queries 4 and 5
    are plain."""
    n = 20
    dist = np.tile(np.arange(n, dtype=np.float32), (6, 1))
    dist[0] = dist[0][::-1]                                             # nearest: 19, 18, 17, ...
    dist[1, 4:9] = 2.5                                                  # five-way tie: 4 5 6 7 8
    g_pids = np.arange(100, 100 + n)
    g_cams = np.zeros(n, np.int64) if not camsets else np.full(n, 0b100, np.int64)       # camera 0 / the set {2}
    q_pids = np.array([1, 2, 3, 4, 5, 6])
    q_cams = np.array([1, 1, 1, 1, 1, 1])
    junk_cam = 1 if not camsets else 0b1010                              # camera 1 / the set {1, 3}
    g_pids[[19, 18, 10]] = 1; g_cams[[19, 18]] = junk_cam               # query 0: 19, 18 junk; 10 a kept match
    g_pids[6] = 2; g_cams[6] = junk_cam                                 # query 1: the middle of the tie is junk
    g_pids[[0, 1, 2, 3, 5, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17]] = 4    # query 3: all of its pid ...
    g_cams[[0, 1, 2, 3, 5, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17]] = junk_cam
    g_cams[[3, 9]] = g_cams[4]                                          # ... but 3 and 9 are kept matches
    k = 8
    idx, dsel, matched, count = R.ranked_ref(dist, q_pids, q_cams, g_pids, g_cams, k, camsets)
    lit = _literal(dist, q_pids, q_cams, g_pids, g_cams, k, camsets)
    for i, row in enumerate(lit):
        c = len(row)
        assert count[i] == c
        assert idx[i, :c].tolist() == [j for j, _, _ in row] and (idx[i, c:] == -1).all()
        assert dsel[i, :c].tolist() == [d for _, d, _ in row] and np.isinf(dsel[i, c:]).all()
        assert matched[i, :c].tolist() == [bool(mt) for _, _, mt in row] and not matched[i, c:].any()
    assert idx[0].tolist() == [17, 16, 15, 14, 13, 12, 11, 10] and matched[0].tolist() == [False] * 7 + [True]
    assert idx[1].tolist() == [0, 1, 2, 4, 5, 7, 8, 3]                  # ties by index, 6 dropped
    assert idx[2].tolist() == list(range(8)) and not matched[2].any()
    assert count.tolist() == [8, 8, 8, 7, 8, 8]
    assert idx[3].tolist() == [3, 4, 6, 9, 10, 18, 19, -1] and matched[3].tolist() == [True, False, False, True] + [False] * 4
    assert dsel.dtype == np.float32 and idx.dtype == np.int64 and matched.dtype == bool and count.dtype == np.int32


def test_generator_plants_junk_at_rank_one():
    """make_case: the labels follow the recipe, and every even query that has junk sits next to its first junk row."""
    for camsets in (False, True):
        q, g, qp, qc, gp, gc = R.make_case(33, 300, 8, False, camsets)
        assert gp.min() >= 0 and gp.max() < 25 and qp.max() < 25 + 6 + 1 and (qp >= 25).any()
        assert qc.max() < 6 and (gc.min() >= 1 and gc.max() < 64 if camsets else gc.max() < 6)
        jm = R.junk_matrix(qp, qc, gp, gc, camsets)
        plant = R.planted(qp, qc, gp, gc, camsets)
        assert len(plant) == 11 and (plant % 2 == 0).all()
        d = ((q[:, None, :].astype(np.float64) - g[None].astype(np.float64)) ** 2).sum(-1)
        for i in plant:
            assert jm[i, d[i].argmin()]
