"""Numpy reference and generators for the ranked lists under the evaluation protocol (tests/test_ranked_lists_*.py), written
from the definition: gallery entry j is JUNK for query i when g_pids[j] == q_pids[i] and the camera test holds -- plain camera
ids: g_cams[j] == q_cams[i]; camera sets: bit q_cams[i] of the mask g_cams[j] is set.  The ranked list of a query is the first
k non-junk entries of the STABLE ranking of its distances (ties by gallery index), padded with index -1, distance +inf and
matched False; count says how many entries are real; matched = the entry has the query's pid."""
import numpy as np

SHAPES = [(300, 3000, 256, 20, 256, True), (70, 513, 100, 50, 128, False), (129, 1000, 2048, 7, 64, True),
          (33, 300, 8, 5, 32, False), (65, 4097, 64, 100, 512, False), (5, 40, 32, 40, 40, False)]      # nq, ng, D, k, sample, dup


def make_features(nq, ng, D, dup, seed=None):
    """The generator of tests/test_stream_topk_gpu.py, restated: N(0,1) queries and gallery; dup: a quarter of the gallery rows
    copied over others (exact ties, ordered by gallery index)."""
    rng = np.random.default_rng(nq * 7 + ng if seed is None else seed)
    q = rng.standard_normal((nq, D)).astype(np.float32)
    g = rng.standard_normal((ng, D)).astype(np.float32)
    if dup:
        src = rng.integers(0, ng, ng // 4); dst = rng.integers(0, ng, ng // 4)
        g[dst] = g[src]
    return q, g


def junk_matrix(q_pids, q_cams, g_pids, g_cams, camsets):
    """bool [nq, ng]: entry j is junk for query i."""
    q_pids, q_cams, g_pids, g_cams = (np.asarray(a, np.int64) for a in (q_pids, q_cams, g_pids, g_cams))
    same = g_pids[None, :] == q_pids[:, None]
    cam = ((g_cams[None, :] >> q_cams[:, None]) & 1) != 0 if camsets else g_cams[None, :] == q_cams[:, None]
    return same & cam


def make_case(nq, ng, D, dup, camsets):
    """(q, g, q_pids, q_cams, g_pids, g_cams): make_features, labels from default_rng(nq + ng) -- n_id = max(4, ng // 12)
    identities, gallery pids in [0, n_id), query pids in [0, n_id + n_id // 4 + 1) (some absent from the gallery), cameras in
    [0, 6), camera-set masks in [1, 64) -- and then every EVEN query that has junk is overwritten by its first junk gallery row
    + 0.05 N(0, 1): unfiltered, that junk row would be its rank 1."""
    q, g = make_features(nq, ng, D, dup)
    rng = np.random.default_rng(nq + ng)
    n_id = max(4, ng // 12)
    g_pids = rng.integers(0, n_id, ng)
    q_pids = rng.integers(0, n_id + n_id // 4 + 1, nq)
    q_cams = rng.integers(0, 6, nq)
    g_cams = rng.integers(1, 64, ng) if camsets else rng.integers(0, 6, ng)
    junk = junk_matrix(q_pids, q_cams, g_pids, g_cams, camsets)
    for i in range(0, nq, 2):
        js = np.nonzero(junk[i])[0]
        if len(js):
            q[i] = g[js[0]] + (0.05 * rng.standard_normal(D)).astype(np.float32)
    return q, g, q_pids.astype(np.int64), q_cams.astype(np.int64), g_pids.astype(np.int64), g_cams.astype(np.int64)


def planted(q_pids, q_cams, g_pids, g_cams, camsets):
    """The even queries make_case overwrote: those that have junk."""
    junk = junk_matrix(q_pids, q_cams, g_pids, g_cams, camsets)
    return np.array([i for i in range(0, len(q_pids), 2) if junk[i].any()], np.int64)


def ranked_ref(dist, q_pids, q_cams, g_pids, g_cams, k, camsets=False):
    """(idx int64 [m, k], dist fp32 [m, k], matched bool [m, k], count int32 [m]) of a given fp32 matrix."""
    dist = np.asarray(dist)
    assert dist.dtype == np.float32 and dist.ndim == 2
    m, n = dist.shape
    junk = junk_matrix(q_pids, q_cams, g_pids, g_cams, camsets)
    order = np.argsort(dist, axis=1, kind="stable")
    idx = np.full((m, k), -1, np.int64)
    dsel = np.full((m, k), np.inf, np.float32)
    matched = np.zeros((m, k), bool)
    count = np.zeros(m, np.int32)
    g_pids = np.asarray(g_pids, np.int64)
    for i in range(m):
        kept = order[i][~junk[i, order[i]]][:k]
        c = len(kept)
        idx[i, :c] = kept
        dsel[i, :c] = dist[i, kept]
        matched[i, :c] = g_pids[kept] == q_pids[i]
        count[i] = c
    return idx, dsel, matched, count


def camset_lists(q_cams, g_masks):
    """The respect_camids=True camera argument of R1_mAP.compute: [[c], ...] for the queries, then one list of camera ids per
    gallery mask."""
    return [[int(c)] for c in q_cams] + [[b for b in range(63) if (int(mk) >> b) & 1] for mk in g_masks]
