"""Float64 NumPy reference of reid_metric.query_expansion / neighbour_expand, written from the definition (no device code):

    U = l2_normalize(cat(q, g)); d = squared L2; every ordering by (d, index);
    sim = min(max(fmaf(-0.5f, d, 1.0f), 0.0f), 1.0f) on the fp32 d;  w = 1 (alpha == 0) | sim (alpha == 1) | sim ** alpha;
    scope "all":   S[i] = sum_t w[i, t] U[idx[i, t]], (idx, d) the k nearest of all N rows, the row itself among them;
    scope "query": S[i] = Uq[i] + sum_t w[i, t] Ug[idx[i, t]], (idx, d) the k - 1 nearest gallery rows; gallery untouched;
    U' = l2_normalize(S); rounds repeats the step.

Shared by tests/test_query_expansion_cpu.py (the reference's own properties, the quality recipe) and
tests/test_query_expansion_gpu.py (the device against it).  `exact_sums` is the exact model of the dyadic kernel cases."""
import numpy as np

F32 = np.float32


def unit(x, eps=1e-12):
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), eps)


def sqdist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)


def neighbours(a, b, k):
    """(idx int64 [m, k], d float32 [m, k]): the k nearest rows of b for every row of a, by stable argsort of (d, index)."""
    d = sqdist(a, b)
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    return idx.astype(np.int64), np.take_along_axis(d, idx, axis=1).astype(F32)


def sim_f32(d):
    """The fp32 similarity of the definition.  -0.5f * d is exact (a power of two), so the separate multiply and add round once,
    like the fmaf."""
    d = np.asarray(d, F32)
    with np.errstate(invalid="ignore"):
        s = F32(1) + F32(-0.5) * d
    s = np.where(np.isnan(s), F32(0), s)                     # fmaxf(NaN, 0) = 0
    return np.minimum(np.maximum(s, F32(0)), F32(1)).astype(F32)


def weights(d, alpha):
    """float64 weights from the fp32 sim (alpha == 0: exactly 1 whatever d is)."""
    d = np.asarray(d, F32)
    if alpha == 0:
        return np.ones(d.shape, np.float64)
    s = sim_f32(d).astype(np.float64)
    return s if alpha == 1 else s ** float(alpha)


def expand(x, idx, d, alpha, self_rows=None):
    """(S float64 [m, D], B float64 [m, D]): the sums and B = sum |w u| (the self row included), the scale of the error bound."""
    x = np.asarray(x, np.float64)
    w = weights(d, alpha)
    rows = x[idx]                                            # [m, k, D]
    S = (w[:, :, None] * rows).sum(axis=1)
    B = (w[:, :, None] * np.abs(rows)).sum(axis=1)
    if self_rows is not None:
        s = np.asarray(self_rows, np.float64)
        S, B = S + s, B + np.abs(s)
    return S, B


def exact_sums(x, idx, w, self_rows=None):
    """The exact model of the dyadic cases: integer rows times dyadic weights, every partial sum representable in fp32, so the
    float64 sum IS the fmaf chain's result.  Returns float32 and asserts that nothing was rounded."""
    x = np.asarray(x, np.float64)
    m, k = idx.shape
    S = np.zeros((m, x.shape[1]), np.float64) if self_rows is None else np.asarray(self_rows, np.float64).copy()
    for t in range(k):
        S = S + np.asarray(w, np.float64)[:, t, None] * x[idx[:, t]]
        assert np.array_equal(S.astype(F32).astype(np.float64), S)
    return S.astype(F32)


def query_expansion_ref(q, g, k=10, alpha=3.0, rounds=1, scope="all"):
    """(q', g') float64 unit rows."""
    nq = len(q)
    Uq, Ug = unit(q), unit(g)
    for _ in range(rounds):
        if scope == "all":
            U = np.concatenate([Uq, Ug])
            idx, d = neighbours(U, U, k)
            U = unit(expand(U, idx, d, alpha)[0])
            Uq, Ug = U[:nq], U[nq:]
        elif scope == "query":
            if k > 1:
                idx, d = neighbours(Uq, Ug, k - 1)
                Uq = unit(expand(Ug, idx, d, alpha, self_rows=Uq)[0])
            else:
                Uq = unit(Uq)
        else:
            raise ValueError(scope)
    return Uq, Ug


def mean_ap(q, g, q_pids, g_pids, q_cams, g_cams):
    """mAP of the squared-L2 ranking by (d, index), entries of the query's pid AND camera removed (utils/eval_reid.py)."""
    d = sqdist(q, g)
    order = np.argsort(d, axis=1, kind="stable")
    aps = []
    for i in range(len(q)):
        o = order[i]
        keep = ~((g_pids[o] == q_pids[i]) & (g_cams[o] == q_cams[i]))
        hit = (g_pids[o][keep] == q_pids[i]).astype(np.float64)
        if hit.sum() == 0:
            continue
        prec = np.cumsum(hit) / (np.arange(len(hit)) + 1.0)
        aps.append((prec * hit).sum() / hit.sum())
    return float(np.mean(aps))


def quality_set(seed):
    """The quality recipe: 24 identities around unit centres at D = 64, 8 gallery and 2 query rows each, noise 0.2 per element;
    queries on camera 0, gallery on camera 1.  Drawn in this order from one generator."""
    rng = np.random.default_rng(seed)
    C = unit(rng.standard_normal((24, 64)))
    g_pids = np.repeat(np.arange(24), 8)
    g = C[g_pids] + 0.2 * rng.standard_normal((len(g_pids), 64))
    q_pids = np.repeat(np.arange(24), 2)
    q = C[q_pids] + 0.2 * rng.standard_normal((len(q_pids), 64))
    return q, g, q_pids, g_pids, np.zeros(len(q_pids), np.int64), np.ones(len(g_pids), np.int64)


def clustered_unit_rows(n, D, n_centres, seed, noise=0.7):
    """n unit rows around n_centres unit centres, noise norm about `noise` (float32)."""
    rng = np.random.default_rng(seed)
    C = unit(rng.standard_normal((n_centres, D)))
    x = C[rng.integers(0, n_centres, n)] + (noise / np.sqrt(D)) * rng.standard_normal((n, D))
    return unit(x).astype(F32)
