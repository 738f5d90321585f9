"""float64 reference of k-reciprocal re-ranking (Zhong et al., CVPR 2017), written from the definition that
reid_metric.re_ranking documents, plus the small-integer feature generators its tests share.

The reference takes the N x N distance matrix as INPUT, so that no discrete decision (a neighbour order, a set membership)
depends on how distances were rounded: the tests hand it exact int64 distances, or the device's own fp32 ones."""
import numpy as np


def rerank_reference(d_all, nq, k1, k2, lam):
    """-> (out float64 [nq, ng], sets: list of N sorted int64 arrays R*(i), Vq float64 [N, N] = V' of every row).

    X = cat(q, g), N = nq + ng, d_all[i, j] = d(i, j); every ordering by (d, index) (a stable argsort).
      1. M_i = max_j d(i, j); od = d / M_i, 0 where M_i == 0
      2. R(i, k) = {j in N_{k+1}(i) : i in N_{k+1}(j)}, N_k(i) the first k columns of row i
      3. kh = int(around(k1 / 2)); R*(i) = R(i, k1) | U {R(c, kh) : c in R(i, k1), 3 |R(c, kh) & R(i, k1)| > 2 |R(c, kh)|}
      4. V(i, j) = exp(-od(i, j)) / sum_{t in R*(i)} exp(-od(i, t)) on R*(i), 0 elsewhere
      5. V'(i) = mean of V(t), t in N_{k2}(i)   (k2 > 1; else V' = V)
      6. s(i, j) = sum_c min(V'(i, c), V'(j, c)); J = 1 - s / (2 - s)
      7. out[i, j] = (1 - lam) J(i, nq + j) + lam od(i, nq + j)"""
    d = np.asarray(d_all, dtype=np.float64)
    N = d.shape[0]
    assert d.shape == (N, N) and 0 < nq < N and 1 <= k1 + 1 <= N and 1 <= k2 <= k1 + 1
    order = np.argsort(d, axis=1, kind="stable")
    M = d.max(axis=1)
    od = np.where(M[:, None] == 0, 0.0, d / np.where(M == 0, 1.0, M)[:, None])
    kh = int(np.around(k1 / 2))

    def member(k):                      # member[i, j] = j in N_{k+1}(i)
        m = np.zeros((N, N), dtype=bool)
        np.put_along_axis(m, order[:, :k + 1], True, axis=1)
        return m

    def recip(i, k, mem):               # R(i, k) in neighbour order
        fwd = order[i, :k + 1]
        return fwd[mem[fwd, i]]

    mem1, memh = member(k1), member(kh)
    sets, V = [], np.zeros((N, N))
    for i in range(N):
        r1 = recip(i, k1, mem1)
        base, star = set(r1.tolist()), set(r1.tolist())
        for c in r1:
            rc = set(recip(int(c), kh, memh).tolist())
            if 3 * len(rc & base) > 2 * len(rc):
                star |= rc
        cols = np.array(sorted(star), dtype=np.int64)
        sets.append(cols)
        if len(cols):
            w = np.exp(-od[i, cols])
            V[i, cols] = w / w.sum()
    if k2 > 1:
        Vq = np.zeros((N, N))
        for t in range(k2):
            Vq += V[order[:, t]]
        Vq /= k2
    else:
        Vq = V
    out = np.empty((nq, N - nq))
    Vg = Vq[nq:]
    for i in range(nq):
        s = np.minimum(Vq[i][None, :], Vg).sum(axis=1)
        out[i] = (1 - lam) * (1 - s / (2 - s)) + lam * od[i, nq:]
    return out, sets, Vq


def int_sqdist(X):
    """Exact squared L2 distances of integer rows, int64 [N, N]."""
    X = np.asarray(X, dtype=np.int64)
    sq = (X * X).sum(axis=1)
    return sq[:, None] + sq[None, :] - 2 * (X @ X.T)


def clustered_int_features(n, D, n_clusters, seed, spread=2, scale=12):
    """n rows of small integers around n_clusters integer centres: many exactly equal distances (ties resolved by index),
    every squared distance far below 2^24, so fp32 arithmetic on them is exact."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(-scale, scale + 1, (n_clusters, D))
    X = centres[rng.integers(0, n_clusters, n)] + rng.integers(-spread, spread + 1, (n, D))
    assert int_sqdist(X).max() < 1 << 24
    return X.astype(np.float32)
