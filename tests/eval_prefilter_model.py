"""A numpy model of the banded count of R1_mAP(streamed=True, prefilter=...) (csrc/stream_consume.hpp, EPI_BAND, and
stream_count_rescore_kernel), shared by tests/test_eval_prefilter_cpu.py and tests/test_eval_prefilter_gpu.py: the outward
rounding helpers, fp32 emulations of both distance kernels, the four-step rule and the input generator of the GPU test.  Not a
test module."""
import numpy as np
import torch

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
FLT_MAX = np.float32(3.402823466e+38)


def mono_key(d):
    """float32 -> uint32 with the same order (mono_key, csrc/stream_common.hpp)"""
    u = np.asarray(d, np.float32).view(np.uint32)
    return u ^ np.where(u >> 31, np.uint32(0xffffffff), np.uint32(0x80000000))


def _step(s, up):
    s = np.asarray(s, np.float32)
    u = s.view(np.uint32).astype(np.int64)
    neg = (u >> 31) != 0
    moved = np.where(neg == up, u - 1, u + 1)
    moved = np.where((u & 0x7fffffff) == 0, 0x00000001 if up else 0x80000001, moved)
    out = moved.astype(np.uint32).view(np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(s) <= FLT_MAX, out, s)                           # inf / NaN stay


def add_up(a, b):
    """add_up (csrc/stream_common.hpp): the fp32 sum moved one step up"""
    with np.errstate(over="ignore", invalid="ignore"):
        return _step(np.asarray(a, np.float32) + np.asarray(b, np.float32), True)


def sub_down(a, b):
    """sub_down: the fp32 difference moved one step down"""
    with np.errstate(over="ignore", invalid="ignore"):
        return _step(np.asarray(a, np.float32) - np.asarray(b, np.float32), False)


def rounded(x, dt):
    """fp32 -> dt (torch's CPU cast: round to nearest even) -> float64, exact"""
    return torch.from_numpy(np.ascontiguousarray(x)).to(DTYPES[dt]).to(torch.float64).numpy()


def row_stats(x, xh):
    x = x.astype(np.float64)
    return ((x - xh) ** 2).sum(1), (xh ** 2).sum(1), (x ** 2).sum(1)


def l2n(x):
    """fp32 rows / their norm, in fp32 steps"""
    n = np.sqrt((x.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    return (x / np.maximum(n, np.float32(1e-12))[:, None]).astype(np.float32)


def emulate(q, g, dt):
    """(d, dh, margin32): the fp32 kernel as the k-ordered chain in fp32 steps (product and sum rounded separately), the 16-bit
    kernel as fp32 accumulation of the exact products of the rounded rows in blocks of 16 -- the emulations of
    tests/test_topk_prefilter_cpu.py --, both with the fp32 rows' norms; the margin as reid_metric computes it: prefilter_margin,
    inflated and rounded up to fp32."""
    from centroids_reid_amd import reid_metric as rm
    M, D = q.shape
    N = g.shape[0]
    qh, gh = rounded(q, dt), rounded(g, dt)
    qq = (q.astype(np.float64) ** 2).sum(1).astype(np.float32)
    gg = (g.astype(np.float64) ** 2).sum(1).astype(np.float32)
    acc = np.zeros((M, N), np.float32)
    gt = np.ascontiguousarray(g.T)
    for k in range(D):
        acc = np.outer(q[:, k], gt[k]).astype(np.float32) + acc
    acch = np.zeros((M, N), np.float32)
    for k0 in range(0, D, 16):
        blk = qh[:, k0:k0 + 16] @ gh[:, k0:k0 + 16].T
        acch = (acch.astype(np.float64) + blk).astype(np.float32)
    s = qq[:, None] + gg[None, :]
    d = (s.astype(np.float64) - 2.0 * acc.astype(np.float64)).astype(np.float32)
    dh = (s.astype(np.float64) - 2.0 * acch.astype(np.float64)).astype(np.float32)
    e2, h2, x2 = row_stats(q, qh)
    ge2, gh2, gx2 = (v.max() for v in row_stats(g, gh))
    x2 = np.maximum(x2, qq.astype(np.float64))
    D8 = -(-D // 8) * 8
    m64 = rm.prefilter_margin(e2, h2, x2, ge2, gh2, gx2, max(gx2, float(np.abs(gg).max())), D8)
    assert (np.abs(dh.astype(np.float64) - d.astype(np.float64)) <= m64[:, None]).all()
    m32 = rm._round_up_f32(torch.from_numpy((1.0 + rm._PREFILTER_INFLATE) * m64)).numpy()
    return d, dh, m32


def banded_count(d, dh, m32, q_pids, g_pids, q_cams, g_cams, cap=128):
    """The four-step rule per query row against the fp32 count on d.  Returns (full, decided, ambiguous): the fp32 histogram
    [M, cap], the histogram of the pairs the rule decides, and the number of ambiguous pairs per row; asserts that every decided
    pair lands in its fp32 slot and that decided + the ambiguous pairs placed by d == full."""
    M, N = d.shape
    full = np.zeros((M, cap), np.int64)
    decided = np.zeros((M, cap), np.int64)
    ambiguous = np.zeros(M, np.int64)
    for i in range(M):
        same = g_pids == q_pids[i]
        pos = np.nonzero(same & (g_cams != q_cams[i]))[0]
        npos = len(pos)
        if npos == 0 or npos > cap:
            continue
        kd = mono_key(d[i])
        order = np.lexsort((pos, kd[pos]))
        K, P = kd[pos][order], pos[order]
        neg = ~same
        # the fp32 count: positives ranked before j by (key, gallery index)
        l_lt = np.searchsorted(K, kd, side="left")
        l_le = np.searchsorted(K, kd, side="right")
        slot = l_lt.copy()
        for j in np.nonzero(neg & (l_le > l_lt))[0]:                             # ties: by gallery index
            slot[j] = l_lt[j] + int((P[l_lt[j]:l_le[j]] < j).sum())
        cnt = neg & (kd <= K[-1]) & (slot < npos)
        np.add.at(full[i], slot[cnt], 1)
        # the rule
        lo, hi = sub_down(dh[i], m32[i]), add_up(dh[i], m32[i])
        with np.errstate(invalid="ignore"):
            fin = (np.abs(dh[i]) <= FLT_MAX) & (np.abs(lo) <= FLT_MAX) & (np.abs(hi) <= FLT_MAX)
        klo, khi = mono_key(lo), mono_key(hi)
        behind = fin & (klo > K[-1])                                             # 1. behind every positive
        l = np.searchsorted(K, klo, side="left")                                 # 2. positives strictly below key(lo)
        inside = (l < npos) & (K[np.minimum(l, npos - 1)] <= khi)                # 3. a positive inside the band
        amb = neg & ~behind & (~fin | inside)
        dec = neg & ~behind & ~amb                                               # 4. slot l
        assert (l[dec] < npos).all()
        assert (~cnt[neg & behind]).all(), "a skipped pair is counted by the fp32 kernel"
        assert cnt[dec].all() and (slot[dec] == l[dec]).all(), "a decided pair is not in its fp32 slot"
        np.add.at(decided[i], l[dec], 1)
        ambiguous[i] = int(amb.sum())
        placed = decided[i].copy()
        np.add.at(placed, slot[amb & cnt], 1)
        assert (placed == full[i]).all()
    return full, decided, ambiguous


def clustered(nq, ng, D, seed):
    """The generator of the GPU test: unit-norm centres for (nq + ng) // 20 identities, a row = its centre + 0.7 / sqrt(D) N(0,1),
    pid = the centre, 10 % of the GALLERY rows get a uniformly random pid, cameras uniform in 0..5; then a pid absent from the
    gallery (query 0), a query whose positives all share its camera (query 1) and a zero-distance positive (of query 3)."""
    rng = np.random.default_rng(seed)
    nid = max((nq + ng) // 20, 2)
    c = rng.standard_normal((nid, D))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    pids = rng.integers(0, nid, nq + ng)
    f = (c[pids] + 0.7 / np.sqrt(D) * rng.standard_normal((nq + ng, D))).astype(np.float32)
    noisy = nq + rng.choice(ng, ng // 10, replace=False)
    pids[noisy] = rng.integers(0, nid, len(noisy))
    cams = rng.integers(0, 6, nq + ng)
    pids[0] = nid + 5
    f[nq + 7] = f[3]; pids[nq + 7] = pids[3]; cams[nq + 7] = (cams[3] + 1) % 6
    cams[nq:][pids[nq:] == pids[1]] = cams[1]
    return f, pids, cams
