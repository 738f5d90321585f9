"""Operands, references and conditions that pin the evaluation side (csrc/dist.hip, rank.hip, stream_eval.hip, stream_h16.hip and
their Python surface in reid_metric.py) against references that share nothing with the kernels.  numpy / torch on the CPU only: no
GPU and no project kernel in here; used by tests/test_eval_exact_cpu.py and tests/test_eval_exact_gpu.py.

EXACT PART.  Features are integers, the same values in fp32, bf16 and f16:
  * most elements come from {+-1, +-2, +-3} -- no zeros, so a dropped or duplicated product always changes a sum;
  * about one element in 64 is a large ODD magnitude with the top bit of the type's significand set (129..255 for bf16,
    1025..2047 for f16, 2049..4095 for fp32), halved per case (255 -> 127 -> ...) until the margin below holds;
  * a quarter of the gallery rows are copied over others (exact ties), one copy is forced between a positive and a negative
    of query 2, and gallery row 7 equals query 3 with the same pid and another camera (a zero distance);
  * query 0's pid is absent from the gallery, query 1's positives all share its camera (two invalid queries);
  * some cases carry a scale of 2^-6 (values that look like normalised features): exactness does not depend on a power of two.
The reference distance is the int64 qq + gg - 2 q.g, the ranking its stable argsort (ties by gallery index), the per-query
(valid, AP, first) the Market-1501 evaluation of oracle.reid_oracle.eval_market on that ranking.

Exactness margin of a case: (max qq + max gg + 2 max_ij sum_k |q_ik| |g_jk|) / 2^24 < 1.  Then every fp32 partial sum of the
products, of the squares, and of the epilogue qq + gg - 2 dot is an integer below 2^24 in ANY order of summation, so a kernel's
distance must EQUAL the reference -- tile shape, k order, work split and MFMA type do not enter.

BOUNDED PART (realistic operands; integers cannot show an accumulation or an epilogue in the wrong type).  u = 2^-24; an fma /
add chain of c terms followed by the 6 levels of a wave sum has the first-order bound (c + 6) u sum |terms|.  Read off
csrc/dist.hip:
  * row_sqnorm_kernel: a lane sums ceil(D / 64) squares (products exact inside the fma)      -> (ceil(D / 64) + 6) u sum x^2;
  * l2norm_rows_kernel: a lane sums 4 squares per 16-byte chunk, ceil(D / 256) chunks          -> s within (4 ceil(D / 256) + 6) u;
    y = x / max(sqrt(s), eps): half the relative error of s, sqrtf within 1 ulp (2 u) and the fp32 division within 2.5 ulp
    (5 u) -- the documented worst case of the device's sqrtf and division (correctly rounded builds do better);
    the type's own rounding of y is Audit.check's half ulp;
  * the square norms l2norm returns are sums over the ROUNDED rows, same chain                  -> (4 ceil(D / 256) + 6) u sum y^2;
  * sqdist kernels, on the stored rows and stored norms: the accumulator carries the project's K u sum |x| |w| rule
    (layer_audit), doubled by the epilogue's -2; one rounding of qq + gg; one of the final fma:
        2 D u sum_k |q_k| |g_k| + u (qq + gg) + u |d|.
None of these bounds is fitted to a run.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np

DTYPES = ("fp32", "bf16", "f16")
BIG = {"bf16": 255, "f16": 2047, "fp32": 4095}       # the largest odd integer of the type's significand (8 / 11 / 12 of 24 bits)
LIMIT = 1 << 24                                      # integers below it are exact in fp32
U = 2.0 ** -24
STREAM_CAPACITY = 4096                               # reid_metric.STREAM_TOPK_CAPACITY
PL_MAX = 128                                         # reid_metric.StreamPlan.MAX_CAP


class Case(NamedTuple):
    name: str
    m: int
    n: int
    D32: int                    # feature width of the fp32 run
    D16: int                    # feature width of the bf16 / f16 runs (a multiple of 8)
    k: int                      # top-k
    sample: int                 # threshold sample of topk_stream
    scale_exp: int = 0          # features are integers * 2^scale_exp
    npid: int = 12
    ncam: int = 3
    overflow: bool = False      # one pid with more than PL_MAX positives

    def D(self, dt):
        return self.D32 if dt == "fp32" else self.D16

    @property
    def labelled(self):
        """large enough for the four special queries and the three special gallery rows"""
        return self.m >= 4 and self.n >= 16


# the materialised kernels: 128 x 128 tiles, k-tiles of 16 (fp32) / 64 (16-bit), the XCD remap over the tile count
MATRIX = [
    Case("1x1", 1, 1, 4, 8, 1, 1),
    Case("127x129", 127, 129, 12, 56, 20, 64, scale_exp=-6),
    Case("128x128", 128, 128, 16, 64, 5, 32),
    Case("129x127", 129, 127, 20, 72, 60, 64),
    Case("3x5tiles", 260, 520, 100, 104, 50, 128, scale_exp=-6, npid=40),
    Case("65x257", 65, 257, 36, 2032, 10, 64),
    Case("70x300", 70, 300, 2048, 2048, 7, 64, scale_exp=-6, npid=20),
    Case("wide", 9, 40, 4104, 4104, 5, 16),                       # D beyond the register-resident row of the normalisation
]
# the streamed kernels: 64 x 256 tiles in units of 64 columns; both instantiations of the fp32 kernel (D % 16 == 0 or not)
STREAM = [
    Case("s1x1", 1, 1, 4, 8, 1, 1),
    Case("s65x257", 65, 257, 4, 8, 5, 32),
    Case("s65x513", 65, 513, 12, 56, 50, 128, scale_exp=-6, npid=30),
    Case("s65x4097", 65, 4097, 16, 64, 100, 512, npid=400, ncam=4),
    Case("s33x300", 33, 300, 20, 72, 5, 32, scale_exp=-6),
    Case("s70x600", 70, 600, 36, 2032, 10, 128, npid=30),
    Case("s129x1000", 129, 1000, 2048, 2048, 7, 64, scale_exp=-6, npid=100, ncam=5),
    Case("s130x700", 130, 700, 100, 104, 20, 128, npid=40),
    Case("s5x40", 5, 40, 16, 64, 40, 40),
]
# every candidate list longer than capacity = 64: all rows redone through the materialised kernels
FALLBACK = Case("cap64", 40, 1500, 20, 72, 40, 64, npid=60)
FALLBACK_CAPACITY = 64
# pid 4 has 200 gallery entries: queries 4..7 overflow the positive list and take the general path
OVERFLOW = Case("overflow", 40, 700, 16, 64, 10, 64, npid=30, ncam=4, overflow=True)
ALL = MATRIX + STREAM + [FALLBACK, OVERFLOW]
BY_NAME = {c.name: c for c in ALL}


class Ref(NamedTuple):
    case: Case
    dt: str
    big: int                    # the large magnitude after halving
    margin: float
    scale: float
    q: np.ndarray               # int64 [m, D]
    g: np.ndarray               # int64 [n, D]
    pids: np.ndarray            # [m + n]
    cams: np.ndarray
    qq: np.ndarray              # int64 [m]
    gg: np.ndarray
    dist: np.ndarray            # int64 [m, n]
    order: np.ndarray           # stable argsort of dist
    valid: np.ndarray
    ap: np.ndarray
    first: np.ndarray
    cmc: np.ndarray
    mAP: float
    topk: np.ndarray

    @property
    def feats(self):
        """float64 [m + n, D]: what the kernels are fed (after a cast to the dtype, which must not change a value)"""
        return np.concatenate([self.q, self.g]).astype(np.float64) * self.scale

    @property
    def fdist(self):
        """the distances as float64, scale applied (a power of four: exact)"""
        return self.dist.astype(np.float64) * (self.scale * self.scale)

    def fnorm(self, v):
        return v.astype(np.float64) * (self.scale * self.scale)


def _features(rows, D, big, rng):
    x = rng.integers(1, 4, (rows, D)) * rng.choice((-1, 1), (rows, D))
    sel = rng.random((rows, D)) < 1.0 / 64
    if big > 3:
        lo = (big + 1) // 2                                              # top bit of the (halved) significand
        mag = 2 * rng.integers(lo // 2, (big + 1) // 2, (rows, D)) + 1   # odd, lo < mag <= big
        x = np.where(sel, mag * np.sign(x), x)
    return x.astype(np.int64)


def _build(case, dt, big):
    m, n, D = case.m, case.n, case.D(dt)
    rng = np.random.default_rng([case.m, case.n, D, DTYPES.index(dt)])
    q, g = _features(m, D, big, rng), _features(n, D, big, rng)
    if big > 3:                                     # at least one large element on either side, at different k
        q[0, 0] = big
        g[0, D - 1] = -big
    src, dst = rng.integers(0, n, n // 4), rng.integers(0, n, n // 4)
    g[dst] = g[src]
    pids = rng.integers(0, case.npid, m + n)
    cams = rng.integers(0, case.ncam, m + n)
    if case.overflow:
        pids[pids == 4] = 5                                              # pid 4 belongs to the overflow block alone
        pids[m:m + 200] = 4
        pids[4:8] = 4
    if case.labelled:
        assert case.npid >= 5 and case.ncam >= 2
        pids[0], pids[1], pids[2], pids[3] = case.npid + 5, 0, 1, 2
        a, b, z = 5, 11, 7
        pids[m + a], cams[m + a] = 1, (cams[2] + 1) % case.ncam          # a positive of query 2 ...
        pids[m + b] = 3
        g[b] = g[a]                                                      # ... tied with a negative behind it
        g[z] = q[3]
        pids[m + z], cams[m + z] = 2, (cams[3] + 1) % case.ncam          # the zero distance
        cams[m:][pids[m:] == 0] = cams[1]                                # every positive of query 1 shares its camera
    else:
        pids[m], cams[m] = pids[0], (cams[0] + 1) % case.ncam            # the first query is valid
    return q, g, pids, cams


def margin_of(q, g):
    """(max qq + max gg + 2 max_ij sum_k |q_ik| |g_jk|) / 2^24 on integer features (float64 BLAS: sums far below 2^53)"""
    qq, gg = (q * q).sum(1), (g * g).sum(1)
    cross = (np.abs(q).astype(np.float64) @ np.abs(g).astype(np.float64).T).max()
    return (float(qq.max()) + float(gg.max()) + 2.0 * float(cross)) / LIMIT


@functools.lru_cache(maxsize=None)
def reference(name, dt):
    """The case's operands (large magnitude halved until the margin is below 1) and everything the GPU tests compare with."""
    from oracle import reid_oracle as ro
    case = BY_NAME[name]
    big = BIG[dt]
    while True:
        q, g, pids, cams = _build(case, dt, big)
        mg = margin_of(q, g)
        if mg < 1.0 or big <= 3:
            break
        big //= 2
    qq, gg = (q * q).sum(1), (g * g).sum(1)
    dist = qq[:, None] + gg[None, :] - 2 * (q @ g.T)                     # int64 throughout
    order = np.argsort(dist, axis=1, kind="stable").astype(np.int64)
    m = case.m
    cmc, mAP, topk, ex = ro.eval_market(order, pids[:m], pids[m:], cams[:m], cams[m:])
    for a in (q, g, pids, cams, qq, gg, dist, order):
        a.setflags(write=False)
    return Ref(case, dt, big, mg, 2.0 ** case.scale_exp, q, g, pids, cams, qq, gg, dist, order, ex["valid"], ex["ap"],
               ex["first"], cmc, mAP, topk)


# ------------------------------------------------------------------------------------------------ counters
def candidate_counts(ref, k=None, sample=None):
    """topk_stream's candidate list per query, by its own rule: stride n // S, tau = the k-th smallest of the strided sample,
    every column with d <= tau."""
    k = ref.case.k if k is None else k
    n = ref.case.n
    S = max(k, min(n, ref.case.sample if sample is None else sample))
    cols = np.arange(0, n, n // S)[:S]
    tau = np.partition(ref.dist[:, cols], k - 1, axis=1)[:, k - 1]
    return (ref.dist <= tau[:, None]).sum(1)


def positive_counts(ref):
    m = ref.case.m
    pos = (ref.pids[m:][None, :] == ref.pids[:m, None]) & (ref.cams[m:][None, :] != ref.cams[:m, None])
    return pos.sum(1)


def tied_columns(ref):
    """per row: the number of columns whose distance occurs more than once in the row"""
    s = np.sort(ref.dist, axis=1)
    if s.shape[1] < 2:
        return np.zeros(s.shape[0], np.int64)
    eq = s[:, 1:] == s[:, :-1]
    tied = np.zeros(s.shape, bool)
    tied[:, 1:] |= eq
    tied[:, :-1] |= eq
    return tied.sum(1)


def pos_neg_ties(ref):
    """number of (query, positive, kept negative) triples at one distance"""
    m = ref.case.m
    same = ref.pids[m:][None, :] == ref.pids[:m, None]
    pos = same & (ref.cams[m:][None, :] != ref.cams[:m, None])
    neg = ~same
    cnt = 0
    for i in range(m):
        cnt += int(np.isin(ref.dist[i][pos[i]], ref.dist[i][neg[i]]).sum())
    return cnt


def zero_distances(ref):
    return int((ref.dist == 0).sum())


# ------------------------------------------------------------------------------------------------ mutations of the reference
def _dist_with_dot(ref, dot):
    return ref.qq[:, None] + ref.gg[None, :] - 2 * dot


def mut_drop_k(ref, k0):
    """a contraction that skips feature index k0"""
    return _dist_with_dot(ref, ref.q @ ref.g.T - np.outer(ref.q[:, k0], ref.g[:, k0]))


def mut_drop_last_step(ref, step=16):
    """a k-loop that stops one 16-deep step early: the indices from (D - 1) // 16 * 16 on are never multiplied"""
    lo = (ref.q.shape[1] - 1) // step * step
    return _dist_with_dot(ref, ref.q[:, :lo] @ ref.g[:, :lo].T)


def mut_repeat_step(ref, step=16):
    """a k-loop that runs its first step twice"""
    hi = min(step, ref.q.shape[1])
    return _dist_with_dot(ref, ref.q @ ref.g.T + ref.q[:, :hi] @ ref.g[:, :hi].T)


def mut_tail_reads_last(ref, unit=64):
    """the columns of the last (partial) 64-column unit all read gallery row n - 1 (a clamped load without its mask).  Returns
    (distances, mask of the columns the mutation touches: the tail but n - 1 itself)."""
    n = ref.case.n
    t0 = (n - 1) // unit * unit
    g2 = ref.g.copy()
    g2[t0:] = ref.g[n - 1]
    touched = np.zeros(n, bool)
    touched[t0:n - 1] = True
    return _dist_with_dot(ref, ref.q @ g2.T), touched


def rank_last_index_first(dist):
    """ties by DESCENDING gallery index: the ranking a kernel with the wrong tie rule returns"""
    n = dist.shape[1]
    return (n - 1 - np.argsort(dist[:, ::-1], axis=1, kind="stable")).astype(np.int64)


# ------------------------------------------------------------------------------------------------ bounded audit (fp64, torch)
def audit_features(kind, rows, D, seed):
    """fp32 [rows, D] test features, row 7 all zero.  'normal': N(0, 1); 'clustered': 12 identity centres N(0, 1) plus 0.3 N(0, 1)
    (rows of one identity are close: small distances, where cancellation in qq + gg - 2 q.g is worst)."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, D), generator=gen)
    if kind == "clustered":
        centres = torch.randn((12, D), generator=gen)
        x = centres[torch.arange(rows) % 12] + 0.3 * x
    x[7] = 0
    return x.float().contiguous()


def sqnorm_chain(D, per_chunk):
    """fma-chain length + wave-sum levels of the two norm kernels: per_chunk = 1 (row_sqnorm: one element per lane and trip,
    ceil(D / 64) trips), per_chunk = 4 (l2norm: one 16-byte chunk per lane and trip, ceil(D / 256) trips)"""
    return per_chunk * math.ceil(D / (64 * per_chunk)) + 6


def sqnorm_ref_bound(x, per_chunk):
    """(fp64 sum of squares of the stored rows, its bound chain * u * sum x^2)"""
    s = (x.double() ** 2).sum(1)
    return s, sqnorm_chain(x.shape[1], per_chunk) * U * s


def normalize_ref_bound(x, eps=1e-12):
    """(fp64 x / max(|x|, eps), the bound of the fp32 value BEFORE the type's rounding): |y| (chain u / 2 + 2 u + 5 u)"""
    xd = x.double()
    nrm = xd.pow(2).sum(1, keepdim=True).sqrt().clamp_min(eps)
    y = xd / nrm
    rel = 0.5 * sqnorm_chain(x.shape[1], 4) * U + 2 * U + 5 * U
    return y, y.abs() * rel


def dist_ref_bound(q, g, qq, gg):
    """(fp64 qq + gg - 2 q.g on the stored rows and the stored fp32 norms, 2 D u sum |q| |g| + u (qq + gg) + u |d|)"""
    qd, gd = q.double(), g.double()
    s = qq.double()[:, None] + gg.double()[None, :]
    d = s - 2.0 * (qd @ gd.t())
    b = 2.0 * q.shape[1] * U * (qd.abs() @ gd.abs().t()) + U * s + U * d.abs()
    return d, b
