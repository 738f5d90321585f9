"""Stage D/E host side: the reference's metric surface on top of the HIP kernels.

Mirrors utils/reid_metric.py (get_euclidean :25-33, get_dist_func :62-68, R1_mAP :71-151)
and utils/eval_reid.py (eval_func :25-92) -- same names, argument meaning and return
values -- but every step runs on the GPU: rows are normalised, the squared-L2 matrix comes
from the MFMA distance kernel, ranking is a device radix sort, and CMC/AP are scanned on the
device; only the final few scalars come back to the host.
"""
from __future__ import annotations

import os
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L

K_LIST = [1, 5, 10, 20, 50]


# --------------------------------------------------------------------------- primitives
def l2_normalize(x: torch.Tensor, out_dtype=torch.float32, eps: float = 1e-12, return_sqnorm=False):
    L.require_gpu(x)
    assert x.dtype == torch.float32 and x.dim() == 2
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    sq = torch.empty(x.shape[0], dtype=torch.float32, device=x.device) if return_sqnorm else None
    L.check(L.lib().creid_l2norm_rows(L.ptr(x), L.ptr(y), L.ptr(sq), x.shape[0], x.shape[1],
                                      L._DT[out_dtype], eps, L.stream()), "creid_l2norm_rows")
    return (y, sq) if return_sqnorm else y


def row_sqnorm(x: torch.Tensor) -> torch.Tensor:
    L.require_gpu(x)
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    L.check(L.lib().creid_row_sqnorm(L.ptr(x), L.ptr(out), x.shape[0], x.shape[1], L.dtype_code(x), L.stream()),
            "creid_row_sqnorm")
    return out


def get_euclidean(x: torch.Tensor, y: torch.Tensor, xx=None, yy=None, **kwargs) -> torch.Tensor:
    """Squared L2 matrix [m, n] fp32 (utils/reid_metric.py:25-33)."""
    L.require_gpu(x, y)
    assert x.dtype == y.dtype and x.shape[1] == y.shape[1]
    xx = row_sqnorm(x) if xx is None else xx
    yy = row_sqnorm(y) if yy is None else yy
    m, n, D = x.shape[0], y.shape[0], x.shape[1]
    out = torch.empty((m, n), dtype=torch.float32, device=x.device)
    L.check(L.lib().creid_sqdist_matrix(L.ptr(x), L.ptr(y), L.ptr(xx), L.ptr(yy), m, n, D, L.dtype_code(x),
                                        L.ptr(out), n, L.stream()), "creid_sqdist_matrix")
    return out


def get_cosine(x: torch.Tensor, y: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """utils/reid_metric.py:51-59: clamp(|1 - cos|, eps).  With unit rows |x-y|^2 = 2 - 2cos, so the
    cosine matrix is derived from the same MFMA kernel: cos = 1 - d/2 on re-normalised rows."""
    xn, xs = l2_normalize(x.float(), eps=eps, return_sqnorm=True)
    yn, ys = l2_normalize(y.float(), eps=eps, return_sqnorm=True)
    d = get_euclidean(xn, yn, xs, ys)
    cos = (xs[:, None] + ys[None, :] - d) * 0.5
    return torch.abs(1 - cos).clamp(min=eps)


_H16 = (torch.bfloat16, torch.float16)


def _pad_width(feats: torch.Tensor, mult: int = 4) -> torch.Tensor:
    """The kernels load 16-byte k-chunks (D % 4 == 0 for fp32, D % 8 == 0 for bf16 / f16).  Zero columns change neither a norm
    nor a dot product, so any other width is padded up -- results identical, no kernel special case."""
    D = feats.shape[1]
    if D % mult == 0:
        return feats
    return torch.nn.functional.pad(feats, (0, mult - D % mult)).contiguous()


def get_dist_func(func_name="euclidean"):
    if func_name == "cosine":
        return get_cosine
    if func_name == "euclidean":
        return get_euclidean
    raise KeyError(func_name)


def rank_rows(distmat: torch.Tensor) -> torch.Tensor:
    """np.argsort(distmat, axis=1) (utils/reid_metric.py:129,132) with (distance, index) order."""
    L.require_gpu(distmat)
    assert distmat.dtype == torch.float32 and distmat.dim() == 2
    m, n = distmat.shape
    out = torch.empty((m, n), dtype=torch.int64, device=distmat.device)
    nbytes = L.lib().creid_rank_rows_workspace_bytes(m, n)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=distmat.device)
    L.check(L.lib().creid_rank_rows(L.ptr(distmat), m, n, n, L.ptr(out), L.ptr(ws), nbytes, L.stream()),
            "creid_rank_rows")
    return out


class _PerQuery(NamedTuple):
    """The per-query results of every evaluation route, on the device: valid u8 [m] (2: the query's positive list overflowed),
    ap f64 [m], first i32 [m] (rank of the first match)."""
    valid: torch.Tensor
    ap: torch.Tensor
    first: torch.Tensor

    @classmethod
    def empty(cls, m, device):
        return cls(torch.empty(m, dtype=torch.uint8, device=device), torch.empty(m, dtype=torch.float64, device=device),
                   torch.empty(m, dtype=torch.int32, device=device))

    @classmethod
    def finalize(cls, npos, hist, cap):
        """creid_stream_finalize: the histogram prefix of a streamed count (npos i32 [m], hist i32 [m, cap]) -> results."""
        m = npos.shape[0]
        out = cls.empty(m, npos.device)
        L.check(L.lib().creid_stream_finalize(L.ptr(npos), L.ptr(hist), m, cap, L.ptr(out.valid), L.ptr(out.ap), L.ptr(out.first),
                                              L.stream()), "creid_stream_finalize")
        return out

    def merge(self, rows, other):
        """The results `other` of the queries `rows` (an index tensor) take the place of these rows' own."""
        for mine, theirs in zip(self, other):
            mine.index_copy_(0, rows, theirs)


def rank_rows_eval(distmat: torch.Tensor, q_pids, g_pids, q_camids, g_camids):
    """rank_rows + the per-query half of eval_func (plain camera ids) in one pass over the distance matrix
    (creid_rank_rows_eval): returns (indices int64 [m, n], valid u8 [m], ap f64 [m], first i32 [m]) -- the index matrix is
    written for the caller but never read back by the evaluation."""
    L.require_gpu(distmat)
    assert distmat.dtype == torch.float32 and distmat.dim() == 2
    m, n = distmat.shape
    dev = distmat.device
    qp, gp, qc, gc = (_dev_i64(a, dev) for a in (q_pids, g_pids, q_camids, g_camids))
    out = torch.empty((m, n), dtype=torch.int64, device=dev)
    res = _PerQuery.empty(m, dev)
    nbytes = L.lib().creid_rank_rows_workspace_bytes(m, n)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    L.check(L.lib().creid_rank_rows_eval(L.ptr(distmat), m, n, n, L.ptr(out), L.ptr(ws), nbytes, L.ptr(qp), L.ptr(gp), L.ptr(qc),
                                         L.ptr(gc), L.ptr(res.valid), L.ptr(res.ap), L.ptr(res.first), L.stream()),
            "creid_rank_rows_eval")
    return (out, *res)


def topk_rows(distmat: torch.Tensor, k: int):
    """(indices int64 [m, k], distances fp32 [m, k]): the first k columns of np.argsort(distmat, axis=1) and the
    distances there (inference/get_similar.py:114-119), selected without sorting the whole row."""
    L.require_gpu(distmat)
    assert distmat.dtype == torch.float32 and distmat.dim() == 2
    m, n = distmat.shape
    if k > 1024 or k * 2 > n:
        idx = rank_rows(distmat)[:, :k].contiguous()
        return idx, torch.gather(distmat, 1, idx)
    dev = distmat.device
    idx = torch.empty((m, k), dtype=torch.int64, device=dev)
    dsel = torch.empty((m, k), dtype=torch.float32, device=dev)
    flags = torch.empty(m, dtype=torch.uint8, device=dev)
    L.check(L.lib().creid_topk_rows(L.ptr(distmat), m, n, n, k, L.ptr(idx), L.ptr(dsel), L.ptr(flags), L.stream()),
            "creid_topk_rows")
    bad = torch.nonzero(flags).flatten()
    if bad.numel():                                         # rows with massive ties at the k-th distance
        sub = distmat.index_select(0, bad).contiguous()
        ridx = rank_rows(sub)[:, :k].contiguous()
        idx.index_copy_(0, bad, ridx)
        dsel.index_copy_(0, bad, torch.gather(sub, 1, ridx))
    return idx, dsel


STREAM_TOPK_CAPACITY = 4096           # candidate slots per query (creid_stream_topk_collect: power of two, 64 .. 8192)
_STREAM_TOPK_CHUNK_BYTES = 256 << 20  # bound on every temporary of topk_stream (sample slice, candidate lists, repaired rows)


def topk_stream_sample(k: int, n: int) -> int:
    """Default threshold sample of topk_stream: S = clamp(max(ceil(k n / 1024), 1024), k, n) gallery rows.  The k-th smallest
    of S evenly strided columns sits near the (k n / S)-th smallest of the row, so a query collects about k n / S <= 1024
    candidates -- a quarter of the default capacity -- and the sample adds S / n ~ k / 1024 of the contraction."""
    return max(k, min(n, max(-(-k * n // 1024), 1024)))


def topk_stream(q: torch.Tensor, g: torch.Tensor, k: int, qq=None, gg=None, *, sample=None, capacity=None, stats=None,
                prefilter=None, g_pack=None, junk=None):
    """topk_rows(get_euclidean(q, g, qq, gg), k) -- (indices int64 [m, k], squared-L2 distances fp32 [m, k]), the same indices
    and the same distance bits, ties by gallery index -- WITHOUT the m x n matrix (fp32, bf16 or f16 features, q and g of one
    dtype, k <= min(n, 1024); 16-bit features run the contraction on the 16-bit MFMA and the threshold sample, the repair and
    the norms through the materialised kernels of the same dtype, so the bits are those of the 16-bit get_euclidean):
      1. threshold: `sample` gallery rows at a fixed stride (a gallery sorted by pid does not bias it) go through the
         materialised kernels; tau[row] = the k-th smallest of the m x sample slice.  The k-th smallest over ANY >= k columns
         bounds the row's true k-th distance from above, and both paths produce the same bits, so the bound is exact;
      2. creid_stream_topk_collect: the full contraction, tile by tile; every (distance <= tau[row], column) is appended to the
         row's candidate list (`capacity` slots);
      3. creid_stream_topk_select: sorts each list by (distance, index) and keeps the first k.
    Rows whose list overflowed (a loose threshold, massive ties) are flagged and redone through get_euclidean + topk_rows in
    bounded row chunks.  `stats` (a dict) receives sample, capacity, fallback_rows and max_candidates.
    prefilter = torch.bfloat16 | torch.float16 (fp32 q and g only; default None: everything above, untouched): the SAME result --
    the indices and distance bits of the fp32 path -- with the contraction on the 16-bit MFMA: see _topk_stream_prefilter.
    g_pack = prefilter_pack(g, prefilter) spares a gallery that is searched many times its rounding pass.
    junk = a JunkFilter over the m queries and the n gallery entries (default None: everything above, untouched): the ranked
    lists of the evaluation protocol -- per query the first k entries that are NOT junk (its own pid seen by its own camera, or
    by a camera set that holds it), in distance order, ties by gallery index: rank_keep_topk(rank_rows(get_euclidean(q, g)), k,
    junk) with the distances gathered, the same bits.  The same three stages: the junk cells of the sample slice are masked to
    +inf before the threshold is taken (a k-th value over junk columns could be too small), the contraction lists an entry
    only if it is not junk (creid_stream_topk_collect_keep), the select is unchanged.  A query with fewer than k non-junk
    entries gets those it has, then index -1 and distance +inf; such rows, like overflowed ones, are flagged and redone through
    get_euclidean + rank_rows + rank_keep_topk in bounded chunks, and count as fallback_rows.  CreidError with prefilter."""
    if junk is not None:
        if not isinstance(junk, JunkFilter):
            raise L.CreidError(f"topk_stream: junk must be a JunkFilter, got {type(junk).__name__}")
        if prefilter is not None or g_pack is not None:
            raise L.CreidError("topk_stream: junk= runs the plain streamed kernels: not with prefilter= (no banded junk test)")
    if q.dtype != g.dtype:
        raise L.CreidError(f"topk_stream needs q and g of one dtype (fp32, bf16 or f16), got {q.dtype} and {g.dtype}")
    L.require_gpu(q, g, qq, gg)
    if q.dtype not in (torch.float32,) + _H16 or q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1]:
        raise L.CreidError("topk_stream needs [m, D] and [n, D] features of one dtype: fp32, bf16 or f16")
    h16 = q.dtype in _H16
    if prefilter is None and g_pack is not None:
        raise L.CreidError("topk_stream: g_pack needs prefilter=torch.bfloat16 or torch.float16")
    if prefilter is not None and (prefilter not in _H16 or q.dtype != torch.float32):
        raise L.CreidError(f"topk_stream: prefilter must be torch.bfloat16 or torch.float16 on fp32 features, got {prefilter} on "
                           f"{q.dtype}")
    m, n, k = q.shape[0], g.shape[0], int(k)
    cap = STREAM_TOPK_CAPACITY if capacity is None else int(capacity)
    if not 1 <= k <= min(n, 1024, cap):
        raise L.CreidError(f"topk_stream: k = {k} outside 1 .. min(n = {n}, 1024, capacity = {cap})")
    S = topk_stream_sample(k, n) if sample is None else max(k, min(n, int(sample)))
    if junk is not None:
        junk.check_shape(m, n)
        L.require_gpu(junk.q_pids, junk.g_pids, junk.q_cams, junk.g_cams)
    if prefilter is not None:
        return _topk_stream_prefilter(q, g, k, qq, gg, prefilter, g_pack, S, cap, stats)
    qq = row_sqnorm(q) if qq is None else qq
    gg = row_sqnorm(g) if gg is None else gg
    q, g = _pad_width(q, 8 if h16 else 4), _pad_width(g, 8 if h16 else 4)
    gs, ggs, js = _topk_sample(g, gg, S, junk)
    idx, dsel, flags, count = _topk_outputs(m, k, q.device)
    step = _topk_chunk_rows(cap, S)
    for r0 in range(0, m, step):
        r1 = min(m, r0 + step)
        qc, qqc = q[r0:r1], qq[r0:r1]
        jc = None if junk is None else junk.rows(slice(r0, r1))
        ds = get_euclidean(qc, gs, qqc, ggs)
        if junk is not None:
            # the k-th smallest over the sample's NON-junk columns: an upper bound of the k-th smallest non-junk distance
            L.check(L.lib().creid_junk_mask_rows(L.ptr(ds), r1 - r0, S, S, L.ptr(jc.q_pids), L.ptr(js.g_pids), L.ptr(jc.q_cams),
                                                 L.ptr(js.g_cams), 1 if junk.camsets else 0, L.stream()), "creid_junk_mask_rows")
        tau = topk_rows(ds, k)[1][:, k - 1].contiguous()
        del ds
        cand = torch.empty((r1 - r0, cap), dtype=torch.int64, device=q.device)
        _topk_collect(qc, g, qqc, gg, tau, cap, cand, count[r0:r1], jc)
        L.check(L.lib().creid_stream_topk_select(L.ptr(cand), L.ptr(count[r0:r1]), r1 - r0, cap, k, L.ptr(idx[r0:r1]),
                                                 L.ptr(dsel[r0:r1]), L.ptr(flags[r0:r1]), L.stream()), "creid_stream_topk_select")
        del tau, cand
    bad = _topk_stream_repair(q, g, k, qq, gg, flags, idx, dsel, junk)
    if stats is not None:
        stats.update(_topk_stats(S, cap, bad, count))
    return idx, dsel


# The pieces the plain and the pre-filtered driver of topk_stream share.
def _topk_outputs(m, k, device):
    """idx int64 [m, k], dsel fp32 [m, k], and -- zeroed -- flags u8 [m] (rows to repair), count i32 [m] (entries listed)."""
    return (torch.empty((m, k), dtype=torch.int64, device=device), torch.empty((m, k), dtype=torch.float32, device=device),
            torch.zeros(m, dtype=torch.uint8, device=device), torch.zeros(m, dtype=torch.int32, device=device))


def _topk_chunk_rows(cap, S):
    """Query rows per chunk: the candidate lists (cap x 8 bytes a row) and the sample slice (S x 4) inside
    _STREAM_TOPK_CHUNK_BYTES, in whole query tiles of 64 rows and at least one."""
    return max(64, _STREAM_TOPK_CHUNK_BYTES // (max(cap * 8, S * 4)) // 64 * 64)


def _topk_sample(g, gg, S, junk=None):
    """The threshold sample: gallery rows 0, stride, 2 stride, ... (S of them), their norms, and junk's filter against them."""
    stride = g.shape[0] // S
    return g[::stride][:S].contiguous(), gg[::stride][:S].contiguous(), None if junk is None else junk.gallery_slice(stride, S)


def _topk_collect(q, g, qq, gg, thr, cap, cand, count, junk=None):
    """creid_stream_topk_collect[_keep][_h16], by the operands' dtype and the filter: every (distance <= thr[row], column) --
    with junk (the filter of THESE query rows): that is not junk -- into the row's list cand [rows, cap]; count += entries."""
    h16 = q.dtype in _H16
    name = "creid_stream_topk_collect" + ("_keep" if junk is not None else "") + ("_h16" if h16 else "")
    dt = (L.dtype_code(q),) if h16 else ()
    keep = () if junk is None else (L.ptr(junk.q_pids), L.ptr(junk.g_pids), L.ptr(junk.q_cams), L.ptr(junk.g_cams),
                                    1 if junk.camsets else 0)
    L.check(getattr(L.lib(), name)(L.ptr(q), L.ptr(g), L.ptr(qq), L.ptr(gg), q.shape[0], g.shape[0], q.shape[1], *dt, L.ptr(thr),
                                   *keep, cap, L.ptr(cand), L.ptr(count), L.stream()), name)


def _topk_stats(S, cap, bad, count):
    return dict(sample=S, capacity=cap, fallback_rows=bad, max_candidates=int(count.max().item()) if count.numel() else 0)


def _topk_stream_repair(q, g, k, qq, gg, flags, idx, dsel, junk=None) -> int:
    """The flagged rows of topk_stream (overflowed lists, NaN rows; with a pre-filter also rows that keep too many entries; with
    junk also rows with fewer than k non-junk entries) redone through the materialised kernels in bounded row chunks, into
    idx / dsel; returns their number.  Plain: get_euclidean + topk_rows; junk: get_euclidean + rank_rows + rank_keep_topk, the
    distances gathered (+inf in the padding)."""
    bad = torch.nonzero(flags).flatten()
    # per gallery entry a row holds its distance -- with junk also its ranked index and the rank's share
    rows = max(1, _STREAM_TOPK_CHUNK_BYTES // (g.shape[0] * (4 if junk is None else 16)))
    for b0 in range(0, bad.numel(), rows):
        sel = bad[b0:b0 + rows]
        d = get_euclidean(q.index_select(0, sel), g, qq.index_select(0, sel), gg)
        if junk is None:
            ridx, rd = topk_rows(d, k)
        else:
            ridx = rank_keep_topk(rank_rows(d), k, junk.rows(sel))[0]
            rd = gather_ranked(d, ridx)
        idx.index_copy_(0, sel, ridx)
        dsel.index_copy_(0, sel, rd)
        del d, ridx, rd
    return int(bad.numel())


def _topk_stream_repair_keep(q, g, k, qq, gg, flags, idx, dsel, junk) -> int:
    return _topk_stream_repair(q, g, k, qq, gg, flags, idx, dsel, junk)


class JunkFilter:
    """The labels the evaluation protocol filters a ranked list with (utils/eval_reid.py:49-58, utils/visrank.py:193-232), as
    int64 tensors: gallery entry j is JUNK for query i when g_pids[j] == q_pids[i] and its camera test holds -- plain camera
    ids: g_cams[j] == q_cams[i]; camsets=True: g_cams[j] is a bitmask of cameras (bit c = camera c, 0..62) and bit q_cams[i]
    is set.  What CMC / mAP drop per query, and what rank_keep_topk / topk_stream(junk=...) / R1_mAP(ranked_topk=...) leave
    out of the ranked lists."""

    def __init__(self, q_pids, q_cams, g_pids, g_cams, camsets=False):
        dev = next((a.device for a in (q_pids, q_cams, g_pids, g_cams) if isinstance(a, torch.Tensor)), torch.device("cpu"))
        self.q_pids, self.q_cams, self.g_pids, self.g_cams = (_dev_i64(a, dev) for a in (q_pids, q_cams, g_pids, g_cams))
        self.camsets = bool(camsets)
        if self.q_pids.dim() != 1 or self.g_pids.dim() != 1 or self.q_cams.shape != self.q_pids.shape or \
                self.g_cams.shape != self.g_pids.shape:
            raise L.CreidError("JunkFilter needs one pid and one camera (or camera-set mask) per query and per gallery entry, got "
                               f"{tuple(self.q_pids.shape)}, {tuple(self.q_cams.shape)}, {tuple(self.g_pids.shape)}, "
                               f"{tuple(self.g_cams.shape)}")

    @classmethod
    def from_labels(cls, pids, camids, num_query, device, respect_camids=False):
        """pids / camids as R1_mAP.compute receives them: [nq + ng] vectors (lists, numpy, tensors), queries first; with
        respect_camids=True camids is a list of camera-id lists ([c] for a query) or a CameraSets, whose device masks and query
        cameras are used as they are.  Camera ids beyond 62 with sets: CreidError."""
        nq = int(num_query)
        p = pids if isinstance(pids, torch.Tensor) else np.asarray(pids)
        if respect_camids:
            q_cams, g_masks = _camset_split(camids, nq)
            return cls(_dev_i64(p[:nq], device), _dev_i64(q_cams, device), _dev_i64(p[nq:], device), _dev_i64(g_masks, device),
                       camsets=True)
        c = camids if isinstance(camids, torch.Tensor) else np.asarray(camids)
        return cls(_dev_i64(p[:nq], device), _dev_i64(c[:nq], device), _dev_i64(p[nq:], device), _dev_i64(c[nq:], device))

    def check_shape(self, m, n):
        if self.q_pids.shape[0] != m or self.g_pids.shape[0] != n:
            raise L.CreidError(f"JunkFilter of {self.q_pids.shape[0]} queries x {self.g_pids.shape[0]} gallery entries on "
                               f"{m} x {n} rows")

    def rows(self, sel):
        """The filter of the queries `sel` (a slice or an index tensor) against the same gallery."""
        out = JunkFilter.__new__(JunkFilter)
        take = (lambda a: a[sel].contiguous()) if isinstance(sel, slice) else (lambda a: a.index_select(0, sel))
        out.q_pids, out.q_cams, out.g_pids, out.g_cams, out.camsets = take(self.q_pids), take(self.q_cams), self.g_pids, \
            self.g_cams, self.camsets
        return out

    def gallery_slice(self, stride, count):
        """The filter of the same queries against gallery entries 0, stride, 2 stride, ... (`count` of them)."""
        out = JunkFilter.__new__(JunkFilter)
        out.q_pids, out.q_cams, out.camsets = self.q_pids, self.q_cams, self.camsets
        out.g_pids, out.g_cams = self.g_pids[::stride][:count].contiguous(), self.g_cams[::stride][:count].contiguous()
        return out

    def matched(self, idx):
        """g_pids[idx] == the row's pid for a list of ranked indices [m, k]; False where idx is the padding (-1)."""
        real = idx >= 0
        return (self.g_pids[idx.clamp(min=0)] == self.q_pids[:, None]) & real


def rank_keep_topk(indices: torch.Tensor, k: int, junk: JunkFilter):
    """From ranked gallery indices int64 [m, n] (rank_rows) the first k entries of every row that are not junk, in order:
    (idx int64 [m, k] padded with -1, matched bool [m, k]: the entry has the query's pid, count int32 [m]: the real entries).
    creid_rank_keep_topk: one wave per query, no atomics.  1 <= k <= 1024."""
    L.require_gpu(indices, junk.q_pids, junk.g_pids, junk.q_cams, junk.g_cams)
    if indices.dtype != torch.int64 or indices.dim() != 2:
        raise L.CreidError("rank_keep_topk needs ranked indices int64 [m, n]")
    m, n = indices.shape
    k = int(k)
    if not 1 <= k <= 1024:
        raise L.CreidError(f"rank_keep_topk: k = {k} outside 1 .. 1024")
    if junk.q_pids.shape[0] != m:
        raise L.CreidError(f"rank_keep_topk: {m} ranked rows but a JunkFilter of {junk.q_pids.shape[0]} queries")
    indices = indices.contiguous()
    dev = indices.device
    idx = torch.empty((m, k), dtype=torch.int64, device=dev)
    matched = torch.empty((m, k), dtype=torch.uint8, device=dev)
    count = torch.empty(m, dtype=torch.int32, device=dev)
    L.check(L.lib().creid_rank_keep_topk(L.ptr(indices), m, n, junk.g_pids.shape[0], k, L.ptr(junk.q_pids), L.ptr(junk.g_pids),
                                         L.ptr(junk.q_cams), L.ptr(junk.g_cams), 1 if junk.camsets else 0, L.ptr(idx),
                                         L.ptr(matched), L.ptr(count), L.stream()), "creid_rank_keep_topk")
    return idx, matched.bool(), count


def gather_ranked(distmat: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """distmat[i, idx[i, :]] for ranked lists padded with -1: +inf in the padding."""
    return torch.gather(distmat, 1, idx.clamp(min=0)).masked_fill_(idx < 0, float("inf"))


# --------------------------------------------------------------------------- open-set operating points (TAR @ FAR)
ROC_DEFAULT_FAR = (1e-4, 1e-3, 1e-2)
ROC_MAX_RATES = 16
_ROC_PASSES = ((0, 11), (11, 11), (22, 10))     # (prefix bits, digit bits) of the three radix passes over a 32-bit key
_ROC_GROUP = 4                                  # targets that share a pass: 4 x 2^11 bins is the LDS table of the kernels


def key_to_distance(key):
    """The fp32 value whose order-preserving key (mono_key of csrc/stream_common.hpp) is `key` (numpy uint32)."""
    key = np.asarray(key, dtype=np.uint32)
    bits = np.where(key & np.uint32(0x80000000), key ^ np.uint32(0x80000000), ~key)
    return bits.astype(np.uint32).view(np.float32)


def _hist_args(junk: JunkFilter, m, n, prefix, prefix_bits, bits, out, device):
    junk.check_shape(m, n)
    L.require_gpu(junk.q_pids, junk.g_pids, junk.q_cams, junk.g_cams)
    prefix_bits, bits = int(prefix_bits), int(bits)
    if prefix_bits == 0:
        nsel, prefix = 1, None
    else:
        if prefix is None:
            raise L.CreidError("distance_histogram: prefix_bits > 0 needs the selectors' prefixes")
        if not (isinstance(prefix, torch.Tensor) and prefix.is_cuda and prefix.dtype == torch.int32):
            p = prefix.cpu().numpy() if isinstance(prefix, torch.Tensor) else np.asarray(prefix)
            prefix = torch.from_numpy(p.astype(np.uint32).view(np.int32).reshape(-1)).to(device)    # the uint32 words, as int32
        prefix = prefix.contiguous()
        nsel = prefix.numel()
    if not 1 <= bits <= 11 or prefix_bits < 0 or prefix_bits + bits > 32 or nsel < 1 or (nsel << bits) > 8192:
        raise L.CreidError(f"distance_histogram: bits = {bits}, prefix_bits = {prefix_bits}, {nsel} selectors outside 1 <= bits <= 11, "
                           "prefix_bits + bits <= 32, selectors x 2^bits <= 8192")
    shape = (nsel, 2, 1 << bits)
    if out is None:
        out = torch.zeros(shape, dtype=torch.int64, device=device)
    elif tuple(out.shape) != shape or out.dtype != torch.int64 or not out.is_cuda or not out.is_contiguous():
        raise L.CreidError(f"distance_histogram: out must be a contiguous int64 device tensor {shape}, got {tuple(out.shape)} {out.dtype}")
    labels = (L.ptr(junk.q_pids), L.ptr(junk.g_pids), L.ptr(junk.q_cams), L.ptr(junk.g_cams), 1 if junk.camsets else 0)
    return labels, (L.ptr(prefix), nsel, prefix_bits, bits, L.ptr(out), L.stream()), out


def distance_histogram(q: torch.Tensor, g: torch.Tensor, junk: JunkFilter, qq=None, gg=None, *, prefix=None, prefix_bits=0, bits=11,
                       out=None) -> torch.Tensor:
    """One radix pass over the distance keys of every query x gallery pair the evaluation protocol keeps, with NO m x n matrix
    (creid_stream_dist_hist[_h16]: the streamed contraction with a counting epilogue).  key(i, j) is the order-preserving
    32-bit key of the squared L2 distance get_euclidean(q, g, qq, gg) holds for the pair, bit for bit (fp32, bf16 or f16 rows).
    A pair that is junk (`junk`, the JunkFilter of these rows) counts nowhere; else it is genuine (class 0: the query's pid) or
    an impostor (class 1).  For selector s the pair counts when prefix_bits == 0 or key >> (32 - prefix_bits) == prefix[s], in
    bin (key >> (32 - prefix_bits - bits)) & (2^bits - 1).  Returns int64 [nsel, 2, 2^bits] on the device (nsel = len(prefix),
    1 without prefix bits); with out= the counts are ADDED into it, so calls over chunks of the queries accumulate.  Integer
    atomics only: two runs, and both work splits, give the same counts.  NaN distances are outside the contract (they are
    counted under whatever key their bits give)."""
    L.require_gpu(q, g)
    if q.dim() != 2 or g.dim() != 2 or q.dtype != g.dtype or q.shape[1] != g.shape[1] or q.dtype not in (torch.float32,) + _H16:
        raise L.CreidError("distance_histogram needs fp32, bf16 or f16 rows [m, D] and [n, D] of one dtype")
    qq = row_sqnorm(q) if qq is None else qq
    gg = row_sqnorm(g) if gg is None else gg
    m, n, D = q.shape[0], g.shape[0], q.shape[1]
    labels, tail, out = _hist_args(junk, m, n, prefix, prefix_bits, bits, out, q.device)
    h16 = q.dtype in _H16
    name = "creid_stream_dist_hist" + ("_h16" if h16 else "")
    dt = (L.dtype_code(q),) if h16 else ()
    L.check(getattr(L.lib(), name)(L.ptr(q), L.ptr(g), L.ptr(qq), L.ptr(gg), m, n, D, *dt, *labels, *tail), name)
    return out


def distance_histogram_matrix(distmat: torch.Tensor, junk: JunkFilter, *, prefix=None, prefix_bits=0, bits=11, out=None) -> torch.Tensor:
    """distance_histogram over an existing fp32 matrix [m, n] (creid_dist_hist_matrix): the keys of its entries, whatever
    distance they hold."""
    L.require_gpu(distmat)
    if distmat.dtype != torch.float32 or distmat.dim() != 2:
        raise L.CreidError("distance_histogram_matrix needs a dense fp32 matrix [m, n]")
    m, n = distmat.shape
    labels, tail, out = _hist_args(junk, m, n, prefix, prefix_bits, bits, out, distmat.device)
    L.check(L.lib().creid_dist_hist_matrix(L.ptr(distmat), m, n, *labels, *tail), "creid_dist_hist_matrix")
    return out


def roc_rates(far):
    """The target false-accept rates of roc_stream / roc_matrix / R1_mAP(roc=...) as a tuple of floats: True = ROC_DEFAULT_FAR;
    CreidError for a rate outside (0, 1], for none and for more than ROC_MAX_RATES."""
    if far is True:
        return ROC_DEFAULT_FAR
    try:
        rates = tuple(float(f) for f in ([far] if isinstance(far, (int, float)) and not isinstance(far, bool) else far))
    except (TypeError, ValueError):
        raise L.CreidError(f"roc: the target rates must be numbers in (0, 1], got {far!r}") from None
    if not 1 <= len(rates) <= ROC_MAX_RATES:
        raise L.CreidError(f"roc: 1 .. {ROC_MAX_RATES} target rates, got {len(rates)}")
    for f in rates:
        if not 0.0 < f <= 1.0:                                      # (NaN fails both comparisons)
            raise L.CreidError(f"roc: target rate {f!r} outside (0, 1]")
    return rates


def _roc_select(pass_fn, far, device, first_hist=None, stats=None):
    """The radix select behind roc_stream / roc_matrix.  pass_fn(prefix, prefix_bits, bits, out) adds one pass's counts into
    out; first_hist: the first pass's counts int64 [1, 2, 2048] when the caller has accumulated them already.  Per group of
    four targets: three passes and three select steps (creid_roc_descend), all enqueued; one read-back at the end."""
    rates = roc_rates(far)
    lib = L.lib()
    pb0, bits0 = _ROC_PASSES[0]
    hist0 = first_hist
    launches = 0
    if hist0 is None:
        hist0 = torch.zeros((1, 2, 1 << bits0), dtype=torch.int64, device=device)
        pass_fn(None, pb0, bits0, hist0)
        launches += 1
    states = []
    for t0 in range(0, len(rates), _ROC_GROUP):
        grp = rates[t0:t0 + _ROC_GROUP]
        nt = len(grp)
        far_d = torch.tensor(grp, dtype=torch.float64).to(device)
        state = torch.zeros((nt, 8), dtype=torch.int64, device=device)
        prefix = torch.zeros(nt, dtype=torch.int32, device=device)
        hist = hist0
        for level, (pb, bits) in enumerate(_ROC_PASSES):
            if level > 0:
                hist = torch.zeros((nt, 2, 1 << bits), dtype=torch.int64, device=device)
                pass_fn(prefix, pb, bits, hist)
                launches += 1
            L.check(lib.creid_roc_descend(L.ptr(hist), nt, bits, level, L.ptr(far_d), L.ptr(state), L.ptr(prefix), L.stream()),
                    "creid_roc_descend")
        states.append(state)
    back = torch.cat([s.flatten() for s in states] + [hist0.flatten()]).cpu().numpy()      # the one host synchronisation
    st = back[:8 * len(rates)].reshape(len(rates), 8)
    h0 = back[8 * len(rates):].reshape(2, 1 << bits0)
    if (st[:, 7] & 1).any():
        raise L.CreidError("roc: no impostor pair (every gallery entry has its query's pid, or the sets are empty): a false-accept "
                           "rate is undefined")
    if (st[:, 7] & 2).any() or ((st[:, 7] >> 8) & 0xff != 32).any():
        raise L.CreidError("roc: the passes' counts do not add up (the distances or labels changed between the passes)")
    fa, ta, n_imp, n_gen = st[:, 2], st[:, 3], st[:, 4], st[:, 5]
    with np.errstate(invalid="ignore", divide="ignore"):
        tar = np.where(n_gen > 0, ta / np.maximum(n_gen, 1).astype(np.float64), np.nan)
    if stats is not None:
        stats.update(passes=launches, groups=len(states))
    edges = key_to_distance(np.arange(1 << bits0, dtype=np.uint32) << np.uint32(32 - bits0))
    return dict(target=np.asarray(rates, dtype=np.float64), threshold=key_to_distance(st[:, 6].astype(np.uint32)),
                false_accepts=fa.copy(), true_accepts=ta.copy(), n_impostor=n_imp.copy(), n_genuine=n_gen.copy(),
                far=fa / n_imp.astype(np.float64), tar=tar, hist=h0.copy(), edges=edges)


def roc_stream(q: torch.Tensor, g: torch.Tensor, junk: JunkFilter, far=ROC_DEFAULT_FAR, qq=None, gg=None, *, stats=None) -> dict:
    """Open-set operating points of a query set against a gallery with NO m x n matrix: for every target false-accept rate f
    the exact distance threshold, by a three-pass radix select on the keys distance_histogram counts.
    Pair classes: junk (what `junk` drops: the query's pid seen by its camera, or by a camera set that holds it) belongs to no
    class; genuine = the same pid and not junk; impostor = another pid.  With N_imp / N_gen the class sizes,
    k = min(floor(f * N_imp), N_imp - 1) and tau = the impostor distance of 0-based rank k in ascending order, a pair is
    ACCEPTED iff its distance is STRICTLY below tau, so false_accepts <= k whatever the ties.  Distances compare by the bits
    get_euclidean(q, g, qq, gg) gives them in the rows' dtype (fp32, bf16 or f16).
    Returns numpy arrays with one entry per target: target (the rates asked for), threshold (fp32, tau in the matrix's own unit
    -- SQUARED L2 here), false_accepts, true_accepts, n_impostor, n_genuine (int64), far = false_accepts / N_imp, tar =
    true_accepts / N_gen (nan when there is no genuine pair); and hist int64 [2, 2048] (genuine, impostor), edges fp32 [2048]:
    the first pass's counts and the lowest distance of each of its bins (an exact, coarse pair of distributions; the bins of
    NaN bit patterns have NaN edges).  CreidError when there is no impostor pair, for a rate outside (0, 1] and for more than
    16 rates.  Up to four targets share the three contractions; the only host synchronisation is the final read-back.  NaN
    distances are outside the contract."""
    qq = row_sqnorm(q) if qq is None else qq
    gg = row_sqnorm(g) if gg is None else gg
    return _roc_select(lambda prefix, pb, bits, out: distance_histogram(q, g, junk, qq, gg, prefix=prefix, prefix_bits=pb, bits=bits,
                                                                        out=out), far, q.device, stats=stats)


def roc_matrix(distmat: torch.Tensor, junk: JunkFilter, far=ROC_DEFAULT_FAR, *, stats=None) -> dict:
    """roc_stream over an existing fp32 matrix [m, n] (cosine, re-ranked, or any other distance): the same definitions on its
    entries; threshold is in the matrix's own unit."""
    return _roc_select(lambda prefix, pb, bits, out: distance_histogram_matrix(distmat, junk, prefix=prefix, prefix_bits=pb, bits=bits,
                                                                               out=out), far, distmat.device, stats=stats)


STREAM_RESCORE_CAPACITY = 1024        # entries of one query creid_stream_topk_rescore re-scores (RS_CAP, csrc/stream_prefilter.hip)
_PREFILTER_INFLATE = 2.0 ** -20       # relative inflation of the margin: covers the float64 arithmetic it is computed with


class PrefilterPack:
    """prefilter_pack's result: `rounded` [r, D8] (the rows rounded once to `dtype`, the width zero-padded to a multiple of 8),
    `stats` float64 [r, 3] = per row |x - xh|^2, |xh|^2, |x|^2, and the `width` of the fp32 rows it was made from."""

    def __init__(self, rounded, stats, width):
        self.rounded, self.stats, self.width, self._maxima = rounded, stats, width, None

    @property
    def dtype(self):
        return self.rounded.dtype

    def maxima(self):
        """The gallery side of prefilter_margin: the column maxima of `stats` as three Python floats (NaN / inf when a row's
        statistics are not finite); one device read, cached."""
        if self._maxima is None:
            self._maxima = tuple(self.stats.amax(dim=0).tolist()) if self.stats.shape[0] else (0.0, 0.0, 0.0)
        return self._maxima


def prefilter_pack(x: torch.Tensor, dtype) -> PrefilterPack:
    """One pass over fp32 rows [r, D] (creid_prefilter_pack): the bf16 / f16 copy -- the bits of x.to(dtype) -- and the per-row sums
    the margin of topk_stream(prefilter=dtype) is computed from, accumulated in double."""
    L.require_gpu(x)
    if dtype not in _H16 or x.dtype != torch.float32 or x.dim() != 2:
        raise L.CreidError(f"prefilter_pack needs fp32 [r, D] rows and torch.bfloat16 or torch.float16, got {x.dtype} and {dtype}")
    width = x.shape[1]
    x = _pad_width(x, 8)
    r, D = x.shape
    y = torch.empty((r, D), dtype=dtype, device=x.device)
    st = torch.empty((r, 3), dtype=torch.float64, device=x.device)
    L.check(L.lib().creid_prefilter_pack(L.ptr(x), r, D, L._DT[dtype], L.ptr(y), L.ptr(st), L.stream()), "creid_prefilter_pack")
    return PrefilterPack(y, st, width)


def prefilter_margin(e2, h2, x2, g_e2, g_h2, g_x2, g_sq, D, parts=False):
    """m_i with |dh_ij - d_ij| <= m_i for every gallery row j, where d is the fp32 distance kernels' value on rows (q_i, g_j) and
    dh the 16-bit kernels' value on the rows rounded once to bf16 / f16 (qh, gh), both with the SAME norm arguments qq_i, gg_j.
    A pure function (numpy arrays, tensors or floats; float64 expected):
      e2, h2, x2        per query row |q - qh|^2, |qh|^2, |q|^2 (the columns of PrefilterPack.stats); x2 also stands for |qq_i|;
      g_e2, g_h2, g_x2  the gallery's maxima of the same three sums;  g_sq >= every |gg_j|;  D the feature width.
    With e = sqrt(e2), Qh = sqrt(h2), Q = sqrt(x2), E, Gh, G the gallery's, u = 2^-24:
      data       = 2 (e G + Qh E)            the exact effect of rounding the operands: |q.g - qh.gh| <= |q - qh||g| + |qh||g - gh|
                                             (Cauchy-Schwarz), doubled by the epilogue's -2;
      arithmetic = 2 D u (Qh Gh + Q G)       the two accumulators: the rule 2 D u sum |q_k||g_k| of tests/eval_exact.py per kernel
                 + 2 u (x2 + g_sq)           the rounding of qq + gg, once per kernel
                 + u (x2 + g_sq + 2 Q G) + u (x2 + g_sq + 2 Qh Gh)      the final fma of either kernel, u |d|.
    The data part comes from the rows themselves, so f16 subnormals, underflow to zero and un-normalised features are covered;
    non-finite statistics give a non-finite margin.  Every term is non-negative and non-decreasing in every argument.
    parts=True returns (data, arithmetic) instead of their sum."""
    def sqrt(v):
        return torch.sqrt(v) if isinstance(v, torch.Tensor) else np.sqrt(v)
    u = 2.0 ** -24
    e, Qh, Q = sqrt(e2), sqrt(h2), sqrt(x2)
    E, Gh, G = sqrt(g_e2), sqrt(g_h2), sqrt(g_x2)
    data = 2.0 * (e * G + Qh * E)
    arith = 2.0 * D * u * (Qh * Gh + Q * G) + 2.0 * u * (x2 + g_sq) + u * (x2 + g_sq + 2.0 * Q * G) + u * (x2 + g_sq + 2.0 * Qh * Gh)
    return (data, arith) if parts else data + arith


def _round_up_f32(x64: torch.Tensor) -> torch.Tensor:
    """fp32 values never below the float64 ones (inf and NaN stay)."""
    f = x64.to(torch.float32)
    return torch.where(f.double() < x64, torch.nextafter(f, torch.full_like(f, float("inf"))), f)


def _topk_stream_prefilter(q, g, k, qq, gg, dtype, g_pack, S, cap, stats):
    """topk_stream on fp32 features with the contraction on the 16-bit MFMA and the result of the fp32 path, bit for bit.
    d: the fp32 distance; dh: the 16-bit streamed kernel's distance on the rows rounded once to `dtype`, given the fp32 rows' own
    qq / gg, so that only the dot product differs; m_i = prefilter_margin >= |dh - d| over row i.
      1. the k pairs of smallest dh have d <= dh_(k) + m_i, so the true k-th distance d_(k) <= dh_(k) + m_i;
      2. every pair of the true top-k, those tied at d_(k) included, has d <= d_(k), hence dh <= dh_(k) + 2 m_i;
      3. the pairs within that cut, re-scored with the fp32 bits and sorted by (d, j), give exactly the fp32 result.
    Stages, in the bounded row chunks of the fp32 path: creid_prefilter_pack of the query chunk (the gallery's once, or the
    caller's g_pack); tau_i = the k-th smallest dh over the strided gallery sample through the materialised 16-bit kernel with the
    same norms (same bits as the streamed one, so tau_i >= dh_(k)); creid_stream_topk_collect_h16 with the threshold
    tau_i + 2 m_i; creid_stream_topk_rescore, which finds dh_(k) in the list, keeps dh <= dh_(k) + 2 m_i and re-scores.
    Roundings between the statistics and the two thresholds: the statistics are double sums of exact terms (relative error below
    (D + 6) 2^-53) and prefilter_margin is a few dozen float64 operations on non-negative terms -- together far below the stated
    inflation 1 + 2^-20; 2 m_i is then rounded UP to fp32 (margin2); the collect threshold is the fp32 sum tau_i + margin2_i moved
    one step up, the kernel's cut the fp32 sum dh_(k) + margin2_i moved one step up: neither is below the real sum.
    Rows the kernel flags (list overflow, fewer than k entries, more than STREAM_RESCORE_CAPACITY kept, a margin that is not
    finite) are redone through get_euclidean + topk_rows on the fp32 tensors like the fp32 path's; a gallery whose statistics are
    not finite (f16 overflow, Inf / NaN) sends the whole call down the fp32 path (stats["prefilter"] is then None).
    stats receives sample, capacity, fallback_rows, max_candidates, prefilter (what ran), max_rescored (the most entries a row
    kept), rescore_capacity, margin_max, kept (int32 [m] on the device: entries kept per row) and -- when it comes in holding
    timing=True -- stage_ms (pack_g, pack_q, sample, collect, rescore, repair, between device events)."""
    m, n = q.shape[0], g.shape[0]
    width = g.shape[1]
    clock = _StageClock(bool(stats) and bool(stats.get("timing")))
    qq = row_sqnorm(q) if qq is None else qq
    gg = row_sqnorm(g) if gg is None else gg
    if g_pack is None:
        g_pack = prefilter_pack(g, dtype)
    elif not isinstance(g_pack, PrefilterPack) or g_pack.dtype != dtype or g_pack.rounded.shape[0] != n or g_pack.width != width:
        raise L.CreidError(f"topk_stream: g_pack is not prefilter_pack(g, {dtype}) of this [{n}, {width}] gallery")
    g_e2, g_h2, g_x2 = g_pack.maxima()
    g_sq = max(g_x2, float(gg.abs().amax().item()))
    if not all(np.isfinite(v) for v in (g_e2, g_h2, g_x2, g_sq)):
        info = {}
        out = topk_stream(q, g, k, qq, gg, sample=S, capacity=cap, stats=info)
        if stats is not None:
            stats.update(info, prefilter=None, max_rescored=0, rescore_capacity=STREAM_RESCORE_CAPACITY, margin_max=float("inf"))
        return out
    q, g = _pad_width(q, 8), _pad_width(g, 8)       # zero columns change neither a norm, a rounding nor an fmaf chain
    gh = g_pack.rounded
    D, dev = q.shape[1], q.device
    clock.mark("pack_g")
    ghs, ggs, _ = _topk_sample(gh, gg, S)
    idx, dsel, flags, count = _topk_outputs(m, k, dev)
    kept = torch.zeros(m, dtype=torch.int32, device=dev)
    margin = torch.empty(m, dtype=torch.float64, device=dev)
    up = torch.tensor(float("inf"), dtype=torch.float32, device=dev)
    step = _topk_chunk_rows(cap, S)
    for r0 in range(0, m, step):
        r1 = min(m, r0 + step)
        qc, qqc = q[r0:r1], qq[r0:r1]
        qp = prefilter_pack(qc, dtype)
        x2 = torch.maximum(qp.stats[:, 2], qqc.abs().double())
        mc = prefilter_margin(qp.stats[:, 0], qp.stats[:, 1], x2, g_e2, g_h2, g_x2, g_sq, D)
        margin[r0:r1] = mc
        margin2 = _round_up_f32(2.0 * (1.0 + _PREFILTER_INFLATE) * mc)
        clock.mark("pack_q")
        tau = topk_rows(get_euclidean(qp.rounded, ghs, qqc, ggs), k)[1][:, k - 1]
        thr = torch.nextafter(tau + margin2, up.expand_as(tau)).contiguous()
        cand = torch.empty((r1 - r0, cap), dtype=torch.int64, device=dev)
        clock.mark("sample")
        _topk_collect(qp.rounded, gh, qqc, gg, thr, cap, cand, count[r0:r1])
        clock.mark("collect")
        L.check(L.lib().creid_stream_topk_rescore(L.ptr(cand), L.ptr(count[r0:r1]), r1 - r0, cap, k, L.ptr(qc), L.ptr(g), L.ptr(qqc),
                                                  L.ptr(gg), n, D, L.ptr(margin2), L.ptr(idx[r0:r1]), L.ptr(dsel[r0:r1]),
                                                  L.ptr(flags[r0:r1]), L.ptr(kept[r0:r1]), L.stream()), "creid_stream_topk_rescore")
        clock.mark("rescore")
        del qp, tau, thr, cand, margin2
    bad = _topk_stream_repair(q, g, k, qq, gg, flags, idx, dsel)      # the fp32 path's repair, on the fp32 tensors
    clock.mark("repair")
    if stats is not None:
        if clock.on:                                        # per stage, summed over the row chunks
            stats["stage_ms"] = clock.stage_ms()
        stats.update(_topk_stats(S, cap, bad, count),
                     prefilter=dtype, max_rescored=int(kept.max().item()) if m else 0, rescore_capacity=STREAM_RESCORE_CAPACITY,
                     margin_max=float(margin.max().item()) if m else 0.0, kept=kept)
    return idx, dsel


RERANK_DEFAULTS = dict(k1=20, k2=6, lambda_value=0.3)
_RERANK_LDS = 64 << 10                # dynamic LDS of every csrc/rerank.hip kernel


def rerank_options(reranking):
    """The `reranking=` argument of R1_mAP / get_similar: False / None -> None; True -> the defaults of re_ranking; a dict of
    k1 / k2 / lambda_value -> those over the defaults."""
    if reranking is None or reranking is False:
        return None
    if reranking is True:
        return dict(RERANK_DEFAULTS)
    if isinstance(reranking, dict) and set(reranking) <= set(RERANK_DEFAULTS):
        return {**RERANK_DEFAULTS, **reranking}
    raise L.CreidError(f"reranking must be False, True or a dict of k1 / k2 / lambda_value, got {reranking!r}")


def _pow2_at_least(v: int) -> int:
    p = 1
    while p < v:
        p *= 2
    return p


def _csr_from_counts(count: torch.Tensor) -> torch.Tensor:
    rowptr = torch.zeros(count.shape[0] + 1, dtype=torch.int64, device=count.device)
    rowptr[1:] = torch.cumsum(count, 0, dtype=torch.int64)
    return rowptr


class _StageClock:
    """Device events at stage boundaries (only when asked for: stats={"timing": True}); the host's waits between two marks
    fall inside the stage that caused them, so the stages add up to the call."""

    def __init__(self, on):
        self.on, self.marks = on, []
        self.mark("start")

    def mark(self, name):
        if self.on:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.marks.append((name, ev))

    def stage_ms(self):
        """Milliseconds per stage name; marks that share a name (row chunks, both normalisations of an expansion round, a
        redone speculation) are summed."""
        self.marks[-1][1].synchronize()
        ms = {}
        for (_, prev), (name, ev) in zip(self.marks, self.marks[1:]):
            ms[name] = ms.get(name, 0.0) + prev.elapsed_time(ev)
        return ms


def re_ranking(q: torch.Tensor, g: torch.Tensor, k1: int = 20, k2: int = 6, lambda_value: float = 0.3, *, stats=None,
               debug=None, prefilter=None) -> torch.Tensor:
    """k-reciprocal re-ranking (Zhong et al., CVPR 2017) of fp32 device features q [nq, D], g [ng, D]: the fp32 [nq, ng]
    matrix (1 - lambda) * Jaccard + lambda * d / max_row(d), to be ranked like a distance matrix -- with no N x N matrix
    (N = nq + ng) at any point: the only [nq, ng] tensors are the result and get_euclidean(q, g).

    X = cat(q, g); d = get_euclidean's squared L2; every ordering is by (d, index).
      1. neighbours N_{k1+1}(i): topk_stream(X, X, k1 + 1);  M_i = max_j d(i, j): get_euclidean over bounded row chunks + amax;
         od = d / M_i (0 where M_i == 0);
      2. creid_rerank_recip: R(i, k) = {j in N_{k+1}(i) : i in N_{k+1}(j)}, R*(i) = R(i, k1) united with every R(c, kh),
         c in R(i, k1), kh = around(k1 / 2), whose overlap with R(i, k1) exceeds 2/3 of it -- sorted CSR rows (count, scan, fill);
      3. creid_rerank_weights: V(i, j) = exp(-od(i, j)) normalised over R*(i);
      4. creid_rerank_expand (k2 > 1): V'(i) = mean of V over N_{k2}(i);
      5. creid_rerank_blend: J(i, j) = 1 - s / (2 - s), s = sum_c min(V'(i, c), V'(j, c)); pairs that share no column keep J = 1.
    The result does not depend on launch order: two calls return the same bits.
    prefilter = torch.bfloat16 | torch.float16 goes to the neighbour search of stage 1 only (topk_stream(prefilter=...): the same
    neighbour table with the contraction on the 16-bit MFMA), so the result keeps its bits.
    Limits (CreidError): CPU tensors; k1 + 1 > min(N, 1024); k2 < 1 or k2 > k1 + 1; lambda outside [0, 1]; and rows that do not
    fit the kernels' LDS (a worst-case R* row of (k1 + 1)(kh + 2) entries: k1 <= 125; the k2 merged rows of one V' row: 4096
    entries; D <= 16380).
    stats (a dict) receives nnz_v, nnz_vprime, max_row_v, max_row_vprime and temp_bytes (per stage, the bytes of the
    temporaries it allocates, from their shapes; the [nq, ng] distance matrix is not a temporary), and -- when it comes in holding timing=True -- stage_ms (per stage, between device events); debug (a dict) receives the neighbour table, the row maxima and the CSR arrays of R* / V
    (rstar_rowptr, rstar_cols, v_vals) and of V' (vprime_rowptr, vprime_cols, vprime_vals)."""
    if not isinstance(q, torch.Tensor) or not isinstance(g, torch.Tensor):
        raise L.CreidError("re_ranking needs device tensors (no CPU fallback)")
    L.require_gpu(q, g)
    if q.dtype != torch.float32 or g.dtype != torch.float32 or q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1]:
        raise L.CreidError("re_ranking needs fp32 [nq, D] and [ng, D] features")
    nq, ng = q.shape[0], g.shape[0]
    N, k1, k2, lam = nq + ng, int(k1), int(k2), float(lambda_value)
    if k1 < 0 or k1 + 1 > min(N, 1024):
        raise L.CreidError(f"re_ranking: k1 + 1 = {k1 + 1} outside 1 .. min(N = {N}, 1024)")
    if k2 < 1 or k2 > k1 + 1:
        raise L.CreidError(f"re_ranking: k2 = {k2} outside 1 .. k1 + 1 = {k1 + 1}")
    if not 0.0 <= lam <= 1.0:
        raise L.CreidError(f"re_ranking: lambda_value = {lambda_value} outside [0, 1]")
    K, kh = k1 + 1, int(np.around(k1 / 2))
    if 4 * (K + kh + 1 + _pow2_at_least(K * (kh + 2))) > _RERANK_LDS:
        raise L.CreidError(f"re_ranking: a worst-case reciprocal row of (k1 + 1)(kh + 2) = {K * (kh + 2)} entries does not fit "
                           "the set kernel's LDS (k1 <= 125)")
    dev, lib, st = q.device, L.lib(), L.stream()
    if nq == 0 or ng == 0:
        return torch.empty((nq, ng), dtype=torch.float32, device=dev)
    X = _pad_width(torch.cat([q, g]).contiguous())
    D = X.shape[1]
    if 4 * (D + 4) > _RERANK_LDS:
        raise L.CreidError(f"re_ranking: D = {D} does not fit the weight kernel's LDS (D <= 16380)")
    clock = _StageClock(bool(stats) and bool(stats.get("timing")))
    xx = row_sqnorm(X)
    temp = {}
    # 1. neighbours and row maxima
    if prefilter is not None and prefilter not in _H16:
        raise L.CreidError(f"re_ranking: prefilter must be torch.bfloat16, torch.float16 or None, got {prefilter}")
    nb, _ = topk_stream(X, X, K, xx, xx, prefilter=prefilter)
    del _
    clock.mark("neighbours")
    rowmax = torch.empty(N, dtype=torch.float32, device=dev)
    rows = max(1, _STREAM_TOPK_CHUNK_BYTES // (N * 4))
    for r0 in range(0, N, rows):
        r1 = min(N, r0 + rows)
        rowmax[r0:r1] = get_euclidean(X[r0:r1], X, xx[r0:r1], xx).amax(dim=1)
    temp["neighbours"] = nb.numel() * 12 + min(_STREAM_TOPK_CHUNK_BYTES, N * STREAM_TOPK_CAPACITY * 8)
    temp["row_maxima"] = min(rows, N) * N * 4
    clock.mark("row_maxima")
    # 2. reciprocal sets: count, scan, fill
    count = torch.empty(N, dtype=torch.int32, device=dev)
    L.check(lib.creid_rerank_recip(L.ptr(nb), N, K, kh, None, L.ptr(count), None, st), "creid_rerank_recip")
    rowptr = _csr_from_counts(count)
    nnz = int(rowptr[-1].item())
    cols = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    L.check(lib.creid_rerank_recip(L.ptr(nb), N, K, kh, L.ptr(rowptr), None, L.ptr(cols), st), "creid_rerank_recip")
    temp["reciprocal_sets"] = N * 4 + (N + 1) * 8 + nnz * 4
    clock.mark("reciprocal_sets")
    # 3. weights
    vals = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)
    L.check(lib.creid_rerank_weights(L.ptr(X), L.ptr(xx), L.ptr(rowmax), N, D, L.ptr(rowptr), L.ptr(cols), L.ptr(vals), st),
            "creid_rerank_weights")
    temp["weights"] = nnz * 4
    lens = rowptr[1:] - rowptr[:-1]
    max_row_v = int(lens.max().item())
    clock.mark("weights")
    # 4. local query expansion
    if k2 > 1:
        merged = lens[nb[:, :k2]].sum(dim=1)
        cap = _pow2_at_least(max(int(merged.max().item()), 1))
        if 12 * cap + 4 * (k2 + 1 + 4) > _RERANK_LDS:
            raise L.CreidError(f"re_ranking: the k2 = {k2} rows merged into one row of V' hold up to {int(merged.max().item())} "
                               "entries; the expansion kernel's LDS takes 4096")
        count2 = torch.empty(N, dtype=torch.int32, device=dev)
        L.check(lib.creid_rerank_expand(L.ptr(nb), N, K, k2, L.ptr(rowptr), L.ptr(cols), L.ptr(vals), cap, None, L.ptr(count2),
                                        None, None, st), "creid_rerank_expand")
        rowptr2 = _csr_from_counts(count2)
        nnz2 = int(rowptr2[-1].item())
        cols2 = torch.empty(max(nnz2, 1), dtype=torch.int32, device=dev)
        vals2 = torch.empty(max(nnz2, 1), dtype=torch.float32, device=dev)
        L.check(lib.creid_rerank_expand(L.ptr(nb), N, K, k2, L.ptr(rowptr), L.ptr(cols), L.ptr(vals), cap, L.ptr(rowptr2), None,
                                        L.ptr(cols2), L.ptr(vals2), st), "creid_rerank_expand")
        temp["expansion"] = N * k2 * 8 + N * 12 + (N + 1) * 8 + nnz2 * 8
        del merged, count2
    else:
        rowptr2, cols2, vals2, nnz2 = rowptr, cols, vals, nnz
        temp["expansion"] = 0
    clock.mark("expansion")
    # 5. blend: the gallery rows of V' column-major (a stable sort keeps the gallery indices ascending inside a column)
    lens2 = rowptr2[1:] - rowptr2[:-1]
    g0, g1, max_row_q, max_row_vp = (int(v) for v in torch.stack([rowptr2[nq], rowptr2[N], lens2[:nq].max(), lens2.max()]).tolist())
    tile = min((ng + 31) // 32 * 32, 128 << 10)
    if max_row_q * 8 + tile // 8 > _RERANK_LDS:
        raise L.CreidError(f"re_ranking: a query row of V' with {max_row_q} entries does not fit the blend kernel's LDS")
    gcols = cols2[g0:g1]
    grows = torch.repeat_interleave(torch.arange(ng, dtype=torch.int32, device=dev), lens2[nq:])
    colrows = grows[torch.sort(gcols, stable=True).indices].contiguous()
    colptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    colptr[1:] = torch.cumsum(torch.bincount(gcols.long(), minlength=N), 0)
    temp["column_index"] = (g1 - g0) * 32 + (N + 1) * 16
    del grows, gcols
    clock.mark("column_index")
    dist = get_euclidean(X[:nq], X[nq:], xx[:nq].contiguous(), xx[nq:].contiguous())
    out = torch.empty_like(dist)
    L.check(lib.creid_rerank_blend(L.ptr(dist), L.ptr(rowmax), nq, ng, lam, L.ptr(rowptr2), L.ptr(cols2), L.ptr(vals2),
                                   L.ptr(colptr), L.ptr(colrows), max_row_q, L.ptr(out), st), "creid_rerank_blend")
    clock.mark("blend")
    if stats is not None:
        stats.update(nnz_v=nnz, nnz_vprime=nnz2, max_row_v=max_row_v, max_row_vprime=max_row_vp, temp_bytes=temp)
        if clock.on:
            stats["stage_ms"] = clock.stage_ms()
    if debug is not None:
        debug.update(neighbours=nb, rowmax=rowmax, rstar_rowptr=rowptr, rstar_cols=cols[:nnz], v_vals=vals[:nnz],
                     vprime_rowptr=rowptr2, vprime_cols=cols2[:nnz2], vprime_vals=vals2[:nnz2], dist=dist)
    return out


QE_DEFAULTS = dict(k=10, alpha=3.0, rounds=1, scope="all")
QE_SCOPES = ("all", "query")


def expansion_options(query_expansion):
    """The `query_expansion=` argument of R1_mAP / get_similar: False / None -> None; True -> the defaults of query_expansion; a
    dict of k / alpha / rounds / scope -> those over the defaults (their values are checked, shapes apart, so that a constructor
    refuses them before any device work)."""
    if query_expansion is None or query_expansion is False:
        return None
    if query_expansion is True:
        return dict(QE_DEFAULTS)
    if isinstance(query_expansion, dict) and set(query_expansion) <= set(QE_DEFAULTS):
        opts = {**QE_DEFAULTS, **query_expansion}
        _check_expansion(opts["k"], opts["alpha"], opts["rounds"], opts["scope"])
        return opts
    raise L.CreidError(f"query_expansion must be False, True or a dict of k / alpha / rounds / scope, got {query_expansion!r}")


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _check_expansion(k, alpha, rounds, scope):
    """The limits of query_expansion that do not depend on the features -> (k, alpha, rounds) as Python numbers."""
    if scope not in QE_SCOPES:
        raise L.CreidError(f"query_expansion: scope must be 'all' or 'query', got {scope!r}")
    if not _is_int(k) or k < 1 or k - (scope == "query") > 1024:
        raise L.CreidError(f"query_expansion: k = {k!r} must be an integer, 1 .. {1024 + (scope == 'query')} for scope={scope!r}")
    if not _is_int(rounds) or rounds < 1:
        raise L.CreidError(f"query_expansion: rounds = {rounds!r} must be an integer >= 1")
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)) or not np.isfinite(alpha) or alpha < 0:
        raise L.CreidError(f"query_expansion: alpha = {alpha!r} must be a finite number >= 0")
    return int(k), float(alpha), int(rounds)


def _neighbour_expand(x, idx, dist, alpha, self_rows):
    """creid_neighbour_expand on checked arguments (x and self_rows of one width, a multiple of 4)."""
    m, k = idx.shape
    out = torch.empty((m, x.shape[1]), dtype=torch.float32, device=x.device)
    L.check(L.lib().creid_neighbour_expand(L.ptr(x), x.shape[0], L.ptr(idx), L.ptr(dist), L.ptr(self_rows), m, k, x.shape[1],
                                           alpha, L.ptr(out), L.stream()), "creid_neighbour_expand")
    return out


def neighbour_expand(x: torch.Tensor, idx: torch.Tensor, dist, alpha: float, self_rows=None) -> torch.Tensor:
    """S [m, D] fp32, S[i] = [self_rows[i] +] sum_t w[i, t] x[idx[i, t]] (creid_neighbour_expand, csrc/neighbour_expand.hip):
    x fp32 [n_src, D], idx int64 [m, k] (k may be 0), dist fp32 [m, k] -- squared L2 of unit rows as topk_stream returns it --
    self_rows fp32 [m, D] or None.  sim = min(max(fmaf(-0.5, dist, 1), 0), 1); w = 1 for alpha == 0 (dist may then be None),
    sim for alpha == 1, else (float) pow((double) sim, (double) alpha).  Each element is an fp32 fmaf chain from 0 in the order
    self row, t = 0, 1, ...: two calls give the same bits, and a row's bits do not depend on the other rows of the call.
    CreidError, before anything is launched: CPU or non-contiguous tensors, other dtypes or shapes, alpha negative or not
    finite, an index outside [0, n_src) (one 16-byte read-back)."""
    if not all(isinstance(t, torch.Tensor) for t in (x, idx)) or not all(t is None or isinstance(t, torch.Tensor) for t in (dist, self_rows)):
        raise L.CreidError("neighbour_expand needs device tensors (no CPU fallback)")
    L.require_gpu(x, idx, dist, self_rows)
    alpha = _check_expansion(1, alpha, 1, "all")[1]
    if x.dtype != torch.float32 or x.dim() != 2 or idx.dtype != torch.int64 or idx.dim() != 2 or x.shape[1] < 1:
        raise L.CreidError("neighbour_expand needs fp32 rows [n_src, D] and int64 indices [m, k]")
    if dist is None and alpha != 0.0:
        raise L.CreidError("neighbour_expand: dist may be None only with alpha == 0")
    if dist is not None and (dist.dtype != torch.float32 or dist.shape != idx.shape):
        raise L.CreidError("neighbour_expand needs fp32 distances of the indices' shape")
    m, k = idx.shape
    if self_rows is not None and (self_rows.dtype != torch.float32 or self_rows.shape != (m, x.shape[1])):
        raise L.CreidError("neighbour_expand needs fp32 self_rows [m, D] of the rows' width")
    if m and k:
        lo, hi = (int(v) for v in torch.stack(torch.aminmax(idx)).tolist())
        if lo < 0 or hi >= x.shape[0]:
            raise L.CreidError(f"neighbour_expand: indices {lo} .. {hi} outside [0, n_src = {x.shape[0]})")
    D = x.shape[1]
    out = _neighbour_expand(_pad_width(x), idx, dist, alpha, None if self_rows is None else _pad_width(self_rows))
    return out if out.shape[1] == D else out[:, :D].contiguous()


def _expanded_rows(X, nq, k, alpha, rounds, scope, prefilter, out_dtype, stats):
    """query_expansion on X = cat(q, g), fp32 [N, D] with D % 4 == 0 and checked options -> (rows [N, D] in out_dtype, their
    square norms fp32 [N] as l2_normalize returns them).  A round is the whole step, its first normalisation included, so that
    rounds = 2 returns the bits of two calls; only the last round's last normalisation writes out_dtype."""
    timing = bool(stats) and bool(stats.get("timing"))
    per_round, stage_ms = [], []
    for r in range(rounds):
        dt = out_dtype if r == rounds - 1 else torch.float32
        clock = _StageClock(timing)
        info = {}
        if scope == "all":
            U = l2_normalize(X)
            clock.mark("normalise")
            idx, d = topk_stream(U, U, k, prefilter=prefilter, stats=info)
            clock.mark("search")
            S = _neighbour_expand(U, idx, d, alpha, None)
            clock.mark("expand")
            del U, idx, d
            X, sq = l2_normalize(S, out_dtype=dt, return_sqnorm=True)
        else:
            # the gallery's rows are final after the normalisation (rounded once when dt is 16-bit); the search reads the fp32 ones
            Uq, (Ug, gg) = l2_normalize(X[:nq]), l2_normalize(X[nq:], return_sqnorm=True)
            g_out = Ug
            if dt != torch.float32:
                g_out, gg = l2_normalize(X[nq:], out_dtype=dt, return_sqnorm=True)
            clock.mark("normalise")
            if k > 1:
                idx, d = topk_stream(Uq, Ug, k - 1, prefilter=prefilter, stats=info)
            else:
                idx = torch.empty((nq, 0), dtype=torch.int64, device=X.device)
                d = torch.empty((nq, 0), dtype=torch.float32, device=X.device)
            clock.mark("search")
            S = _neighbour_expand(Ug, idx, d, alpha, Uq)
            clock.mark("expand")
            del Uq, Ug, idx, d
            q_out, qq = l2_normalize(S, out_dtype=dt, return_sqnorm=True)
            X, sq = torch.cat([q_out, g_out]), torch.cat([qq, gg])
            del q_out, g_out
        del S
        clock.mark("normalise")
        info.pop("kept", None)                              # (a device tensor of the pre-filtered search; the counters stay)
        per_round.append(info)
        if timing:
            stage_ms.append(clock.stage_ms())                   # both normalisations under one name
    if stats is not None:
        stats.update(per_round[-1], rounds_stats=per_round)
        if timing:
            stats["stage_ms"] = stage_ms
    return X, sq


def query_expansion(q: torch.Tensor, g: torch.Tensor, k: int = 10, alpha: float = 3.0, rounds: int = 1, scope: str = "all", *,
                    prefilter=None, out_dtype=torch.float32, return_sqnorm=False, stats=None):
    """Neighbour-based feature expansion of fp32 device features q [nq, D], g [ng, D] -> (q', g'), unit rows: average query
    expansion (Chum et al., ICCV 2007) with the alpha weighting of Radenovic et al. (TPAMI 2019), and -- scope="all" -- the
    database-side augmentation of Arandjelovic and Zisserman (CVPR 2012) with it.  Every row is replaced by the
    similarity-weighted sum of its nearest neighbours, normalised again; rank the result like any other features.

    U = l2_normalize(cat(q, g)); d = topk_stream's squared L2, every ordering by (d, index);
    sim = min(max(fmaf(-0.5, d, 1), 0), 1) (the cosine of unit rows); w = 1 for alpha == 0, sim for alpha == 1, else
    (float) pow((double) sim, (double) alpha).
      scope="all":   (idx, d) = topk_stream(U, U, k) over all N = nq + ng rows -- a row's own entry is one of its neighbours like
                     any other --; S[i] = sum_t w[i, t] U[idx[i, t]].
      scope="query": (idx, d) = topk_stream(Uq, Ug, k - 1); S[i] = Uq[i] + sum_t w[i, t] Ug[idx[i, t]]; the gallery rows are
                     l2_normalize(g) and nothing else (k = 1: no search, S = Uq).
    U' = l2_normalize(S); rounds = r repeats the whole step on U', its first normalisation included: the bits of r calls.
    S is an fp32 fmaf chain in the order of t (neighbour_expand), so the result does not depend on launch order: two calls
    return the same bits.
    Expansion is blind to labels: it sees neither pids nor cameras, so the neighbours it averages include gallery rows of the
    query's own identity taken by the query's own camera -- the entries the evaluation later removes from the ranking.
    prefilter = torch.bfloat16 | torch.float16 goes to topk_stream only (the same neighbour table with the contraction on the
    16-bit MFMA), so the result keeps its bits.  out_dtype: the dtype of the LAST normalisation (bf16 / f16: the rows the 16-bit
    evaluation modes use, rounded once; all expansion arithmetic stays fp32).  return_sqnorm=True -> (q', g', qq, gg), the square
    norms l2_normalize returns with the rows.
    Temporaries: the [N, k] neighbour tables, topk_stream's bounded chunks, and [N, D] fp32 buffers for the rows and their sums.
    stats (a dict) receives topk_stream's counters of the last round, rounds_stats (one dict per round) and -- when it comes in
    holding timing=True -- stage_ms: one dict per round (search, expand, normalise; between device events).
    Limits (CreidError, before anything is launched): CPU tensors; not fp32 [nq, D] / [ng, D] of one width; scope="all":
    k outside 1 .. min(N, 1024); scope="query": k < 1 or k - 1 > min(ng, 1024); alpha negative or not finite; rounds < 1."""
    if not isinstance(q, torch.Tensor) or not isinstance(g, torch.Tensor):
        raise L.CreidError("query_expansion needs device tensors (no CPU fallback)")
    k, alpha, rounds = _check_expansion(k, alpha, rounds, scope)
    L.require_gpu(q, g)
    if q.dtype != torch.float32 or g.dtype != torch.float32 or q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1]:
        raise L.CreidError("query_expansion needs fp32 [nq, D] and [ng, D] features of one width")
    if prefilter is not None and prefilter not in _H16:
        raise L.CreidError(f"query_expansion: prefilter must be torch.bfloat16, torch.float16 or None, got {prefilter}")
    if out_dtype not in (torch.float32,) + _H16:
        raise L.CreidError(f"query_expansion: out_dtype must be torch.float32, torch.bfloat16 or torch.float16, got {out_dtype}")
    nq, D = q.shape
    _check_expansion_shape(k, scope, nq, g.shape[0])
    X = _pad_width(torch.cat([q, g]).contiguous())
    U, sq = _expanded_rows(X, nq, k, alpha, rounds, scope, prefilter, out_dtype, stats)
    if U.shape[1] != D:
        U = U[:, :D]
    qo, go = U[:nq].contiguous(), U[nq:].contiguous()
    return (qo, go, sq[:nq].contiguous(), sq[nq:].contiguous()) if return_sqnorm else (qo, go)


def _check_expansion_shape(k, scope, nq, ng):
    if scope == "all" and k > min(nq + ng, 1024):
        raise L.CreidError(f"query_expansion(scope='all'): k = {k} outside 1 .. min(N = {nq + ng}, 1024)")
    if scope == "query" and k - 1 > min(ng, 1024):
        raise L.CreidError(f"query_expansion(scope='query'): k - 1 = {k - 1} outside 0 .. min(ng = {ng}, 1024)")


def _dev_i64(a, device):
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=torch.int64).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a), dtype=np.int64), device=device)


def _camset_masks(g_camids):
    """list of camera-id lists -> int64 bitmasks (camera ids must be < 63)."""
    out = np.zeros(len(g_camids), np.int64)
    for j, cs in enumerate(g_camids):
        for c in np.atleast_1d(cs):
            c = int(c)
            if not 0 <= c < 63:
                raise L.CreidError("camera-set evaluation supports camera ids 0..62")
            out[j] |= np.int64(1) << np.int64(c)
    return out


class CameraSets(list):
    """The camera-set list R1_mAP.compute(respect_camids=True) receives -- `[[c], ...]` for the queries, then one list of camera
    ids per gallery entry (modelling/bases.py:250-253) -- together with what the camera-aware centroid index already holds of
    it: `masks` (int64 device tensor, one bitmask per gallery entry, bit c = camera c) and `q_cams` (int64 numpy vector of the
    queries' cameras).  A plain list: everything that reads the lists keeps working; the streamed evaluation reads the two
    attributes instead and neither walks the lists nor uploads the masks again."""

    def __init__(self, lists, masks, q_cams):
        super().__init__(lists)
        self.masks = masks
        self.q_cams = np.ascontiguousarray(q_cams, dtype=np.int64)


def _check_query_cams(qc):
    if qc.size and (qc.min() < 0 or qc.max() >= 63):                              # the kernels shift a 64-bit mask by it
        raise L.CreidError("camera-set evaluation supports camera ids 0..62")
    return qc


def _camset_split(camids, nq):
    """respect_camids=True camera argument -> (query cameras int64 [nq] inside 0..62, gallery masks: the carrier's device tensor
    or an int64 numpy vector)."""
    if isinstance(camids, CameraSets):
        return _check_query_cams(camids.q_cams), camids.masks
    qc = np.asarray([int(np.atleast_1d(c)[0]) for c in camids[:nq]], np.int64)
    return _check_query_cams(qc), _camset_masks(camids[nq:])


def eval_func_device(indices: torch.Tensor, q_pids, g_pids, q_camids, g_camids, max_rank=50, camsets=False):
    """Device half of eval_func: returns device tensors (cmc f32[max_rank], mAP f64[1], topk f64[5],
    nvalid i64[1], valid u8[m], ap f64[m], first i32[m]).  camsets: g_camids is a list of camera-id lists, or the int64
    bitmasks themselves (tensor / numpy vector) next to a numpy vector of plain query cameras."""
    L.require_gpu(indices)
    dev = indices.device
    m, n = indices.shape
    if n < max_rank:  # utils/eval_reid.py:33-35
        max_rank = n
        print("Note: number of gallery samples is quite small, got {}".format(n))
    if camsets and isinstance(g_camids, (torch.Tensor, np.ndarray)):
        q_camids = _check_query_cams(np.asarray(q_camids, np.int64))
    elif camsets:
        q_camids, g_camids = _camset_split(list(q_camids) + list(g_camids), m)
    qp, gp, qc, gc = (_dev_i64(a, dev) for a in (q_pids, g_pids, q_camids, g_camids))
    res = _PerQuery.empty(m, dev)
    lib = L.lib()
    fn = lib.creid_cmc_ap_ranked_camsets if camsets else lib.creid_cmc_ap_ranked
    L.check(fn(L.ptr(indices), m, n, L.ptr(qp), L.ptr(gp), L.ptr(qc), L.ptr(gc), L.ptr(res.valid), L.ptr(res.ap), L.ptr(res.first),
               L.stream()), "creid_cmc_ap_ranked")
    return (*eval_reduce_device(*res, max_rank), *res)


def _pack_results(cmc, mAP, topk, valid, ap, tail=()):
    """Everything the host needs of an evaluation as ONE float64 device tensor, so that one read-back (one synchronisation
    instead of five) fetches it: [cmc (max_rank) | mAP | topk (5) | valid (m) | ap (m) | tail], exact for the f32 / u8 members.
    tail: float64 device tensors that ride along."""
    return torch.cat([cmc.double(), mAP, topk, valid.double(), ap, *tail])


def _unpack_results(pack, max_rank, q_pids):
    """The read-back of _pack_results (q_pids: the m queries' pids, a numpy vector) -> (cmc f32 [max_rank], mAP float,
    topk f64 [5], valid bool [m], ap f64 [m], tail f64, single_performance f64 [n_valid, 3] = rows [q_idx, q_pid, AP])."""
    pack = pack.cpu().numpy()
    m, o = len(q_pids), max_rank + 6
    valid, ap = pack[o:o + m] == 1, pack[o + m:o + 2 * m]
    vi = np.nonzero(valid)[0]
    single = np.stack([vi.astype(np.float64), q_pids[vi].astype(np.float64), ap[vi]], axis=1)
    return pack[:max_rank].astype(np.float32), float(pack[max_rank]), pack[max_rank + 1:o].copy(), valid, ap, pack[o + 2 * m:], single


def eval_func(indices, q_pids, g_pids, q_camids, g_camids, max_rank=50, respect_camids=False):
    """utils/eval_reid.py:25-92: returns (all_cmc float32[max_rank], mAP float, all_topk float64[5],
    single_performance float64[n_valid, 3] = rows [q_idx, q_pid, AP])."""
    if not isinstance(indices, torch.Tensor):
        raise L.CreidError("eval_func needs a device tensor of ranked indices (no CPU fallback)")
    cmc, mAP, topk, nvalid, valid, ap, first = eval_func_device(indices, q_pids, g_pids, q_camids, g_camids, max_rank,
                                                                camsets=bool(respect_camids))
    qp = np.asarray(q_pids.cpu() if isinstance(q_pids, torch.Tensor) else q_pids)
    cmc, mAP, topk, _, _, _, single = _unpack_results(_pack_results(cmc, mAP, topk, valid, ap), cmc.shape[0], qp)
    return cmc, mAP, topk, single


# --------------------------------------------------------------------------- streamed (metric-only) evaluation
_CAP_HINT = {}      # (queries, gallery) -> positive-list capacity of the last streamed evaluation of that shape (a speculation
                    # that R1_mAP._compute_streamed verifies; never trusted)


_LABEL_STAGE = {}   # (device, length) -> (pinned [2, length] int64 staging tensor, event of its last upload)


def _upload_labels(p, c, device):
    """[2, len] int64 device tensor of (pids, camids) through a reused page-locked staging buffer: the copy is enqueued on the
    current stream instead of blocking the host the way a pageable upload does (the evaluation's clock includes this upload;
    the device is still normalising the features while it runs).  The buffer is reused only after its previous upload has
    completed (event), whatever the caller did in between."""
    dev = torch.device(device)
    if dev.type != "cuda":
        return torch.from_numpy(np.stack([p, c])).to(dev)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), len(p))
    ent = _LABEL_STAGE.get(key)
    if ent is None:
        if len(_LABEL_STAGE) > 8:
            _LABEL_STAGE.clear()
        ent = _LABEL_STAGE[key] = (torch.empty((2, len(p)), dtype=torch.int64, pin_memory=True), torch.cuda.Event())
    else:
        ent[1].synchronize()
    stage, ev = ent
    h = stage.numpy()
    np.copyto(h[0], p); np.copyto(h[1], c)
    lab = stage.to(dev, non_blocking=True)
    ev.record(torch.cuda.current_stream(dev))
    return lab


class StreamPlan:
    """Index for the streamed evaluation (csrc/stream_eval.hip): the gallery grouped by pid (CSR), every query's slot in
    it, and the per-query number of positives (same pid, different camera) which fixes the LDS list capacity `cap`.
    Queries with more than 128 positives are listed in `overflow` and must take the general (materialised) path.  Holds
    device tensors only.

    `StreamPlan.on_device(...)` (what R1_mAP uses) builds it with creid_stream_plan: one upload of the label vectors, a
    counting sort on the GPU, and an 8-byte read-back for `cap`.  The constructor is the host (numpy) construction of the
    same index -- kept for label sets whose pid range is too sparse for a dense counting sort, and as the checker of the
    device build in tests/test_stream_eval_gpu.py.

    camsets=True (both constructions): the gallery entries carry camera SETS as int64 bitmasks and a positive is a same-pid
    entry whose set does not hold the query's camera (creid_stream_plan_camsets; tests/test_camset_stream_*)."""

    MAX_CAP = 128
    MAX_DENSE_RANGE = 1 << 24          # pid range the device counting sort accepts (2 x int32 scratch + int64 CSR per slot)

    camsets = False

    @classmethod
    def on_device(cls, pids, camids, num_query, device, camsets=False, g_cam_masks=None):
        """pids / camids: host vectors [nq + ng] as R1_mAP.compute receives them (utils/reid_metric.py:112).
        camsets=True (respect_camids, utils/eval_reid.py:51-55): the gallery entries carry camera SETS -- camids[nq:] are int64
        bitmasks (bit c = camera c), camids[:nq] the queries' plain cameras (0..62, else CreidError); a same-pid entry is a
        positive iff the query's camera is not in its set.  g_cam_masks: the gallery masks as an int64 device tensor [ng]
        (CameraSets.masks); camids may then hold the nq query cameras only, and no mask is uploaded."""
        p = np.ascontiguousarray(np.asarray(pids), dtype=np.int64)
        c = np.ascontiguousarray(np.asarray(camids), dtype=np.int64)
        nq = int(num_query)
        m, n = nq, len(p) - nq
        if camsets:
            _check_query_cams(c[:nq])
            if g_cam_masks is not None and len(c) < len(p):
                c = np.concatenate([c[:nq], np.zeros(n, np.int64)])
            if len(c) != len(p):
                raise L.CreidError(f"StreamPlan.on_device(camsets=True): {len(p)} pids but {len(c)} camera entries")
        host_masks = lambda: c[nq:] if g_cam_masks is None else g_cam_masks.cpu().numpy()
        if n <= 0:
            return cls(p[:nq], p[nq:], c[:nq], host_masks(), device, camsets=camsets)
        pmin, pmax = int(p[nq:].min()), int(p[nq:].max())
        R = pmax - pmin + 1
        if R > cls.MAX_DENSE_RANGE:
            return cls(p[:nq], p[nq:], c[:nq], host_masks(), device, camsets=camsets)
        self = cls.__new__(cls)
        self.m, self.n = m, n
        self.camsets = bool(camsets)
        lab = _upload_labels(p, c, device)                                        # ONE upload: [2, nq + ng] int64
        self.q_pids, self.g_pids, self.q_cams, self.g_cams = lab[0, :nq], lab[0, nq:], lab[1, :nq], lab[1, nq:]
        if camsets and g_cam_masks is not None:
            L.require_gpu(g_cam_masks)
            assert g_cam_masks.dtype == torch.int64 and g_cam_masks.shape == (n,)
            self.g_cams = g_cam_masks.contiguous()
        # one allocation for the index: [csr_off int64 (R + 1) | g_order | q_slot | n_pos | stats | scratch (2 R)] int32
        mm = max(m, 1)
        ws = torch.empty(2 * (R + 1) + n + 2 * mm + 2 + 2 * R, dtype=torch.int32, device=device)
        self.csr_off = ws[:2 * (R + 1)].view(torch.int64)
        o = 2 * (R + 1)
        self.g_order = ws[o:o + n]; o += n
        self.q_slot = ws[o:o + mm]; o += mm
        self._n_pos_dev = ws[o:o + mm]; o += mm
        self._stats = ws[o:o + 2]; o += 2
        scratch = ws[o:o + 2 * R]
        build = L.lib().creid_stream_plan_camsets if camsets else L.lib().creid_stream_plan
        L.check(build(L.ptr(self.q_pids), L.ptr(self.g_pids), L.ptr(self.q_cams), L.ptr(self.g_cams), m, n,
                      pmin, R, L.ptr(self.csr_off), L.ptr(self.g_order), L.ptr(self.q_slot),
                      L.ptr(self._n_pos_dev), L.ptr(self._stats), L.ptr(scratch), L.stream()),
                "creid_stream_plan")
        self._n_pos = None
        self.cap = None                      # resolved by finish(): the only host read, 8 bytes
        return self

    def finish(self):
        """Read back {max positives, #overflow queries} (the one synchronisation of the device build) and fix `cap`."""
        if self.cap is not None:
            return self
        mx, nover = (int(v) for v in self._stats.cpu().tolist())
        cap = 2
        while cap < max(mx, 1):
            cap *= 2
        self.cap = cap
        self.overflow = np.nonzero(self.n_pos > self.MAX_CAP)[0] if nover else np.zeros(0, np.int64)
        return self

    @property
    def n_pos(self):
        if self._n_pos is None:
            self._n_pos = self._n_pos_dev[:self.m].cpu().numpy().astype(np.int64)
        return self._n_pos

    def __init__(self, q_pids, g_pids, q_camids, g_camids, device, camsets=False):
        """camsets=True: g_camids are int64 camera-set bitmasks, q_camids plain cameras 0..62 (see on_device)."""
        qp = np.ascontiguousarray(np.asarray(q_pids), dtype=np.int64)
        gp = np.ascontiguousarray(np.asarray(g_pids), dtype=np.int64)
        qc = np.ascontiguousarray(np.asarray(q_camids), dtype=np.int64)
        gc = np.ascontiguousarray(np.asarray(g_camids), dtype=np.int64)
        self.m, self.n = len(qp), len(gp)
        self.camsets = bool(camsets)
        if camsets:
            _check_query_cams(qc)
        order = np.argsort(gp, kind="stable").astype(np.int32)            # by pid, gallery index ascending inside
        upid, start = np.unique(gp[order], return_index=True)
        csr = np.concatenate([start, [self.n]]).astype(np.int64)
        slot = np.searchsorted(upid, qp)
        slot_c = np.minimum(slot, max(len(upid) - 1, 0))
        hit = (slot < len(upid)) & (upid[slot_c] == qp) if len(upid) else np.zeros(self.m, bool)
        same_pid = np.where(hit, csr[slot_c + 1] - csr[slot_c], 0) if len(upid) else np.zeros(self.m, np.int64)
        if camsets:
            # same pid AND the query's camera in the entry's set: per query camera, the set's members counted per pid group
            same_cam = np.zeros(self.m, np.int64)
            g_slot = np.searchsorted(upid, gp)
            for cam in np.unique(qc):
                per_pid = np.bincount(g_slot[((gc >> cam) & 1) != 0], minlength=max(len(upid), 1))
                sel = hit & (qc == cam)
                same_cam[sel] = per_pid[slot_c[sel]]
        else:
            # same pid AND same camera (the removed entries): count through a combined key
            cmin = int(min(gc.min(initial=0), qc.min(initial=0)))
            span = int(max(gc.max(initial=0), qc.max(initial=0))) - cmin + 1
            pmin = int(min(gp.min(initial=0), qp.min(initial=0)))
            gk = (gp - pmin) * span + (gc - cmin)
            qk = (qp - pmin) * span + (qc - cmin)
            uk, cnt = np.unique(gk, return_counts=True)
            ks = np.searchsorted(uk, qk)
            ks_c = np.minimum(ks, max(len(uk) - 1, 0))
            same_cam = np.where((ks < len(uk)) & (uk[ks_c] == qk), cnt[ks_c], 0) if len(uk) else np.zeros(self.m, np.int64)
        self._n_pos = (same_pid - same_cam).astype(np.int64)
        self.overflow = np.nonzero(self._n_pos > self.MAX_CAP)[0]
        mx = int(self._n_pos[self._n_pos <= self.MAX_CAP].max(initial=1))
        cap = 2
        while cap < mx:
            cap *= 2
        self.cap = cap
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=device)
        self.q_slot = t(np.where(hit, slot_c, -1), np.int32)
        self.csr_off, self.g_order = t(csr, np.int64), t(order, np.int32)
        self.q_pids, self.g_pids, self.q_cams, self.g_cams = t(qp, np.int64), t(gp, np.int64), t(qc, np.int64), t(gc, np.int64)


class _PosLists(NamedTuple):
    """The positives of every query as the streamed count reads them: key / idx i32 [m, cap] (distance keys ascending and the
    gallery entries behind them), npos i32 [m] (negative: more positives than `cap`), and the histogram hist i32 [m, cap] the
    count bumps."""
    cap: int
    key: torch.Tensor
    idx: torch.Tensor
    npos: torch.Tensor
    hist: torch.Tensor

    def rows(self, sel):
        """The lists of the queries `sel` (an index tensor), gathered, with a fresh histogram."""
        return _PosLists(self.cap, self.key.index_select(0, sel), self.idx.index_select(0, sel), self.npos.index_select(0, sel),
                         torch.zeros((sel.shape[0], self.cap), dtype=torch.int32, device=sel.device))


def _stream_poslist(fq, fg, qq, gg, plan: StreamPlan) -> _PosLists:
    """creid_stream_poslist[_h16][_camsets], by the rows' dtype and plan.camsets (camera sets only change which same-pid
    entries are positives: another poslist, the same count and finalize): the positives' distances of every query, and a
    zeroed histogram."""
    m, n, D, cap, dev = fq.shape[0], fg.shape[0], fq.shape[1], plan.cap, fq.device
    h16 = fq.dtype in _H16
    pl = _PosLists(cap, torch.empty((m, cap), dtype=torch.int32, device=dev), torch.empty((m, cap), dtype=torch.int32, device=dev),
                   torch.empty(m, dtype=torch.int32, device=dev), torch.zeros((m, cap), dtype=torch.int32, device=dev))
    name = "creid_stream_poslist" + ("_h16" if h16 else "")
    dt = (L.dtype_code(fq),) if h16 else ()
    L.check(getattr(L.lib(), name + ("_camsets" if plan.camsets else ""))(
        L.ptr(fq), L.ptr(fg), L.ptr(qq), L.ptr(gg), m, n, D, *dt, L.ptr(plan.q_slot), L.ptr(plan.csr_off), L.ptr(plan.g_order),
        L.ptr(plan.q_cams), L.ptr(plan.g_cams), cap, L.ptr(pl.key), L.ptr(pl.idx), L.ptr(pl.npos), L.stream()), name)
    return pl


def _stream_count(fq, fg, qq, gg, q_pids, g_pids, pl: _PosLists):
    """creid_stream_count[_h16]: the streamed contraction with the in-register count epilogue, into pl.hist."""
    h16 = fq.dtype in _H16
    name = "creid_stream_count" + ("_h16" if h16 else "")
    dt = (L.dtype_code(fq),) if h16 else ()
    L.check(getattr(L.lib(), name)(L.ptr(fq), L.ptr(fg), L.ptr(qq), L.ptr(gg), fq.shape[0], fg.shape[0], fq.shape[1], *dt,
                                   L.ptr(q_pids), L.ptr(g_pids), pl.cap, L.ptr(pl.key), L.ptr(pl.idx), L.ptr(pl.npos),
                                   L.ptr(pl.hist), L.stream()), name)


def stream_eval(fq, fg, qq, gg, plan: StreamPlan):
    """Per-query (valid u8[m], AP f64[m], first-match rank i32[m]) with no m x n matrix: positives' distances ->
    streamed MFMA contraction with an in-register count epilogue -> histogram prefix.  valid == 2 marks a query
    whose positive list overflowed the plan's capacity (see StreamPlan.overflow).  fp32 features run on the f32 MFMA
    (csrc/stream_eval.hip), bf16 / f16 features (D % 8 == 0) on the 16-bit MFMA (csrc/stream_h16.hip).  A plan that has not
    read its capacity back yet is finished first (StreamPlan.finish: one synchronisation)."""
    if plan.cap is None:
        plan.finish()
    L.require_gpu(fq, fg, qq, gg)
    assert fq.dtype == fg.dtype and fq.dtype in (torch.float32,) + _H16
    assert (fq.shape[0], fg.shape[0]) == (plan.m, plan.n)
    pl = _stream_poslist(fq, fg, qq, gg, plan)
    _stream_count(fq, fg, qq, gg, plan.q_pids, plan.g_pids, pl)
    return _PerQuery.finalize(pl.npos, pl.hist, pl.cap)


EVAL_PREFILTER_CAPACITY = 1024        # ambiguous pairs a query may list (creid_stream_count_band_h16: power of two, 64 .. 8192)


def _stream_eval_prefilter(fq, fg, qq, gg, plan: StreamPlan, dtype, acap, clock):
    """stream_eval on fp32 features with the counting contraction on the 16-bit MFMA and the fp32 path's histogram, element for
    element.  d: the fp32 kernels' distance; dh: the 16-bit streamed kernel's distance on the rows rounded once to `dtype`, given
    the fp32 rows' own qq / gg; m_i = prefilter_margin >= |dh - d| over row i (query statistics against the gallery's maxima, as in
    _topk_stream_prefilter; inflated by 1 + 2^-20 and rounded UP to fp32), so d_ij lies in [dh_ij - m_i, dh_ij + m_i].  The
    positives' keys are the fp32 ones (creid_stream_poslist on the fp32 rows).  Per negative, with lo / hi the band's ends rounded
    outwards: behind every positive when key(lo) is beyond the last positive's key; else l = #positives with key < key(lo), all
    ranked before it whatever d is; if positive l lies inside the band (key <= key(hi)) the pair is ambiguous and listed, else
    every positive from l on is behind it and hist[i][l] is bumped -- the slot the fp32 kernel finds.
    creid_stream_count_rescore gives every listed pair its fp32 bits and the fp32 epilogue's search.
    Everything is enqueued without a host read: the gallery's maxima stay on the device, so non-finite ones (f16 overflow, Inf /
    NaN) flag every row with a positive list on the device, and the caller's repair runs the fp32 count on all of them; queries
    with more positives than the list holds (npos < 0) are never flagged: their results come from the caller's general path.
    Returns (valid, ap, first, state); state holds what the caller's read-back and repair need."""
    L.require_gpu(fq, fg, qq, gg)
    assert fq.dtype == fg.dtype == torch.float32 and fq.shape[1] % 8 == 0
    m, n, D = fq.shape[0], fg.shape[0], fq.shape[1]
    assert (m, n) == (plan.m, plan.n)
    dev, lib, st = fq.device, L.lib(), L.stream()
    cap, dt = plan.cap, L._DT[dtype]
    qp, gp = prefilter_pack(fq, dtype), prefilter_pack(fg, dtype)
    gmax = torch.cat([gp.stats.amax(dim=0), gg.abs().amax().double().reshape(1)]) if n else torch.zeros(4, dtype=torch.float64, device=dev)
    x2 = torch.maximum(qp.stats[:, 2], qq.abs().double())
    margin = prefilter_margin(qp.stats[:, 0], qp.stats[:, 1], x2, gmax[0], gmax[1], gmax[2], torch.maximum(gmax[2], gmax[3]), D)
    margin32 = _round_up_f32((1.0 + _PREFILTER_INFLATE) * margin)
    clock.mark("pack")
    amb = torch.empty((m, acap), dtype=torch.int32, device=dev)
    amb_count = torch.zeros(m, dtype=torch.int32, device=dev)
    flags = torch.zeros(m, dtype=torch.uint8, device=dev)
    pl = _stream_poslist(fq, fg, qq, gg, plan)
    clock.mark("poslist")
    L.check(lib.creid_stream_count_band_h16(L.ptr(qp.rounded), L.ptr(gp.rounded), L.ptr(qq), L.ptr(gg), m, n, D, dt,
                                            L.ptr(plan.q_pids), L.ptr(plan.g_pids), cap, L.ptr(pl.key), L.ptr(pl.idx),
                                            L.ptr(pl.npos), L.ptr(margin32), acap, L.ptr(amb), L.ptr(amb_count), L.ptr(pl.hist), st),
            "creid_stream_count_band_h16")
    clock.mark("count")
    L.check(lib.creid_stream_count_rescore(L.ptr(amb), L.ptr(amb_count), m, acap, L.ptr(fq), L.ptr(fg), L.ptr(qq), L.ptr(gg), n, D,
                                           cap, L.ptr(pl.key), L.ptr(pl.idx), L.ptr(pl.npos), L.ptr(pl.hist), L.ptr(flags), st),
            "creid_stream_count_rescore")
    # a gallery out of range: every row to the fp32 count, except those that have no list and take the general path
    flags = torch.where(torch.isfinite(gmax).all(), flags, (pl.npos >= 0).to(torch.uint8))
    res = _PerQuery.finalize(pl.npos, pl.hist, cap)
    clock.mark("rescore")
    state = dict(flags=flags, ambiguous=amb_count, gmax=gmax, margin_max=margin.max().reshape(1) if m else gmax[:1] * 0, lists=pl)
    return (*res, state)


def _stream_eval_prefilter_repair(fq, fg, qq, gg, plan: StreamPlan, state, rows, valid, ap, first):
    """The rows creid_stream_count_rescore flagged, redone with the fp32 creid_stream_count on the gathered rows (their q, qq,
    q_pids, positive lists and a fresh histogram) and merged into valid / ap / first."""
    sel = torch.as_tensor(rows, device=fq.device)
    pl = state["lists"].rows(sel)
    _stream_count(fq.index_select(0, sel), fg, qq.index_select(0, sel), gg, plan.q_pids.index_select(0, sel), plan.g_pids, pl)
    _PerQuery(valid, ap, first).merge(sel, _PerQuery.finalize(pl.npos, pl.hist, pl.cap))


def eval_reduce_device(valid, ap, first, max_rank):
    """Means over valid queries (utils/eval_reid.py:86-90) on the device: (cmc f32[max_rank], mAP f64[1],
    topk f64[5], nvalid i64[1])."""
    dev = valid.device
    cmc = torch.empty(max_rank, dtype=torch.float32, device=dev)
    mAP = torch.empty(1, dtype=torch.float64, device=dev)
    topk = torch.empty(5, dtype=torch.float64, device=dev)
    nvalid = torch.empty(1, dtype=torch.int64, device=dev)
    L.check(L.lib().creid_eval_reduce(L.ptr(valid), L.ptr(ap), L.ptr(first), valid.shape[0], max_rank, L.ptr(cmc),
                                      L.ptr(mAP), L.ptr(topk), L.ptr(nvalid), L.stream()), "creid_eval_reduce")
    return cmc, mAP, topk, nvalid


class R1_mAP:
    """utils/reid_metric.py:71-151.  `pl_module` only needs `.hparams` (SOLVER.DISTANCE_FUNC,
    MODEL.USE_CENTROIDS); trainer/logger lookups of the reference are optional here."""

    def __init__(self, pl_module=None, num_query=0, max_rank=50, feat_norm=True, dist_func="euclidean",
                 compute_dtype=torch.float32, streamed=False, reranking=False, prefilter=None, prefilter_capacity=None,
                 query_expansion=False, ranked_topk=None, roc=None):
        """streamed=True: metric-only evaluation that never materialises the distance / index matrices (euclidean; plain
        camera ids or, with compute(respect_camids=True), camera sets; compute_dtype fp32, bf16 or f16 -- the 16-bit modes
        run the 16-bit MFMA and return exactly what their materialised evaluation returns); `last` then holds the per-query
        results only.  streamed=False keeps
        `last["distmat"]` / `last["indices"]` (what the rank-index parity tests and get_similar read).
        reranking=True (the defaults of re_ranking) or a dict of k1 / k2 / lambda_value: on the materialised euclidean fp32 path
        the k-reciprocal re-ranked matrix takes the place of `distmat`; ranking and evaluation are unchanged.  CreidError with
        streamed=True, a 16-bit compute_dtype, the cosine distance or compute_chunked.
        prefilter=torch.bfloat16 | torch.float16 (streamed=True, fp32, euclidean, plain camera ids): the streamed evaluation with
        its counting contraction on the 16-bit MFMA and the results of the fp32 streamed evaluation -- valid and first bit for bit,
        ap within the order of its float64 additions (_stream_eval_prefilter).  prefilter_capacity (default
        EVAL_PREFILTER_CAPACITY; a power of two, 64 .. 8192): the ambiguous pairs a query may list; queries that list more are
        redone on the fp32 kernel.  `last["prefilter"]` then holds dtype (None when the gallery's statistics were not finite and
        every row took the fp32 kernel), capacity, margin_max, fallback_rows, ambiguous (int32 [m] on the device: pairs listed per
        query) and -- when `last` came in holding {"prefilter": {"timing": True}} -- stage_ms (pack, poslist, count, rescore,
        repair, between device events).  CreidError with streamed=False, another compute_dtype or distance, or reranking; and
        from compute(respect_camids=True).
        query_expansion=True (the defaults of query_expansion) or a dict of k / alpha / rounds / scope: the rows are normalised
        to fp32, expanded by their nearest neighbours (reid_metric.query_expansion: blind to pids and cameras) and the sums
        normalised into compute_dtype; everything behind the normalisation -- either distance, streamed or not, compute_chunked,
        re-ranking, camera sets -- then runs on the expanded rows, exactly as R1_mAP(feat_norm=False) runs on the rows
        query_expansion returns.  `prefilter` also goes to the expansion's neighbour search.  `last["query_expansion"]` holds the
        options and query_expansion's stats (stage_ms when `last` came in holding {"query_expansion": {"timing": True}}).
        CreidError with feat_norm=False: expansion is defined on unit rows.
        ranked_topk=K (an int, 1 .. 1024; default None: nothing changes): after the metrics, `last["ranked"]` holds the ranked
        lists the metrics are defined on -- per query the first K' = min(K, gallery size) gallery entries that are not junk (the
        query's pid seen by its camera, or by a camera set that holds it: utils/eval_reid.py:49-58, what utils/visrank.py:193-232
        draws) -- as device tensors: indices int64 [nq, K'] (padded with -1), distances fp32 [nq, K'] (+inf in the padding),
        matched bool [nq, K'] (the entry has the query's pid) and count int32 [nq] (the real entries).  On every route and with
        every other option; streamed routes build them with topk_stream(junk=...) on the rows the evaluation multiplied (no
        matrix; with prefilter= too, by the plain streamed kernels), materialised ones with rank_keep_topk on `last["indices"]`.
        The metrics returned are those of the same call without the keyword.
        roc=True (the rates ROC_DEFAULT_FAR = 1e-4, 1e-3, 1e-2) or a tuple of up to 16 false-accept rates in (0, 1] (default
        None: nothing changes): after the metrics, `last["roc"]` holds the open-set operating points of the evaluation's own
        distances -- the dict of roc_stream: per rate the exact threshold (in the unit of the route's matrix: squared L2 on the
        euclidean routes), false / true accepts under the STRICT test distance < threshold, the class sizes, far and tar, and
        the first pass's genuine / impostor histograms.  Junk pairs belong to no class.  On every route and with every other
        option: streamed routes run roc_stream on the rows and norms the evaluation multiplied (no matrix; with prefilter= by the
        plain fp32 kernels), materialised ones roc_matrix on their own `distmat` (cosine, re-ranked, streamed=False); the cosine
        loop of compute_chunked counts the first pass chunk by chunk and forms every chunk's matrix again for the two later
        passes.  The metrics returned are those of the same call without the keyword, bit for bit."""
        self.roc = None if roc is None or roc is False else roc_rates(roc)
        if ranked_topk is not None and not (_is_int(ranked_topk) and 1 <= ranked_topk <= 1024):
            raise L.CreidError(f"R1_mAP(ranked_topk=...) must be an int, 1 .. 1024, got {ranked_topk!r}")
        self.ranked_topk = None if ranked_topk is None else int(ranked_topk)
        self.reranking = rerank_options(reranking)
        self.query_expansion = expansion_options(query_expansion)
        if self.query_expansion is not None and not feat_norm:
            raise L.CreidError("R1_mAP(query_expansion=...) expands unit rows: not with feat_norm=False")
        self._qe_info = None
        self.streamed = streamed
        self.num_query = num_query
        self.max_rank = max_rank
        self.feat_norm = feat_norm
        self.pl_module = pl_module
        self.compute_dtype = compute_dtype
        if pl_module is not None and hasattr(pl_module, "hparams"):
            try:
                dist_func = pl_module.hparams.SOLVER.DISTANCE_FUNC
            except (AttributeError, KeyError):
                pass
        self.dist_name = dist_func
        self.dist_func = get_dist_func(dist_func)
        self.last = {}
        if self.reranking is not None and (streamed or compute_dtype != torch.float32 or dist_func != "euclidean"):
            raise L.CreidError("R1_mAP(reranking=...) re-ranks the materialised euclidean fp32 matrix: not with streamed=True, "
                               f"compute_dtype={compute_dtype} or dist_func={dist_func!r}")
        self.prefilter = prefilter
        self.prefilter_capacity = EVAL_PREFILTER_CAPACITY if prefilter_capacity is None else int(prefilter_capacity)
        if prefilter is not None:
            if prefilter not in _H16:
                raise L.CreidError(f"R1_mAP(prefilter=...) must be torch.bfloat16 or torch.float16, got {prefilter}")
            if not streamed or compute_dtype != torch.float32 or dist_func != "euclidean" or self.reranking is not None:
                raise L.CreidError("R1_mAP(prefilter=...) is the streamed euclidean fp32 evaluation: not with streamed=False, "
                                   f"compute_dtype={compute_dtype}, dist_func={dist_func!r} or reranking")
            c = self.prefilter_capacity
            if c < 64 or c > 8192 or c & (c - 1):
                raise L.CreidError(f"R1_mAP(prefilter_capacity=...) must be a power of two, 64 .. 8192, got {c}")

    def _normalised(self, feats, out_dtype=None):
        """The feat_norm=True rows of every path and their square norms: l2_normalize, or -- query_expansion -- the expanded rows
        with the norms row_sqnorm gives them, the ones a feat_norm=False evaluation of these rows works with."""
        out_dtype = self.compute_dtype if out_dtype is None else out_dtype
        if self.query_expansion is None:
            return l2_normalize(feats, out_dtype=out_dtype, return_sqnorm=True)
        o = self.query_expansion
        _check_expansion_shape(o["k"], o["scope"], self.num_query, feats.shape[0] - self.num_query)
        info = {"timing": True} if (self.last.get("query_expansion") or {}).get("timing") else {}
        f, _ = _expanded_rows(feats, self.num_query, o["k"], float(o["alpha"]), o["rounds"], o["scope"], self.prefilter, out_dtype,
                              info)
        info.pop("timing", None)
        self._qe_info = {**o, **info}
        return f, row_sqnorm(f)

    def _rows(self, feats):
        """The rows one evaluation multiplies and their square norms, the same tensors on every route: euclidean -- normalised
        (or expanded) into compute_dtype, or cast to it; cosine -- fp32, and no norms (get_cosine normalises again).  Prints
        what the reference prints, so once per evaluation."""
        if self.dist_name != "euclidean":
            return (self._normalised(feats, torch.float32)[0] if self.feat_norm else feats), None
        if self.feat_norm:
            print("The test feature is normalized")
            return self._normalised(feats)
        f = feats if self.compute_dtype == torch.float32 else feats.to(self.compute_dtype)
        return f, row_sqnorm(f)

    def _keep_expansion_info(self):
        if self._qe_info is not None:
            self.last["query_expansion"] = self._qe_info

    def _ranked_from_indices(self, indices, distmat, junk):
        """The materialised routes' `last["ranked"]`: the first K' non-junk entries of the ranked rows and their distances."""
        idx, matched, count = rank_keep_topk(indices, min(self.ranked_topk, indices.shape[1]), junk)
        return dict(indices=idx, distances=gather_ranked(distmat, idx), matched=matched, count=count)

    def _roc_from_matrix(self, distmat, junk):
        """The materialised routes' `last["roc"]`: the operating points of their own matrix."""
        return roc_matrix(distmat, junk, self.roc)

    def compute(self, feats, pids, camids, respect_camids=False):
        if not isinstance(feats, torch.Tensor) or not feats.is_cuda:
            raise L.CreidError("R1_mAP.compute needs device features (no CPU fallback)")
        if self.prefilter is not None and respect_camids:
            raise L.CreidError("R1_mAP(prefilter=...) evaluates plain camera ids: not with respect_camids=True")
        feats = _pad_width(feats.float().contiguous())
        nq = self.num_query
        if self.streamed and self.dist_name == "euclidean" and self.compute_dtype in (torch.float32,) + _H16:
            return self._compute_streamed(feats, pids, camids, camsets=bool(respect_camids))
        f, sq = self._rows(feats)
        if self.dist_name != "euclidean":
            distmat = self.dist_func(f[:nq].contiguous(), f[nq:].contiguous())
        elif self.reranking is not None:
            distmat = re_ranking(f[:nq], f[nq:], **self.reranking)
        else:
            distmat = get_euclidean(f[:nq], f[nq:], sq[:nq].contiguous(), sq[nq:].contiguous())
        pids = np.asarray(pids)
        if respect_camids:                      # (ragged list-of-lists of camera sets: keep as a list)
            indices = rank_rows(distmat)
            cmc, mAP, all_topk, single = eval_func(indices, pids[:nq], pids[nq:], camids[:nq], camids[nq:],
                                                   self.max_rank, respect_camids)
            self.last = dict(distmat=distmat, indices=indices, single_performance=single)
            if self.ranked_topk is not None:
                self.last["ranked"] = self._ranked_from_indices(
                    indices, distmat, JunkFilter.from_labels(pids, camids, nq, feats.device, respect_camids=True))
            if self.roc is not None:
                self.last["roc"] = self._roc_from_matrix(
                    distmat, JunkFilter.from_labels(pids, camids, nq, feats.device, respect_camids=True))
            self._keep_expansion_info()
            return cmc, mAP, all_topk
        # np.argsort + eval_func's per-query loop in ONE pass: the ranked rows are evaluated while they are still in LDS
        camids = np.asarray(camids)
        indices, valid, ap, first = rank_rows_eval(distmat, pids[:nq], pids[nq:], camids[:nq], camids[nq:])
        max_rank = self.max_rank
        if distmat.shape[1] < max_rank:         # utils/eval_reid.py:33-35
            max_rank = distmat.shape[1]
            print("Note: number of gallery samples is quite small, got {}".format(distmat.shape[1]))
        cmc, mAP, topk, _ = eval_reduce_device(valid, ap, first, max_rank)
        cmc_h, mAP_h, topk_h, _, _, _, single = _unpack_results(_pack_results(cmc, mAP, topk, valid, ap), max_rank, pids[:nq])
        self.last = dict(distmat=distmat, indices=indices, single_performance=single, valid=valid, ap=ap, first=first)
        if self.ranked_topk is not None:
            self.last["ranked"] = self._ranked_from_indices(indices, distmat, JunkFilter.from_labels(pids, camids, nq, feats.device))
        if self.roc is not None:
            self.last["roc"] = self._roc_from_matrix(distmat, JunkFilter.from_labels(pids, camids, nq, feats.device))
        self._keep_expansion_info()
        return cmc_h, mAP_h, topk_h

    def _compute_streamed(self, feats, pids, camids, camsets=False):
        """camsets: `camids` is the respect_camids=True argument (a list of camera-id lists, or a CameraSets); the gallery
        entries' sets become bitmasks and the same three launches run on them (StreamPlan(camsets=True))."""
        nq = self.num_query
        g_masks = None
        if camsets:
            q_cams, g_masks = _camset_split(camids, nq)           # (raises before anything is launched)
        # exactly the rows and norms of the materialised branch of compute(): both paths multiply the same tensors
        if self.compute_dtype in _H16:
            feats = _pad_width(feats, 8)
        f, sq = self._rows(feats)
        pids = np.asarray(pids)
        hint_key = (nq, len(pids) - nq) + (("camsets",) if camsets else ())       # (a capacity learnt on sets is no guide for ids)
        plan_kw = {}
        if camsets:
            on_dev = isinstance(g_masks, torch.Tensor)
            camids = q_cams if on_dev else np.concatenate([q_cams, g_masks])      # plain query cameras, then the masks
            plan_kw = dict(camsets=True, g_cam_masks=g_masks if on_dev else None)
        else:
            camids = np.asarray(camids)
        # index built on the device BEHIND the normalisation launch.  Its 8-byte read-back (finish: the positive-list
        # capacity) would be a host synchronisation in the middle of the pipeline; an evaluation of the same shape as an
        # earlier one instead ASSUMES that call's capacity, enqueues everything, and checks the assumption against the
        # plan's statistics in the final read-back (wrong -> the contraction is redone with the right capacity; a capacity
        # larger than needed gives identical results)
        plan = StreamPlan.on_device(pids, camids, nq, feats.device, **plan_kw)
        hint = _CAP_HINT.get(hint_key) if os.environ.get("CREID_EVAL_SPECULATE", "1") == "1" else None
        speculative = plan.cap is None and bool(hint)  # 0 = "do not speculate": the last label set of this shape had overflow queries
        if speculative:
            plan.cap, plan.overflow = hint, np.zeros(0, np.int64)
        if plan.cap is None:
            plan.finish()
        fq, fg = f[:nq], f[nq:]
        qq, gg = sq[:nq].contiguous(), sq[nq:].contiguous()
        pf = clock = None
        if self.prefilter is not None:
            # zero columns behind the normalised rows change neither a norm, a rounding nor an fmaf chain
            fq, fg = _pad_width(fq, 8), _pad_width(fg, 8)
            clock = _StageClock(bool((self.last.get("prefilter") or {}).get("timing")))
        max_rank = min(self.max_rank, fg.shape[0])
        for _ in range(2):  # a speculation that fails is redone once, synchronously, on the same rows and the same clock
            if self.prefilter is not None:
                valid, ap, first, pf = _stream_eval_prefilter(fq, fg, qq, gg, plan, self.prefilter, self.prefilter_capacity, clock)
                res = _PerQuery(valid, ap, first)
            else:
                res = stream_eval(fq, fg, qq, gg, plan)
            if len(plan.overflow):
                # queries with more positives than the LDS list holds: the general path on just those rows
                rows = torch.as_tensor(plan.overflow, device=feats.device)
                d = get_euclidean(fq.index_select(0, rows), fg, qq.index_select(0, rows), gg)
                res.merge(rows, eval_func_device(rank_rows(d), pids[:nq][plan.overflow], plan.g_pids, camids[:nq][plan.overflow],
                                                 plan.g_cams, self.max_rank, camsets=camsets)[4:])
            cmc, mAP, topk, _ = eval_reduce_device(*res, max_rank)
            # riding along: the plan's statistics, and in front of them the pre-filter's [flags (m) | gallery maxima (4) | margin max]
            tail = [plan._stats.double() if speculative else torch.zeros(2, dtype=torch.float64, device=feats.device)]
            if pf is not None:
                tail = [pf["flags"].double(), pf["gmax"], pf["margin_max"]] + tail
            cmc_h, mAP_h, topk_h, _, _, tail, single = _unpack_results(_pack_results(cmc, mAP, topk, res.valid, res.ap, tail),
                                                                       max_rank, pids[:nq])
            if not speculative:
                if getattr(plan, "_stats", None) is not None:
                    _CAP_HINT[hint_key] = 0 if len(plan.overflow) else plan.cap
                break
            need = 2
            while need < max(int(tail[-2]), 1):
                need *= 2
            nover = int(tail[-1])
            # a label set with overflow queries (> 128 positives) cannot be speculated on (their list is only known to the
            # synchronous plan): remember that instead of a capacity, so that evaluations of this shape stop redoing
            _CAP_HINT[hint_key] = 0 if nover > 0 else need
            if need <= plan.cap and nover == 0:
                break
            plan.cap, speculative = None, False                  # the assumed capacity was too small: redo, synchronously
            plan.finish()
        info = None
        if pf is not None:
            bad = np.setdiff1d(np.nonzero(tail[:nq] != 0)[0], plan.overflow)   # (the general path's rows keep their results)
            if len(bad):
                # rows whose list overflowed: the fp32 count on just those rows, merged and reduced again (a second read-back,
                # only when it happens)
                _stream_eval_prefilter_repair(fq, fg, qq, gg, plan, pf, bad, *res)
                cmc, mAP, topk, _ = eval_reduce_device(*res, max_rank)
                cmc_h, mAP_h, topk_h, _, _, _, single = _unpack_results(_pack_results(cmc, mAP, topk, res.valid, res.ap),
                                                                        max_rank, pids[:nq])
            clock.mark("repair")
            info = dict(dtype=self.prefilter if np.isfinite(tail[nq:nq + 4]).all() else None, capacity=self.prefilter_capacity,
                        margin_max=float(tail[nq + 4]), fallback_rows=int(len(bad)), ambiguous=pf["ambiguous"])
            # per stage, summed over a redone speculation: the failed attempt's read-back and plan.finish() lie between its
            # `rescore` mark and the second attempt's `pack` mark, so they are billed to `pack`
            if clock.on:
                info["stage_ms"] = clock.stage_ms()
        valid, ap, first = res
        self.last = dict(valid=valid, ap=ap, first=first, single_performance=single, plan=plan)
        if info is not None:
            self.last["prefilter"] = info
        if self.ranked_topk is not None:
            # the lists the metrics above are defined on, from the rows and norms the evaluation multiplied: no matrix either
            junk = JunkFilter(plan.q_pids, plan.q_cams, plan.g_pids, plan.g_cams, camsets=plan.camsets)
            ridx, rdist = topk_stream(fq, fg, min(self.ranked_topk, fg.shape[0]), qq, gg, junk=junk)
            self.last["ranked"] = dict(indices=ridx, distances=rdist, matched=junk.matched(ridx),
                                       count=(ridx >= 0).sum(1, dtype=torch.int32))
        if self.roc is not None:
            # the operating points of the distances the metrics above rank by, from the same rows and norms: no matrix either
            junk = JunkFilter(plan.q_pids, plan.q_cams, plan.g_pids, plan.g_cams, camsets=plan.camsets)
            self.last["roc"] = roc_stream(fq, fg, junk, self.roc, qq, gg)
        self._keep_expansion_info()
        return cmc_h, mAP_h, topk_h

    def compute_chunked(self, feats, pids, camids, query_chunk=4096, respect_camids=False):
        """Galleries whose m x n matrix must not be materialised (the reference's `_commpute_batches_double` path,
        utils/reid_metric.py:93-110,126-129, chunks the gallery on the host): the euclidean distance (fp32, bf16 or f16
        compute dtype) goes through the streamed kernels in ONE pass with no matrix at all; the cosine distance processes
        `query_chunk` query rows at a time (distance tile, rank, CMC/AP scan on the device, only per-query results kept).
        respect_camids=True (camera sets, as in compute()): the streamed kernels only -- CreidError with the cosine distance."""
        if not isinstance(feats, torch.Tensor) or not feats.is_cuda:
            raise L.CreidError("R1_mAP.compute_chunked needs device features (no CPU fallback)")
        if self.reranking is not None:
            raise L.CreidError("R1_mAP.compute_chunked never holds the [nq, ng] matrix that reranking replaces: use compute()")
        if self.prefilter is not None and respect_camids:
            raise L.CreidError("R1_mAP(prefilter=...) evaluates plain camera ids: not with respect_camids=True")
        from .parallel import merge_eval_results
        euclid = self.dist_name == "euclidean"
        feats = _pad_width(feats.float().contiguous())
        if euclid and self.compute_dtype in (torch.float32,) + _H16:
            return self._compute_streamed(feats, pids, camids, camsets=bool(respect_camids))
        if respect_camids:
            raise L.CreidError("R1_mAP.compute_chunked(respect_camids=True) runs the streamed euclidean kernels only "
                               f"(dist_func={self.dist_name!r}, compute_dtype={self.compute_dtype})")
        nq = self.num_query
        # SOLVER.DISTANCE_FUNC = cosine (utils/reid_metric.py:51-59,93-110 works with either function): the same query-chunk
        # loop on the cosine matrix
        f, sq = self._rows(feats)
        g, gg = f[nq:].contiguous(), (sq[nq:].contiguous() if sq is not None else None)
        pids = np.asarray(pids); camids = np.asarray(camids)
        dev = feats.device
        gp, gc = _dev_i64(pids[nq:], dev), _dev_i64(camids[nq:], dev)
        vs, aps, firsts = [], [], []
        junk = JunkFilter.from_labels(pids, camids, nq, dev) if self.ranked_topk is not None or self.roc is not None else None
        ranked = []
        chunk_dist = lambda lo, hi: (get_euclidean(f[lo:hi], g, sq[lo:hi].contiguous(), gg) if euclid
                                     else self.dist_func(f[lo:hi].contiguous(), g))
        roc_hist0 = torch.zeros((1, 2, 1 << _ROC_PASSES[0][1]), dtype=torch.int64, device=dev) if self.roc is not None else None
        for lo in range(0, nq, query_chunk):
            hi = min(nq, lo + query_chunk)
            d = chunk_dist(lo, hi)
            idx = rank_rows(d)
            if self.ranked_topk is not None:                      # per chunk, before its matrix and indices are freed
                ranked.append(self._ranked_from_indices(idx, d, junk.rows(slice(lo, hi))))
            if roc_hist0 is not None:                             # the first radix pass rides along
                distance_histogram_matrix(d, junk.rows(slice(lo, hi)), bits=_ROC_PASSES[0][1], out=roc_hist0)
            del d
            _, _, _, _, v, a, fr = eval_func_device(idx, pids[lo:hi], gp, camids[lo:hi], gc, self.max_rank)
            vs.append(v); aps.append(a); firsts.append(fr)
            del idx
        v = torch.cat(vs).cpu().numpy() > 0; a = torch.cat(aps).cpu().numpy(); fr = torch.cat(firsts).cpu().numpy()
        if junk is not None:
            self.last = {}
        if self.ranked_topk is not None:
            self.last["ranked"] = {key: torch.cat([r[key] for r in ranked]) for key in ranked[0]}
        if self.roc is not None:
            def later_pass(prefix, pb, bits, out):                # the two later passes: every chunk's matrix once more
                for lo in range(0, nq, query_chunk):
                    hi = min(nq, lo + query_chunk)
                    distance_histogram_matrix(chunk_dist(lo, hi), junk.rows(slice(lo, hi)), prefix=prefix, prefix_bits=pb, bits=bits,
                                              out=out)
            self.last["roc"] = _roc_select(later_pass, self.roc, dev, first_hist=roc_hist0)
        self._keep_expansion_info()
        return merge_eval_results(v, a, fr, min(self.max_rank, g.shape[0]))
