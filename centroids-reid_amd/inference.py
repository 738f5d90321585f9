"""Second caller of stages A + D + E: embedding extraction and similarity search with
the reference's on-disk formats.

Mirrors inference/inference_utils.py:104-159 (`_inference`, `run_inference`, `create_pid_path_index`,
`calculate_centroids`) and inference/get_similar.py:99-137 (normalise -> distance -> argsort -> top-k dict ->
`results.npy` / `query_embeddings.npy` / `query_paths.npy`), inference/create_embeddings.py:75-97
(`embeddings.npy`, `paths.npy`).  All arithmetic runs on the device through the same kernels as evaluation;
files are written with numpy exactly like the reference (dict-of-dicts pickled by np.save).
"""
from __future__ import annotations

from pathlib import Path
from typing import Callable, Dict, List

import numpy as np
import torch

from . import _lib as L
from . import reid_metric as rm
from .transforms import RaggedImages


def _inference(model, batch, use_cuda=True, normalize_with_bn=True, transform=None):
    """inference_utils.py:104-113: eval-mode backbone (+ BNNeck).  `data` is the reference's fp32 NCHW batch, or -- with
    `transform` = ReidTransforms(cfg).build_transforms(is_train=False) -- a uint8 [B, H, W, 3] batch of resized images: the test
    transform (build.py:27-31 after the Resize) then runs on the device and writes the stem convolution's operand directly.
    Images that are NOT resized come as a transforms.RaggedImages or as a plain list of uint8 [h, w, 3] arrays of any sizes
    (packed here): the Resize then runs on the device as well, with Pillow's result byte for byte."""
    model.eval()
    with torch.no_grad():
        data, _, filename = batch
        data = _as_batch_data(data)
        if isinstance(data, RaggedImages) or data.dtype == torch.uint8:
            if transform is None:
                raise ValueError("uint8 image batches need `transform` (transforms.ReidTransforms(cfg).build_transforms(False))")
            if callable(transform) and getattr(transform, "_lazy_cfg", None) is not None:
                transform = transform()                          # built on the first uint8 batch only (run_inference)
            # the device-side transform IS a GPU kernel: a uint8 batch goes to the device whatever `use_cuda` says (the flag only
            # keeps the reference's meaning for float batches, which a CPU-resident model could not run here anyway)
            # (a RaggedImages is resized to the transform's size first, on the device too: transforms.DeviceTransform.resize_batch)
            data = transform(data.cuda(), layout="stem", dtype=model.backbone.engine_for(False).dtype)   # (bf16x3: fp32)
        else:
            data = data.cuda() if use_cuda else data
        _, global_feat = model.backbone(data)
        if normalize_with_bn:
            global_feat = model.bn(global_feat)
        return global_feat, filename


def _as_batch_data(data):
    """A loader batch's `data` as run_inference handles it: a tensor, or a RaggedImages (a list of images is packed)."""
    if isinstance(data, (list, tuple)):
        return RaggedImages.pack(data)
    return data


def _can_join(a, b) -> bool:
    """Whether two batches' `data` can be concatenated into one forward."""
    if isinstance(a, RaggedImages) or isinstance(b, RaggedImages):
        return isinstance(a, RaggedImages) and isinstance(b, RaggedImages) and a.device == b.device
    return a.dtype == b.dtype and a.shape[1:] == b.shape[1:] and a.device == b.device


def run_inference(model, val_loader, cfg=None, print_freq=0, use_cuda=True, transform=None, macro_batch=512):
    """inference_utils.py:116-131 -> (embeddings float32 [N, D] ndarray, paths ndarray); the embeddings are
    also kept on the device in `run_inference.last_device_embeddings` for a following get_similar().  A loader of uint8
    [B, H, W, 3] batches is normalised on the device (`transform`, or the test transform built from `cfg`); a loader of
    RaggedImages, or of plain lists of uint8 [h, w, 3] arrays of any sizes, is resized there first (transforms.py).

    macro_batch (round 5): consecutive loader batches are concatenated until at least this many images are waiting and embedded
    with ONE forward -- the eval-mode forward treats every image independently (BatchNorm folded to running statistics, eval-mode
    BNNeck), and every kernel variant the library may pick for another batch size produces the same bits, so the embeddings are
    IDENTICAL to the per-batch ones (tests/test_centroid_eval_gpu.py), while a forward of 512 images runs at 78 k images/s against
    65 k for the reference's TEST.IMS_PER_BATCH = 128 (profiles/r05_embed_batch_sweep.md: the persistent convolution kernels
    only pipeline across tiles when a workgroup owns more than one).  0 / None: one forward per loader batch, as the reference."""
    embs, paths = [], []
    if transform is None and cfg is not None:
        # built lazily: a float loader never touches cfg.INPUT.* (a partial cfg without those keys stays usable)
        built = {}

        def _lazy():
            if "t" not in built:
                from .transforms import ReidTransforms
                built["t"] = ReidTransforms(cfg).build_transforms(is_train=False)
            return built["t"]
        _lazy._lazy_cfg = cfg
        transform = _lazy
    pend, npend = [], 0

    def flush():
        nonlocal pend, npend
        if not pend:
            return
        if len(pend) == 1:
            data = pend[0][0]
        elif isinstance(pend[0][0], RaggedImages):
            data = RaggedImages.cat([b[0] for b in pend])
        else:
            data = torch.cat([b[0] for b in pend])
        names = [n for b in pend for n in list(b[2])]
        e, p = _inference(model, (data, None, names), use_cuda, transform=transform)
        embs.append(e.float())
        paths.extend(list(p))
        pend, npend = [], 0
    for batch in val_loader:
        data = _as_batch_data(batch[0])
        if pend and not _can_join(pend[0][0], data):
            flush()                                              # batches that cannot be concatenated go separately
        pend.append((data, *batch[1:]))
        npend += len(data)
        if not macro_batch or npend >= macro_batch:
            flush()
    flush()
    dev = torch.cat(embs)
    run_inference.last_device_embeddings = dev
    return dev.cpu().numpy(), np.array(paths)


def create_pid_path_index(paths: List[str], func: Callable[[str], str]) -> Dict[str, list]:
    """inference_utils.py:134-144."""
    index: Dict[str, list] = {}
    for i, p in enumerate(paths):
        index.setdefault(func(p), []).append(i)
    return index


def calculate_centroids(embeddings, pid_path_index):
    """inference_utils.py:147-159: per-PID mean embedding -> (centroids [n_pid, D] float32, pid keys as str)."""
    keys = list(pid_path_index.keys())
    order = np.concatenate([np.asarray(pid_path_index[k], np.int64) for k in keys])
    offsets = np.concatenate([[0], np.cumsum([len(pid_path_index[k]) for k in keys])]).astype(np.int64)
    emb = embeddings if isinstance(embeddings, torch.Tensor) else torch.from_numpy(np.asarray(embeddings, np.float32))
    emb = emb.float().cuda().contiguous()
    out = torch.empty((len(keys), emb.shape[1]), dtype=torch.float32, device=emb.device)
    order_t = torch.as_tensor(order, device=emb.device)        # named: must outlive the launch
    off_t = torch.as_tensor(offsets, device=emb.device)
    L.check(L.lib().creid_gather_mean_rows(L.ptr(emb), L.ptr(order_t), L.ptr(off_t), len(keys), emb.shape[1],
                                           L.ptr(out), L.stream()), "creid_gather_mean_rows")
    return out.cpu().numpy(), np.array(keys, dtype=np.str_)


def save_embeddings(save_dir, embeddings, paths):
    """inference/create_embeddings.py:92-97."""
    d = Path(save_dir); d.mkdir(exist_ok=True, parents=True)
    np.save(d / "embeddings.npy", np.asarray(embeddings))
    np.save(d / "paths.npy", np.asarray(paths))


def load_gallery(load_dir):
    d = Path(load_dir)
    return np.load(d / "embeddings.npy", allow_pickle=True), np.load(d / "paths.npy", allow_pickle=True)


STREAM_MATRIX_BYTES = 1 << 30      # get_similar(streamed="auto"): an m x n fp32 matrix beyond this is not materialised whole


def _similar_materialised(q, g, topk, distance_func):
    """The m x n matrix and its ranking: (indices, distances) as host arrays."""
    return _select_rows(rm.get_dist_func(distance_func)(x=q, y=g).contiguous(), topk)


def _select_rows(distmat, topk):
    if topk:                                                   # top-k selection kernel: no full sort of the row
        indices, dist_sel = rm.topk_rows(distmat, min(int(topk), distmat.shape[1]))
    else:
        indices = rm.rank_rows(distmat)
        dist_sel = torch.gather(distmat, 1, indices)
    return indices.cpu().numpy(), dist_sel.cpu().numpy()


def get_similar(embeddings, paths, embeddings_gallery, paths_gallery, topk=0, normalize_features=True,
                distance_func="euclidean", streamed="auto", stats=None, compute_dtype=torch.float32, reranking=False,
                prefilter=None, query_expansion=False):
    """inference/get_similar.py:99-125 -> {query_path: {"indices", "paths", "distances"}} (numpy arrays).

    streamed: False -- the m x n distance matrix is written and every row selected from it (get_dist_func + topk_rows /
    rank_rows).  True -- reid_metric.topk_stream: the same indices and distance bits with no matrix; squared-L2 top-k only
    (CreidError for cosine, topk = 0 or k > 1024).  "auto" -- the matrix path unless it would exceed STREAM_MATRIX_BYTES; then
    the streamed path when the call is streamable and its threshold sample is at most a quarter of the gallery, else the
    matrix path over chunks of query rows (the result is the same, the matrix never exists whole).
    compute_dtype: torch.float32 (default, the reference's arithmetic), torch.bfloat16 or torch.float16 -- the (optionally
    normalised) features are rounded ONCE to that type and every path works on the rounded features with the 16-bit MFMA
    kernels (half the gallery bytes; the distances stay fp32).  The three paths still agree bit for bit with one another.
    reranking: True (the defaults of reid_metric.re_ranking) or a dict of k1 / k2 / lambda_value -- the k-reciprocal re-ranked
    matrix is ranked in place of the distance matrix and the returned "distances" are its values; always the materialised path
    (CreidError with streamed=True, a 16-bit compute_dtype or the cosine distance).
    prefilter: torch.bfloat16 or torch.float16 -- reid_metric.topk_stream(prefilter=...): the fp32 result, bit for bit, with the
    contraction on the 16-bit MFMA.  "auto" then streams whenever the call is streamable (squared L2, 1 <= k <= 1024), whatever
    the matrix size; CreidError with streamed=False, a 16-bit compute_dtype, reranking, or a call that cannot stream.
    query_expansion: True (the defaults of reid_metric.query_expansion) or a dict of k / alpha / rounds / scope -- the normalised
    rows are expanded by their nearest neighbours before the search (fp32 arithmetic, the last normalisation into compute_dtype;
    blind to labels; `prefilter` also goes to its neighbour search) and every path then runs on the expanded rows, as it would on
    reid_metric.query_expansion's result with normalize_features=False.  CreidError, before any upload, with
    normalize_features=False: expansion is defined on unit rows.  stats["query_expansion"] holds the options and its stats.
    stats (a dict) receives "path" ("materialised" | "streamed" | "chunked" | "reranked"), topk_stream's counters ("prefilter"
    among them: what ran) and re_ranking's statistics.
    Open-set use ("is this person or item in the gallery at all?"): the returned squared-L2 "distances" compare directly with
    the `threshold` reid_metric.roc_stream / R1_mAP(roc=...) gives for a false-accept rate on validation data of the same
    normalisation and compute_dtype -- an entry is accepted iff its distance is STRICTLY below the threshold."""
    rr = rm.rerank_options(reranking)
    if rr is not None and (streamed is True or compute_dtype != torch.float32 or distance_func != "euclidean"):
        raise L.CreidError("get_similar(reranking=...) re-ranks the materialised squared-L2 fp32 matrix: not with streamed=True, "
                           f"compute_dtype={compute_dtype} or distance_func={distance_func!r}")
    qe = rm.expansion_options(query_expansion)
    if qe is not None and not normalize_features:
        raise L.CreidError("get_similar(query_expansion=...) expands unit rows: not with normalize_features=False")
    if streamed not in (True, False, "auto"):
        raise ValueError(f"streamed must be True, False or 'auto', got {streamed!r}")
    if prefilter is not None:
        if prefilter not in (torch.bfloat16, torch.float16):
            raise L.CreidError(f"get_similar: prefilter must be torch.bfloat16, torch.float16 or None, got {prefilter}")
        if streamed is False or compute_dtype != torch.float32 or rr is not None:
            raise L.CreidError("get_similar(prefilter=...) pre-filters the streamed fp32 top-k: not with streamed=False, "
                               f"compute_dtype={compute_dtype} or reranking")
    if compute_dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise L.CreidError(f"get_similar: compute_dtype must be torch.float32, torch.bfloat16 or torch.float16, got {compute_dtype}")
    q = torch.as_tensor(np.asarray(embeddings, np.float32)).cuda() if not isinstance(embeddings, torch.Tensor) else embeddings.float().cuda()
    g = torch.as_tensor(np.asarray(embeddings_gallery, np.float32)).cuda() if not isinstance(embeddings_gallery, torch.Tensor) else embeddings_gallery.float().cuda()
    qe_info = {}
    if qe is not None:
        q, g = rm.query_expansion(q.contiguous(), g.contiguous(), **qe, prefilter=prefilter, out_dtype=compute_dtype, stats=qe_info)
    elif normalize_features:
        q, g = rm.l2_normalize(q.contiguous(), out_dtype=compute_dtype), rm.l2_normalize(g.contiguous(), out_dtype=compute_dtype)
    elif compute_dtype != torch.float32:
        q, g = q.to(compute_dtype), g.to(compute_dtype)
    if compute_dtype != torch.float32:                         # the 16-bit kernels load 8-element k-chunks; zero columns change nothing
        q, g = rm._pad_width(q, 8), rm._pad_width(g, 8)
    q, g = q.contiguous(), g.contiguous()
    m, n = q.shape[0], g.shape[0]
    k = min(int(topk), n) if topk else 0
    streamable = distance_func == "euclidean" and 1 <= k <= 1024
    if (streamed is True or prefilter is not None) and not streamable:
        raise L.CreidError("get_similar(streamed=True) and get_similar(prefilter=...) are squared-L2 top-k retrieval with "
                           f"1 <= k <= 1024: got distance_func={distance_func!r}, topk={topk}")
    big = m * n * 4 > STREAM_MATRIX_BYTES
    info = {}
    if rr is not None:
        idx, dist_sel = _select_rows(rm.re_ranking(q, g, **rr, stats=info), topk)
        info["path"] = "reranked"
    elif streamed is True or prefilter is not None or (streamed == "auto" and big and streamable and
                                                       rm.topk_stream_sample(k, n) <= n // 4):
        indices, dist_sel = rm.topk_stream(q, g, k, stats=info, prefilter=prefilter)
        idx, dist_sel = indices.cpu().numpy(), dist_sel.cpu().numpy()
        info["path"] = "streamed"
    elif streamed == "auto" and big:
        rows = max(1, STREAM_MATRIX_BYTES // (n * 4))
        parts = [_similar_materialised(q[r0:r0 + rows], g, topk, distance_func) for r0 in range(0, m, rows)]
        idx, dist_sel = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        info["path"] = "chunked"
    else:
        idx, dist_sel = _similar_materialised(q, g, topk, distance_func)
        info["path"] = "materialised"
    if qe is not None:
        info["query_expansion"] = {**qe, **qe_info}
    if stats is not None:
        stats.update(info)
    paths_gallery = np.asarray(paths_gallery)
    return {qp: {"indices": idx[i, :], "paths": paths_gallery[idx[i, :]], "distances": dist_sel[i, :]}
            for i, qp in enumerate(paths)}


def save_results(out_dir, results, embeddings, paths):
    """inference/get_similar.py:127-137."""
    d = Path(out_dir); d.mkdir(exist_ok=True, parents=True)
    np.save(d / "results.npy", results)
    np.save(d / "query_embeddings.npy", np.asarray(embeddings))
    np.save(d / "query_paths.npy", np.asarray(paths))
