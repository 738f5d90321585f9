"""GPU: the C entry points behind the evaluation and retrieval host code, call by call.  The parity tests pin what every route
computes; this pins what it launches: `L.lib` is wrapped (the recording proxy of tests/test_layer_audit_gpu.py, kept in
order) and the sequence of creid_* symbols each call reads is compared with the list written down here.  A launch added, lost
or reordered by a change of reid_metric.py shows up as a different list."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NQ, NG, D = 70, 513, 100

PLAN = ["creid_l2norm_rows", "creid_stream_plan"]
TAIL = ["creid_stream_finalize", "creid_eval_reduce"]
STREAMED_FP32 = PLAN + ["creid_stream_poslist", "creid_stream_count"] + TAIL
RANKED = ["creid_sqdist_matrix", "creid_junk_mask_rows", "creid_topk_rows", "creid_stream_topk_collect_keep",
          "creid_stream_topk_select"]
EVAL_CALLS = {
    "fp32-first": STREAMED_FP32,
    "fp32-second": STREAMED_FP32,
    "bf16": PLAN + ["creid_stream_poslist_h16", "creid_stream_count_h16"] + TAIL,
    "prefilter": PLAN + ["creid_prefilter_pack", "creid_prefilter_pack", "creid_stream_poslist", "creid_stream_count_band_h16",
                         "creid_stream_count_rescore"] + TAIL,
    "camsets": ["creid_l2norm_rows", "creid_stream_plan_camsets", "creid_stream_poslist_camsets", "creid_stream_count"] + TAIL,
    "ranked": STREAMED_FP32 + RANKED,
    "materialised": ["creid_l2norm_rows", "creid_sqdist_matrix", "creid_rank_rows_workspace_bytes", "creid_rank_rows_eval",
                     "creid_eval_reduce"],
}
TOPK_CALLS = {
    "fp32": ["creid_sqdist_matrix", "creid_topk_rows", "creid_stream_topk_collect", "creid_stream_topk_select"],
    "junk": ["creid_sqdist_matrix", "creid_junk_mask_rows", "creid_topk_rows", "creid_stream_topk_collect_keep",
             "creid_stream_topk_select"],
}


class _LibProxy:
    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        if name.startswith("creid_"):
            self._calls.append(name)
        return getattr(self._lib, name)


@pytest.fixture
def recorded(monkeypatch):
    """record(fn) -> the creid_* symbols fn read from the library, in order."""
    from centroids_reid_amd import _lib as L
    real = L.lib()

    def record(fn):
        calls = []
        with monkeypatch.context() as mp:
            mp.setattr(L, "lib", lambda: _LibProxy(real, calls))
            fn()
            torch.cuda.synchronize()
        return calls
    return record


def _eval_case():
    rng = np.random.default_rng(NQ * 7 + NG)
    feats = torch.from_numpy(rng.standard_normal((NQ + NG, D)).astype(np.float32)).cuda()
    return feats, rng.integers(0, 9, NQ + NG), rng.integers(0, 2, NQ + NG)


def test_evaluation_entry_points(recorded, capsys):
    """R1_mAP.compute at 70 x 513 x 100, 9 pids over 2 cameras (17 .. 35 positives per query: capacity 64, no query beyond
    128): the first streamed call of a shape reads the plan's statistics before it launches, the second speculates on the
    capacity the first one learnt -- the same launches either way."""
    from centroids_reid_amd import reid_metric as rm
    feats, pids, cams = _eval_case()
    camsets = [[int(c)] for c in cams]
    runs = {
        "fp32-first": (dict(streamed=True), cams, False),
        "fp32-second": (dict(streamed=True), cams, False),
        "bf16": (dict(streamed=True, compute_dtype=torch.bfloat16), cams, False),
        "prefilter": (dict(streamed=True, prefilter=torch.bfloat16), cams, False),
        "camsets": (dict(streamed=True), camsets, True),
        "ranked": (dict(streamed=True, ranked_topk=5), cams, False),
        "materialised": (dict(streamed=False), cams, False),
    }
    got = {}
    for name, (kw, camids, respect) in runs.items():
        if name != "fp32-second":
            rm._CAP_HINT.clear()
        metric = rm.R1_mAP(num_query=NQ, **kw)
        got[name] = recorded(lambda: metric.compute(feats, pids, camids, respect_camids=respect))
        if name.startswith("fp32"):
            assert rm._CAP_HINT == {(NQ, NG): 64}
        if name == "prefilter":
            assert metric.last["prefilter"]["fallback_rows"] == 0
    for name, calls in got.items():
        print(name, calls)
    assert got == EVAL_CALLS


def test_topk_stream_entry_points(recorded):
    """topk_stream at 150 x 700 x 40, k = 5, sample 64, in one row chunk and with nothing to repair: the sample slice, its
    threshold, the collect and the select; with junk= the mask of the sample slice in front of the threshold."""
    from centroids_reid_amd import reid_metric as rm
    rng = np.random.default_rng(150 * 7 + 700)
    q = torch.from_numpy(rng.standard_normal((150, 40)).astype(np.float32)).cuda()
    g = torch.from_numpy(rng.standard_normal((700, 40)).astype(np.float32)).cuda()
    qq, gg = rm.row_sqnorm(q), rm.row_sqnorm(g)
    lab = lambda hi, n: torch.from_numpy(rng.integers(0, hi, n)).cuda()
    junk = rm.JunkFilter(lab(40, 150), lab(3, 150), lab(40, 700), lab(3, 700))
    got = {}
    for name, kw in (("fp32", {}), ("junk", dict(junk=junk))):
        stats = {}
        got[name] = recorded(lambda: rm.topk_stream(q, g, 5, qq, gg, sample=64, stats=stats, **kw))
        assert stats["fallback_rows"] == 0
    for name, calls in got.items():
        print(name, calls)
    assert got == TOPK_CALLS
