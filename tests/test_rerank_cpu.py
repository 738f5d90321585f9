"""CPU: the float64 reference of k-reciprocal re-ranking (tests/rerank_ref.py) on examples small enough to check by hand,
its limiting cases, and the refusals of the device API that need no device."""
import numpy as np
import pytest
import torch

from rerank_ref import clustered_int_features, int_sqdist, rerank_reference


def test_reference_on_a_line_of_twelve_points():
    """x_i = i, i = 0 .. 11, k1 = 6 (seven neighbours, kh = 3).  Ties by index: row 3 lists 3 2 4 1 5 0 6.
    R(0, 6) = {0, 1, 2, 3} (4, 5, 6 do not list 0 back).  R(3, 3) = {1, 2, 3, 4} shares 3 of its 4 members with it
    (9 > 8), so 4 joins R*(0); R(1, 3) and R(2, 3) are subsets.  At the other end R(11, 6) = {8, 9, 10, 11} and
    R(8, 3) = {7, 8, 9} shares only 2 of 3 (6 > 6 fails), so 7 stays out of R*(11)."""
    d = int_sqdist(np.arange(12)[:, None])
    out, sets, Vq = rerank_reference(d, 3, 6, 2, 0.3)
    expected = [[0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 3, 4, 5, 6, 7],
                [1, 2, 3, 4, 5, 6, 7, 8], [3, 4, 5, 6, 7, 8, 9], [4, 5, 6, 7, 8, 9, 10], [5, 6, 7, 8, 9, 10, 11],
                [6, 7, 8, 9, 10, 11], [7, 8, 9, 10, 11], [8, 9, 10, 11]]
    assert [s.tolist() for s in sets] == expected
    assert out.shape == (3, 9) and np.isfinite(out).all() and out.min() >= 0 and out.max() <= 1
    # V'(0) = (V(0) + V(1)) / 2 lives on R*(0) | R*(1) = {0 .. 4} and sums to one
    assert np.nonzero(Vq[0])[0].tolist() == [0, 1, 2, 3, 4] and abs(Vq[0].sum() - 1) < 1e-15
    # query 0 and gallery row 11 share no column: J = 1, and od(0, 11) = 1 (the row's maximum)
    assert out[0, 8] == 1.0
    # closer gallery points rank first for the end point of a line
    assert (np.diff(out[0]) >= 0).all()


def _case(seed=3, n=60, nq=12, D=4):
    return int_sqdist(clustered_int_features(n, D, 5, seed)), nq


def test_lambda_one_returns_the_scaled_distance():
    d, nq = _case()
    out, _, _ = rerank_reference(d, nq, 6, 3, 1.0)
    od = d / d.max(axis=1, keepdims=True)
    assert np.array_equal(out, od[:nq, nq:])


def test_k2_one_leaves_the_weight_rows():
    d, nq = _case()
    _, sets, Vq = rerank_reference(d, nq, 6, 1, 0.3)
    od = d / d.max(axis=1, keepdims=True)
    for i, cols in enumerate(sets):
        assert np.nonzero(Vq[i])[0].tolist() == cols.tolist()
        w = np.exp(-od[i, cols])
        assert np.array_equal(Vq[i, cols], w / w.sum())


def test_duplicate_block_gives_an_empty_row_and_no_nan():
    """k1 + 2 identical rows: each lists the k1 + 1 lowest-indexed copies, so the last copy is in nobody's list (not even its
    own) and R* of it is empty -- a zero row of V, J = 1 against everything, nothing divided by zero."""
    k1 = 3
    X = clustered_int_features(30, 4, 3, 1)
    X[10:10 + k1 + 2] = X[10]
    d = int_sqdist(X)
    out, sets, Vq = rerank_reference(d, 15, k1, 1, 0.3)            # the block lies inside the queries
    last = 10 + k1 + 1
    assert last not in np.argsort(d[last], kind="stable")[:k1 + 1]
    assert sets[last].tolist() == [] and not Vq[last].any()
    assert all(sets[i].tolist() == [10, 11, 12, 13] for i in range(10, last))
    assert np.isfinite(out).all() and np.isfinite(Vq).all()
    od = d / d.max(axis=1, keepdims=True)
    assert np.array_equal(out[last], (1 - 0.3) + 0.3 * od[last, 15:])
    out2, _, Vq2 = rerank_reference(d, 15, k1, 2, 0.3)
    assert np.isfinite(out2).all() and np.isfinite(Vq2).all()


def test_all_rows_equal_has_zero_maxima_and_no_nan():
    out, sets, _ = rerank_reference(np.zeros((6, 6)), 2, 2, 2, 0.3)
    assert np.isfinite(out).all()
    assert [s.tolist() for s in sets[:3]] == [[0, 1, 2]] * 3 and sets[5].tolist() == []


def test_api_refuses_cpu_tensors_and_bad_options():
    from centroids_reid_amd import _lib as L
    from centroids_reid_amd import reid_metric as rm
    with pytest.raises(L.CreidError):
        rm.re_ranking(torch.zeros(4, 8), torch.zeros(30, 8))
    with pytest.raises(L.CreidError):
        rm.re_ranking(np.zeros((4, 8), np.float32), np.zeros((30, 8), np.float32))
    with pytest.raises(L.CreidError):
        rm.R1_mAP(num_query=1, reranking=True).compute(torch.zeros(4, 8), [0, 0, 1, 1], [0, 1, 0, 1])
    for kw in (dict(streamed=True), dict(compute_dtype=torch.bfloat16), dict(compute_dtype=torch.float16),
               dict(dist_func="cosine")):
        with pytest.raises(L.CreidError):
            rm.R1_mAP(num_query=1, reranking=True, **kw)
    with pytest.raises(L.CreidError):
        rm.R1_mAP(num_query=1, reranking={"k": 3})
    with pytest.raises(L.CreidError):
        rm.R1_mAP(num_query=1, reranking=True).compute_chunked(torch.zeros(4, 8), [0, 0, 1, 1], [0, 1, 0, 1])
    assert rm.rerank_options(False) is None and rm.rerank_options(None) is None
    assert rm.rerank_options(True) == dict(k1=20, k2=6, lambda_value=0.3)
    assert rm.rerank_options({"k2": 3}) == dict(k1=20, k2=3, lambda_value=0.3)
    assert rm.R1_mAP(num_query=1).reranking is None
