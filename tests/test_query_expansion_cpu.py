"""CPU: the float64 reference of query expansion (tests/qe_ref.py) against its own definition, the option parsing and every
refusal that happens before device work, and the quality recipe on the reference."""
import numpy as np
import pytest
import torch

import qe_ref as R


def _rows(seed, nq=12, ng=40, D=16):
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((6, D))
    q = C[rng.integers(0, 6, nq)] + 0.3 * rng.standard_normal((nq, D))
    g = C[rng.integers(0, 6, ng)] + 0.3 * rng.standard_normal((ng, D))
    return q, g


# ------------------------------------------------------------------------------------------ the reference itself
def test_reference_alpha0_is_the_plain_neighbour_mean():
    q, g = _rows(0)
    U = R.unit(np.concatenate([q, g]))
    idx, _ = R.neighbours(U, U, 5)
    assert np.array_equal(idx[:, 0], np.arange(len(U)))                      # a row is its own nearest neighbour
    mean = R.unit(U[idx].mean(axis=1))
    q2, g2 = R.query_expansion_ref(q, g, k=5, alpha=0, scope="all")
    np.testing.assert_allclose(np.concatenate([q2, g2]), mean, rtol=0, atol=1e-15)
    # classic AQE: the query and its k - 1 nearest gallery rows, gallery untouched
    idx, _ = R.neighbours(U[:len(q)], U[len(q):], 4)
    mean_q = R.unit(U[:len(q)] + U[len(q):][idx].sum(axis=1))
    q3, g3 = R.query_expansion_ref(q, g, k=5, alpha=0, scope="query")
    np.testing.assert_allclose(q3, mean_q, rtol=0, atol=1e-15)
    assert np.array_equal(g3, U[len(q):])


def test_reference_weights():
    d = np.array([-0.5, 0, 0.5, 1, 1.5, 2, 2.5, np.nan], np.float32)
    assert np.array_equal(R.sim_f32(d), np.array([1, 1, .75, .5, .25, 0, 0, 0], np.float32))
    assert np.array_equal(R.weights(d, 0), np.ones(8))                       # exactly 1, also where sim == 0 or d is NaN
    assert np.array_equal(R.weights(d, 1), R.sim_f32(d).astype(np.float64))
    np.testing.assert_allclose(R.weights(d, 3), R.sim_f32(d).astype(np.float64) ** 3, rtol=1e-15)


@pytest.mark.parametrize("scope", ["all", "query"])
def test_reference_two_rounds_are_two_single_rounds(scope):
    q, g = _rows(1)
    a = R.query_expansion_ref(q, g, k=4, alpha=2.0, rounds=2, scope=scope)
    b = R.query_expansion_ref(*R.query_expansion_ref(q, g, k=4, alpha=2.0, scope=scope), k=4, alpha=2.0, scope=scope)
    for x, y in zip(a, b):
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-15)


def test_reference_query_scope_k1_is_the_identity():
    q, g = _rows(2)
    q2, g2 = R.query_expansion_ref(q, g, k=1, alpha=3.0, scope="query")
    np.testing.assert_allclose(q2, R.unit(q), rtol=0, atol=1e-15)
    assert np.array_equal(g2, R.unit(g))


def test_exact_model_refuses_inexact_sums():
    x = np.array([[1.0, 3.0]])
    idx = np.zeros((1, 2), np.int64)
    assert np.array_equal(R.exact_sums(x, idx, np.array([[0.5, 0.25]])), np.array([[0.75, 2.25]], np.float32))
    with pytest.raises(AssertionError):
        R.exact_sums(x, idx, np.array([[1.0, 2.0 ** -30]]))


# ------------------------------------------------------------------------------------------ options and refusals
def test_expansion_options():
    from centroids_reid_amd import _lib as L, reid_metric as rm
    assert rm.QE_DEFAULTS == dict(k=10, alpha=3.0, rounds=1, scope="all")
    assert rm.expansion_options(False) is None and rm.expansion_options(None) is None
    assert rm.expansion_options(True) == rm.QE_DEFAULTS and rm.expansion_options(True) is not rm.QE_DEFAULTS
    assert rm.expansion_options({}) == rm.QE_DEFAULTS
    assert rm.expansion_options(dict(k=5, scope="query")) == dict(k=5, alpha=3.0, rounds=1, scope="query")
    assert rm.expansion_options(dict(alpha=0, rounds=3)) == dict(k=10, alpha=0, rounds=3, scope="all")
    for bad in ("all", 3, [("k", 3)], dict(k1=3), dict(k=3, lambda_value=0.3)):
        with pytest.raises(L.CreidError):
            rm.expansion_options(bad)


BAD_OPTIONS = [dict(k=0), dict(k=-1), dict(k=2.5), dict(k=1025), dict(k=1026, scope="query"), dict(alpha=-0.5),
               dict(alpha=float("inf")), dict(alpha=float("nan")), dict(alpha="3"), dict(rounds=0), dict(rounds=1.5),
               dict(scope="gallery"), dict(scope=None)]


@pytest.mark.parametrize("bad", BAD_OPTIONS, ids=[str(b) for b in BAD_OPTIONS])
def test_bad_options_are_refused_before_device_work(bad):
    """No GPU here: a refusal that came after any device work could not raise CreidError for the options."""
    from centroids_reid_amd import _lib as L, inference, reid_metric as rm
    with pytest.raises(L.CreidError, match="query_expansion"):
        rm.R1_mAP(num_query=2, query_expansion=bad)
    q, g = torch.zeros(2, 8), torch.zeros(6, 8)
    with pytest.raises(L.CreidError, match="query_expansion"):
        rm.query_expansion(q, g, **bad)
    with pytest.raises(L.CreidError, match="query_expansion"):
        inference.get_similar(q.numpy(), ["a", "b"], g.numpy(), list("cdefgh"), topk=2, query_expansion=bad)


def test_expansion_needs_unit_rows_and_device_tensors():
    from centroids_reid_amd import _lib as L, inference, reid_metric as rm
    with pytest.raises(L.CreidError, match="feat_norm"):
        rm.R1_mAP(num_query=2, feat_norm=False, query_expansion=True)
    with pytest.raises(L.CreidError, match="feat_norm"):
        rm.R1_mAP(num_query=2, feat_norm=False, query_expansion=dict(k=3))
    rm.R1_mAP(num_query=2, feat_norm=False, query_expansion=False)           # nothing changes without the keyword
    assert rm.R1_mAP(num_query=2, query_expansion=dict(k=3)).query_expansion == dict(k=3, alpha=3.0, rounds=1, scope="all")
    q, g = np.zeros((2, 8), np.float32), np.zeros((6, 8), np.float32)
    with pytest.raises(L.CreidError, match="normalize_features"):
        inference.get_similar(q, ["a", "b"], g, list("cdefgh"), topk=2, normalize_features=False, query_expansion=True)
    with pytest.raises(L.CreidError):                                          # no CPU fallback
        rm.query_expansion(torch.zeros(2, 8), torch.zeros(6, 8), k=3)
    with pytest.raises(L.CreidError):
        rm.neighbour_expand(torch.zeros(6, 8), torch.zeros((2, 3), dtype=torch.int64), torch.zeros(2, 3), 3.0)
    with pytest.raises(L.CreidError):
        rm.query_expansion(q, g, k=3)                                          # arrays are not device tensors


def test_model_base_takes_the_keyword():
    import inspect
    from centroids_reid_amd.bases import ModelBase
    assert inspect.signature(ModelBase.__init__).parameters["eval_query_expansion"].default is None


# ------------------------------------------------------------------------------------------ quality
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_expansion_improves_map_on_the_reference(seed):
    q, g, qp, gp, qc, gc = R.quality_set(seed)
    base = R.mean_ap(R.unit(q), R.unit(g), qp, gp, qc, gc)
    both = R.mean_ap(*R.query_expansion_ref(q, g, k=5, alpha=3, scope="all"), qp, gp, qc, gc)
    aqe = R.mean_ap(*R.query_expansion_ref(q, g, k=5, alpha=3, scope="query"), qp, gp, qc, gc)
    print(f"seed {seed}: mAP none {base:.4f}  all {both:.4f} ({both - base:+.4f})  query {aqe:.4f} ({aqe - base:+.4f})")
    assert both >= base + 0.05
    assert aqe >= base + 0.02
