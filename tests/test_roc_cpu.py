"""CPU: the open-set operating points without a GPU -- the numpy reference against itself (the three-pass radix model of
tests/roc_ref.py equals its sort-based form, and the wrong readings of the definition are told apart), and the argument
refusals of the four entry points through the built library (every refusal comes before any launch, so none needs a device)."""
import ctypes

import numpy as np
import pytest

import roc_ref as R

E_ARG, E_DTYPE, E_SHAPE = -1, -2, -4


# --------------------------------------------------------------------------- the reference against itself
def _tied_keys(rng, n, distinct, both_sides=True):
    """n uint32 keys drawn from `distinct` values: long runs of equal keys, on both sides of 0x80000000 (the keys of negative
    and of positive distances) unless told otherwise."""
    lo, hi = (0x7f000000, 0x81000000) if both_sides else (0x80000000, 0xc0000000)
    pool = rng.integers(lo, hi, distinct, dtype=np.uint64).astype(np.uint32)
    return pool[rng.integers(0, distinct, n)]


KEY_CASES = {
    "heavy_ties": lambda rng: (_tied_keys(rng, 500, 7), _tied_keys(rng, 5000, 9)),
    "sign_branch": lambda rng: (_tied_keys(rng, 300, 40), np.concatenate([_tied_keys(rng, 2000, 50),
                                                                           np.asarray([0x7fffffff, 0x80000000, 0x80000001], np.uint32)])),
    "all_equal": lambda rng: (np.full(100, 0x80123456, np.uint32), np.full(1000, 0x80123456, np.uint32)),
    "distinct": lambda rng: (rng.integers(0, 1 << 32, 400, dtype=np.uint64).astype(np.uint32),
                             rng.integers(0, 1 << 32, 3000, dtype=np.uint64).astype(np.uint32)),
    "single_impostor": lambda rng: (_tied_keys(rng, 10, 3), np.asarray([0x80000000], np.uint32)),
    "no_genuine": lambda rng: (np.zeros(0, np.uint32), _tied_keys(rng, 777, 5)),
    "extremes": lambda rng: (np.asarray([0, 0xffffffff], np.uint32), np.asarray([0, 0, 0xffffffff, 0xffffffff, 5], np.uint32)),
}
# k = 0 (tiny rates), k = N - 1 (rate 1.0: the clamp), and ranks inside the runs
KEY_RATES = (1e-9, 1e-4, 1e-3, 1e-2, 0.1, 0.5, 0.9999, 1.0)


@pytest.mark.parametrize("case", sorted(KEY_CASES))
def test_radix_model_equals_sort_reference(case):
    gen, imp = KEY_CASES[case](np.random.default_rng(len(case)))
    ref = R.operating_points(gen, imp, KEY_RATES)
    key, fa, ta, k = R.radix_select(gen, imp, KEY_RATES)
    assert ref["k"][0] == 0 and ref["k"][-1] == len(imp) - 1
    np.testing.assert_array_equal(k, ref["k"])
    np.testing.assert_array_equal(key, ref["key"])
    np.testing.assert_array_equal(fa, ref["false_accepts"])
    np.testing.assert_array_equal(ta, ref["true_accepts"])
    assert (fa <= k).all()
    assert np.isnan(ref["tar"]).all() == (len(gen) == 0)


def test_key_is_monotone_and_invertible():
    d = np.asarray([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, np.inf], np.float32)
    k = R.mono_key(d)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert k[3] == 0x7fffffff and k[4] == 0x80000000
    np.testing.assert_array_equal(R.key_to_float(k).view(np.uint32), d.view(np.uint32))


def _small_case():
    """A 6 x 30 matrix with ties: distances are small integers, every query has junk, genuine and impostor entries."""
    rng = np.random.default_rng(5)
    dist = rng.integers(0, 6, (6, 30)).astype(np.float32)
    q_pids, q_cams = np.arange(6) % 3, np.arange(6) % 2
    g_pids, g_cams = rng.integers(0, 3, 30), rng.integers(0, 2, 30)
    return dist, q_pids, q_cams, g_pids, g_cams


def test_reference_mutants_are_caught():
    """`<=` for `<`, junk counted as genuine, `ceil` for `floor`: each changes a field of at least one case."""
    dist, qp, qc, gp, gc = _small_case()
    rates = (0.07, 0.33, 1.0)
    ref = R.roc_ref(dist, qp, qc, gp, gc, rates)
    assert (ref["false_accepts"] <= ref["k"]).all() and (ref["false_accepts"] < ref["k"]).any()
    differs = lambda other, keys: any(not np.array_equal(ref[k], other[k]) for k in keys)
    le = R.roc_ref(dist, qp, qc, gp, gc, rates, mutant="le")
    assert differs(le, ("false_accepts", "true_accepts")) and (le["false_accepts"] > le["k"]).any()
    junk = R.roc_ref(dist, qp, qc, gp, gc, rates, mutant="junk")
    assert differs(junk, ("n_genuine",)) and differs(junk, ("true_accepts", "hist"))
    # floor and ceil part where rate x N_imp is not an integer: 0.07 x N_imp below
    assert (np.float64(0.07) * ref["n_impostor"][0]) % 1 != 0
    ce = R.roc_ref(dist, qp, qc, gp, gc, rates, mutant="ceil")
    assert differs(ce, ("k",))
    # ... and the next rank is another distance once the distances are distinct (inside a run of ties both ranks agree)
    dist = np.random.default_rng(6).permutation(dist.size).reshape(dist.shape).astype(np.float32)
    ref = R.roc_ref(dist, qp, qc, gp, gc, rates)
    ce = R.roc_ref(dist, qp, qc, gp, gc, rates, mutant="ceil")
    np.testing.assert_array_equal(ref["false_accepts"], ref["k"])
    assert differs(ce, ("threshold",)) and differs(ce, ("false_accepts",))


def test_hist_reference_adds_up():
    dist, qp, qc, gp, gc = _small_case()
    gen, imp = R.class_keys(dist, qp, qc, gp, gc)
    junk = R.junk_matrix(qp, qc, gp, gc, False)
    assert len(gen) + len(imp) + junk.sum() == dist.size
    h0 = R.hist_ref(dist, qp, qc, gp, gc, None, 0, 11)
    assert h0.shape == (1, 2, 2048) and h0[0, 0].sum() == len(gen) and h0[0, 1].sum() == len(imp)
    pre = R.probe_prefixes(imp, 11)
    h1 = R.hist_ref(dist, qp, qc, gp, gc, pre, 11, 11)
    np.testing.assert_array_equal(h1[0], h1[2])                      # the duplicated prefix
    assert h1[3].sum() == 0                                          # the prefix no key has
    assert h1[0, 1].sum() == h0[0, 1, pre[0]] and h1[1, 0].sum() == h0[0, 0, pre[1]]


# --------------------------------------------------------------------------- argument refusals, through the built library
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import centroids_reid_amd._lib as L
    return L.lib()


class _Args:
    """A valid call of each entry point on host memory nobody reads: the refusals come before any launch."""

    def __init__(self):
        self.buf = ctypes.create_string_buffer(4096)
        self.p = ctypes.c_void_p(ctypes.addressof(self.buf))
        self.kw = dict(m=4, n=16, D=16, dtype=1, nsel=1, prefix_bits=0, bits=11, null=())

    def call(self, lib, name, **over):
        a = {**self.kw, **over}
        P = lambda what: None if what in a["null"] else self.p
        labels = (P("q_pids"), P("g_pids"), P("q_cams"), P("g_cams"), 0)
        tail = (P("prefix"), a["nsel"], a["prefix_bits"], a["bits"], P("hist"), None)
        rows = (P("q"), P("g"), P("qq"), P("gg"), a["m"], a["n"], a["D"])
        if name == "creid_stream_dist_hist":
            return lib.creid_stream_dist_hist(*rows, *labels, *tail)
        if name == "creid_stream_dist_hist_h16":
            return lib.creid_stream_dist_hist_h16(*rows, a["dtype"], *labels, *tail)
        assert name == "creid_dist_hist_matrix"
        return lib.creid_dist_hist_matrix(P("dist"), a["m"], a["n"], *labels, *tail)


HIST_ENTRIES = ("creid_stream_dist_hist", "creid_stream_dist_hist_h16", "creid_dist_hist_matrix")


@pytest.mark.parametrize("name", HIST_ENTRIES)
def test_hist_entry_points_refuse_bad_radix_arguments(lib, name):
    A = _Args()
    for bad in (dict(bits=0), dict(bits=12), dict(bits=-1), dict(prefix_bits=22, bits=11), dict(prefix_bits=-1),
                dict(nsel=0, prefix_bits=11), dict(nsel=-3, prefix_bits=11), dict(nsel=5, prefix_bits=11, bits=11),
                dict(nsel=9, prefix_bits=11, bits=10), dict(nsel=2, prefix_bits=0), dict(nsel=4, prefix_bits=0, bits=4)):
        assert A.call(lib, name, **bad) == E_SHAPE, (name, bad)
    # the limits themselves are shapes the entry points take: with m == 0 they return 0 without a launch
    for ok in (dict(bits=1), dict(bits=11), dict(nsel=4, prefix_bits=11, bits=11), dict(nsel=8, prefix_bits=22, bits=10),
               dict(nsel=4096, prefix_bits=31, bits=1)):
        assert A.call(lib, name, m=0, **ok) == 0, (name, ok)


@pytest.mark.parametrize("name", HIST_ENTRIES)
def test_hist_entry_points_refuse_null_pointers_and_sizes(lib, name):
    A = _Args()
    ptrs = ["q_pids", "g_pids", "q_cams", "g_cams", "hist"] + (["dist"] if name.endswith("matrix") else ["q", "g", "qq", "gg"])
    for what in ptrs:
        assert A.call(lib, name, null=(what,)) == E_ARG, (name, what)
    assert A.call(lib, name, null=("prefix",), prefix_bits=11) == E_ARG
    assert A.call(lib, name, m=0, null=tuple(ptrs) + ("prefix",)) == 0           # an empty query set: a no-op
    assert A.call(lib, name, m=-1) == E_ARG and A.call(lib, name, n=0) == E_ARG
    assert A.call(lib, name, m=0x7ffffff1) == E_SHAPE and A.call(lib, name, n=0x7ffffff1) == E_SHAPE
    # a refusal of the radix arguments comes before the empty query set and before the pointers
    assert A.call(lib, name, m=0, bits=12) == E_SHAPE
    assert A.call(lib, name, bits=12, null=("hist",)) == E_SHAPE


def test_streamed_hist_entry_points_keep_their_familys_width_and_dtype_tests(lib):
    A = _Args()
    assert A.call(lib, "creid_stream_dist_hist", D=6) == E_SHAPE                 # fp32: D % 4
    assert A.call(lib, "creid_stream_dist_hist", D=0) == E_ARG
    assert A.call(lib, "creid_stream_dist_hist_h16", D=12) == E_SHAPE            # 16-bit: D % 8
    assert A.call(lib, "creid_stream_dist_hist_h16", D=(1 << 20) + 8) == E_SHAPE
    for dt in (0, 3, 7):
        assert A.call(lib, "creid_stream_dist_hist_h16", dtype=dt) == E_DTYPE
    assert A.call(lib, "creid_stream_dist_hist_h16", dtype=0, D=12) == E_SHAPE   # shape before dtype, as in the family
    assert A.call(lib, "creid_stream_dist_hist_h16", dtype=0, m=0) == E_DTYPE    # ... and both before the empty query set


def test_roc_descend_refuses(lib):
    A = _Args()
    p = A.p
    for nsel, bits, level in ((0, 11, 0), (5, 11, 0), (1, 0, 0), (1, 12, 0), (9, 10, 2), (1, 11, -1), (1, 11, 32)):
        assert lib.creid_roc_descend(p, nsel, bits, level, p, p, p, None) == E_SHAPE, (nsel, bits, level)
    for i in range(4):
        ptrs = [p, p, p, p]
        ptrs[i] = None
        assert lib.creid_roc_descend(ptrs[0], 4, 11, 0, ptrs[1], ptrs[2], ptrs[3], None) == E_ARG


def test_python_surface_refuses_before_any_launch(lib):
    """Rates outside (0, 1], none, more than 16: CreidError from roc_rates, which R1_mAP(roc=...) and ModelBase(eval_roc=...) go
    through at construction; CPU tensors are refused for being on the CPU."""
    import torch
    from centroids_reid_amd import _lib as L, reid_metric as rm
    assert rm.roc_rates(True) == (1e-4, 1e-3, 1e-2) and rm.roc_rates((0.5, 1)) == (0.5, 1.0) and rm.roc_rates(0.25) == (0.25,)
    for bad in ((0.0,), (-0.1,), (1.5,), (float("nan"),), (), tuple([0.1] * 17), ("x",)):
        with pytest.raises(L.CreidError):
            rm.roc_rates(bad)
        with pytest.raises(L.CreidError):
            rm.R1_mAP(num_query=2, roc=bad)
    assert rm.R1_mAP(num_query=2).roc is None and rm.R1_mAP(num_query=2, roc=True).roc == rm.ROC_DEFAULT_FAR
    assert len(rm.R1_mAP(num_query=2, roc=tuple([0.1] * 16)).roc) == 16
    junk = rm.JunkFilter(np.zeros(4), np.zeros(4), np.ones(16), np.zeros(16))
    with pytest.raises(L.CreidError, match="CPU"):
        rm.distance_histogram(torch.zeros(4, 8), torch.zeros(16, 8), junk)
    with pytest.raises(L.CreidError, match="CPU"):
        rm.roc_matrix(torch.zeros(4, 16), junk)
    # the keys' inverse on the host: the reference's
    k = np.asarray([0, 0x7fffffff, 0x80000000, 0x80000001, 0xbf800000, 0xffffffff], np.uint32)
    np.testing.assert_array_equal(rm.key_to_distance(k).view(np.uint32), R.key_to_float(k).view(np.uint32))
