"""The conditions under which tests/test_eval_exact_gpu.py may demand EQUALITY, checked on the reference alone (no GPU, no
project kernel): every case of the GPU tables stays below the exactness margin, its values are representable in its dtype, the
int64 reference is the fp64 distance, the lists the fast paths keep are far from their capacities, every labelled case has a
positive-negative tie and a zero distance -- and the inputs are SENSITIVE: the kernel mistakes the tables are built for each
change nearly every distance (or the ranking) of every case, so none of them can pass the GPU file.  The shape tables are
pinned too: trimming one fails here."""
import numpy as np
import pytest
import torch

import eval_exact as ee

TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CASE_DT = [(c.name, dt) for c in ee.ALL for dt in ee.DTYPES]


@pytest.fixture(params=CASE_DT, ids=[f"{n}-{d}" for n, d in CASE_DT])
def ref(request):
    return ee.reference(*request.param)


def test_margin_dtype_round_trip_and_fp64_distance(ref):
    assert ref.margin < 1.0
    assert ref.big > 3 and max(np.abs(ref.q).max(), np.abs(ref.g).max()) == ref.big     # the large magnitudes are there
    assert not (ref.q == 0).any() and not (ref.g == 0).any()
    f = torch.from_numpy(ref.feats)
    back = f.to(TORCH_DT[ref.dt]).double()
    assert torch.equal(back, f)                                           # the cast the GPU tests make changes no value
    m = ref.case.m
    d64 = torch.cdist(f[:m], f[m:], compute_mode="donot_use_mm_for_euclid_dist") ** 2
    exp = torch.from_numpy(ref.fdist)
    assert float((d64 - exp).abs().max()) <= 1e-9 * max(1.0, float(exp.max()))       # sqrt then square: a few fp64 ulps
    assert torch.equal(exp.float().double(), exp)                         # every reference distance is an fp32 number
    assert int(ref.dist.max()) < ee.LIMIT and int(ref.qq.max()) < ee.LIMIT and int(ref.gg.max()) < ee.LIMIT


def test_lists_stay_inside_their_capacities(ref):
    c = ref.case
    cand = ee.candidate_counts(ref)
    assert c.k <= cand.min() and cand.max() <= ee.STREAM_CAPACITY // 2
    if c is ee.FALLBACK:
        assert cand.min() > ee.FALLBACK_CAPACITY                          # every row overflows capacity = 64
    pos = ee.positive_counts(ref)
    if c.overflow:
        over = np.nonzero(pos > ee.PL_MAX)[0]
        assert over.tolist() == [4, 5, 6, 7] and np.delete(pos, over).max() <= ee.PL_MAX
    else:
        assert pos.max() <= ee.PL_MAX


def test_ties_zero_distance_and_invalid_queries(ref):
    c = ref.case
    if not c.labelled:
        assert c.m < 4 or c.n < 16                                        # too small to hold them: only the 1 x 1 cases
        assert ref.valid[0]
        return
    assert ee.pos_neg_ties(ref) >= 1 and ee.zero_distances(ref) >= 1
    assert ref.dist[3, 7] == 0 and ref.dist[2, 5] == ref.dist[2, 11]
    assert ee.tied_columns(ref).min() >= 2
    assert not ref.valid[0] and not ref.valid[1] and ref.valid[2] and ref.valid[3]
    assert ref.dist[3].min() == 0                                         # nothing is nearer than the zero distance


def test_kernel_mistakes_change_the_distances(ref):
    """Each mistake must move >= 95 % of the distances it touches, so a kernel that makes it cannot pass by luck."""
    D = ref.q.shape[1]
    changed = lambda d: float((d != ref.dist).mean())
    for k0 in (0, D // 2, D - 1):
        assert changed(ee.mut_drop_k(ref, k0)) == 1.0                     # no zero element: every distance moves
    assert changed(ee.mut_drop_last_step(ref)) >= 0.95
    assert changed(ee.mut_repeat_step(ref)) >= 0.95
    tail, touched = ee.mut_tail_reads_last(ref)
    assert np.array_equal(tail[:, ~touched], ref.dist[:, ~touched])
    if touched.any():
        assert float((tail[:, touched] != ref.dist[:, touched]).mean()) >= 0.95


def test_tail_mistake_is_exercised():
    """the column-tail mutation is vacuous where the last unit holds one column (257, 513, 4097): enough cases have a real tail"""
    n_real = sum(1 for c in ee.ALL if (c.n - 1) % 64 >= 1)
    assert n_real >= 8


def test_wrong_tie_rule_changes_rank_or_ap(ref):
    from oracle import reid_oracle as ro
    c = ref.case
    if not c.labelled:
        return
    wrong = ee.rank_last_index_first(ref.dist)
    assert (wrong[:, :c.k] != ref.order[:, :c.k]).any()                   # the top-k prefix moves
    m = c.m
    _, _, _, ex = ro.eval_market(wrong, ref.pids[:m], ref.pids[m:], ref.cams[:m], ref.cams[m:])
    assert np.array_equal(ex["valid"], ref.valid)
    assert ((ex["first"] != ref.first) | (ex["ap"] != ref.ap)).sum() >= 1
    assert ex["ap"][2] != ref.ap[2]                                       # query 2: the forced positive-negative tie


def test_shape_tables_contain_the_edges():
    mat, st = ee.MATRIX, ee.STREAM
    for v in (1, 127, 128, 129):                                          # around the 128-wide materialised tile
        assert any(c.m == v for c in mat) and any(c.n == v for c in mat)
    assert any((-(-c.m // 128)) * (-(-c.n // 128)) % 8 not in (0, 1) and c.m > 256 and c.n > 512 for c in mat)   # XCD remap
    assert any(c.m == 65 for c in st) and {257, 513, 4097} <= {c.n for c in st}       # around the 64 x 256 streamed tile
    assert any(c.m == 1 and c.n == 1 for c in st) and any(c.k == c.n for c in st)
    for tab in (mat, st):
        assert {c.D32 for c in tab} >= {4, 12, 16, 20, 36, 100, 2048}
        assert {c.D16 for c in tab} >= {8, 56, 64, 72, 104, 2032, 2048}
        assert any(c.scale_exp == -6 for c in tab) and any(c.scale_exp == 0 for c in tab)
    assert any(c.D32 % 16 == 0 for c in st) and any(c.D32 % 16 for c in st)           # both fp32 streamed instantiations
    assert all(c.D16 % 8 == 0 and c.D32 % 4 == 0 for c in ee.ALL)
    assert ee.OVERFLOW.overflow and ee.FALLBACK_CAPACITY == 64
    assert len({c.name for c in ee.ALL}) == len(ee.ALL)


def test_audit_bounds_are_first_order_sums():
    """the bound helpers on a case small enough to check by hand: D = 8, one row each"""
    q = torch.tensor([[1.0, -2, 3, 0.5, 0, 0, 0, 0]]); g = torch.tensor([[2.0, 1, -1, 4, 0, 0, 0, 0]])
    qq, gg = (q ** 2).sum(1), (g ** 2).sum(1)
    d, b = ee.dist_ref_bound(q, g, qq, gg)
    assert float(d) == 14.25 + 22 - 2 * (2 - 2 - 3 + 2)
    assert float(b) == pytest.approx(ee.U * (2 * 8 * 9.0 + 36.25 + 38.25))
    assert ee.sqnorm_chain(2048, 1) == 38 and ee.sqnorm_chain(2048, 4) == 38 and ee.sqnorm_chain(104, 4) == 10
    s, sb = ee.sqnorm_ref_bound(q, 1)
    assert float(s) == 14.25 and float(sb) == pytest.approx(7 * ee.U * 14.25)
    x = ee.audit_features("clustered", 20, 16, 1)
    y, yb = ee.normalize_ref_bound(x)
    assert torch.equal(y[7], torch.zeros(16, dtype=torch.float64)) and float(yb[7].max()) == 0.0
    assert float(((y ** 2).sum(1) - 1).abs()[:7].max()) < 1e-14
