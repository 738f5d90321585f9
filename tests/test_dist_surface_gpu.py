"""The general-distance loss surface of csrc/heads.hip over the C ABI -- creid_rownorm_fwd / _bwd, creid_triplet_cosine_fwd / _bwd,
creid_hard_mine_from_dist, creid_clamp_sqrt_inplace, creid_gather_mean_rows -- against tests/opt_ref.py (float64 references, derived
bounds, bit-exact expectations) at the shapes no recording covers: D off the 256-thread stride and the float4 width, N off the
64-lane stride, ties everywhere, zero rows, rows under eps, rows whose squares underflow, duplicate and antipodal unit rows, unit
rows whose dot product is exactly 1 (the clamp is active, no gradient) or rounds to either side of it.

Mined indices are judged inside the decision windows of tests/heads_audit.py (mine64, here with the cosine distance and its
bound): equal to the float64 first index where the window decides, inside it otherwise; the loss, coef and dx take the kernel's
own mined operands.  Worst error / bound per family: profiles/opt_edges.md."""
import numpy as np
import pytest
import torch

import opt_ref as orf

pytestmark = pytest.mark.gpu

f32 = np.float32
E_SHAPE = -4
RATIOS = orf.Ratios()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in sorted(RATIOS.worst):
        print(f"\ndist_surface| {fam}: worst error / bound {RATIOS.worst[fam]:.4g}", end="")
    print("\ndist_surface| cases: " + ", ".join(f"{k} {v}" for k, v in sorted(RATIOS.cases.items())))


def L():
    from centroids_reid_amd import _lib
    _lib.lib()
    return _lib


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def empty(*shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device="cuda")


# ------------------------------------------------------------------------------------------------ row normalisation
def rownorm_fwd(xd, mode, eps):
    l = L()
    N, D = xd.shape
    y, norm = torch.full((N, D), 9.0, device="cuda"), torch.full((N,), 9.0, device="cuda")
    assert l.lib().creid_rownorm_fwd(l.ptr(xd), N, D, mode, eps, l.ptr(y), l.ptr(norm), l.stream()) == 0
    return y, norm


@pytest.mark.parametrize("D", [1, 3, 63, 64, 255, 256, 257, 1000, 2048])
@pytest.mark.parametrize("N", [1, 5])
def test_rownorm_forward_and_backward(N, D):
    l = L()
    for mode in (0, 1):
        for eps in (1e-12, 1e-3):
            x, dy = orf.rownorm_inputs(N, D, 10 * D + mode)
            xd, dyd = cu(x), cu(dy)
            y, norm = rownorm_fwd(xd, mode, eps)
            dx = torch.full((N, D), 9.0, device="cuda")
            assert l.lib().creid_rownorm_bwd(l.ptr(xd), l.ptr(norm), l.ptr(dyd), N, D, mode, eps, l.ptr(dx), l.stream()) == 0
            orf.check_rownorm(RATIOS, "rownorm", x, dy, mode, eps, dict(y=host(y), norm=host(norm), dx=host(dx)))
            if N == 5:
                assert float(norm[3]) == 0.0 and not host(y)[3].any(), "the zero row"


# ------------------------------------------------------------------------------------------------ mining on a given matrix
@pytest.mark.parametrize("N", [2, 3, 63, 64, 65, 130])
def test_hard_mine_from_dist_returns_first_indices_and_matrix_entries(N):
    l = L()
    for levels in (4, 2, 1):                                    # (1: every distance equal -- the first positive, the first negative)
        dist, labels = orf.mine_inputs(N, N + levels, levels)
        dd, ld = cu(dist), cu(labels)
        ap, an = empty(N), empty(N)
        pi, ni = empty(N, dtype=torch.int32), empty(N, dtype=torch.int32)
        assert l.lib().creid_hard_mine_from_dist(l.ptr(dd), l.ptr(ld), N, l.ptr(ap), l.ptr(an), l.ptr(pi), l.ptr(ni), l.stream()) == 0
        wap, wan, wpi, wni = orf.mine_expect(dist, labels)
        assert np.array_equal(host(pi), wpi) and np.array_equal(host(ni), wni), "not the first index of the extremum"
        assert orf.same_bits(host(ap), wap) and orf.same_bits(host(an), wan), "not a copy of the matrix entry"
    # continuous values with the signs of zero and a subnormal among them: still bit-copies
    dist = np.random.default_rng(N).standard_normal((N, N)).astype(f32)
    dist[0, :2] = (-0.0, 1e-40)
    dd = cu(dist)
    assert l.lib().creid_hard_mine_from_dist(l.ptr(dd), l.ptr(ld), N, l.ptr(ap), l.ptr(an), l.ptr(pi), l.ptr(ni), l.stream()) == 0
    wap, wan, wpi, wni = orf.mine_expect(dist, labels)
    assert np.array_equal(host(pi), wpi) and np.array_equal(host(ni), wni)
    assert orf.same_bits(host(ap), wap) and orf.same_bits(host(an), wan)
    RATIOS.count("mine_from_dist")


# ------------------------------------------------------------------------------------------------ the cosine triplet
def cosine_fwd(xu, labels, mask, margin):
    l = L()
    N, D = xu.shape
    o = dict(dist_ap=empty(N), dist_an=empty(N), p_idx=empty(N, dtype=torch.int32), n_idx=empty(N, dtype=torch.int32),
             coef=torch.full((N,), 9.0, device="cuda"), out4=empty(4), dist_mat=empty(N, N))
    rc = l.lib().creid_triplet_cosine_fwd(l.ptr(xu), l.ptr(labels), l.ptr(mask), N, D, margin, l.ptr(o["dist_ap"]), l.ptr(o["dist_an"]),
                                          l.ptr(o["p_idx"]), l.ptr(o["n_idx"]), l.ptr(o["coef"]), l.ptr(o["out4"]), l.ptr(o["dist_mat"]),
                                          l.stream())
    return rc, o


@pytest.mark.parametrize("D", [4, 36, 260, 2048])
@pytest.mark.parametrize("N", [4, 6, 17, 33])
def test_cosine_triplet_forward_and_backward(N, D):
    l = L()
    x, labels = orf.unit_inputs(N, D, 100 * N + D)
    xu, _ = rownorm_fwd(cu(x), 0, 1e-12)                         # the unit rows are the device's own
    xu_h = host(xu)
    assert orf.same_bits(xu_h[1], xu_h[0]) and orf.same_bits(xu_h[2], -xu_h[0]) and xu_h[3, 0] == 1.0 and not xu_h[3, 1:].any()
    ld = cu(labels)
    mask = np.ones(N, np.uint8)
    mask[[1, N - 1]] = 0
    gdev = cu(np.array([0.625], f32))
    for margin, m, g, gptr in ((0.3, None, 1.0, None), (0.3, mask, 0.5, gdev), (-1.0, None, 1.0, gdev), (-1.0, mask, 2.0, None), (0.0, None, 1.0, None)):
        rc, o = cosine_fwd(xu, ld, None if m is None else cu(m), margin)
        assert rc == 0
        dev = {k: host(v) for k, v in o.items()}
        fam = "cos_hinge" if margin >= 0 else "cos_soft"
        orf.cos_forward_check(RATIOS, fam, xu_h, labels, m, margin, dev)
        assert dev["dist_mat"][3, 3] == f32(1e-12), "u.u == 1 exactly: the clamp value"
        dx0 = np.random.default_rng(N + D).standard_normal((N, D)).astype(f32)
        dxd = cu(dx0)
        assert l.lib().creid_triplet_cosine_bwd(l.ptr(xu), N, D, l.ptr(o["dist_ap"]), l.ptr(o["dist_an"]), l.ptr(o["p_idx"]),
                                                l.ptr(o["n_idx"]), l.ptr(o["coef"]), l.ptr(gptr), g, l.ptr(dxd), l.stream()) == 0
        orf.cos_backward_check(RATIOS, fam, xu_h, dev, g * (0.625 if gptr is not None else 1.0), dx0, host(dxd))


def test_cosine_triplet_refuses_what_it_cannot_hold():
    for N, D in ((4, 6), (4, 16384), (5, 16380)):                # D % 4 != 0; (D + N) * 4 bytes of LDS over 64 KiB, by 16 and by 4 bytes
        xu = torch.zeros(N, D, device="cuda")
        rc, o = cosine_fwd(xu, cu(np.arange(N, dtype=np.int64) % 2), None, 0.3)
        assert rc == E_SHAPE, (N, D, rc)
        assert float(o["coef"][0]) == 9.0, "a refused call wrote its outputs"


def test_unit_rows_land_above_below_and_on_one_and_the_diagonal_is_the_kernels_own_sum():
    """u.u of an fp32 unit row rounds to 1, above it or below it, and every anchor is its own positive candidate (row 0 has a
    bit-copy besides).  Over the 16 shapes of the sweep each of the three happens many times: counted here with the kernel's dot
    product re-formed in its own order (opt_ref.wave_dot32), which the device's dist_mat entries -- the diagonal, the duplicate
    pair, the antipodal pair -- must equal bit for bit."""
    tally = dict(above=0, below=0, on=0)
    for N in (4, 6, 17, 33):
        for D in (4, 36, 260, 2048):
            x, labels = orf.unit_inputs(N, D, 100 * N + D)
            xu, _ = rownorm_fwd(cu(x), 0, 1e-12)
            rc, o = cosine_fwd(xu, cu(labels), None, 0.3)
            assert rc == 0
            xu_h, dm = host(xu), host(o["dist_mat"])
            for a, j in [(j, j) for j in range(N)] + [(0, 1), (1, 0), (0, 2), (2, 1)]:
                dot, d = orf.cos_dist32(xu_h[a], xu_h[j])
                assert orf.same_bits(dm[a, j], d), f"N {N} D {D}: dist_mat[{a}, {j}] = {dm[a, j]!r}, the kernel's sum re-formed gives {d!r}"
                if a == j:
                    tally["above" if dot > 1 else "below" if dot < 1 else "on"] += 1
                elif (a, j) == (0, 1):
                    assert orf.same_bits(dm[0, 1], dm[0, 0])      # the duplicate: the very sum of the diagonal entry
    print(f"\ndist_surface| u.u over the sweep: {tally}", end="")
    assert min(tally.values()) >= 5, tally                       # (the fp32 model of the rows gives 30 / 56 / 154)


# ------------------------------------------------------------------------------------------------ clamp + sqrt
@pytest.mark.parametrize("n", orf.EW_SIZES + [orf.EW_TRIP + 1])
def test_clamp_sqrt_is_the_rounded_root_of_the_clamped_value(n):
    l = L()
    for lo in (1e-12, 0.25):
        lo = float(f32(lo))
        d = orf.wild(n, n + 3)
        edge = np.array([-1.0, -0.0, 0.0, lo / 2, lo, np.nextafter(f32(lo), f32(1)), 4.0, 1e30, 3e38, 1e-40, -1e-30], f32)
        k = min(n, edge.size)
        d[n - k:] = edge[:k][::-1]                              # (the edge values end the buffer: the last one is past the cap)
        dd = cu(d)
        assert l.lib().creid_clamp_sqrt_inplace(l.ptr(dd), n, lo, l.stream()) == 0
        want = orf.clamp_sqrt_expect(d, lo)
        assert d[-1] == -1.0 and want[-1] != d[-1]              # a kernel that never reached the last element could not leave it right
        orf.exact_bits(RATIOS, "clamp_sqrt", f"n {n} lo {lo}", host(dd), want)
    RATIOS.count("clamp_sqrt")
    assert l.lib().creid_clamp_sqrt_inplace(l.ptr(dd), 0, lo, l.stream()) == 0


# ------------------------------------------------------------------------------------------------ per-segment row means
@pytest.mark.parametrize("D", [1, 255, 256, 257, 2048])
def test_gather_mean_rows_sums_in_list_order(D):
    """Segments of 1, 2, 7 and 300 rows over a non-monotone order with one row in two segments: a sequential fp32 sum in list
    order and one division, bit for bit.  An EMPTY segment would be 0 / 0; no caller can pass one -- bases.py builds its groups
    from np.unique / non-empty selections (an empty camera selection is skipped, on the host and in the device index alike),
    inference.create_pid_path_index only ever appends to a list it has just created, and the reference's own loop raises on an
    empty index list -- so the kernel keeps its contract of non-empty segments and none is run here."""
    l = L()
    emb, order, off = orf.gather_inputs(D, D)
    out = torch.full((len(off) - 1, D), 9.0, device="cuda")
    ed, od, fd = cu(emb), cu(order), cu(off)
    assert l.lib().creid_gather_mean_rows(l.ptr(ed), l.ptr(od), l.ptr(fd), len(off) - 1, D, l.ptr(out), l.stream()) == 0
    orf.exact_bits(RATIOS, "gather_mean", f"D {D}", host(out), orf.gather_mean_expect(emb, order, off))
    RATIOS.count("gather_mean")
    assert np.array_equal(host(ed), emb)
