"""The kernels of csrc/elementwise.hip -- BatchNorm statistics / finalize / apply / backward, the one-launch finalize + apply, the
fused stem tail, max-pool, global average pool, NHWC -> NCHW, IBN -- against the float64 reference of tests/ew_ref.py at the
shapes where they can go wrong and that no network of the benchmark produces: one row, ragged rows, channel counts whose
16-byte chunks per row (3, 5, 6, 9, 10, 18) do not divide the 256-thread workgroup, statistics of 194 / 513 / 770 partial rows
(the unrolled finalize loops and the CW = 4 variant), tensors past the grid cap of the grid-stride kernels (a thread makes a
second trip and must still be on its own channels), ties and all-negative windows in the pool, the second image group and the
quarter-lane wrap of the IBN finalize, the channel and row tails of the average pool.

Two layers, as ew_ref.py lays out: statistics-derived quantities against float64 within bounds that follow from the kernels'
summation; element-wise results against the float64 expression evaluated with the DEVICE'S OWN coefficients within the two or
three fp32 roundings of that expression plus half an ulp of storage.  Pool values, tap codes and gradients, the average pool's
backward, the layout transform, mask bits and masked gradients are exact; fused forms are bit-identical to the launches they
replace.  ReLU masks: the inputs keep every pre-activation clear of zero by more than the device may be off, the agreement of
the float64 and the device decision is asserted, never skipped; the backward takes the device forward's mask.

NaN and infinite inputs are out of scope.  Case counts, the largest error-to-bound ratio per family and the file's run time:
profiles/ew_edge_sweep.md."""
import numpy as np
import pytest
import torch

import ew_ref as er

pytestmark = pytest.mark.gpu

f32 = np.float32
MOM, EPS = 0.1, 1e-5                                     # handed to the ABI as fp32 ...
MOM_R, EPS_R = float(f32(MOM)), float(f32(EPS))          # ... which is what the reference evaluates
E_ARG, E_SHAPE = -1, -4
RATIOS = er.Ratios()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in sorted(RATIOS.worst):
        print(f"\new_edges| {fam}: worst error / bound {RATIOS.worst[fam]:.4g}", end="")
    print("\new_edges| cases: " + ", ".join(f"{k} {v}" for k, v in sorted(RATIOS.cases.items())))


def L():
    from centroids_reid_amd import _lib
    _lib.lib()
    return _lib


def dev(t, kind):
    return er.to_storage(t, kind).contiguous().cuda()


def d32(t):
    return er.t64(t).float().contiguous().cuda()


def empty32(*shape):
    return torch.empty(shape, dtype=torch.float32, device="cuda")


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def code(kind):
    return L()._DT[er.TORCH_DT[kind]]


# ------------------------------------------------------------------------------------------------ BatchNorm, device side
def col_finalize(x, M, C, kind, gamma, beta, rm, rv):
    """creid_col_stats -> creid_bn2d_finalize (training): (partial, mean, invstd, ss); rm / rv updated in place."""
    l = L()
    lib, st = l.lib(), l.stream()
    rows = lib.creid_col_stats_rows(M)
    partial = empty32(rows, 2, C)
    l.check(lib.creid_col_stats(l.ptr(x), M, C, code(kind), l.ptr(partial), st), "col_stats")
    mean, invstd, ss = empty32(C), empty32(C), empty32(2, C)
    l.check(lib.creid_bn2d_finalize(l.ptr(partial), rows, C, M, l.ptr(rm), l.ptr(rv), 1, MOM, EPS, l.ptr(gamma), l.ptr(beta), l.ptr(mean),
                                    l.ptr(invstd), l.ptr(ss), st), "bn2d_finalize")
    return partial, mean, invstd, ss


def bn_forward(d):
    """The training forward of the three launches; returns the device tensors (t) and their CPU copies for the checks (dev)."""
    l = L()
    lib, st = l.lib(), l.stream()
    kind, M, C = d["kind"], d["M"], d["C"]
    t = dict(x=dev(d["x"], kind), gamma=d32(d["gamma"]), beta=d32(d["beta"]), rm=d32(d["rmean"]), rv=d32(d["rvar"]))
    t["partial"], t["mean"], t["invstd"], t["ss"] = col_finalize(t["x"], M, C, kind, t["gamma"], t["beta"], t["rm"], t["rv"])
    t["y"] = torch.empty_like(t["x"])
    t["bits"] = torch.empty(M * C // 8, dtype=torch.uint8, device="cuda") if kind != "fp32" else None
    relu = 1 if d["relu"] else 0
    if d["res_mode"] == "dual":
        t["res"], t["gamma2"], t["beta2"] = dev(d["res"], kind), d32(d["gamma2"]), d32(d["beta2"])
        rm2, rv2 = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        _, t["mean2"], t["invstd2"], t["ss2"] = col_finalize(t["res"], M, C, kind, t["gamma2"], t["beta2"], rm2, rv2)
        l.check(lib.creid_bn2d_apply_dual_mask(l.ptr(t["x"]), l.ptr(t["ss"]), l.ptr(t["res"]), l.ptr(t["ss2"]), relu, M, C, code(kind),
                                               l.ptr(t["y"]), l.ptr(t["bits"]), st), "bn2d_apply_dual_mask")
    else:
        t["res"] = dev(d["res"], kind) if d["res"] is not None else None
        l.check(lib.creid_bn2d_apply_mask(l.ptr(t["x"]), l.ptr(t["ss"]), l.ptr(t["res"]), relu, M, C, code(kind), l.ptr(t["y"]),
                                          l.ptr(t["bits"]), st), "bn2d_apply_mask")
    out = dict(mean=t["mean"].cpu(), invstd=t["invstd"].cpu(), ss=t["ss"].cpu(), rmean=t["rm"].cpu(), rvar=t["rv"].cpu(), y=t["y"].cpu(),
               bits=t["bits"].cpu().numpy() if t["bits"] is not None else None)
    if d["res_mode"] == "dual":
        out["ss2"] = t["ss2"].cpu()
    return t, out


def bn_backward(t, d, x, mean, invstd, gamma, dg0, db0, act=None, mask=None, want_gm=True, reduce2=None):
    """creid_bn2d_bwd_mask / _reduce2 over (x, t['g']); the accumulators start at dg0 / db0.  Returns device tensors."""
    l = L()
    lib, st = l.lib(), l.stream()
    kind, M, C = d["kind"], d["M"], d["C"]
    o = dict(partial=empty32(lib.creid_bn2d_bwd_rows(M), 2, C), sums=empty32(3, C), dgamma=dg0.clone(), dbeta=db0.clone(),
             dx=torch.empty_like(x), gm=torch.empty_like(x) if want_gm else None)
    if reduce2 is None:
        l.check(lib.creid_bn2d_bwd_mask(l.ptr(x), l.ptr(t["g"]), l.ptr(act), l.ptr(mask), l.ptr(mean), l.ptr(invstd), l.ptr(gamma), M, C,
                                        code(kind), l.ptr(o["partial"]), 0, l.ptr(o["sums"]), l.ptr(o["dgamma"]), l.ptr(o["dbeta"]),
                                        l.ptr(o["dx"]), l.ptr(o["gm"]), st), "bn2d_bwd_mask")
    else:
        x2, mean2, invstd2 = reduce2
        o["partial2"] = torch.empty_like(o["partial"])
        l.check(lib.creid_bn2d_bwd_mask_reduce2(l.ptr(x), l.ptr(t["g"]), l.ptr(mask), l.ptr(mean), l.ptr(invstd), l.ptr(gamma), M, C,
                                                code(kind), l.ptr(o["partial"]), 0, l.ptr(o["sums"]), l.ptr(o["dgamma"]),
                                                l.ptr(o["dbeta"]), l.ptr(o["dx"]), l.ptr(x2), l.ptr(mean2), l.ptr(invstd2),
                                                l.ptr(o["partial2"]), st), "bn2d_bwd_mask_reduce2")
    return o


def run_bn_case(M, C, kind, seed, **kw):
    d = er.bn_inputs(M, C, kind, seed, momentum=MOM_R, eps=EPS_R, **kw)
    t, fwd = bn_forward(d)
    er.check_bn_forward(RATIOS, d, fwd)
    # ---- backward: the mask is the device forward's
    rng = np.random.default_rng(seed + 1)
    dg0, db0 = rng.standard_normal(C).astype(f32), rng.standard_normal(C).astype(f32)
    g0, b0 = torch.from_numpy(dg0).cuda(), torch.from_numpy(db0).cuda()
    t["g"] = dev(d["g"], kind)
    is16, relu = kind != "fp32", d["relu"]
    arg = (t, d, t["x"], t["mean"], t["invstd"], t["gamma"], g0, b0)
    main = bn_backward(*arg, act=t["y"] if (relu and not is16) else None, mask=t["bits"] if (relu and is16) else None)
    er.check_bn_backward(RATIOS, d, fwd, {k: (v.cpu() if v is not None else None) for k, v in main.items()}, dg0, db0)
    keys = ("sums", "dgamma", "dbeta", "dx")
    if relu and is16:                               # the `act` form reads y instead of the bits: the same numbers, bit for bit
        alt = bn_backward(*arg, act=t["y"])
        for k in keys + ("gm",):
            assert same_bits(alt[k], main[k]), f"act form vs mask-bit form: {k} differs"
    if is16 and d["res_mode"] == "dual":
        # one pass = dx of this BatchNorm + the column sums of the residual branch's, as the two separate launches
        m = t["bits"] if relu else None
        two = bn_backward(*arg, mask=m, reduce2=(t["res"], t["mean2"], t["invstd2"]))
        for k in keys:
            assert same_bits(two[k], main[k]), f"reduce2 vs bn2d_bwd_mask: {k} differs"
        sep = bn_backward(t, d, t["res"], t["mean2"], t["invstd2"], t["gamma2"], g0, b0, mask=m, want_gm=False)
        assert same_bits(two["partial2"], sep["partial"]), "reduce2: the second BatchNorm's partial rows differ from its own launch"
    return d, t, fwd


# Every variant on every shape.  Past the grid cap each one takes another way through the apply kernels:
#   dual / plain / none    creid_bn2d_apply_dual_mask, creid_bn2d_apply_mask with and without a residual (launchers of their own);
#   ReLU, 16-bit           the backward with the mask bits (two-chunk loop) and again in the act form (one-chunk loop); reduce2;
#   ReLU, fp32             the act form;
#   no ReLU                the backward's two-chunk loop with neither act nor bits -- the only way into that loop in fp32.
ALL_VARIANTS = [(r, relu) for r in ("none", "plain", "dual") for relu in (True, False)]
BN_CASES = [pytest.param(_M, _C, _k, _r, _relu, id=f"M{_M}_C{_C}_{_k}_{_r}_{'relu' if _relu else 'lin'}")
            for _M, _C, _kinds, _ in er.BN_SHAPES for _k in _kinds for _r, _relu in ALL_VARIANTS]


@pytest.mark.parametrize("M,C,kind,res_mode,relu", BN_CASES)
def test_bn_train_forward_backward(M, C, kind, res_mode, relu):
    run_bn_case(M, C, kind, 1000 + M + C, res_mode=res_mode, relu=relu)


@pytest.mark.parametrize("kind", er.KINDS)
@pytest.mark.parametrize("ratio", [16.0, 256.0])
@pytest.mark.parametrize("M,C", er.RATIO_SHAPES)
def test_bn_large_mean_over_std(M, C, ratio, kind):
    """The one-pass variance loses (mean / std)^2 of its precision; the bound says so and the kernel has to stay inside it."""
    run_bn_case(M, C, kind, 2000 + M, ratio=ratio, relu=False)


@pytest.mark.parametrize("kind", er.KINDS)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("M,C", [(300, 40), (129, 24)])
def test_bn_constant_channel(M, C, relu, kind):
    d, t, fwd = run_bn_case(M, C, kind, 3000 + M, relu=relu, const_channel=3)
    assert float(fwd["mean"][3]) == 0.125 and abs(float(fwd["invstd"][3]) - EPS_R ** -0.5) <= 2 * er.U32 * EPS_R ** -0.5


# ------------------------------------------------------------------------------------------------ finalize + apply in one launch
@pytest.mark.parametrize("kind", er.KINDS)
@pytest.mark.parametrize("M,C,row_blocks", er.FIN_APPLY_CASES)
def test_bn_finalize_apply_one_launch(M, C, row_blocks, kind):
    l = L()
    lib, st = l.lib(), l.stream()
    d = er.bn_inputs(M, C, kind, 4000 + M, res_mode="plain", relu=True, momentum=MOM_R, eps=EPS_R)
    t, fwd = bn_forward(d)
    er.check_bn_forward(RATIOS, d, fwd, fam="bn_fin_apply")
    rows = t["partial"].shape[0]
    assert rows <= 1024
    rm, rv = d32(d["rmean"]), d32(d["rvar"])
    mean, invstd, ss, y = empty32(C), empty32(C), empty32(2, C), torch.empty_like(t["x"])
    bits = torch.empty_like(t["bits"]) if t["bits"] is not None else None
    l.check(lib.creid_bn2d_finalize_apply_mask(l.ptr(t["partial"]), rows, C, M, l.ptr(rm), l.ptr(rv), MOM, EPS, l.ptr(t["gamma"]),
                                               l.ptr(t["beta"]), l.ptr(mean), l.ptr(invstd), l.ptr(ss), l.ptr(t["x"]), l.ptr(t["res"]), 1,
                                               code(kind), l.ptr(y), l.ptr(bits), row_blocks, st), "bn2d_finalize_apply_mask")
    for name, a, b in (("mean", mean, t["mean"]), ("invstd", invstd, t["invstd"]), ("scale_shift", ss, t["ss"]), ("running_mean", rm, t["rm"]),
                       ("running_var", rv, t["rv"]), ("y", y, t["y"])) + ((("bits", bits, t["bits"]),) if bits is not None else ()):
        assert same_bits(a, b), f"finalize + apply in one launch vs the two launches: {name} differs"


@pytest.mark.parametrize("kind", er.KINDS)
def test_bn_finalize_apply_refuses(kind):
    l = L()
    lib, st = l.lib(), l.stream()

    def call(rows, C, M):
        part, x = torch.zeros((rows, 2, C), device="cuda"), torch.zeros((M, C), dtype=er.TORCH_DT[kind], device="cuda")
        v = [empty32(C) for _ in range(6)]
        return lib.creid_bn2d_finalize_apply_mask(l.ptr(part), rows, C, M, l.ptr(v[0]), l.ptr(v[1]), MOM, EPS, l.ptr(v[2]), l.ptr(v[3]),
                                                  l.ptr(v[4]), l.ptr(v[5]), l.ptr(empty32(2, C)), l.ptr(x), None, 1, code(kind),
                                                  l.ptr(torch.empty_like(x)), None, 0, st)
    assert call(1025, 64, 256) == E_SHAPE
    assert call(2, 40, 256) == E_SHAPE
    assert call(2, 64, 256) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ max-pool and the stem tail
def _pool_case(shape, kind, mode, seed):
    x = er.pool_inputs(shape, kind, mode, seed)
    if mode == "relu":
        assert float((x == 0).double().mean()) >= 0.5, "post-ReLU input: at least half zeros"
        assert bool((x[0, :2, :2] == 0).all()), "post-ReLU input: the first window of image 0 is all zero"
    if mode == "negative":
        assert bool((x < 0).all())
    B, H, W, C = shape
    return x, er.pool_grad((B, H // 2, W // 2, C), seed + 1)


@pytest.mark.parametrize("kind", er.KINDS)
@pytest.mark.parametrize("mode", er.POOL_MODES)
@pytest.mark.parametrize("shape", er.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_exact(shape, mode, kind):
    from centroids_reid_amd import layers as ly
    x, dy = _pool_case(shape, kind, mode, 50)
    y, idx = ly.maxpool_fwd(dev(x, kind))
    dx = ly.maxpool_bwd(dev(dy, kind), idx, shape[1], shape[2])
    er.check_pool(RATIOS, x, y.cpu(), idx.cpu(), dy, dx.cpu(), kind)


@pytest.mark.parametrize("kind", er.KINDS)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("mode", er.POOL_MODES)
@pytest.mark.parametrize("shape", er.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_tail_fused_equals_separate(shape, mode, relu, kind):
    """creid_bn2d_apply_maxpool3x3s2 = apply then pool; creid_bn2d_bwd_pooled = pool backward then creid_bn2d_bwd: bit for bit."""
    from centroids_reid_amd import layers as ly
    l = L()
    lib, st = l.lib(), l.stream()
    B, H, W, C = shape
    M = B * H * W
    x, dy = _pool_case(shape, kind, mode, 60)
    rng = np.random.default_rng(61)
    # scales of both signs (a negative one turns the all-negative map positive), one channel scaled to zero: every tap ties
    sc = rng.standard_normal(C) + np.where(np.arange(C) % 2 == 0, 0.5, -0.5)
    sc[1] = 0.0
    ss = torch.from_numpy(np.stack([sc, 0.3 * rng.standard_normal(C)]).astype(f32)).cuda()
    xd, dyd = dev(x, kind), dev(dy, kind)
    t = torch.empty_like(xd)
    l.check(lib.creid_bn2d_apply(l.ptr(xd), l.ptr(ss), None, 1 if relu else 0, M, C, code(kind), l.ptr(t), st), "bn2d_apply")
    y_sep, idx_sep = ly.maxpool_fwd(t)
    y = torch.empty_like(y_sep)
    idx = torch.empty_like(idx_sep)
    l.check(lib.creid_bn2d_apply_maxpool3x3s2(l.ptr(xd), l.ptr(ss), 1 if relu else 0, B, H, W, C, code(kind), l.ptr(y), l.ptr(idx), st),
            "bn2d_apply_maxpool3x3s2")
    assert same_bits(y, y_sep), "fused apply + pool: values differ from apply then pool"
    assert same_bits(idx, idx_sep), "fused apply + pool: tap codes differ from apply then pool"
    er.check_pool(RATIOS, t.cpu().double(), y.cpu(), idx.cpu(), None, None, kind, fam="stem_tail")
    # backward
    mean, invstd = d32(0.3 * rng.standard_normal(C)), d32(0.5 + rng.random(C))
    gamma = d32(1 + 0.2 * rng.standard_normal(C))
    act = t if relu else None
    g_full = ly.maxpool_bwd(dyd, idx, H, W)
    acc = [torch.from_numpy(rng.standard_normal(C).astype(f32)).cuda() for _ in range(2)]
    rows = lib.creid_bn2d_bwd_rows(M)
    out = []
    for fused in (False, True):
        o = dict(partial=empty32(rows, 2, C), sums=empty32(3, C), dgamma=acc[0].clone(), dbeta=acc[1].clone(), dx=torch.empty_like(xd))
        if fused:
            l.check(lib.creid_bn2d_bwd_pooled(l.ptr(xd), l.ptr(dyd), l.ptr(idx), B, H, W, l.ptr(act), l.ptr(mean), l.ptr(invstd), l.ptr(gamma),
                                              C, code(kind), l.ptr(o["partial"]), l.ptr(o["sums"]), l.ptr(o["dgamma"]), l.ptr(o["dbeta"]),
                                              l.ptr(o["dx"]), st), "bn2d_bwd_pooled")
        else:
            l.check(lib.creid_bn2d_bwd(l.ptr(xd), l.ptr(g_full), l.ptr(act), l.ptr(mean), l.ptr(invstd), l.ptr(gamma), M, C, code(kind),
                                       l.ptr(o["partial"]), 0, l.ptr(o["sums"]), l.ptr(o["dgamma"]), l.ptr(o["dbeta"]), l.ptr(o["dx"]), None,
                                       st), "bn2d_bwd")
        out.append(o)
    for k in ("partial", "sums", "dgamma", "dbeta", "dx"):
        assert same_bits(out[0][k], out[1][k]), f"pooled backward vs pool backward then bn2d_bwd: {k} differs"


@pytest.mark.parametrize("kind", er.KINDS)
@pytest.mark.parametrize("H,W", [(3, 4), (4, 3), (5, 5)])
def test_pool_backward_refuses_odd_extents(H, W, kind):
    """The kernels walk H / 2 x W / 2 windows and W / 2 column pairs: an odd extent is refused, as by the forward."""
    l = L()
    lib, st = l.lib(), l.stream()
    B, C = 2, 8
    dt = er.TORCH_DT[kind]
    oh, ow = (H + 1) // 2, (W + 1) // 2
    dy = torch.zeros((B, oh, ow, C), dtype=dt, device="cuda")
    idx = torch.zeros((B, oh, ow, C), dtype=torch.uint8, device="cuda")
    x = torch.zeros((B, H, W, C), dtype=dt, device="cuda")
    dx = torch.full_like(x, 7.0)
    assert lib.creid_maxpool3x3s2_fwd(l.ptr(x), B, H, W, C, code(kind), l.ptr(dy), l.ptr(idx), st) == E_ARG
    assert lib.creid_maxpool3x3s2_bwd(l.ptr(dy), l.ptr(idx), B, H, W, C, code(kind), l.ptr(dx), st) == E_ARG
    v = [empty32(C) for _ in range(5)]
    assert lib.creid_bn2d_bwd_pooled(l.ptr(x), l.ptr(dy), l.ptr(idx), B, H, W, None, l.ptr(v[0]), l.ptr(v[1]), l.ptr(v[2]), C, code(kind),
                                     l.ptr(empty32(lib.creid_bn2d_bwd_rows(B * H * W), 2, C)), l.ptr(empty32(3, C)), l.ptr(v[3]), l.ptr(v[4]),
                                     l.ptr(dx), st) == E_ARG
    assert bool((dx == 7.0).all()), "a refused call must not write"


# ------------------------------------------------------------------------------------------------ average pool and layout
@pytest.mark.parametrize("kind", er.KINDS)
@pytest.mark.parametrize("B,HW,C", er.GAP_SHAPES)
def test_gap_and_layout(B, HW, C, kind):
    l = L()
    lib, st = l.lib(), l.stream()
    rng = np.random.default_rng(B + HW + C)
    x = er.round_to(torch.from_numpy(rng.standard_normal((B, HW, C)) + 0.3), kind)
    xd = dev(x, kind)
    feat = empty32(B, C)
    l.check(lib.creid_gap_fwd(l.ptr(xd), B, HW, C, code(kind), l.ptr(feat), st), "gap_fwd")
    ref, mean_abs = er.gap_fwd(x)
    RATIOS.check("gap_fwd", "feat", feat.cpu(), ref, er.gap_fwd_bound(mean_abs, HW))
    counter = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    for n in range(3):
        feat2 = torch.zeros_like(feat)
        l.check(lib.creid_gap_fwd_count(l.ptr(xd), B, HW, C, code(kind), l.ptr(feat2), l.ptr(counter), st), "gap_fwd_count")
        assert int(counter.item()) == 6 + n and same_bits(feat2, feat)
    dfeat = torch.from_numpy(rng.standard_normal((B, C)).astype(f32))
    dx = torch.empty_like(xd)
    l.check(lib.creid_gap_bwd(l.ptr(dfeat.cuda()), B, HW, C, code(kind), l.ptr(dx), st), "gap_bwd")
    RATIOS.exact("gap_bwd", "dx", dx.cpu(), er.gap_bwd(dfeat.numpy(), HW, kind))
    y = empty32(B, C, HW)
    l.check(lib.creid_nhwc_to_nchw_f32(l.ptr(xd), B, HW, C, code(kind), l.ptr(y), st), "nhwc_to_nchw_f32")
    RATIOS.exact("nhwc_to_nchw", "y", y.cpu(), er.nhwc_to_nchw(x))
    RATIOS.count("gap_and_layout")


# ------------------------------------------------------------------------------------------------ IBN
def ibn_forward(d, t=None):
    l = L()
    lib, st = l.lib(), l.stream()
    kind, B, HW, C, c_in = d["kind"], d["B"], d["HW"], d["C"], d["c_in"]
    rpi = lib.creid_ibn_rows_per_image(HW)
    t = dict(x=dev(d["x"], kind), rm=d32(d["rmean"]), rv=d32(d["rvar"]), partial=empty32(B * rpi * 2, C), mean=empty32(B, C),
             invstd=empty32(B, C), ss=empty32(B, 2, C), **{k: d32(d[k]) for k in ("in_w", "in_b", "bn_w", "bn_b")})
    t["y"] = torch.empty_like(t["x"])
    t["bits"] = torch.empty(B * HW * C // 8, dtype=torch.uint8, device="cuda") if kind != "fp32" else None
    l.check(lib.creid_ibn_fwd_mask(l.ptr(t["x"]), B, HW, C, c_in, l.ptr(t["in_w"]), l.ptr(t["in_b"]), l.ptr(t["bn_w"]), l.ptr(t["bn_b"]),
                                   l.ptr(t["rm"]), l.ptr(t["rv"]), 1 if d["training"] else 0, MOM, EPS, 1 if d["relu"] else 0, code(kind),
                                   l.ptr(t["partial"]), 0, l.ptr(t["mean"]), l.ptr(t["invstd"]), l.ptr(t["ss"]), l.ptr(t["y"]),
                                   l.ptr(t["bits"]), st), "ibn_fwd_mask")
    return t, dict(mean=t["mean"].cpu(), invstd=t["invstd"].cpu(), ss=t["ss"].cpu(), rmean=t["rm"].cpu(), rvar=t["rv"].cpu(), y=t["y"].cpu(),
                   bits=t["bits"].cpu().numpy() if t["bits"] is not None else None)


def ibn_backward(t, d, acc0, act=None, mask=None):
    l = L()
    lib, st = l.lib(), l.stream()
    kind, B, HW, C, c_in = d["kind"], d["B"], d["HW"], d["C"], d["c_in"]
    rpi = lib.creid_ibn_rows_per_image(HW)
    o = dict(coef=empty32(B, 3, C), dx=torch.empty_like(t["x"]), d_in_w=acc0[0].clone(), d_in_b=acc0[1].clone(), d_bn_w=acc0[2].clone(),
             d_bn_b=acc0[3].clone())
    part, per_img = empty32(B * rpi * 2, C), empty32(B, 2, c_in)
    l.check(lib.creid_ibn_bwd_mask(l.ptr(t["x"]), l.ptr(t["g"]), l.ptr(act), l.ptr(mask), l.ptr(t["mean"]), l.ptr(t["invstd"]), B, HW, C, c_in,
                                   l.ptr(t["in_w"]), l.ptr(t["bn_w"]), code(kind), l.ptr(part), 0, l.ptr(o["coef"]), l.ptr(per_img),
                                   l.ptr(o["d_in_w"]), l.ptr(o["d_in_b"]), l.ptr(o["d_bn_w"]), l.ptr(o["d_bn_b"]), l.ptr(o["dx"]), st),
            "ibn_bwd_mask")
    return o


@pytest.mark.parametrize("kind", er.KINDS)
@pytest.mark.parametrize("training,relu", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("B,HW,C,c_in", er.IBN_SHAPES)
def test_ibn_forward_backward(B, HW, C, c_in, training, relu, kind):
    d = er.ibn_inputs(B, HW, C, c_in, kind, 7000 + B + HW, relu=relu, training=training, momentum=MOM_R, eps=EPS_R)
    t, fwd = ibn_forward(d)
    er.check_ibn_forward(RATIOS, d, fwd)
    if not training:
        return                                                    # the backward kernels differentiate the training forward
    rng = np.random.default_rng(B + HW)
    a0 = [rng.standard_normal(n).astype(f32) for n in (c_in, c_in, C - c_in, C - c_in)]
    acc0 = [torch.from_numpy(a).cuda() for a in a0]
    t["g"] = dev(d["g"], kind)
    is16 = kind != "fp32"
    main = ibn_backward(t, d, acc0, act=t["y"] if (relu and not is16) else None, mask=t["bits"] if (relu and is16) else None)
    er.check_ibn_backward(RATIOS, d, fwd, {k: v.cpu() for k, v in main.items()}, a0)
    if relu and is16:
        alt = ibn_backward(t, d, acc0, act=t["y"])
        for k in main:
            assert same_bits(alt[k], main[k]), f"act form vs mask-bit form: {k} differs"


@pytest.mark.parametrize("kind", er.KINDS)
def test_ibn_refuses_channel_counts_that_do_not_divide_the_workgroup(kind):
    l = L()
    lib, st = l.lib(), l.stream()
    B, HW, C, c_in = 2, 9, 24, 8
    x = torch.zeros((B, HW, C), dtype=er.TORCH_DT[kind], device="cuda")
    y = torch.full_like(x, 7.0)
    v = [empty32(C) for _ in range(6)]
    part, bc = empty32(B * 2, C), [empty32(B, 3, C) for _ in range(3)]
    assert lib.creid_ibn_fwd_mask(l.ptr(x), B, HW, C, c_in, l.ptr(v[0]), l.ptr(v[1]), l.ptr(v[2]), l.ptr(v[3]), l.ptr(v[4]), l.ptr(v[5]), 1, MOM,
                                  EPS, 1, code(kind), l.ptr(part), 0, l.ptr(bc[0]), l.ptr(bc[1]), l.ptr(bc[2]), l.ptr(y), None, st) == E_SHAPE
    assert lib.creid_ibn_bwd_mask(l.ptr(x), l.ptr(x), None, None, l.ptr(bc[0]), l.ptr(bc[1]), B, HW, C, c_in, l.ptr(v[0]), l.ptr(v[2]),
                                  code(kind), l.ptr(part), 0, l.ptr(bc[2]), l.ptr(empty32(B, 2, c_in)), l.ptr(v[1]), l.ptr(v[3]), l.ptr(v[4]),
                                  l.ptr(v[5]), l.ptr(y), st) == E_SHAPE
    assert bool((y == 7.0).all()), "a refused call must not write"
