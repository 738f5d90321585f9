"""GPU: the head section of a training step (train_ctl_model.py:59-152 between the backbone's forward and backward) against
fp64 at production shapes.  Both routes are driven over the C ABI on given feature matrices -- the separate launches in the
order CTLModel._forward_backward_fused issues them, and creid_ctl_heads_fused (its intermediates are read out of its workspace,
laid out by csrc/heads.hip heads_carve) -- and every tensor either leaves behind is judged by tests/heads_audit.py on the
operands the kernel read: distances, mined indices and hinge decisions (decision windows, first-index ties), losses,
coefficients, both triplet backwards, center loss and its gradients, BNNeck statistics / output / backward, the three classifier
GEMMs, cross entropy, the leave-one-out centroids and their adjoint, the logged scalars, and the end products dfeat, g (rounded
once to g_dtype, times the f16 loss scale), d_fc_weight, d_centers, d_bn_weight, d_bn_bias, running_mean / running_var,
bn_batches_tracked, the lonely count.  With single-pass GEMMs the two routes must also agree bit for bit.

Every bar is derived in heads_audit.py from the kernels' summation order; measured values live in profiles/heads_audit.md.
Nothing here provokes a fault: refused shapes return an error code before any launch."""
import ctypes as C
import math

import pytest
import torch

import heads_audit as ha
import layer_audit as la

pytestmark = pytest.mark.gpu

CFG = ha.configs()
F32 = torch.float32


def _dev(cfg):
    inp = {k: v.cuda() for k, v in ha.make_inputs(cfg).items()}
    inp["nbt0"], inp["lonely0"] = 3, 2                       # the counters are incremented, not set
    return inp


def _state(inp):
    """fresh copies of everything a route accumulates into or updates in place"""
    return dict(d_centers=inp["d_centers0"].clone(), d_fc=inp["d_fc0"].clone(), d_bnw=inp["d_bnw0"].clone(), d_bnb=inp["d_bnb0"].clone(),
                rm=inp["rm0"].clone(), rv=inp["rv0"].clone(), nbt=torch.full((), inp["nbt0"], dtype=torch.int64, device="cuda"),
                lonely=torch.full((1,), inp["lonely0"], dtype=torch.int32, device="cuda"))


def _end(cfg, s, dfeat, g, stats, splits):
    torch.cuda.synchronize()
    return dict(dfeat=dfeat, g=g, stats=stats, d_centers=s["d_centers"], d_fc_weight=s["d_fc"], d_bn_weight=s["d_bnw"],
                d_bn_bias=s["d_bnb"], rm=s["rm"], rv=s["rv"], nbt=int(s["nbt"]), lonely=int(s["lonely"]), splits=splits)


def run_separate(cfg, inp, splits):
    """the separate launches, in the order of CTLModel._forward_backward_fused; each backward that feeds dfeat also runs once into
    a zeroed buffer of its own, so that it is audited alone"""
    from centroids_reid_amd import _lib as L, ops
    lib, st, p = L.lib(), L.stream(), L.ptr
    P, K, D, Cc, B, HW = cfg.P, cfg.K, cfg.D, cfg.C, cfg.B, cfg.HW
    feat, labels, real = inp["feat"], inp["labels"], inp["real"]
    mask = real if cfg.masked else None
    e = lambda *s: torch.empty(*s, dtype=F32, device="cuda")                      # noqa: E731
    z = lambda *s: torch.zeros(*s, dtype=F32, device="cuda")                      # noqa: E731
    ei = lambda *s: torch.empty(*s, dtype=torch.int32, device="cuda")             # noqa: E731
    s = _state(inp)
    it = {}
    n = 4 * (K + 1) + 2
    scal = z(n)
    out4, lc, lx = scal[:4 * (K + 1)].view(K + 1, 4), scal[4 * (K + 1):4 * (K + 1) + 1], scal[4 * (K + 1) + 1:]
    dfeat = z(B, D)
    # query triplet
    q = dict(dap=e(B), dan=e(B), pi=ei(B), ni=ei(B), coef=e(B))
    it["dist_q"] = e(B, B)
    L.check(lib.creid_triplet_fwd_batched(p(feat), p(labels), p(mask), 1, B, D, cfg.margin, p(q["dap"]), p(q["dan"]), p(q["pi"]),
                                          p(q["ni"]), p(q["coef"]), p(out4[0]), p(it["dist_q"]), st), "triplet_fwd")
    it["dx_triplet"] = z(B, D)
    for dx in (it["dx_triplet"], dfeat):
        L.check(lib.creid_triplet_bwd_batched(p(feat), 1, B, D, p(q["dap"]), p(q["dan"]), p(q["pi"]), p(q["ni"]), p(q["coef"]), None,
                                              cfg.w_query, p(dx), st), "triplet_bwd")
    it.update({k + "_q": v for k, v in q.items()})
    # center loss
    centers = inp["centers"]
    it["row_c"], it["dx_center"] = e(B), z(B, D)
    if cfg.masked:
        L.check(lib.creid_center_loss_fwd_masked(p(feat), p(labels), p(centers), p(real), B, centers.shape[0], D, p(it["row_c"]), p(lc), st), "center_fwd")
        for dx, dc in ((it["dx_center"], None), (dfeat, s["d_centers"])):
            L.check(lib.creid_center_loss_bwd_masked(p(feat), p(labels), p(centers), p(it["row_c"]), p(real), B, D, None, cfg.w_center,
                                                     p(dx), p(dc), st), "center_bwd")
    else:
        L.check(lib.creid_center_loss_fwd(p(feat), p(labels), p(centers), B, centers.shape[0], D, p(it["row_c"]), p(lc), st), "center_fwd")
        for dx, dc in ((it["dx_center"], None), (dfeat, s["d_centers"])):
            L.check(lib.creid_center_loss_bwd(p(feat), p(labels), p(centers), p(it["row_c"]), B, D, None, cfg.w_center, p(dx), p(dc), st),
                    "center_bwd")
    # BNNeck -> classifier -> cross entropy
    bw, bb, W = inp["bn_w"], inp["bn_b"], inp["W"]
    s["nbt"] += 1
    it["bnf"], it["sm"], it["si"] = e(B, D), e(D), e(D)
    if cfg.masked:
        L.check(lib.creid_bn1d_fwd_masked(p(feat), p(real), B, D, p(bw), p(bb), p(s["rm"]), p(s["rv"]), cfg.momentum, cfg.bn_eps,
                                          p(it["bnf"]), p(it["sm"]), p(it["si"]), st), "bn_fwd")
    else:
        L.check(lib.creid_bn1d_fwd(p(feat), B, D, p(bw), p(bb), p(s["rm"]), p(s["rv"]), 1, cfg.momentum, cfg.bn_eps, p(it["bnf"]),
                                   p(it["sm"]), p(it["si"]), st), "bn_fwd")
    it["logits"] = ops.gemm_f32(it["bnf"], D, 1, W, 1, D, B, Cc, D, split_k=splits[0])
    it["row_x"], it["dlogits"] = e(B), e(B, Cc)
    if cfg.masked:
        L.check(lib.creid_xent_ls_masked(p(it["logits"]), p(labels), p(real), B, Cc, cfg.eps, cfg.w_xent, p(it["row_x"]), p(lx),
                                         p(it["dlogits"]), st), "xent")
    else:
        L.check(lib.creid_xent_ls(p(it["logits"]), p(labels), B, Cc, cfg.eps, cfg.w_xent, p(it["row_x"]), p(lx), p(it["dlogits"]), st), "xent")
    it["dbnf"] = ops.gemm_f32(it["dlogits"], Cc, 1, W, D, 1, B, D, Cc, split_k=splits[1])
    ops.gemm_f32(it["dlogits"], 1, Cc, it["bnf"], D, 1, Cc, D, B, out=s["d_fc"], beta=1.0)
    it["dx_bn"] = z(B, D)
    for dx, dw, db in ((it["dx_bn"], None, None), (dfeat, s["d_bnw"], s["d_bnb"])):
        if cfg.masked:
            L.check(lib.creid_bn1d_bwd_masked(p(feat), p(it["dbnf"]), p(real), B, D, p(bw), p(it["sm"]), p(it["si"]), p(dx), p(dw), p(db), st), "bn_bwd")
        else:
            L.check(lib.creid_bn1d_bwd(p(feat), p(it["dbnf"]), B, D, p(bw), p(it["sm"]), p(it["si"]), p(dx), p(dw), p(db), st), "bn_bwd")
    # leave-one-out centroids and the K rounds
    R = 2 * P
    it["cent"], it["valid"], it["emb"] = e(K, P, D), ei(K, P), e(K, R, D)
    it["lab"], it["cnorm"] = torch.empty((K, R), dtype=torch.int64, device="cuda"), e(K * P)
    it["demb"] = z(K, R, D)
    r = dict(dap=e(K * R), dan=e(K * R), pi=ei(K * R), ni=ei(K * R), coef=e(K * R))
    if cfg.masked:
        it["rows"], it["inv_rounds"] = torch.empty((K, R), dtype=torch.uint8, device="cuda"), e(1)
        L.check(lib.creid_loo_emb_fwd_rows_lonely(p(feat), p(real), p(labels), P, K, D, p(it["cent"]), p(it["valid"]), p(it["emb"]),
                                                  p(it["lab"]), p(it["cnorm"]), p(it["rows"]), p(s["lonely"]), st), "loo_fwd")
        L.check(lib.creid_triplet_fwd_batched_rows(p(it["emb"]), p(it["lab"]), p(it["rows"]), K, R, D, cfg.margin, 4, p(r["dap"]), p(r["dan"]),
                                                   p(r["pi"]), p(r["ni"]), p(r["coef"]), p(out4[1:]), st), "rounds_fwd")
        L.check(lib.creid_ctl_round_scale(p(out4[1:]), K, p(it["inv_rounds"]), st), "round_scale")
        gdev, gs = it["inv_rounds"], cfg.w_centroid
    else:
        L.check(lib.creid_loo_emb_fwd(p(feat), p(real), p(labels), P, K, D, p(it["cent"]), p(it["valid"]), p(it["emb"]), p(it["lab"]),
                                      p(it["cnorm"]), st), "loo_fwd")
        L.check(lib.creid_triplet_fwd_batched(p(it["emb"]), p(it["lab"]), None, K, R, D, cfg.margin, p(r["dap"]), p(r["dan"]), p(r["pi"]),
                                              p(r["ni"]), p(r["coef"]), p(out4[1:]), None, st), "rounds_fwd")
        gdev, gs = None, cfg.w_centroid / K
    L.check(lib.creid_triplet_bwd_batched(p(it["emb"]), K, R, D, p(r["dap"]), p(r["dan"]), p(r["pi"]), p(r["ni"]), p(r["coef"]), p(gdev), gs,
                                          p(it["demb"]), st), "rounds_bwd")
    it.update({k + "_r": v for k, v in r.items()})
    it["dfeat_pre"] = dfeat.clone()
    L.check(lib.creid_loo_emb_bwd(p(it["demb"]), p(real), P, K, D, p(dfeat), st), "loo_bwd")
    # logged scalars, g
    wv = ha.loss_weight_vector(cfg).cuda()
    stats = e(n + 7)
    if cfg.masked:
        L.check(lib.creid_ctl_step_stats_rows(p(scal), p(wv), n, K, P, p(it["cnorm"]), p(it["rows"]), p(stats), st), "stats")
    else:
        L.check(lib.creid_ctl_step_stats(p(scal), p(wv), n, K, p(it["cnorm"]), K * P, p(stats), st), "stats")
    src = dfeat
    if cfg.scale:
        amp = torch.tensor([cfg.scale, 1.0 / cfg.scale], dtype=F32, device="cuda")
        src = torch.empty_like(dfeat)
        L.check(lib.creid_amp_scale(p(dfeat), dfeat.numel(), p(amp), p(src), st), "amp_scale")
    g = torch.zeros((B * HW, D), dtype=ha.G_DT[cfg.g_dtype], device="cuda")
    rc = lib.creid_gap_bwd(p(src), B, HW, D, cfg.g_dtype, p(g), st)
    if D % 8:            # creid_gap_bwd moves 8-channel chunks: it refuses such a width before any launch; the heads end at dfeat
        torch.cuda.synchronize()
        assert rc == -1 and not bool(g.any())
        g = None
    else:
        L.check(rc, "gap_bwd")
    it["scal"] = scal
    return it, _end(cfg, s, dfeat, g, stats, splits)


def _carve(B, P, K, D, Cc):
    """byte offsets of csrc/heads.hip heads_carve (every member rounded up to 256 bytes) -> {name: (offset, count, dtype)}"""
    off, out = 0, {}
    R = K * 2 * P

    def take(name, count, dt, size):
        nonlocal off
        out[name] = (off, count, dt)
        off += (count * size + 255) // 256 * 256

    n_logits = (B * Cc + 3) // 4 * 4
    z0 = off
    take("_zero", B * D + R * D + n_logits + B * D, F32, 4)
    out["dfeat_pre"], out["demb"] = (z0, B * D, F32), (z0 + 4 * B * D, R * D, F32)
    out["logits"], out["dbnf"] = (z0 + 4 * (B * D + R * D), B * Cc, F32), (z0 + 4 * (B * D + R * D + n_logits), B * D, F32)
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    for name, count, dt, size in (("dlogits", B * Cc, F32, 4), ("bnf", B * D, F32, 4), ("sm", D, F32, 4), ("si", D, F32, 4), ("row_c", B, F32, 4),
                                  ("row_x", B, F32, 4), ("scal", 4 * (K + 1) + 2, F32, 4), ("inv_rounds", 1, F32, 4), ("dap_q", B, F32, 4),
                                  ("dan_q", B, F32, 4), ("coef_q", B, F32, 4), ("pi_q", B, i32, 4), ("ni_q", B, i32, 4), ("dap_r", R, F32, 4),
                                  ("dan_r", R, F32, 4), ("coef_r", R, F32, 4), ("pi_r", R, i32, 4), ("ni_r", R, i32, 4), ("cent", K * P * D, F32, 4),
                                  ("valid", K * P, i32, 4), ("emb", R * D, F32, 4), ("lab", R, i64, 8), ("cnorm", K * P, F32, 4), ("rows", R, u8, 1)):
        take(name, count, dt, size)
    del out["_zero"]
    return out, off


def fused_args(cfg, inp, s, splits, g, stats, dfeat_out, ws, nbytes, amp):
    from centroids_reid_amd import _lib as L
    a = L.CtlHeads()
    a.B, a.P, a.K, a.D, a.num_classes, a.num_centers, a.HW = cfg.B, cfg.P, cfg.K, cfg.D, cfg.C, inp["centers"].shape[0], cfg.HW
    a.g_dtype, a.masked, a.split_logits, a.split_dbnf = cfg.g_dtype, 1 if cfg.masked else 0, splits[0], splits[1]
    a.margin, a.xent_eps, a.w_query, a.w_center = cfg.margin, cfg.eps, cfg.w_query, cfg.w_center
    a.w_xent, a.w_centroid, a.bn_momentum, a.bn_eps = cfg.w_xent, cfg.w_centroid, cfg.momentum, cfg.bn_eps
    wv = ha.loss_weight_vector(cfg).cuda()
    keep = [wv]
    for name, t in (("feat", inp["feat"]), ("labels", inp["labels"]), ("is_real", inp["real"]), ("centers", inp["centers"]),
                    ("bn_weight", inp["bn_w"]), ("bn_bias", inp["bn_b"]), ("bn_running_mean", s["rm"]), ("bn_running_var", s["rv"]),
                    ("fc_weight", inp["W"]), ("loss_weights", wv), ("amp_state", amp), ("d_centers", s["d_centers"]),
                    ("d_bn_weight", s["d_bnw"]), ("d_bn_bias", s["d_bnb"]), ("d_fc_weight", s["d_fc"]), ("bn_batches_tracked", s["nbt"]),
                    ("lonely", s["lonely"] if cfg.masked else None), ("stats", stats), ("g", g), ("dfeat_out", dfeat_out), ("workspace", ws)):
        setattr(a, name, None if t is None else t.data_ptr())
    a.workspace_bytes = nbytes
    return a, keep


def run_fused(cfg, inp, splits):
    from centroids_reid_amd import _lib as L
    lib = L.lib()
    P, K, D, Cc, B, HW = cfg.P, cfg.K, cfg.D, cfg.C, cfg.B, cfg.HW
    s = _state(inp)
    n = 4 * (K + 1) + 2
    nbytes = lib.creid_ctl_heads_workspace_bytes(B, P, K, D, Cc)
    lay, total = _carve(B, P, K, D, Cc)
    assert total == nbytes, "the workspace layout of heads_carve changed: update _carve"
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    stats = torch.empty(n + 7, dtype=F32, device="cuda")
    g = torch.empty((B * HW, D), dtype=ha.G_DT[cfg.g_dtype], device="cuda")
    dfeat_out = torch.empty((B, D), dtype=F32, device="cuda")
    amp = torch.tensor([cfg.scale, 1.0 / cfg.scale], dtype=F32, device="cuda") if cfg.scale else None
    a, keep = fused_args(cfg, inp, s, splits, g, stats, dfeat_out, ws, nbytes, amp)
    L.check(lib.creid_ctl_heads_fused(C.byref(a), L.stream()), "creid_ctl_heads_fused")
    torch.cuda.synchronize()
    it = {}
    size = {F32: 4, torch.int32: 4, torch.int64: 8, torch.uint8: 1}
    for name, (off, count, dt) in lay.items():
        it[name] = ws[off:off + count * size[dt]].view(dt).clone()
    R = 2 * P
    for name, shape in (("dfeat_pre", (B, D)), ("demb", (K, R, D)), ("logits", (B, Cc)), ("dbnf", (B, D)), ("dlogits", (B, Cc)), ("bnf", (B, D)),
                        ("cent", (K, P, D)), ("valid", (K, P)), ("emb", (K, R, D)), ("lab", (K, R)), ("rows", (K, R))):
        it[name] = it[name].view(*shape)
    return it, _end(cfg, s, dfeat_out, g, stats, splits)


def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b):
    if not torch.is_tensor(a):
        return a == b
    return torch.equal(_bits(a).reshape(-1), _bits(b).reshape(-1))


def _report(A, conds, cfg, assert_conds=True):
    ha.check_conditions_note(A, "decisions", conds)
    print("\n" + A.table())
    print(A.op_summary())
    for tag, n, und, act, ties in conds:
        print(f"[{A.tag}] {tag:<8} anchors {n:>3} undecided {und:>2} active {act:>3} first-index ties {ties}")
    assert not A.failures, "\n".join(A.failures)
    if assert_conds:
        ha.assert_conditions(cfg, conds)


CASES = [("bench", (1, 1)), ("bench", (32, 12)), ("bench_mask", (1, 1)), ("bench_mask", (32, 12)), ("s2s", (1, 1)), ("s2s", (32, 12)),
         ("s2s_mask", (1, 1)), ("s2s_mask", (32, 12)), ("bench_f32", (1, 1)), ("bench_f16", (1, 1)), ("bench_mask_f16", (32, 12)),
         ("p2k2", (1, 1)), ("k16", (1, 1)), ("b256", (1, 1)), ("d264", (1, 1)), ("d264", (32, 12)), ("skip_round", (1, 1)),
         ("skip_round", (32, 12)), ("skip_all", (1, 1)), ("accumulate", (32, 12)), ("accumulate_mask", (1, 1))]


@pytest.mark.parametrize("name,splits", CASES, ids=[f"{n}-{s[0]}x{s[1]}" for n, s in CASES])
def test_heads_both_routes_against_fp64(name, splits):
    """one fp64 judgement per route; with single-pass GEMMs (1, 1) the fused call must also equal the separate launches bit for
    bit -- intermediates and end products, with and without the mask"""
    cfg = CFG[name]
    inp = _dev(cfg)
    A = la.Audit(f"{name} {splits[0]}x{splits[1]}")
    it_s, end_s = run_separate(cfg, inp, splits)
    conds = ha.audit_route(A, cfg, inp, it_s, end_s, "separate")
    it_f, end_f = run_fused(cfg, inp, splits)
    conds_f = ha.audit_route(A, cfg, inp, it_f, end_f, "fused")
    A.exact("fused", "same decisions as separate", conds == conds_f)
    if splits == (1, 1):
        skip = set() if cfg.masked else {"rows", "inv_rounds"}
        diff = [k for k in it_f if k in it_s and k not in skip and not _same(it_f[k], it_s[k])]
        diff += [k for k in end_f if not _same(end_f[k], end_s[k])]
        A.exact("fused", "bit-identical to separate", not diff, ", ".join(diff))
    _report(A, conds, cfg)
    if name.startswith("bench"):                        # the bit-identical rows of make_inputs put a first-index tie in front of the kernel
        assert sum(c[4] for c in conds) >= 1


@pytest.mark.parametrize("name,rc", [("b320", -4), ("d260", -4), ("soft", -1)])
def test_heads_separate_launches_beyond_the_fused_call(name, rc):
    """B = 320 (two trips of triplet_bwd_body's 256-anchor compaction), D % 8 != 0, the soft-margin loss: the fused call refuses them
    with an error code (no launch), the separate launches are audited"""
    from centroids_reid_amd import _lib as L
    cfg = CFG[name]
    inp = _dev(cfg)
    s = _state(inp)
    nbytes = L.lib().creid_ctl_heads_workspace_bytes(cfg.B, cfg.P, cfg.K, cfg.D, cfg.C)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    stats, dfo = torch.zeros(4 * (cfg.K + 1) + 9, device="cuda"), torch.zeros(cfg.B, cfg.D, device="cuda")
    g = torch.zeros((cfg.B * cfg.HW, cfg.D), dtype=ha.G_DT[cfg.g_dtype], device="cuda")
    a, keep = fused_args(cfg, inp, s, (1, 1), g, stats, dfo, ws, nbytes, None)
    assert L.lib().creid_ctl_heads_fused(C.byref(a), L.stream()) == rc
    torch.cuda.synchronize()
    assert not bool(g.any()) and not bool(ws.any()) and int(s["nbt"]) == inp["nbt0"]          # nothing was launched
    A = la.Audit(name)
    it, end = run_separate(cfg, inp, (32, 12))
    _report(A, ha.audit_route(A, cfg, inp, it, end, "separate"), cfg)


def test_center_loss_alone_beyond_the_listed_branch():
    """creid_center_loss_fwd / _bwd at B = 1100: center_bwd_body re-discovers a class's members instead of listing them in LDS
    (B > 1024); labels repeat (up to a handful of members per class), the accumulators start non-zero"""
    from centroids_reid_amd import _lib as L
    lib, st, p = L.lib(), L.stream(), L.ptr
    B, D, Cc, w = 1100, 2048, 751, 5e-4
    g = torch.Generator().manual_seed(7)
    x = (0.4 + 0.35 * torch.randn(B, D, generator=g)).clamp_min(0).cuda()
    labels = torch.randint(0, Cc, (B,), generator=g).cuda()
    centers = (0.3 * torch.randn(Cc, D, generator=g)).cuda()
    dcen0, dx0 = (0.01 * torch.randn(Cc, D, generator=g)).cuda(), (0.01 * torch.randn(B, D, generator=g)).cuda()
    row, lc, dx, dcen = torch.empty(B, device="cuda"), torch.empty(1, device="cuda"), torch.zeros(B, D, device="cuda"), dcen0.clone()
    L.check(lib.creid_center_loss_fwd(p(x), p(labels), p(centers), B, Cc, D, p(row), p(lc), st), "center_fwd")
    L.check(lib.creid_center_loss_bwd(p(x), p(labels), p(centers), p(row), B, D, None, w, p(dx), p(dcen), st), "center_bwd")
    acc = dx0.clone()
    L.check(lib.creid_center_loss_bwd(p(x), p(labels), p(centers), p(row), B, D, None, w, p(acc), None, st), "center_bwd")
    torch.cuda.synchronize()
    A = la.Audit("center B=1100")
    members = int(torch.bincount(labels).max())
    on = torch.ones(B, dtype=torch.bool, device="cuda")
    ref = ha.audit_center(A, "separate", x.double(), labels, centers.double(), row, lc, dx, dcen, dcen0.double(), on, w, members)
    tot = dx0.double() + ref
    A.check("separate", "center bwd dx accumulate", acc, tot, 7 * la.U * ref.abs() + la.U * tot.abs(), F32, sigma=la.U * tot.abs())
    print("\n" + A.table() + "\n" + A.op_summary())
    assert not A.failures, "\n".join(A.failures)


def test_loo_emb_bwd_refuses_more_than_16_instances():
    from centroids_reid_amd import _lib as L
    P, K, D = 2, 17, 64
    demb = torch.ones(K, 2 * P, D, device="cuda")
    real = torch.ones(P * K, dtype=torch.uint8, device="cuda")
    dfeat = torch.full((P * K, D), 3.0, device="cuda")
    assert L.lib().creid_loo_emb_bwd(L.ptr(demb), L.ptr(real), P, K, D, L.ptr(dfeat), L.stream()) == -4      # CREID_E_SHAPE
    torch.cuda.synchronize()
    assert bool((dfeat == 3.0).all())                                                                          # nothing was launched


GEMM_SHAPES = [(64, 751, 2048), (56, 1000, 2048), (64, 751, 264)]            # (B, classes, D) of bench, s2s, d264


@pytest.mark.parametrize("B,Cc,D", GEMM_SHAPES)
def test_gemm_f32_against_fp64(B, Cc, D):
    """creid_gemm_f32 at the three head geometries: logits = bnf W^T (row-major x transposed), dbnf = dlogits W, dW += dlogits^T bnf
    (transposed A), split_k 1 / 12 / 32 (the weight gradient has K = B: four 16-deep k-tiles, so most slices are empty), beta = 0
    and beta = 1.  Bound: (K + split + 1) u sum |a||b| (the MFMA chain and one atomic per slice) + u |beta C0 + result|."""
    from centroids_reid_amd import ops
    g = torch.Generator().manual_seed(B + Cc + D)
    bnf = torch.randn(B, D, generator=g).cuda()
    W = (0.01 * torch.randn(Cc, D, generator=g)).cuda()
    dl = (1e-3 * torch.randn(B, Cc, generator=g)).cuda()
    A = la.Audit(f"gemm {B}x{Cc}x{D}")
    geo = {"fwd": (bnf, D, 1, W, 1, D, B, Cc, D, lambda: bnf.double() @ W.double().t(), lambda: bnf.abs().double() @ W.abs().double().t()),
           "dgrad": (dl, Cc, 1, W, D, 1, B, D, Cc, lambda: dl.double() @ W.double(), lambda: dl.abs().double() @ W.abs().double()),
           "wgrad": (dl, 1, Cc, bnf, D, 1, Cc, D, B, lambda: dl.double().t() @ bnf.double(), lambda: dl.abs().double().t() @ bnf.abs().double())}
    for tag, (a, sam, sak, b, sbk, sbn, M, N, Kd, ref, mag) in geo.items():
        ref, mag = ref(), mag()
        c0 = (ref.abs().mean() * torch.randn(M, N, generator=g).cuda().double()).float()
        for split in (1, 12, 32):
            for beta in (0.0, 1.0):
                out = c0.clone() if beta else torch.full((M, N), float("nan"), device="cuda")
                ops.gemm_f32(a, sam, sak, b, sbk, sbn, M, N, Kd, out=out, beta=beta, split_k=split)
                want = ref + beta * c0.double()
                A.check(tag, f"split {split} beta {beta:g}", out, want, (Kd + split + 1) * la.U * mag + la.U * want.abs(), F32,
                        sigma=math.sqrt(Kd) * la.U * mag + la.U * want.abs())
    print("\n" + A.table())
    assert not A.failures, "\n".join(A.failures)


def test_heads_on_real_backbone_features():
    """the features of one bf16 benchmark-shape forward (seeded weights, synthetic images) instead of the generator; the two input
    conditions are recorded for this distribution, not asserted"""
    from oracle import backbone_oracle as bo
    from centroids_reid_amd.bench_train import make_model
    cfg = CFG["bench"]
    torch.manual_seed(0)
    model = make_model(num_classes=cfg.C, dtype=torch.bfloat16, K=cfg.K)
    model.backbone.base.load_state_dict(bo.make_state_dict("resnet50", 1, seed=11))
    x = bo.synthetic_images(cfg.B, 256, 128, seed=5).cuda()
    _, feat = model.backbone.engine.forward(x.contiguous().float(), True, False)
    assert feat.shape == (cfg.B, cfg.D) and feat.dtype == F32 and bool(torch.isfinite(feat).all())
    for fakes, name in ((None, "real features"), (ha.MASK1, "real features, mask")):
        c = ha.Cfg(name, cfg.P, cfg.K, fakes=fakes, dup=False)
        inp = _dev(c)
        inp["feat"] = feat.clone().contiguous()
        A = la.Audit(name)
        it, end = run_separate(c, inp, (32, 12))
        conds = ha.audit_route(A, c, inp, it, end, "separate")
        it, end = run_fused(c, inp, (32, 12))
        ha.audit_route(A, c, inp, it, end, "fused")
        _report(A, conds, c, assert_conds=False)
