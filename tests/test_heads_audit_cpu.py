"""CPU: the heads audit (tests/heads_audit.py) on an fp32 torch emulation of the head kernels at the benchmark shape (P 16 x K 4,
D 2048, 751 classes).  The unmutated emulation passes every check; each mutation a head kernel could plausibly carry is caught.
The same file asserts the two conditions on the synthetic inputs of EVERY audited configuration with the fp64 reference alone:
at most 5 % of a problem's anchors (or two) undecided, 20-80 % of the hinges active -- so the GPU audit never leans on inputs
whose triplet gradient is all zero, or on decisions fp32 cannot take.  The same functions judge the real kernels in
tests/test_heads_audit_gpu.py."""
import pytest
import torch

import heads_audit as ha
import layer_audit as la

F32 = torch.float32


def _trunc_bf16(v):
    return (v.float().contiguous().view(torch.int32) & ~0xFFFF).view(F32).to(torch.bfloat16)


def _mine32(xs, lab, ex, last_index=False):
    """the kernel's expanded form in fp32: sqrt(max(xx + yy - 2 x.y, 1e-12)); every (anchor, row) dot product by the same
    reduction, so bit-identical rows give bit-equal distances; first-index arg-max / arg-min"""
    N = xs.shape[0]
    n2 = (xs * xs).sum(1)
    dot = torch.empty(N, N)
    for i in range(0, N, 16):
        dot[i:i + 16] = (xs[i:i + 16, None, :] * xs[None]).sum(-1)
    d = torch.sqrt(((n2[:, None] + n2[None]) - 2.0 * dot).clamp_min(1e-12))
    same = lab[:, None] == lab[None]
    idx = torch.arange(N)[None].expand(N, N)
    res = []
    for cand, sign in ((same & ex[None], 1.0), (~same & ex[None], -1.0)):
        s = torch.where(cand, sign * d, torch.full_like(d, -float("inf")))
        best = s.max(1).values
        hit = s == best[:, None]
        i = torch.where(hit, idx, torch.full_like(idx, -1)).max(1).values if last_index else \
            torch.where(hit, idx, torch.full_like(idx, N)).min(1).values
        res += [sign * best, i.clamp(0, N - 1).int()]
    return d, res[0], res[2], res[1], res[3]


def _loss32(dap, dan, on, margin, min_a):
    n = float(on.sum())
    if n == 0 or n < min_a:
        return torch.zeros(4), torch.zeros_like(dap)
    m = on.float()
    dap, dan = torch.where(on, dap, torch.zeros(())), torch.where(on, dan, torch.zeros(()))
    if margin >= 0:
        v = (dap - dan + margin) * m
        act = v > 0
        l, coef = (v * act).sum(), act.float() / n
    else:
        z = dap - dan
        l, coef = (torch.nn.functional.softplus(z) * m).sum(), torch.sigmoid(z) / n * m
    return torch.stack([l / n, (dap * m).sum() / n, (dan * m).sum() / n, torch.tensor(n)]), coef


def emulate(cfg, inp, mut=()):
    """One head pass in fp32 torch, laid out like the tensors a route leaves behind (heads_audit.audit_route's `it` / `end`)."""
    P, K, D, C, B, HW = cfg.P, cfg.K, cfg.D, cfg.C, cfg.B, cfg.HW
    x, labels, real = inp["feat"], inp["labels"], inp["real"]
    on = real.bool() if cfg.masked else torch.ones(B, dtype=torch.bool)
    m = on.float()[:, None]
    nb = float(on.sum())
    it, end = {}, {}
    # leave-one-out centroids
    x3, r = x.view(P, K, D), real.view(P, K).bool()
    cent, valid = torch.zeros(K, P, D), torch.zeros(K, P, dtype=torch.int32)
    for i in range(K):
        acc, cnt = torch.zeros(P, D), torch.zeros(P)
        for s in range(K):
            if s != i:
                w = (r[:, i] & r[:, s]).float()
                acc, cnt = acc + x3[:, s] * w[:, None], cnt + w
        den = torch.full_like(cnt, K - 1.0) if "loo_div_k1" in mut else cnt.clamp_min(1.0)
        cent[i], valid[i] = acc / den[:, None], cnt.int()
    it["cent"], it["valid"] = cent, valid
    it["emb"] = torch.cat([x3.permute(1, 0, 2), cent], 1).contiguous()
    it["lab"] = labels.view(P, K).t().repeat(1, 2).contiguous()
    it["cnorm"] = cent.pow(2).sum(-1).sqrt().reshape(-1)
    rows = (valid > 0).repeat(1, 2)
    it["rows"] = rows.to(torch.uint8)
    end["lonely"] = int((r & (valid.t() == 0)).sum())
    # triplet problems
    scal = torch.zeros(4 * (K + 1) + 2)
    last = "last_index" in mut
    d, dap, dan, pi, ni = _mine32(x, labels, torch.ones(B, dtype=torch.bool), last)
    scal[:4], coef = _loss32(dap, dan, on, cfg.margin, 0)
    it.update(dist_q=d, dap_q=dap, dan_q=dan, pi_q=pi, ni_q=ni, coef_q=coef)
    it["dx_triplet"] = ha.triplet_bwd64(x.double(), dap, dan, pi, ni, coef, cfg.w_query)[0].float()
    rr = {k: [] for k in ("dap", "dan", "pi", "ni", "coef")}
    for i in range(K):
        ex = rows[i] if cfg.masked else torch.ones(2 * P, dtype=torch.bool)
        _, a, b, c, e = _mine32(it["emb"][i], it["lab"][i], ex, last)
        scal[4 * (i + 1):4 * (i + 2)], cf = _loss32(a, b, ex, cfg.margin, 4 if cfg.masked else 0)
        for k, v in zip(rr, (a, b, c, e, cf)):
            rr[k].append(v)
    for k, v in rr.items():
        it[k + "_r"] = torch.stack(v).reshape(-1)
    nv = int((scal[4:4 * (K + 1)].view(K, 4)[:, 3] >= 4).sum())
    inv_r = (1.0 / K if "round_mean_k" in mut else (1.0 / nv if nv else 0.0))
    it["inv_rounds"] = torch.tensor([inv_r])
    g_round = cfg.w_centroid * (inv_r if cfg.masked else 1.0 / K)
    it["demb"] = torch.stack([ha.triplet_bwd64(it["emb"][i].double(), rr["dap"][i], rr["dan"][i], rr["pi"][i], rr["ni"][i],
                                               rr["coef"][i], g_round)[0].float() for i in range(K)])
    # center loss
    cy = inp["centers"][labels]
    it["row_c"] = ((x * x).sum(1) + (cy * cy).sum(1)) - 2.0 * (x * cy).sum(1)
    n_c = float(B) if "center_div_B" in mut else nb
    scal[4 * (K + 1)] = ((it["row_c"].clamp(1e-12, 1e12) * m[:, 0]).sum() + n_c * (C - 1) * 1e-12) / n_c
    gc = cfg.w_center * (1.0 if "center_no_2" in mut else 2.0) / n_c
    it["dx_center"] = gc * (x - cy) * m
    end["d_centers"] = inp["d_centers0"] + torch.zeros(C, D).index_add_(0, labels, gc * (cy - x) * m)   # members first, ONE += (center_bwd_body)
    # BNNeck -> classifier -> cross entropy
    n_b = float(B) if "bn_div_B" in mut else nb
    mean = (x * m).sum(0) / n_b
    t = (x - mean) * m
    m2 = (t * t).sum(0)
    var = m2 / n_b
    it["sm"], it["si"] = mean, 1.0 / torch.sqrt(var + cfg.bn_eps)
    mo = cfg.momentum
    end["rm"] = (1 - mo) * inp["rm0"] + mo * mean
    end["rv"] = (1 - mo) * inp["rv0"] + mo * (var if "rv_biased" in mut else m2 / (n_b - 1))
    end["nbt"] = 1
    xh = (x - mean) * it["si"]
    it["bnf"] = (xh * inp["bn_w"] + inp["bn_b"]) * m
    W = inp["W"]
    it["logits"] = z = it["bnf"] @ W.t()
    zc = z - z.max(1, keepdim=True).values
    se = zc.exp().sum(1, keepdim=True)
    p = zc.exp() / se
    tgt = torch.zeros_like(z) if "no_smoothing" in mut else torch.full_like(z, cfg.eps / C)
    tgt[torch.arange(B), labels] += 1.0 - cfg.eps
    n_x = float(B) if "xent_div_B" in mut else nb
    it["dlogits"] = (p - tgt) * (cfg.w_xent / n_x) * m
    logp = zc - se.log()
    it["row_x"] = -((1 - cfg.eps) * logp.gather(1, labels[:, None])[:, 0] + cfg.eps / C * logp.sum(1)) * m[:, 0]
    scal[4 * (K + 1) + 1] = it["row_x"].sum() / n_x
    dl = it["dlogits"]
    it["dbnf"] = dl[:, :704] @ W[:704] if "drop_k_slice" in mut else dl @ W       # 12 slices of 64: the last one holds 47
    end["d_fc_weight"] = inp["d_fc0"] + dl.t() @ it["bnf"]
    dy = it["dbnf"] * m
    s1, s2 = dy.sum(0), (dy * xh * m).sum(0)
    it["dx_bn"] = (inp["bn_w"] * it["si"] / nb) * (nb * dy - s1 - xh * s2) * m
    end["d_bn_weight"], end["d_bn_bias"] = inp["d_bnw0"] + s2, inp["d_bnb0"] + s1
    it["dfeat_pre"] = it["dx_triplet"] + it["dx_center"] + it["dx_bn"]
    # leave-one-out adjoint, g
    de, rf = it["demb"], r.float()
    dq = de[:, :P].permute(1, 0, 2)
    dc = de[:, P:].permute(1, 0, 2) * (rf / valid.t().float().clamp_min(1.0))[:, :, None]
    end["dfeat"] = it["dfeat_pre"] + (dq + (dc.sum(1, keepdim=True) - dc) * rf[:, :, None]).reshape(B, D)
    v = end["dfeat"]
    if cfg.scale and "no_loss_scale" not in mut:
        v = v * cfg.scale
    if "no_hw" not in mut:
        v = v * (1.0 / HW)
    gdt = ha.G_DT[cfg.g_dtype]
    v = _trunc_bf16(v) if "g_trunc" in mut else v.to(gdt)
    end["g"] = v[:, None, :].expand(B, HW, D)
    # logged scalars
    it["scal"] = scal
    wv = ha.loss_weight_vector(cfg)
    n = scal.numel()
    rl = torch.zeros(n, dtype=torch.bool)
    rl[4:4 * (K + 1):4] = True
    o4r = scal[4:4 * (K + 1)].view(K, 4)
    if cfg.masked:
        vr = (o4r[:, 3] >= 4).float()
        terms = scal * wv * torch.where(rl, torch.tensor(inv_r), torch.tensor(1.0))
        rmean = (o4r * vr[:, None]).sum(0) * inv_r
        ex = rows[:, P:].float()
        l2 = sum((it["cnorm"].view(K, P)[k] * ex[k]).sum() / ex[k].sum() for k in range(K) if vr[k] > 0) * inv_r if nv else torch.zeros(())
    else:
        terms, rmean, l2 = scal * wv, o4r.mean(0), it["cnorm"].mean()
    end["stats"] = torch.cat([terms, terms.sum()[None], terms[rl].sum()[None], rmean, torch.as_tensor(l2).reshape(1)])
    return it, end


def _audit(cfg, mut=()):
    torch.manual_seed(0)
    inp = ha.make_inputs(cfg)
    it, end = emulate(cfg, inp, mut)
    A = la.Audit("cpu")
    conds = ha.audit_route(A, cfg, inp, it, end, cfg.name)
    return A, conds


CFG = ha.configs()


@pytest.mark.parametrize("name", ["bench", "bench_mask", "bench_f16", "skip_round", "skip_all", "accumulate_mask"])
def test_unmutated_emulation_passes(name):
    A, conds = _audit(CFG[name])
    assert not A.failures, "\n".join(A.failures)
    ha.assert_conditions(CFG[name], conds)
    if name.startswith("bench"):
        assert sum(c[4] for c in conds) >= 1, "no decided anchor whose best candidate is a group of bit-identical rows"


@pytest.mark.parametrize("name,mut,op", [
    ("bench", "center_no_2", "center bwd dx"), ("bench_mask", "center_div_B", "center loss"), ("bench_mask", "bn_div_B", "bn save_mean"),
    ("bench_mask", "xent_div_B", "dlogits"), ("bench", "rv_biased", "running_var"), ("bench_mask", "loo_div_k1", "loo cent"),
    ("bench", "last_index", "p_idx [query]"), ("bench", "no_smoothing", "dlogits"), ("bench", "drop_k_slice", "dbnf = dlogits @ W"),
    ("bench", "no_hw", " g:"), ("bench_f16", "no_loss_scale", " g:"), ("bench", "g_trunc", " g: bias"),
    ("skip_round", "round_mean_k", "inv_rounds")])
def test_mutation_is_caught(name, mut, op):
    """each mutation fails the check of the op that carries it (on its own operands: the error is not left to travel)"""
    A, _ = _audit(CFG[name], (mut,))
    assert any(op in f for f in A.failures), (mut, A.failures)


@pytest.mark.parametrize("name", sorted(CFG))
def test_input_conditions_hold_for_every_configuration(name):
    cfg = CFG[name]
    rows = ha.input_conditions(cfg)
    ha.assert_conditions(cfg, rows)
    if cfg.masked:                                      # the mask patterns do what their names say
        inp = ha.make_inputs(cfg)
        lonely = ha.loo64(cfg, inp["feat"].double(), inp["labels"], inp["real"])[4][1]
        kept = [n for tag, n, *_ in rows[1:] if n]
        if name == "skip_round":
            assert len(kept) == cfg.K - 1
        if name == "skip_all":
            assert not kept and lonely == cfg.P
        if name == "bench_mask":
            assert lonely == 1 and len(kept) == cfg.K


def test_window_rules():
    """mine64 on a hand-made problem: a clear winner is decided, two candidates inside each other's bound are not, and a group of
    bit-identical rows counts as one candidate whose first index is the expected one"""
    x = torch.zeros(6, 4, dtype=torch.float64)
    x[1, 0], x[2, 0], x[3, 0], x[4, 0], x[5, 0] = 3.0, 3.0, 3.0 + 1e-9, 10.0, 10.0 + 1e-9
    lab = torch.tensor([0, 0, 0, 0, 1, 1])
    d = ha.pdist64(x)
    b = torch.full_like(d, 1e-6)
    m = ha.mine64(d, b, lab, torch.ones(6, dtype=torch.bool), ha.row_classes(x), 0.5)
    assert not bool(m["p_dec"][0]) and set(m["p_win"][0].nonzero()[:, 0].tolist()) == {1, 2, 3}      # 3 is a different row
    assert not bool(m["n_dec"][0]) and set(m["n_win"][0].nonzero()[:, 0].tolist()) == {4, 5}
    m = ha.mine64(d, torch.full_like(d, 1e-12), lab, torch.ones(6, dtype=torch.bool), ha.row_classes(x), 0.5)
    assert bool(m["p_dec"][0]) and int(m["p_idx"][0]) == 3 and bool(m["n_dec"][0]) and int(m["n_idx"][0]) == 4
    x[3, 0] = 2.0
    d = ha.pdist64(x)
    m = ha.mine64(d, b, lab, torch.ones(6, dtype=torch.bool), ha.row_classes(x), 0.5)
    assert bool(m["p_dec"][0]) and bool(m["p_tie"][0]) and int(m["p_idx"][0]) == 1                   # rows 1 and 2 are one candidate
