"""Audit of the training step's heads against fp64: reference operations, first-order bounds of the kernels' fp32 evaluation and
the comparison of one route's stored tensors, shared by tests/test_heads_audit_gpu.py (the C entry points: separate launches and
creid_ctl_heads_fused) and tests/test_heads_audit_cpu.py (fp32 torch emulations of the kernels, with mutations the audit must
catch, and the two conditions on the synthetic inputs).

Everything here is plain torch in float64 on whatever device the operands live on; nothing calls the project's kernels.  The
comparison rule is tests/layer_audit.py's (Audit.check: element-wise bound, bias of 16-bit outputs, relative L2; Audit.exact).
As there, every op is judged on the operands the kernel READ (the stored fp32 tensors of the step), so an error does not
travel: `audit_route` walks the tensors one route left behind (dict `it`) and its end products (dict `end`).

u = 2^-24.  Summation bounds are read off csrc/heads.hip: a thread's fma / add chain of n terms and the 6 levels of a wave
sum (plus 3 adds over the 4 waves of a 256-thread workgroup) give (n + 9) u sum |terms| to first order.

Discrete decisions (mining, hinge).  With b_d the distance bound, an anchor's hardest positive / negative is DECIDED when the
fp64 best candidate beats every other candidate by more than the sum of their two b_d (candidates that are bit-identical rows
count as one: their fp32 distances are bit-equal, and the kernel must then return the FIRST index); the hinge is decided when
|ap - an + margin| > b_d(ap) + b_d(an).  On decided anchors the kernel's index / coefficient must equal the fp64 one, on the
others the index must lie inside the window and the coefficient be 0 or 1 / n.  Everything downstream takes the kernel's own
(p_idx, n_idx, coef) as operands.  mine64 takes any distance matrix with its bound: the euclidean kind here (pdist64, dist_bound),
the cosine kind of creid_triplet_cosine_fwd in tests/opt_ref.py (cos_dist64, cos_dist_bound, triplet_cos_bwd64 below).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

import layer_audit as la

U = la.U
F64 = torch.float64
G_DT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}       # CREID_F32 / CREID_BF16 / CREID_F16


@dataclass
class Cfg:
    name: str
    P: int
    K: int
    D: int = 2048
    C: int = 751
    HW: int = 128
    fakes: tuple | None = None          # indices of padded rows; None: all real, the unmasked schedule
    margin: float = 0.5                 # < 0: soft margin (separate launches only)
    eps: float = 0.1
    w_query: float = 1.0
    w_centroid: float = 1.0
    w_center: float = 5e-4
    w_xent: float = 1.0
    momentum: float = 0.1
    bn_eps: float = 1e-5
    g_dtype: int = 1
    scale: float | None = None          # f16 loss scale (amp_state[0])
    a_lo: float = 0.3                   # identity separation, spread linearly from hard (close) to easy (far)
    a_hi: float = 1.0
    seed: int = 0
    dup: bool = True                    # instances 1, 2 (and 3) of identity P // 2 bit-identical (K >= 3): the hardest positive of
    #                                     its instance 0 is a tie that must resolve to the first index
    prefill: bool = False               # d_centers / d_fc_weight / d_bn_* start non-zero

    @property
    def B(self):
        return self.P * self.K

    @property
    def masked(self):
        return self.fakes is not None


def make_inputs(cfg: Cfg):
    """Non-negative clustered features x[p, k] = clamp(0.4 + a_p (c_p - 0.5) + 0.35 n, 0) (pooled ReLU outputs), c_p uniform per
    identity, n normal per element, a_p from a_lo to a_hi over the identities; parameters of the heads; all fp32 on the host."""
    g = torch.Generator().manual_seed(1000 + cfg.seed)
    P, K, D, C = cfg.P, cfg.K, cfg.D, cfg.C
    a = torch.linspace(cfg.a_lo, cfg.a_hi, P)
    c = torch.rand(P, D, generator=g)
    n = torch.randn(P, K, D, generator=g)
    x = (0.4 + a[:, None, None] * (c[:, None, :] - 0.5) + 0.35 * n).clamp_min(0.0).float()
    if cfg.dup and K >= 3:
        x[P // 2, 2:4] = x[P // 2, 1]
    labels = ((torch.arange(P) * 3) % C).repeat_interleave(K)
    assert labels.unique().numel() == P
    real = torch.ones(P * K, dtype=torch.uint8)
    if cfg.fakes is not None:
        real[list(cfg.fakes)] = 0
    inp = {"feat": x.view(P * K, D).contiguous(), "labels": labels.long(), "real": real,
           "centers": torch.randn(C, D, generator=g) * 0.3, "W": torch.randn(C, D, generator=g) * 0.01,
           "bn_w": 1.0 + 0.1 * torch.randn(D, generator=g), "bn_b": 0.1 * torch.randn(D, generator=g),
           "rm0": 0.1 * torch.randn(D, generator=g), "rv0": 1.0 + 0.1 * torch.rand(D, generator=g)}
    shapes = {"d_centers0": (C, D), "d_fc0": (C, D), "d_bnw0": (D,), "d_bnb0": (D,)}
    for k, s in shapes.items():
        inp[k] = 0.01 * torch.randn(*s, generator=g) if cfg.prefill else torch.zeros(*s)
    return inp


def loss_weight_vector(cfg: Cfg):
    """CTLModel._loss_weight_vector: weights aligned with the scalar buffer [out4 (K + 1 rows), center, xent]; the masked schedule
    carries the whole centroid weight in the round slots (the device divides by the number of valid rounds)."""
    K = cfg.K
    w = torch.zeros(4 * (K + 1) + 2)
    w[0] = cfg.w_query
    w[4:4 * (K + 1):4] = cfg.w_centroid / (1 if cfg.masked else K)
    w[4 * (K + 1)] = cfg.w_center
    w[4 * (K + 1) + 1] = cfg.w_xent
    return w


# ------------------------------------------------------------------------------------------- distances, mining, hinge
def pdist64(x):
    """true pairwise distance sqrt(sum (x - y)^2) of the rows of fp64 x [N, D] (direct form, no cancellation)"""
    N = x.shape[0]
    out = torch.empty(N, N, dtype=F64, device=x.device)
    for i in range(0, N, 16):
        out[i:i + 16] = (x[i:i + 16, None, :] - x[None]).pow(2).sum(-1).sqrt()
    return out


def dist_bound(x, d):
    """triplet_mine_body: |x|^2, |y|^2 and x.y are each a per-lane fma chain of ceil(D / 64) terms + 6 wave-sum levels, then
    saa + sjj (one rounding) and fma(-2, dot, .) (one more): the expanded square is off by
        e <= (ceil(D / 64) + 8) u (|x|^2 + |y|^2 + 2 |x|.|y|),
    and sqrt(max(s + e', 1e-12)) differs from d = sqrt(s) by |e| / (d + sqrt(s - e)) <= min(e / d, sqrt(e)) (the cancellation in
    xx + yy - 2 x.y is what this term is for; it is ~e / 2d for d >> sqrt(e)), + 1e-6 for the clamp, + u d for sqrtf."""
    D = x.shape[1]
    n2, ax = (x * x).sum(1), x.abs()
    e = (math.ceil(D / 64) + 8) * U * (n2[:, None] + n2[None] + 2.0 * (ax @ ax.t()))
    den = d + torch.sqrt((d * d - e).clamp_min(0.0))
    b = torch.minimum(e / den.clamp_min(1e-300), torch.sqrt(e))
    return b + 1e-6 + U * (d + b)


def cos_dist64(x):
    """the cosine kind of triplet_mine_body on rows the caller has scaled to unit length: clamp(|1 - x.y|, 1e-12), fp64 x [N, D]"""
    return (1.0 - x @ x.t()).abs().clamp_min(1e-12)


def cos_dist_bound(x, d):
    """KIND 1 of triplet_mine_body: x.y is a per-lane chain of 4 ceil(D / 256) fma + 6 wave-sum levels, then 1 - dot rounds once
    (exactly, near 1); abs and the clamp are 1-Lipschitz.  The same window machinery (mine64) takes this bound as b."""
    D = x.shape[1]
    ax = x.abs()
    e = (4 * math.ceil(D / 256) + 6) * U * (ax @ ax.t())
    return e + U * (d + e)


def triplet_cos_bwd64(x, dap, dan, pi, ni, coef, g):
    """triplet_bwd_body<1> on its stored operands: every active anchor a contributes, for its positive (weight -coef) and its
    negative (+coef), w sign(1 - x_a.x_o) x_o to row a and w sign(.) x_a to row o -- nothing where the stored distance is the
    clamp value (<= 1e-12: no gradient).  The kernel recomputes x_r.x_o (chain of ceil(D / 256) fma, 6 wave levels, 3 adds): where
    |1 - x_r.x_o| is within that sum's error the sign it takes is undecided, and the term enters the bound with its whole
    magnitude, twice (the reference takes the fp64 sign).  Otherwise (nt + 3) u |g| sum |w| |x_o|: the products, the running
    sum, g * acc.  Returns (g dx, bound); the caller adds the accumulator's start and its rounding."""
    N, D = x.shape
    e_rel = (math.ceil(D / 256) + 9) * U
    dx, mag, loose = (torch.zeros(N, D, dtype=F64) for _ in range(3))
    nt = torch.zeros(N, dtype=F64)
    clampv = torch.tensor(1e-12, dtype=torch.float32)
    for a in range(N):
        c = float(coef[a])
        if c == 0.0:
            continue
        for o, dist, w in ((int(pi[a]), dap[a], -c), (int(ni[a]), dan[a], c)):
            if not bool(torch.as_tensor(dist, dtype=torch.float32) > clampv):
                continue
            v = 1.0 - float(x[a] @ x[o])
            und = abs(v) <= e_rel * float(x[a].abs() @ x[o].abs())
            s = (v > 0) - (v < 0)
            for r, q in ((a, o), (o, a)):
                dx[r] += w * s * x[q]
                nt[r] += 1
                (loose if und else mag)[r] += abs(c) * x[q].abs() * (2.0 if und else 1.0)
    return g * dx, abs(g) * ((nt[:, None] + 3) * U * mag + loose)


def row_classes(x):
    """rep[j] = first row bit-identical to row j"""
    N = x.shape[0]
    rep = torch.arange(N, device=x.device)
    for j in range(N):
        if int(rep[j]) == j:
            same = (x[j + 1:] == x[j]).all(1)
            rep[j + 1:][same & (rep[j + 1:] > j)] = j
    return rep


def mine64(d, b, labels, exists, rep, margin):
    """Batch-hard mining of one problem in fp64 with its decision windows.  d, b [N, N]; exists bool [N] (candidate rows).
    Returns dict: p_idx / n_idx (first index of the best), p_win / n_win (bool [N, N] windows), p_dec / n_dec / h_dec (decided),
    ap, an, v = ap - an + margin."""
    N = d.shape[0]
    same = labels[:, None] == labels[None]
    idx = torch.arange(N, device=d.device)
    out = {}
    for key, cand, sign in (("p", same & exists[None], 1.0), ("n", (~same) & exists[None], -1.0)):
        s = torch.where(cand, sign * d, torch.full_like(d, -math.inf))
        best = s.max(1).values
        full = lambda v: torch.full((N, N), v, dtype=torch.long, device=d.device)        # noqa: E731
        first = torch.where(s == best[:, None], idx[None].expand(N, N), full(N)).min(1).values
        first = first.clamp_max(N - 1)
        bb = b.gather(1, first[:, None])
        win = cand & (best[:, None] - s <= bb + b)
        rmax = torch.where(win, rep[None].expand(N, N), full(-1)).max(1).values
        rmin = torch.where(win, rep[None].expand(N, N), full(N)).min(1).values
        out[key + "_idx"], out[key + "_win"], out[key + "_dec"] = first, win, rmax == rmin
        out["a" + key], out["b" + key] = sign * best, bb[:, 0]
        out[key + "_tie"] = win.sum(1) > 1                     # a decided anchor whose window holds bit-identical rows
    out["v"] = out["ap"] - out["an"] + margin
    out["h_dec"] = out["v"].abs() > out["bp"] + out["bn"]
    return out


def triplet_problems(cfg: Cfg, feat64, labels, real, emb64=None, lab=None):
    """The triplet problems of one step as (tag, x [N, D], labels [N], exists [N] bool, on [N] bool (anchors in the loss),
    min_anchors): the query triplet (every row a candidate, padded anchors dropped after mining) and the K centroid rounds
    (rows of identities without a real query AND another real instance do not exist; < 4 anchors: the round is skipped)."""
    P, K = cfg.P, cfg.K
    r = real.bool()
    probs = [("query", feat64, labels, torch.ones_like(r), r if cfg.masked else torch.ones_like(r), 0)]
    if emb64 is None:
        _, emb64, lab, _, _ = loo64(cfg, feat64, labels, real)
    r2 = r.view(P, K)
    for i in range(K):
        ex = r2[:, i] & ((r2.sum(1) - r2[:, i].long()) > 0) if cfg.masked else torch.ones(P, dtype=torch.bool, device=r.device)
        ex2 = torch.cat([ex, ex])
        probs.append((f"round{i}", emb64[i], lab[i], ex2, ex2, 4 if cfg.masked else 0))
    return probs


def input_conditions(cfg: Cfg, inp=None):
    """The two conditions on a synthetic configuration, from the fp64 reference alone: per triplet problem (that is not skipped)
    the number of anchors, of undecided anchors (mining or hinge) and of anchors with an active hinge, and the number of decided
    anchors whose best candidate is a group of bit-identical rows."""
    inp = inp or make_inputs(cfg)
    f = inp["feat"].double()
    rows = []
    for tag, x, lab, ex, on, min_a in triplet_problems(cfg, f, inp["labels"], inp["real"]):
        n = int(on.sum())
        if n == 0 or n < min_a:
            rows.append((tag, 0, 0, 0, 0))
            continue
        d = pdist64(x)
        m = mine64(d, dist_bound(x, d), lab, ex, row_classes(x), cfg.margin)
        und = on & ~(m["p_dec"] & m["n_dec"] & (m["h_dec"] if cfg.margin >= 0 else True))
        ties = on & m["p_dec"] & m["n_dec"] & (m["p_tie"] | m["n_tie"])
        rows.append((tag, n, int(und.sum()), int((on & (m["v"] > 0)).sum()), int(ties.sum())))
    return rows


def assert_conditions(cfg: Cfg, rows):
    """<= 5 % undecided anchors per problem (two where 5 % is fewer than two); 20-80 % active hinges in problems of >= 16 anchors,
    at least one active (and, with more than two anchors, one inactive) in smaller ones.  No hinge with the soft margin."""
    for tag, n, und, act, _ in rows:
        if n == 0:
            continue
        assert und <= max(2, int(0.05 * n)), (cfg.name, tag, n, und)
        if cfg.margin < 0:
            continue
        if n >= 16:
            assert 0.2 * n <= act <= 0.8 * n, (cfg.name, tag, n, act)
        else:
            assert act >= 1 and (n <= 2 or act < n), (cfg.name, tag, n, act)


# ------------------------------------------------------------------------------------------- fp64 reference operations
def loo64(cfg: Cfg, feat64, labels, real):
    """Leave-one-out centroids and the rounds' operands: cent [K, P, D] (mean of the OTHER real instances of identity p if slot i
    is real, else 0), emb [K, 2P, D] (queries, then centroids), lab [K, 2P], valid [K, P] (the count), rows [K, 2P] (identity p
    takes part in round i: slot i real and another real instance), lonely = real instances without a real partner."""
    P, K, D = cfg.P, cfg.K, cfg.D
    f = feat64.view(P, K, D)
    r = real.view(P, K).to(F64)
    tot = (f * r[:, :, None]).sum(1, keepdim=True)
    cnt = (r.sum(1, keepdim=True) - r) * r                                # [P, K]
    cent = (tot - f * r[:, :, None]) * r[:, :, None] / cnt.clamp_min(1.0)[:, :, None]
    cent = cent.permute(1, 0, 2).contiguous()                             # [K, P, D]
    emb = torch.cat([f.permute(1, 0, 2), cent], 1)
    lab = labels.view(P, K).t().repeat(1, 2).contiguous()
    valid = cnt.t().contiguous()
    rows = (valid > 0).repeat(1, 2)
    lonely = int(((r > 0) & (cnt == 0)).sum())
    return cent, emb, lab, valid, (rows, lonely)


def triplet_bwd64(x, dap, dan, pi, ni, coef, g):
    """triplet_bwd_body on its stored operands: dx[r] = g sum_terms w (x_r - x_other), w = +-coef / dist (0 where dist <= 1e-6).
    The kernel rounds w (1), the difference (1), the product (1), the running sum (<= nt), g (1) and g * acc (1):
    (nt + 5) u |g| sum |w| |x_r - x_other|, nt = the number of terms of row r."""
    N, D = x.shape
    act = (coef != 0).nonzero()[:, 0]
    dx, mag = torch.zeros(N, D, dtype=F64, device=x.device), torch.zeros(N, D, dtype=F64, device=x.device)
    nt = torch.zeros(N, dtype=F64, device=x.device)
    if act.numel():
        c = coef[act].double()
        p, n = pi[act].long(), ni[act].long()
        wp = torch.where(dap[act] > 1e-6, c / dap[act].double(), torch.zeros_like(c))[:, None]
        wn = torch.where(dan[act] > 1e-6, c / dan[act].double(), torch.zeros_like(c))[:, None]
        tp, tn = wp * (x[act] - x[p]), wn * (x[act] - x[n])
        for t, sgn, other in ((tp, 1.0, p), (tn, -1.0, n)):
            dx.index_add_(0, act, sgn * t)
            dx.index_add_(0, other, -sgn * t)
            mag.index_add_(0, act, t.abs())
            mag.index_add_(0, other, t.abs())
            nt.index_add_(0, act, torch.ones_like(c))
            nt.index_add_(0, other, torch.ones_like(c))
    return g * dx, (nt[:, None] + 5) * U * abs(g) * mag


def bn_fwd64(x, on):
    """BatchNorm1d statistics over the rows `on`: mean, sum of squared deviations, row count"""
    nb = float(on.sum())
    m = on.to(F64)[:, None]
    mean = (x * m).sum(0) / nb
    t = (x - mean) * m
    m2 = (t * t).sum(0)
    return mean, m2, nb


def xent64(z, y, on, eps, gscale):
    """label-smoothed cross entropy over the rows `on`: row losses, dlogits = (softmax - t) gscale / n, log-softmax"""
    Cc = z.shape[1]
    logp = torch.log_softmax(z, 1)
    t = torch.full_like(z, eps / Cc)
    t[torch.arange(z.shape[0], device=z.device), y] += 1.0 - eps
    m = on.to(F64)[:, None]
    row = -(t * logp).sum(1) * m[:, 0]
    return row, (logp.exp() - t) * (gscale / float(on.sum())) * m, logp, t


def audit_center(A, layer, x, labels, centers, row_c, loss, dx, dcen, dcen0, on_rows, w_center, max_members):
    """Center loss on fp64 x [B, D]: the row terms, the loss on the STORED rows (clamp state and the B (C - 1) 1e-12 term
    included) and both gradients.  row: three ceil(D / 256)-term fma chains + 9, xx + cc and the fma:
    (ceil(D / 256) + 11) u (xx + cc + 2 |x|.|c|).  Gradients: g = w 2 / n (3 roundings), x - c (1), the product (1): 6 u;
    d_centers: the <= max_members members of a class summed in batch order, then ONE += into the accumulator.  Returns dx."""
    B, D = x.shape
    f32 = torch.float32
    nb = float(on_rows.sum())
    msk = on_rows.to(F64)
    cy = centers[labels]
    row_ref = (x - cy).pow(2).sum(1)
    rmag = (x * x).sum(1) + (cy * cy).sum(1) + 2 * (x.abs() * cy.abs()).sum(1)
    b = (math.ceil(D / 256) + 11) * U * rmag
    A.check(layer, "center row_sq", row_c, row_ref, b, f32, sigma=b)
    rc = row_c.double()
    clamp_on = (rc >= 1e-12) & (rc <= 1e12)
    lc_ref = ((rc.clamp(1e-12, 1e12) * msk).sum() + nb * (centers.shape[0] - 1) * 1e-12) / nb
    b = (math.ceil(B / 256) + 12) * U * lc_ref.abs()
    A.check(layer, "center loss", loss, lc_ref, b, f32, sigma=b)
    gc = w_center * 2.0 / nb
    live = (clamp_on & on_rows).to(F64)[:, None]
    dxc = gc * (x - cy) * live
    if dx is not None:
        A.check(layer, "center bwd dx", dx, dxc, 7 * U * dxc.abs(), f32, sigma=7 * U * dxc.abs())
    dc = torch.zeros_like(centers).index_add_(0, labels, gc * (cy - x) * live)
    dcm = torch.zeros_like(centers).index_add_(0, labels, abs(gc) * (cy - x).abs() * live)
    dc_ref = dcen0 + dc
    b = (max_members + 6) * U * dcm + U * dc_ref.abs()
    A.check(layer, "d_centers", dcen, dc_ref, b, f32, sigma=b)
    return dxc


# ------------------------------------------------------------------------------------------- one route against fp64
def audit_route(A: la.Audit, cfg: Cfg, inp, it, end, layer):
    """Audit the tensors one route left behind.  inp: the step's inputs (make_inputs layout, on the tensors' device); it: the
    stored intermediates (fp32 / int tensors; optional keys are checked when present); end: the end products.  Returns the list
    of (problem, anchors, undecided, active) rows.  Bounds are derived next to each check."""
    P, K, D, C, B, HW = cfg.P, cfg.K, cfg.D, cfg.C, cfg.B, cfg.HW
    dev = inp["feat"].device
    f32 = torch.float32
    x = inp["feat"].double()
    labels, real = inp["labels"], inp["real"]
    on_rows = real.bool() if cfg.masked else torch.ones(B, dtype=torch.bool, device=dev)
    nb = float(on_rows.sum())
    msk = on_rows.to(F64)[:, None]
    scal = it["scal"].double()

    def chk(op, got, ref, b, sigma=None):
        # sigma (the statistical accumulation error of the relative-L2 bar): sqrt(n) u mag where given (the GEMMs, the distances),
        # otherwise the worst-case bound itself -- the bar is then implied by the element-wise check and never tighter than it
        A.check(layer, op, got, ref, b, f32, sigma=b if sigma is None else sigma)

    conds = []

    # ---- leave-one-out centroids and the rounds' operands.  cent: <= K - 1 sequential adds and one division: (K + 1) u sum|f| / cnt
    cent, emb64, lab64, valid, (rows, lonely) = loo64(cfg, x, labels, real)
    f3 = x.view(P, K, D).abs() * real.view(P, K, 1).to(F64)
    cmag = ((f3.sum(1, keepdim=True) - f3) / valid.t().clamp_min(1.0)[:, :, None]).permute(1, 0, 2) * (valid > 0)[:, :, None]
    chk("loo cent", it["cent"], cent, (K + 1) * U * cmag)
    A.exact(layer, "loo emb queries", torch.equal(it["emb"][:, :P], inp["feat"].view(P, K, D).permute(1, 0, 2)))
    A.exact(layer, "loo emb centroids", torch.equal(it["emb"][:, P:], it["cent"]))
    A.exact(layer, "loo lab", torch.equal(it["lab"], lab64))
    A.exact(layer, "loo valid", torch.equal(it["valid"].long(), valid.long()))
    if cfg.masked:
        A.exact(layer, "loo row_exists", torch.equal(it["rows"].bool(), rows))
        A.exact(layer, "lonely count", int(end["lonely"]) == int(inp.get("lonely0", 0)) + lonely, f"{int(end['lonely'])} vs +{lonely}")
    # cnorm = sqrt(sum c^2) of the STORED centroid: ceil(D / 256) fma chain + 9, half of it through the root, + sqrtf
    cn = it["cent"].double().pow(2).sum(-1).sqrt()
    chk("cnorm", it["cnorm"].view(K, P), cn, ((math.ceil(D / 256) + 9) / 2 + 1) * U * cn)

    # ---- the triplet problems: query, then the K rounds (on the STORED embedding rows)
    emb_st = it["emb"].double()
    probs = triplet_problems(cfg, x, labels, real, emb_st, it["lab"])
    q = {k: it[k + "_q"] for k in ("dap", "dan", "pi", "ni", "coef")}
    rnd = {k: it[k + "_r"].view(K, 2 * P) for k in ("dap", "dan", "pi", "ni", "coef")}
    gq = cfg.w_query
    g_round = cfg.w_centroid * (float(it["inv_rounds"]) if cfg.masked else 1.0 / K)
    dx_parts = {}
    demb_ref, demb_b = [], []
    n_valid = 0
    for k, (tag, xs, lab, ex, on, min_a) in enumerate(probs):
        kk = q if k == 0 else {n: v[k - 1] for n, v in rnd.items()}
        o4 = scal[4 * k:4 * k + 4]
        n = int(on.sum())
        N = xs.shape[0]
        if n == 0 or n < min_a:                                    # a skipped round: zero loss, zero coefficients
            A.exact(layer, f"skipped [{tag}]", bool((kk["coef"] == 0).all()) and bool((o4 == 0).all()))
            conds.append((tag, 0, 0, 0, 0))
            dxk, bk = torch.zeros_like(xs), torch.zeros_like(xs)
        else:
            n_valid += k > 0
            d = pdist64(xs)
            bd = dist_bound(xs, d)
            m = mine64(d, bd, lab, ex, row_classes(xs), cfg.margin)
            if k == 0 and "dist_q" in it:
                chk("pairwise distance", it["dist_q"], d, bd, sigma=bd / math.sqrt(math.ceil(D / 64) + 8) + U * d)
            sel = on.nonzero()[:, 0]
            bad = []
            for key in ("p", "n"):
                got = kk[key[0] + "i"].long()[sel]
                inside = (got >= 0) & (got < N)
                gi = got.clamp(0, N - 1)
                ok = inside & torch.where(m[key + "_dec"][sel], gi == m[key + "_idx"][sel], m[key + "_win"][sel].gather(1, gi[:, None])[:, 0])
                bad.append(int((~ok).sum()))
                A.exact(layer, f"{key}_idx [{tag}]", bad[-1] == 0, f"{bad[-1]} anchors")
                if bad[-1] == 0:                                   # the mined distance at the kernel's own index
                    chk(f"dist_a{key} [{tag}]", kk["da" + key][sel], d[sel].gather(1, gi[:, None])[:, 0], bd[sel].gather(1, gi[:, None])[:, 0])
            tie = on & m["p_dec"] & m["n_dec"] & (m["p_tie"] | m["n_tie"])
            und = on & ~(m["p_dec"] & m["n_dec"] & (m["h_dec"] if cfg.margin >= 0 else True))
            conds.append((tag, n, int(und.sum()), int((on & (m["v"] > 0)).sum()), int(tie.sum())))
            # coefficient and loss on the STORED distances
            zero = torch.zeros((), dtype=F64, device=dev)               # (anchors outside the loss may hold +-inf: no candidate)
            ap, an = torch.where(on, kk["dap"].double(), zero), torch.where(on, kk["dan"].double(), zero)
            coef = kk["coef"]
            one = (torch.ones((), dtype=f32, device=dev) / torch.tensor(float(n), dtype=f32, device=dev))
            A.exact(layer, f"coef off-anchors [{tag}]", bool((coef[~on] == 0).all()))
            if cfg.margin >= 0:
                dec = on & m["p_dec"] & m["n_dec"] & m["h_dec"]
                want = torch.where(m["v"] > 0, one, torch.zeros_like(one)).to(f32)
                nbad = int((coef[dec] != want[dec]).sum()) + int(((coef[on] != 0) & (coef[on] != one)).sum())
                A.exact(layer, f"coef (hinge) [{tag}]", nbad == 0, f"{nbad} anchors")
                act = (coef != 0) & on
                v = (ap - an + cfg.margin) * act.to(F64)
                lmag = ((ap.abs() + an.abs() + cfg.margin) * act.to(F64)).sum()
            else:                                                  # soft margin: z = ap - an (1), expf (2), 1 + (1), two divisions
                z = ap - an
                cref = torch.sigmoid(z) / n * on.to(F64)
                chk(f"coef (soft) [{tag}]", coef, cref, (8 + z.abs()) * U * cref)
                v = torch.nn.functional.softplus(z) * on.to(F64)
                lmag = ((ap.abs() + an.abs() + 4 * v.abs()) * on.to(F64)).sum()
            # a thread's ceil(N / 256) terms, wave sum, 3 adds, one division; 2 roundings inside each term
            cs = (math.ceil(N / 256) + 12) * U
            o4ref = torch.stack([v.sum() / n, (ap * on.to(F64)).sum() / n, (an * on.to(F64)).sum() / n, torch.tensor(float(n), dtype=F64, device=dev)])
            o4b = torch.stack([cs * lmag / n, cs * (ap.abs() * on.to(F64)).sum() / n, cs * (an.abs() * on.to(F64)).sum() / n,
                               torch.zeros((), dtype=F64, device=dev)])
            chk(f"out4 [{tag}]", o4, o4ref, o4b)
            dxk, bk = triplet_bwd64(xs, kk["dap"], kk["dan"], kk["pi"], kk["ni"], coef, gq if k == 0 else g_round)
        if k == 0:
            dx_parts["triplet"] = (dxk, bk)
            if "dx_triplet" in it:
                chk("query triplet bwd", it["dx_triplet"], dxk, bk + U * dxk.abs())
        else:
            demb_ref.append(dxk)
            demb_b.append(bk)
    demb_ref, demb_b = torch.stack(demb_ref), torch.stack(demb_b)
    chk("rounds triplet bwd (demb)", it["demb"], demb_ref, demb_b + U * demb_ref.abs())
    if cfg.masked:
        chk("inv_rounds", it["inv_rounds"], torch.tensor([1.0 / n_valid if n_valid else 0.0], dtype=F64, device=dev), U)

    # ---- center loss
    lc_w = scal[4 * (K + 1)]
    dxc = audit_center(A, layer, x, labels, inp["centers"].double(), it["row_c"], lc_w, it.get("dx_center"), end["d_centers"],
                       inp["d_centers0"].double(), on_rows, cfg.w_center, K)
    dx_parts["center"] = (dxc, 6 * U * dxc.abs())

    # ---- BNNeck forward.  mean: 8 row lanes of ceil(B / 8) adds, 8 partials, one division: (ceil(B / 8) + 9) u sum|x| / n.
    # m2 = sum (x - mean_k)^2 around the kernel's own fp32 mean (off by dmean: + n dmean^2, second order), each term 3 roundings:
    # (ceil(B / 8) + 12) u m2.  invstd = 1 / sqrt(m2 / n + eps): half the relative error of the variance + 3 roundings.
    mean, m2, _ = bn_fwd64(x, on_rows)
    ch = math.ceil(B / 8)
    dmean = (ch + 9) * U * (x.abs() * msk).sum(0) / nb
    dm2 = (ch + 12) * U * m2 + nb * dmean * dmean
    var = m2 / nb
    inv = 1.0 / torch.sqrt(var + cfg.bn_eps)
    dinv = inv * (0.5 * (dm2 / nb) / (var + cfg.bn_eps) * 1.01 + 4 * U)
    chk("bn save_mean", it["sm"], mean, dmean)
    chk("bn save_invstd", it["si"], inv, dinv)
    mo = cfg.momentum
    rm_ref = (1 - mo) * inp["rm0"].double() + mo * mean
    chk("running_mean", end["rm"], rm_ref, mo * dmean + 3 * U * ((1 - mo) * inp["rm0"].double().abs() + mo * mean.abs()))
    unb = m2 / (nb - 1) if nb > 1 else var
    rv_ref = (1 - mo) * inp["rv0"].double() + mo * unb
    chk("running_var (unbiased)", end["rv"], rv_ref, mo * (dm2 / max(nb - 1, 1) + 2 * U * unb) + 3 * U * rv_ref.abs())
    A.exact(layer, "bn_batches_tracked", int(end["nbt"]) == int(inp.get("nbt0", 0)) + 1)
    # y = (x - mean) invstd w + b on the STORED statistics: three products / one add, 4 u |product| + u |y|; padded rows exactly 0
    sm, si, w = it["sm"].double(), it["si"].double(), inp["bn_w"].double()
    xh = (x - sm) * si
    y_ref = (xh * w + inp["bn_b"].double()) * msk
    chk("bnf", it["bnf"], y_ref, (4 * U * (xh * w).abs() + U * y_ref.abs()) * msk)
    if cfg.masked:
        A.exact(layer, "bnf padded rows zero", bool((it["bnf"][~on_rows] == 0).all()))

    # ---- classifier GEMMs on their stored operands: K u sum|a||b| (+ the atomics of a split: one rounding per slice)
    bnf, Wd = it["bnf"].double(), inp["W"].double()
    s_l, s_d = end.get("splits", (1, 1))
    mg = bnf.abs() @ Wd.abs().t()
    chk("logits", it["logits"], bnf @ Wd.t(), (D + s_l + 1) * U * mg, sigma=math.sqrt(D) * U * mg)

    # ---- cross entropy on the STORED logits.  se: ceil(C / 256) adds + 9; p = expf(z - mx) / se: expf 2 u, its argument's rounding
    # u |z - mx| (relative, through exp), the division: (ceil(C / 256) + 14 + |z - mx|) u p; (p - t) gb: 3 more roundings.
    z = it["logits"].double()
    row_x, dl_ref, logp, t = xent64(z, labels, on_rows, cfg.eps, cfg.w_xent)
    zc = z - z.max(1, keepdim=True).values
    cc = math.ceil(C / 256)
    gb = cfg.w_xent / nb
    p = logp.exp()
    chk("dlogits", it["dlogits"], dl_ref, (abs(gb) * ((cc + 14 + zc.abs()) * U * p + 3 * U * (p + t))) * msk)
    lse = torch.logsumexp(zc, 1)
    dlse = (cc + 12) * U + 2 * U * lse.abs()
    zy = zc.gather(1, labels[:, None])[:, 0]
    b_row = (1 - cfg.eps) * (U * zy.abs() + dlse + 2 * U * (zy - lse).abs()) \
        + cfg.eps / C * ((cc + 10) * U * zc.abs().sum(1) + C * (dlse + 2 * U * lse.abs()) + U * logp.sum(1).abs()) + 3 * U * row_x.abs()
    chk("xent row loss", it["row_x"], row_x, b_row * msk[:, 0])
    lx_ref = it["row_x"].double().sum() / nb
    chk("xent loss", scal[4 * (K + 1) + 1], lx_ref, (math.ceil(B / 256) + 11) * U * it["row_x"].double().abs().sum() / nb)
    if cfg.masked:
        A.exact(layer, "dlogits padded rows zero", bool((it["dlogits"][~on_rows] == 0).all()))
    dl = it["dlogits"].double()
    md = dl.abs() @ Wd.abs()
    chk("dbnf = dlogits @ W", it["dbnf"], dl @ Wd, (C + s_d + 1) * U * md, sigma=math.sqrt(C) * U * md)
    dW = dl.t() @ bnf
    mw = dl.abs().t() @ bnf.abs()
    dW_ref = inp["d_fc0"].double() + dW
    chk("d_fc_weight", end["d_fc_weight"], dW_ref, (B + 2) * U * mw + U * dW_ref.abs(), sigma=math.sqrt(B) * U * mw)

    # ---- BNNeck backward on the stored dbnf / statistics.  sdy: (ceil(B / 8) + 9) u sum|dy|; sdyx: xhat costs 2 roundings and
    # the fma one: (ceil(B / 8) + 12) u sum|dy xhat|.  dx = k (n dy - sdy - xhat sdyx), k = w invstd / n (3 roundings): every term
    # of the bracket is rounded at its own magnitude (the cancellation between them is what the absolute terms are for).
    dy = it["dbnf"].double() * msk
    xhm = xh * msk
    s1, s2 = dy.sum(0), (dy * xhm).sum(0)
    ds1 = (ch + 9) * U * dy.abs().sum(0)
    ds2 = (ch + 12) * U * (dy * xhm).abs().sum(0)
    kf = (w * si / nb)
    dxb = kf * (nb * dy - s1 - xh * s2) * msk
    bxb = (kf.abs() * (5 * U * (nb * dy.abs() + s1.abs() + (xh * s2).abs()) + ds1 + xh.abs() * ds2) + 4 * U * dxb.abs()) * msk
    dx_parts["bn"] = (dxb, bxb)
    if "dx_bn" in it:
        chk("bn bwd dx", it["dx_bn"], dxb, bxb + U * dxb.abs())
    dbw_ref, dbb_ref = inp["d_bnw0"].double() + s2, inp["d_bnb0"].double() + s1
    chk("d_bn_weight", end["d_bn_weight"], dbw_ref, ds2 + U * dbw_ref.abs())
    chk("d_bn_bias", end["d_bn_bias"], dbb_ref, ds1 + U * dbb_ref.abs())

    # ---- the sum so far (query triplet, center, BNNeck accumulated in that order), then the leave-one-out adjoint on the STORED demb:
    # dfeat[p, s] = acc + demb[s][p] + sum_{i != s, both real} demb[i][P + p] / cnt_i: <= K + 1 adds and a division per term
    pre = sum(v[0] for v in dx_parts.values())
    pre_b = sum(v[1] for v in dx_parts.values()) + 3 * U * sum(v[0].abs() for v in dx_parts.values())
    if "dfeat_pre" in it:
        chk("dfeat before the adjoint", it["dfeat_pre"], pre, pre_b)
    de = it["demb"].double()
    r2 = real.view(P, K).to(F64)
    dq = de[:, :P].permute(1, 0, 2)                                          # [P, K(s), D]
    dc = de[:, P:].permute(1, 0, 2) * (r2 / valid.t().clamp_min(1.0))[:, :, None]     # round i's share per member, real i only
    adj = dq + (dc.sum(1, keepdim=True) - dc) * r2[:, :, None]
    adjm = dq.abs() + (dc.abs().sum(1, keepdim=True) - dc.abs()) * r2[:, :, None]
    df_ref = pre + adj.reshape(B, D)
    df_b = pre_b + (K + 3) * U * (adjm.reshape(B, D) + pre.abs())
    chk("dfeat", end["dfeat"], df_ref, df_b)

    # ---- g = dfeat / HW on the STORED dfeat, times the f16 loss scale, rounded ONCE to g_dtype: the scale (1), 1 / HW (1), the product (1)
    if end["g"] is not None:                                   # (None: a width the pooling backward does not take, D % 8 != 0)
        gdt = G_DT[cfg.g_dtype]
        g3 = end["g"].view(B, HW, D)
        A.exact(layer, "g broadcast over the map", bool((g3 == g3[:, :1]).all()))
        g_ref = end["dfeat"].double() * (cfg.scale or 1.0) / HW
        A.check(layer, "g", g3[:, 0], g_ref, 3 * U * g_ref.abs(), gdt)
        A.check(layer, "g (last position)", g3[:, HW - 1], g_ref, 3 * U * g_ref.abs(), gdt)

    # ---- the logged scalars on the stored scalar buffer
    wv = loss_weight_vector(cfg).to(dev).double()
    n = 4 * (K + 1) + 2
    is_round = torch.zeros(n, dtype=torch.bool, device=dev)
    is_round[4:4 * (K + 1):4] = True
    o4r = scal[4:4 * (K + 1)].view(K, 4)
    if cfg.masked:
        vr = o4r[:, 3] >= 4
        nv = int(vr.sum())
        inv_r = 1.0 / nv if nv else 0.0
        terms = scal * wv * torch.where(is_round, torch.full_like(scal, inv_r), torch.ones_like(scal))
        rmean = (o4r * vr[:, None].to(F64)).sum(0) * inv_r
        ex = it["rows"].view(K, 2 * P)[:, P:].to(F64)
        l2 = sum((it["cnorm"].double().view(K, P)[k] * ex[k]).sum() / ex[k].sum() for k in range(K) if bool(vr[k])) * inv_r if nv else scal.new_zeros(())
        A.exact(layer, "valid rounds", nv == n_valid, f"{nv} vs {n_valid}")
    else:
        terms = scal * wv
        rmean = o4r.mean(0)
        l2 = it["cnorm"].double().mean()
    ref = torch.cat([terms, terms.sum()[None], terms[is_round].sum()[None], rmean, l2.reshape(1)])
    sa = terms.abs().sum()
    bnd = torch.cat([3 * U * terms.abs(), ((n + 3) * U * sa)[None], ((K + 3) * U * sa)[None], (K + 3) * U * o4r.abs().sum(0),
                     ((K * P / 64 + P + K + 10) * U * l2.abs()).reshape(1)])
    chk("stats", end["stats"], ref, bnd)
    return conds


def check_conditions_note(A: la.Audit, layer, conds):
    for tag, n, und, act, ties in conds:
        A.note(layer, f"decisions [{tag}]", f"anchors {n} undecided {und} active {act} first-index ties {ties}")


# ------------------------------------------------------------------------------------------- the audited configurations
MASK1 = (5, 10, 11, 19, 25, 26, 27, 36, 37, 38, 39)     # P 16 x K 4: one fake; two in one identity; a fake last slot; identity 6
#                                                          left with one real instance (lonely); identity 9 with none
SKIP1 = tuple(4 * p + 3 for p in range(15))             # slot 3 real in identity 15 only: round 3 is skipped, rounds 0-2 survive
SKIPALL = tuple(i for i in range(64) if i % 4 != (i // 4) % 4)     # one real instance per identity: every round is skipped
NONDEFAULT = dict(w_query=0.7, w_centroid=1.3, w_center=5e-4, w_xent=0.5)


def configs():
    """name -> Cfg.  The separation range (a_lo, a_hi) is tuned per (D, P, K) on the host so that the two input conditions hold
    (tests/test_heads_audit_cpu.py asserts them for every entry with the fp64 reference alone)."""
    c = [Cfg("bench", 16, 4), Cfg("bench_mask", 16, 4, fakes=MASK1),
         Cfg("s2s", 14, 4, C=1000, HW=400), Cfg("s2s_mask", 14, 4, C=1000, HW=400, fakes=(2, 21, 22, 55)),
         Cfg("bench_f32", 16, 4, g_dtype=0), Cfg("bench_f16", 16, 4, g_dtype=2, scale=1024.0),
         Cfg("bench_mask_f16", 16, 4, g_dtype=2, scale=1024.0, fakes=MASK1),
         Cfg("p2k2", 2, 2, g_dtype=0, HW=8, a_lo=0.0, a_hi=0.2), Cfg("k16", 16, 16, g_dtype=0, HW=8), Cfg("b256", 64, 4, g_dtype=0, HW=8),
         Cfg("d264", 16, 4, D=264, g_dtype=0, HW=8, a_lo=0.2, a_hi=1.6),
         Cfg("b320", 80, 4, g_dtype=0, HW=8), Cfg("d260", 16, 4, D=260, g_dtype=0, HW=8, a_lo=0.2, a_hi=1.6),
         Cfg("soft", 16, 4, margin=-1.0, g_dtype=0, HW=8),
         Cfg("skip_round", 16, 4, fakes=SKIP1), Cfg("skip_all", 16, 4, fakes=SKIPALL),
         Cfg("accumulate", 16, 4, prefill=True, **NONDEFAULT), Cfg("accumulate_mask", 16, 4, prefill=True, fakes=MASK1, **NONDEFAULT)]
    return {x.name: x for x in c}
