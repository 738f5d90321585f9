"""Exact checks of the convolution launches against an fp64 reference of the same convolution (shared by
tests/test_plan_sweep_gpu.py, tests/test_conv_edge_sweep_gpu.py and tests/test_conv_exact_cpu.py).

Operands are small integers ({-2..2}): every product is an integer and every partial sum is bounded by 4 K (forward, data
gradient; K <= 4608) or 4 M (weight gradient; M <= 3.3 M), both below 2^24.  The fp32 accumulators are therefore exact in any
summation order, split or k-grouping, the fp64 reference is exact however its GEMM runs, and the expected 16-bit output is the one
correctly rounded value of the exact result (|y| <= 18432 < the f16 maximum).  So outputs are compared bit for bit (as values:
+0 == -0), the weight gradient over the whole fp32 tensor; a missing, extra or misplaced product term changes a result by >= 1.

`run_geometry` runs one geometry (B, (cin, cout, k, stride, h, w)) through forward with statistics, folded-affine forward (plain,
residual + ReLU), data gradient (with and without add_src) and weight gradient (plain, accumulate=True).  Its plan keys default to
`plan_keys`, the expressions of bench_train.conv_plan_keys, so it also serves shapes that belong to no network."""
import json
import os
import zlib

import torch
import torch.nn.functional as F

PLANS = {(e["kind"], *e["key"]): tuple(e["plan"]) for e in
         json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "centroids-reid_amd",
                                     "tuned_plans.json")))["plans"]}
CHUNK_ELEMS = 1 << 26          # fp64 reference rows per chunk: <= 512 MB per tensor
# sums of squares of one 128-pixel tile: exact while every partial sum is < 2^24; above, each of the 128 fused multiply-adds and
# merges rounds once: |error| <= 128 * 2^-24 * sum (+ 2 ulp of slack for the merges of partial tiles) -- and so is their fp64 total
SUMSQ_REL = 130 * 2.0 ** -24


def out_hw(k, s, h, w):
    p = k // 2
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def plan_keys(B, cin, cout, k, s, h, w):
    """The launch-plan keys (kind, M, N, K, mode) of one convolution, as bench_train.conv_plan_keys derives them (mode =
    transposed | stride << 1, | 8 for the folded eval-mode epilogue)."""
    oh, ow = out_hw(k, s, h, w)
    m_out, kk = B * oh * ow, cin * k * k
    return {"fwd": (1, m_out, cout, kk, s << 1), "fwd_eval": (1, m_out, cout, kk, (s << 1) | 8),
            "dgrad": (1, B * h * w, cin, cout * k * k, 1 | (s << 1)), "wgrad": (0, m_out, cout, kk, s << 1)}


def c64_covers(oh, ow):
    """launch_conv3x3_c64 (conv_stream.hip): whole 128-pixel row blocks of a 32 / 64 wide image, or 16 x 8 blocks"""
    full_rows = ow in (32, 64) and (oh * ow) % 128 == 0
    return full_rows or (ow % 16 == 0 and oh % 8 == 0)


# ------------------------------------------------------------------------------------ fp64 reference (NHWC, tap by tap)
def _taps(k, s, oh, ow):
    for r in range(k):
        for c in range(k):
            yield r, c, (slice(r, r + s * (oh - 1) + 1, s), slice(c, c + s * (ow - 1) + 1, s))


def _chunk(B, per_image):
    """images per reference chunk: a multiple of 32 (every output map of a batch that needs more than one chunk has a multiple of
    4 pixels, so a chunk is whole 128-row statistics tiles), at most CHUNK_ELEMS elements per tensor"""
    return min(B, 32 * max(1, CHUNK_ELEMS // (32 * per_image)))


def ref_fwd(x, w, s, p, b0, b1):
    """y[b0:b1] of conv2d(x NHWC, w OIHW), fp64"""
    k, cout, cin = w.shape[2], w.shape[0], w.shape[1]
    xp = F.pad(x[b0:b1].double(), (0, 0, p, p, p, p))
    oh, ow = (xp.shape[1] - k) // s + 1, (xp.shape[2] - k) // s + 1
    y = torch.zeros((b1 - b0) * oh * ow, cout, dtype=torch.float64, device=x.device)
    wd = w.double()
    for r, c, (sr, sc) in _taps(k, s, oh, ow):
        y += xp[:, sr, sc, :].reshape(-1, cin) @ wd[:, :, r, c].t()
    return y.view(b1 - b0, oh, ow, cout)


def ref_dgrad(dy, w, s, p, H, W, b0, b1):
    """dx[b0:b1] of the same convolution: the transposed scatter of every tap, fp64"""
    k, cout, cin = w.shape[2], w.shape[0], w.shape[1]
    n, oh, ow = b1 - b0, dy.shape[1], dy.shape[2]
    dxp = torch.zeros(n, H + 2 * p, W + 2 * p, cin, dtype=torch.float64, device=dy.device)
    g = dy[b0:b1].double().reshape(-1, cout)
    wd = w.double()
    for r, c, (sr, sc) in _taps(k, s, oh, ow):
        dxp[:, sr, sc, :] += (g @ wd[:, :, r, c]).view(n, oh, ow, cin)
    return dxp[:, p:p + H, p:p + W, :]


def ref_wgrad(x, dy, k, s, p):
    """dw OIHW, fp64 (exact: integer sums far below 2^53)"""
    B, H, W, cin = x.shape
    oh, ow, cout = dy.shape[1], dy.shape[2], dy.shape[3]
    dw = torch.zeros(cout, cin, k, k, dtype=torch.float64, device=x.device)
    nb = _chunk(B, max(H * W * cin, oh * ow * cout))
    for b0 in range(0, B, nb):
        b1 = min(B, b0 + nb)
        xp = F.pad(x[b0:b1].double(), (0, 0, p, p, p, p))
        g = dy[b0:b1].double().reshape(-1, cout).t()
        for r, c, (sr, sc) in _taps(k, s, oh, ow):
            dw[:, :, r, c] += g @ xp[:, sr, sc, :].reshape(-1, cin)
    return dw


# ------------------------------------------------------------------------------------ the sweep
def _count(key, what):
    from centroids_reid_amd import _lib as L
    return int(L.lib().creid_tune_count(*key, what))


def _declines(key, plan, dtype, launch):
    """Launches that find a plan and are DOCUMENTED to run another kernel (conv_igemm.hip launch_igemm):
      * kernel 2 (the first persistent 1x1 kernel, conv_stream.hip) is bf16-only and has the plain epilogue only: f16 launches
        and folded eval-mode launches of its shapes take the built-in rule;
      * layer1's 3 x 3, 64 -> 64 forward runs conv3x3_c64_kernel ahead of every plan (statistics or plain affine epilogue, no
        residual): its plans only run with CREID_C64_3X3=0."""
    if key[0] == 1 and plan[2] == 2 and (dtype == torch.float16 or launch.startswith("aff")):
        return True
    if key[0] == 1 and key[2] == 64 and key[3] == 576 and (key[4] & 7) == 2 and launch in ("fwd", "aff_plain"):
        return True
    return False


def route_counters():
    """(halo-kernel launches, tap-fused weight-gradient launches) so far"""
    from centroids_reid_amd import _lib as L
    return int(L.lib().creid_igemm_halo_launches()), int(L.lib().creid_wgrad_taps_launches())


class Sweep:
    """dtype; plans_on: the shipped plans are registered and each launch checks the counters of its key.  strict (default): a
    plan found must also be applied, or be one of `_declines`; not strict: a decline is recorded in `declined` and is no failure
    (a foreign image under a production key: the kernels' own coverage checks decide).  expect_route: None, or
    f(launch name) -> (halo, taps), each True / False / None: whether the launch must (not) advance creid_igemm_halo_launches /
    creid_wgrad_taps_launches."""
    def __init__(self, dtype, plans_on, strict=True, expect_route=None):
        self.dtype, self.plans_on, self.strict, self.expect_route = dtype, plans_on, strict, expect_route
        self.applied, self.looked_up, self.declined, self.failures = set(), set(), set(), []
        self.launches, self.compared, self.routes_confirmed = 0, 0, 0

    def launch(self, key, name, fn, geom):
        """run fn(); with plans registered, check the counters of `key` (a registered plan must be found, and applied unless
        `_declines` says otherwise)"""
        self.launches += 1
        if self.expect_route is not None:
            want_route, c0 = self.expect_route(name), route_counters()
            out = self._launch(key, name, fn, geom)
            c1 = route_counters()
            for what, w_, a, b in (("halo kernel", want_route[0], c0[0], c1[0]), ("tap-fused weight gradient", want_route[1], c0[1], c1[1])):
                if w_ is not None and (b > a) != w_:
                    self.failures.append(f"{name} {geom}: {what} {'did not run' if w_ else 'ran'}, its coverage rule says otherwise")
                elif w_ is not None:
                    self.routes_confirmed += 1
            return out
        return self._launch(key, name, fn, geom)

    def _launch(self, key, name, fn, geom):
        plan = PLANS.get(key) if self.plans_on else None
        if plan is None:
            return fn()
        h0, d0 = _count(key, 0), _count(key, 1)
        out = fn()
        h1, d1 = _count(key, 0), _count(key, 1)
        want = _declines(key, plan, self.dtype, name)
        if h1 > h0:
            self.looked_up.add(key)
        if h1 <= h0:
            self.failures.append(f"{name} {geom}: plan {key} -> {plan} registered but not looked up")
        elif not self.strict:
            (self.declined if d1 != d0 else self.applied).add(key)
        elif want and d1 == d0:
            self.failures.append(f"{name} {geom}: plan {key} -> {plan} applied, expected the documented decline")
        elif not want and d1 != d0:
            self.failures.append(f"{name} {geom}: plan {key} -> {plan} found but declined")
        elif not want:
            self.applied.add(key)
        return out

    def compare(self, name, geom, key, got, exp, row0, state):
        """exact comparison of one chunk (rows of the [M, C] view starting at row0); the first mismatch and the count go in state"""
        self.compared += 1
        bad = got.double() != exp.double()
        n = int(bad.sum())
        if n:
            st = state.setdefault(name, [0, None, key])
            if st[1] is None:
                i = int(bad.reshape(-1).nonzero()[0])
                r, c = divmod(i, exp.shape[-1])
                st[1] = (row0 + r, c, float(got.reshape(-1)[i]), float(exp.reshape(-1)[i]))
            st[0] += n

    def report(self, geom, state):
        for name, (n, first, key) in state.items():
            plan = PLANS.get(key) if self.plans_on else None
            self.failures.append(f"{name} {geom} key {key} plan {plan if plan is not None else 'built-in rule'}: {n} mismatches, "
                                 f"first at (row, col) {first[:2]}: got {first[2]} expected {first[3]}")


def _rd(t, dtype):
    """round fp64 to the output dtype (RNE, like the kernels' f32 -> bf16 / f16 conversions), as fp64"""
    return t.float().to(dtype).double()


def _check_stats(sw, name, geom, key, pt, ref, row0, state):
    """pt [rows, 2, C] fp64 against the reference (sum, sum of squares, largest |y|) of the same rows: sums exact; sums of squares
    exact where every partial sum stays below 2^24 (128 squares of the largest |y|), within SUMSQ_REL elsewhere"""
    t1, t2, ymax = ref
    sw.compare(name + "_stats_sum", geom, key, pt[:, 0], t1, row0, state)
    exact = 128 * ymax * ymax < 2.0 ** 24
    sw.compare(name + "_stats_sumsq_exact", geom, key, torch.where(exact, pt[:, 1], t2), t2, row0, state)
    over = (pt[:, 1] - t2).abs() > SUMSQ_REL * t2
    sw.compare(name + "_stats_sumsq_bound", geom, key, torch.where(over, pt[:, 1], t2), t2, row0, state)


def run_geometry(sw, B, shape, keys=None, monkeypatch=None, rules_too=True):
    """One geometry: B images, shape = (cin, cout, k, stride, h, w); keys default to plan_keys(B, *shape).  With the plans
    registered (sw.plans_on) every launch runs a second time with the registry cleared (the built-in rules), unless rules_too is
    False."""
    from centroids_reid_amd import layers as ly
    cin, cout, k, s, h, w = shape
    if keys is None:
        keys = plan_keys(B, *shape)
    p, dt = k // 2, sw.dtype
    geom = f"B={B} {cin}->{cout} k{k} s{s} {h}x{w}"
    gen = torch.Generator(device="cuda").manual_seed(zlib.crc32(repr((B, shape)).encode()))

    def ints(shape_, lo=-2, hi=2):
        return torch.randint(lo, hi + 1, shape_, generator=gen, device="cuda", dtype=torch.int8)

    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    M = B * oh * ow
    x8, w8, dy8 = ints((B, h, w, cin)), ints((cout, cin, k, k)), ints((B, oh, ow, cout))
    res8, add8 = ints((B, oh, ow, cout)), ints((B, h, w, cin))
    dw0 = ints((cout, cin, k, k), -3, 3).float()
    ss = torch.stack([torch.randint(1, 5, (cout,), generator=gen, device="cuda") * 0.5,
                      torch.randint(-8, 9, (cout,), generator=gen, device="cuda") * 0.25]).float().contiguous()
    x, dy, res, add = x8.to(dt), dy8.to(dt), res8.to(dt), add8.to(dt)
    krsc, crsk = ly.weight_prep(w8.float(), dt)
    c64 = keys["fwd"][2] == 64 and keys["fwd"][3] == 576 and s == 1
    # the 3 x 3 c64 kernel's statistics rows are per 16 x 8 / row block of ONE image (compared per image below); where it declines
    # (launch_conv3x3_c64) the tile kernels write 128 consecutive pixels per row
    c64_rows = c64 and dt != torch.float32 and c64_covers(oh, ow)

    def launches():
        o = {}
        aff_key = keys["fwd_eval"] if sw.plans_on and keys["fwd_eval"] in PLANS else keys["fwd"]
        o["fwd"] = sw.launch(keys["fwd"], "fwd", lambda: ly.conv2d_fwd(x, krsc, s, p, with_stats=True), geom)
        o["aff_res_relu"] = sw.launch(aff_key, "aff_res_relu", lambda: ly.conv2d_fwd_affine(x, krsc, s, p, ss, res, True), geom)
        o["aff_plain"] = sw.launch(aff_key, "aff_plain", lambda: ly.conv2d_fwd_affine(x, krsc, s, p, ss, None, False), geom)
        if c64 and dt != torch.float32:               # the plans the c64 kernel pre-empts, pinned too
            monkeypatch.setenv("CREID_C64_3X3", "0")
            try:
                o["fwd_noc64"] = sw.launch(keys["fwd"], "fwd_noc64", lambda: ly.conv2d_fwd(x, krsc, s, p, with_stats=True), geom)
                o["aff_plain_noc64"] = sw.launch(aff_key, "aff_plain_noc64",
                                                 lambda: ly.conv2d_fwd_affine(x, krsc, s, p, ss, None, False), geom)
            finally:
                monkeypatch.delenv("CREID_C64_3X3")
        o["dgrad"] = sw.launch(keys["dgrad"], "dgrad", lambda: ly.conv2d_dgrad(dy, crsk, (h, w), s, p), geom)
        o["dgrad_add"] = sw.launch(keys["dgrad"], "dgrad_add", lambda: ly.conv2d_dgrad(dy, crsk, (h, w), s, p, add_src=add), geom)
        o["wgrad"] = sw.launch(keys["wgrad"], "wgrad", lambda: ly.conv2d_wgrad(x, dy, k, s, p), geom)
        o["wgrad_acc"] = sw.launch(keys["wgrad"], "wgrad_acc",
                                   lambda: ly.conv2d_wgrad(x, dy, k, s, p, out=dw0.clone(), accumulate=True), geom)
        return o

    outs = [("", launches())]
    if sw.plans_on and rules_too:
        # the built-in rules at the same M: what every batch size without plans runs
        from centroids_reid_amd import _lib as L
        sw.plans_on = False
        try:
            L.lib().creid_tune_clear()
            outs.append(("rules:", launches()))
        finally:
            L.lib().creid_tune_clear()
            L.load_tuned_plans()
            sw.plans_on = True
    torch.cuda.synchronize()

    state = {}
    is16 = dt != torch.float32
    rd = (lambda t: _rd(t, dt)) if is16 else (lambda t: t.float().double())
    sc, sh = ss[0].double(), ss[1].double()
    nb = _chunk(B, max(h * w * cin, oh * ow * cout))
    assert nb >= B or (nb * oh * ow) % 128 == 0, "a reference chunk must be whole statistics tiles"
    for b0 in range(0, B, nb):
        b1 = min(B, b0 + nb)
        r0, r1 = b0 * oh * ow, b1 * oh * ow
        y = ref_fwd(x8, w8, s, p, b0, b1).reshape(-1, cout)
        ey = rd(y)
        v = y * sc + sh                                            # exact: dyadic scale / shift, |v| < 2^22
        e_res = rd(torch.relu(rd(v) + res8[b0:b1].reshape(-1, cout).double()))   # the 16-bit kernels round before the residual add
        e_plain = rd(v)
        # statistics (a 128-pixel tile per partial row, each column sum an exact fp32 integer < 128 * 4 K): the tile kernels' rows
        # are 128 consecutive pixels and are compared row by row -- the last, partial tile padded with zeros: rows beyond M must
        # contribute nothing; the 3 x 3 c64 kernel tiles 16 x 8 image blocks, so its rows are compared per image -- the per-image
        # row blocks IBN reads (backbone._conv_bn, oh * ow % 128 == 0)
        ypad = F.pad(y, (0, 0, 0, (-y.shape[0]) % 128)).view(-1, 128, cout)
        tile = (ypad.sum(1), (ypad * ypad).sum(1), ypad.abs().amax(1))
        img = None
        if (oh * ow) % 128 == 0:
            yi = y.view(b1 - b0, oh * ow, cout)
            img = (yi.sum(1), (yi * yi).sum(1), yi.abs().amax(1))
        del ypad
        for tag, o in outs:
            for nm in ("fwd", "fwd_noc64"):
                if nm not in o:
                    continue
                pt = o[nm][1][r0 // 128:r0 // 128 + tile[0].shape[0]].double()
                if nm == "fwd" and c64_rows:
                    assert img is not None
                    pt, ref, row0 = pt.view(b1 - b0, -1, 2, cout).sum(1), img, b0
                else:
                    ref, row0 = tile, r0 // 128
                _check_stats(sw, tag + nm, geom, keys["fwd"], pt, ref, row0, state)
        for tag, o in outs:
            sw.compare(tag + "fwd", geom, keys["fwd"], o["fwd"][0].view(-1, cout)[r0:r1], ey, r0, state)
            if "fwd_noc64" in o:
                sw.compare(tag + "fwd_noc64", geom, keys["fwd"], o["fwd_noc64"][0].view(-1, cout)[r0:r1], ey, r0, state)
                sw.compare(tag + "aff_plain_noc64", geom, keys["fwd"], o["aff_plain_noc64"].view(-1, cout)[r0:r1], e_plain, r0, state)
            sw.compare(tag + "aff_res_relu", geom, keys["fwd_eval"], o["aff_res_relu"].view(-1, cout)[r0:r1], e_res, r0, state)
            sw.compare(tag + "aff_plain", geom, keys["fwd_eval"], o["aff_plain"].view(-1, cout)[r0:r1], e_plain, r0, state)
        del y, ey, v, e_res, e_plain
        # data gradient: image rows b0..b1 of dx
        ri0, ri1 = b0 * h * w, b1 * h * w
        dx = ref_dgrad(dy8, w8, s, p, h, w, b0, b1).reshape(-1, cin)
        edx, edx_add = rd(dx), rd(rd(dx) + add8[b0:b1].reshape(-1, cin).double())
        for tag, o in outs:
            sw.compare(tag + "dgrad", geom, keys["dgrad"], o["dgrad"].view(-1, cin)[ri0:ri1], edx, ri0, state)
            sw.compare(tag + "dgrad_add", geom, keys["dgrad"], o["dgrad_add"].view(-1, cin)[ri0:ri1], edx_add, ri0, state)
        del dx, edx, edx_add
    dw = ref_wgrad(x8, dy8, k, s, p)
    for tag, o in outs:
        sw.compare(tag + "wgrad", geom, keys["wgrad"], o["wgrad"].view(cout, -1), dw.view(cout, -1), 0, state)
        sw.compare(tag + "wgrad_acc", geom, keys["wgrad"], o["wgrad_acc"].view(cout, -1), (dw + dw0.double()).view(cout, -1), 0, state)
    sw.report(geom, state)
    del outs
    torch.cuda.empty_cache()


def assert_clean(sw, what):
    assert not sw.failures, f"{what}: {len(sw.failures)} failure(s):\n" + "\n".join(sw.failures[:40])
