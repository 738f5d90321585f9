"""tests/opt_ref.py checked on the CPU, without the library:

  1. the references against independent evaluations: the float64 Adam against torch.optim.Adam in float64 over several steps, the
     amp_update model against torch's GradScaler rule (torch._amp_update_scale_) wherever the clamp is inactive, the closed form
     of the row normalisation's backward and the cosine triplet's gradient against autograd in float64, mining against a loop;
  2. the fp32 models of the kernels pass every bound at every generator case and size class (grids capped at one or two
     workgroups reach the second grid-stride trip and the scalar tail at a thousand elements);
  3. the bounds have teeth: each mutant of the fp32 model (opt_ref.MUTANTS_*) fails at least one of them at a small size.  The
     output names every mutant and the check that caught it (-s shows it).

The host's powf stands in for the device's in the model; how far each is from float64: profiles/opt_edges.md."""
import numpy as np
import pytest
import torch

import heads_audit as ha
import opt_ref as orf

f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ 1. the references
def test_adam64_matches_torch_adam_in_float64():
    hp = orf.hyper_params(lr=1e-3, wd=5e-4)
    rng = np.random.default_rng(0)
    n = 257
    p0 = rng.standard_normal(n).astype(f32)
    grads = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 0)).astype(f32) for _ in range(6)]
    pt = torch.nn.Parameter(torch.from_numpy(p0.astype(f64)))
    opt = torch.optim.Adam([pt], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"])
    p, m, v = p0.astype(f64), np.zeros(n), np.zeros(n)
    for t, g in enumerate(grads, 1):
        pt.grad = torch.from_numpy(g.astype(f64))
        opt.step()
        bc1, bc2s = orf.bias_corr64(hp["b1"], hp["b2"], t)
        # (adam64 takes fp32 operands: feed the float64 trajectory through its formula by hand)
        gg = hp["wd"] * p + g.astype(f64) * hp["gscale"]
        m = hp["b1"] * m + (1 - hp["b1"]) * gg
        v = hp["b2"] * v + (1 - hp["b2"]) * gg * gg
        p = p - hp["lr"] / bc1 * m / (np.sqrt(v) / bc2s + hp["eps"])
        np.testing.assert_allclose(p, pt.detach().numpy(), rtol=1e-13, atol=1e-15)
    # and adam64 itself IS that formula on fp32 operands (one step, against the lines above)
    a = orf.adam_inputs(64, 3)
    r = orf.adam64(*a, hp, *orf.bias_corr64(hp["b1"], hp["b2"], 3))
    pa, ga, ma, va = (x.astype(f64) for x in a)
    gg = hp["wd"] * pa + ga
    m2, v2 = hp["b1"] * ma + (1 - hp["b1"]) * gg, hp["b2"] * va + (1 - hp["b2"]) * gg * gg
    bc1, bc2s = orf.bias_corr64(hp["b1"], hp["b2"], 3)
    np.testing.assert_allclose(r["p"], pa - hp["lr"] / bc1 * m2 / (np.sqrt(v2) / bc2s + hp["eps"]), rtol=1e-14, atol=0)
    np.testing.assert_allclose(r["m"], m2, rtol=1e-15)
    np.testing.assert_allclose(r["v"], v2, rtol=1e-15)
    zero = np.zeros(4, f32)
    r = orf.adam64(zero, zero, zero, zero, hp, bc1, bc2s)          # v' = 0: the denominator is eps alone, nothing moves
    assert not r["p"].any() and not r["v"].any() and np.isfinite(r["bp"]).all()


def test_amp_update_model_is_gradscalers_rule_where_the_clamp_is_inactive():
    rng = np.random.default_rng(1)
    for growth, backoff, interval in ((2.0, 0.5, 3), (1.7, 0.3, 1), (2.0, 0.5, 2000)):
        # torch multiplies the fp32 scale by the factor as a DOUBLE and rounds once; the kernel (and the model) receive the
        # factor as fp32.  Identical for factors fp32 holds (2, 0.5: the defaults), within one ulp of the scale otherwise -- so
        # each call starts from the model's state
        exact = float(f32(growth)) == growth and float(f32(backoff)) == backoff
        tracker = torch.tensor([0], dtype=torch.int32)
        state, flags = [f32(65536.0), f32(1) / f32(65536.0)], [0, 0, 0]
        skipped = 0
        for _ in range(40):
            found = int(rng.random() < 0.3)
            scale = torch.tensor([float(state[0])])
            torch._amp_update_scale_(scale, tracker, torch.tensor([float(found)]), growth, backoff, interval)
            if not 1.0 <= float(scale) <= 16777216.0:
                break
            flags[0] = found
            skipped += found
            state, flags = orf.amp_update_model(state, flags, growth, backoff, interval)
            assert abs(float(state[0]) - float(scale)) <= (0.0 if exact else 2.0 ** -23 * float(scale))
            assert flags == [0, int(tracker), skipped]
            assert state[1] == f32(1) / state[0]
    for seq in orf.AMP_SEQUENCES:
        orf.run_amp_sequence(seq, orf.amp_update_model)
    s, f = orf.amp_update_model([f32(1), f32(1)], [1, 3, 0], 2.0, 0.5, 2000)
    assert float(s[0]) == 1.0 and f == [0, 0, 1]                   # the clamp at 1
    s, f = orf.amp_update_model([f32(2 ** 24), f32(2.0 ** -24)], [0, 0, 0], 2.0, 0.5, 1)
    assert float(s[0]) == 2.0 ** 24 and f == [0, 0, 0]             # and at 2^24


def test_rownorm_closed_form_is_autograd_of_the_reference_formula():
    for mode in (0, 1):
        for eps in (1e-12, 1e-3):
            x32, dy32 = orf.rownorm_inputs(5, 63, 7)
            x = orf.t64(x32)[:4].clone().requires_grad_(True)           # (autograd of a norm that underflowed is not a reference)
            y, n = orf.rownorm64(x, mode, eps)
            (y * orf.t64(dy32)[:4]).sum().backward()
            dx, _ = orf.rownorm_bwd_with(x32[:4], n.detach(), dy32[:4], mode, eps)
            torch.testing.assert_close(dx, x.grad, rtol=1e-12, atol=1e-300)
            yd, _ = orf.rownorm_y_with(x32[:4], n.detach(), mode, eps)
            torch.testing.assert_close(yd, y.detach(), rtol=1e-15, atol=0)
            n = n.detach()
            assert bool((n[:3] > 0).all()) and float(n[3]) == 0.0
            if eps == 1e-3:
                assert float(n[2]) < eps < float(n[0])                  # rows on both sides of the branch


def test_cosine_reference_gradient_is_autograd():
    x32, labels = orf.unit_inputs(17, 36, 5)
    xu = orf.t64(x32)
    xu = (xu / xu.norm(dim=1, keepdim=True)).float().double()
    N = xu.shape[0]
    d = ha.cos_dist64(xu)
    m = ha.mine64(d, ha.cos_dist_bound(xu, d), torch.from_numpy(labels), torch.ones(N, dtype=torch.bool), ha.row_classes(xu), 0.3)
    pi, ni = m["p_idx"], m["n_idx"]
    r = torch.arange(N)
    xa = xu.clone().requires_grad_(True)
    da = (1.0 - xa @ xa.t()).abs().clamp_min(1e-12)
    v = da[r, pi] - da[r, ni] + 0.3
    loss = torch.clamp(v, min=0).mean()
    loss.backward()
    coef = ((v > 0).double() / N).detach()
    dx, bound = ha.triplet_cos_bwd64(xu, d[r, pi].float(), d[r, ni].float(), pi, ni, coef, 1.0)
    assert bool(((dx - xa.grad).abs() <= bound + 1e-15).all())        # (undecided signs: the bound carries the whole term)
    assert float(bound.max()) > 0 and float(xa.grad.abs().max()) > 0
    # the window machinery serves this kind as it serves the euclidean one: the duplicate of row 0 is one class, first index wins
    assert int(ha.row_classes(orf.t64(x32))[1]) == 0


def test_small_references():
    dist, labels = orf.mine_inputs(65, 2)
    ap, an, pi, ni = orf.mine_expect(dist, labels)
    for a in range(65):
        pos = [j for j in range(65) if labels[j] == labels[a]]
        neg = [j for j in range(65) if labels[j] != labels[a]]
        bp = max(pos, key=lambda j: (dist[a, j], -j))
        bn = min(neg, key=lambda j: (dist[a, j], j))
        assert (pi[a], ni[a], ap[a], an[a]) == (bp, bn, dist[a, bp], dist[a, bn])
    emb, order, off = orf.gather_inputs(257, 3)
    got = orf.gather_mean_expect(emb, order, off)
    assert list(np.diff(off)) == [1, 2, 7, 300] and (np.diff(order) < 0).any() and list(order).count(5) >= 2
    for s in range(4):
        want = emb[order[off[s]:off[s + 1]]].astype(f64).mean(0)
        np.testing.assert_allclose(got[s], want, rtol=(off[s + 1] - off[s] + 1) * 2.0 ** -24, atol=1e-6)
    assert orf.same_bits(got[0], emb[order[0]])
    d = np.array([-1.0, 0.0, 1e-13, 1e-12, 4.0, 1e30], f32)
    np.testing.assert_array_equal(orf.clamp_sqrt_expect(d, 1e-12)[:4], np.sqrt(f32(1e-12)))
    assert orf.clamp_sqrt_expect(d, 1e-12)[4] == 2.0


# ------------------------------------------------------------------------------------------------ 2. the models pass
CAPS = (1, 2, 4096)


def run_dev(R, n, preset, hp, seed, cap=4096, mut=None, fam="adam_dev"):
    inp = orf.adam_inputs(n, seed)
    hyper0 = np.array([hp["lr"], preset, 0, 0, 0, 0.25, -3.0, 7.0], f32)
    dev, hyper1 = orf.adam_dev_model(*inp, hyper0, hp, cap_blocks=cap, mut=mut)
    orf.judge_adam_dev(R, fam, f"n {n} preset {preset} cap {cap}", inp, hp, hyper0, dev, hyper1)


def run_host(R, n, step, hp, seed, cap=4096, mut=None, fam="adam_host"):
    inp = orf.adam_inputs(n, seed)
    bc1, bc2s = orf.bias_corr32(hp["b1"], hp["b2"], step)
    orf.check_bias_corr(R, fam + "_bc", "host powf", bc1, bc2s, hp["b1"], hp["b2"], step)
    if n:
        dev = orf.adam_model(*inp, hp, bc1, bc2s, host=True, cap_blocks=cap, mut=mut)
        orf.check_adam(R, fam, f"n {n} step {step} cap {cap}", inp, hp, bc1, bc2s, dev)


def test_fp32_models_pass_every_bound():
    R = orf.Ratios()
    seed = 0
    for wd, gscale in ((5e-4, 1.0), (0.0, 1.0), (5e-4, 0.37), (0.0, 1.0 / 4)):
        hp = orf.hyper_params(wd=wd, gscale=gscale)
        for preset in orf.PRESET_STEPS:
            for n in orf.DEV_SIZES[:-1] + [2052, 4100]:
                for cap in CAPS:
                    seed += 1
                    run_dev(R, n, preset, hp, seed, cap)
            for n in orf.HOST_SIZES[:-1] + [2053, 2049 + 1024]:
                for cap in CAPS:
                    seed += 1
                    run_host(R, n, preset + 1, hp, seed, cap)
    for fam, worst in sorted(R.worst.items()):
        print(f"\nopt_ref| model {fam}: worst error / bound {worst:.3g}", end="")
        assert worst <= 1.0
    assert R.worst["adam_dev_p"] > 0.01 and R.worst["adam_dev_m"] > 0.01 and R.worst["adam_dev_v"] > 0.01, "bounds far too loose"
    # a skipped step and an empty buffer
    inp = orf.adam_inputs(8, 1)
    h0 = np.array([1e-3, 5, 0.1, 0.2, 0, 0, 0, 0], f32)
    dev, h1 = orf.adam_dev_model(*inp, h0, orf.hyper_params(), skip=1)
    assert orf.same_bits(h1, h0) and all(orf.same_bits(dev[k], a) for k, a in zip("pmv", (inp[0], inp[2], inp[3])))
    # the loss scaler's element-wise kernels and the SGD step are their own expectations; the non-finite check at every placement
    for n, cap in ((8, 4096), (1028, 1), (2052, 1)):
        g = orf.finite_gradients(n, n)
        for inv in (f32(1) / f32(65536.0), f32(1) / f32(1000.0), f32(1)):
            out, raised = orf.unscale_model(g, inv, cap)
            assert not raised
            orf.check_unscale("finite", g, inv, [0, 3, 2], out, [0, 3, 2])
            for bad in orf.NONFINITE:
                for at in (0, n // 2, n - 1):
                    gb = g.copy()
                    gb[at] = bad
                    out, raised = orf.unscale_model(gb, inv, cap)
                    assert raised
                    orf.check_unscale("placed", gb, inv, [0, 3, 2], out, [1, 3, 2])


def test_rownorm_model_passes_and_the_product_that_underflowed_does_not():
    R = orf.Ratios()
    for D in (1, 3, 63, 64, 255, 256, 257, 1000, 2048):
        for mode in (0, 1):
            for eps in (1e-12, 1e-3):
                x, dy = orf.rownorm_inputs(5, D, D + mode)
                orf.check_rownorm(R, "rownorm", x, dy, mode, eps, orf.rownorm_model(x, dy, mode, eps))
    assert max(R.worst.values()) <= 1.0
    # b = xg / (n * den * den): n ~ 1e-22 and den = 1e-12 multiply to zero in fp32 -- the form the kernel had
    x, dy = orf.rownorm_inputs(5, 64, 64)
    x[4, 1:] = 0
    x[4, 0] = 1e-22
    old = orf.rownorm_model(x, dy, 1, 1e-12, b_order="n*den*den")
    assert not np.isfinite(old["dx"][4]).all() and np.isfinite(old["dx"][:4]).all()
    with pytest.raises(AssertionError):
        orf.check_rownorm(orf.Ratios(), "rownorm", x, dy, 1, 1e-12, old)
    orf.check_rownorm(R, "rownorm", x, dy, 1, 1e-12, orf.rownorm_model(x, dy, 1, 1e-12))


def test_cosine_model_passes_and_last_index_ties_do_not():
    R = orf.Ratios()
    for N in (4, 6, 17, 33):
        for D in (4, 36, 260):
            x, labels = orf.unit_inputs(N, D, 100 * N + D)
            xu = orf.rownorm_model(x, x, 0, 1e-12)["y"]
            assert orf.same_bits(xu[1], xu[0]) and orf.same_bits(xu[2], -xu[0]) and xu[3, 0] == 1.0
            mask = np.ones(N, np.uint8)
            mask[[1, N - 1]] = 0
            dx0 = np.random.default_rng(N).standard_normal((N, D)).astype(f32)
            for margin, m, g in ((0.3, None, 1.0), (0.3, mask, 0.5), (-1.0, mask, 2.0), (0.0, None, 1.0)):
                fam = "cos_hinge" if margin >= 0 else "cos_soft"
                dev, dx = orf.cos_model(xu, labels, m, margin, g, dx0)
                orf.cos_forward_check(R, fam, xu, labels, m, margin, dev)
                orf.cos_backward_check(R, fam, xu, dev, g, dx0, dx)
                assert dev["dist_mat"][3, 3] == f32(1e-12) and dev["p_idx"][2] == 0       # rows 0, 1 tie as row 2's positive: the first
            dev, _ = orf.cos_model(xu, labels, None, 0.3, 1.0, dx0, flip_ties=True)
            with pytest.raises(AssertionError, match="first index"):
                orf.cos_forward_check(orf.Ratios(), "cos", xu, labels, None, 0.3, dev)
    for fam, worst in sorted(R.worst.items()):
        print(f"\nopt_ref| model {fam}: worst error / bound {worst:.3g}", end="")
    assert max(R.worst.values()) <= 1.0


# ------------------------------------------------------------------------------------------------ 3. the mutants fail
def caught(name, fn):
    try:
        fn()
    except AssertionError as e:
        print(f"\nopt_ref| mutant '{name}' caught by: {str(e).splitlines()[0][:150]}", end="")
        return True
    print(f"\nopt_ref| mutant '{name}' SURVIVED", end="")
    return False


def test_every_adam_mutant_fails_a_bound():
    hp = orf.hyper_params(wd=5e-4, gscale=0.5)
    # (size, grid cap, preset step, host entry point): 64 elements for the element-wise faults -- enough of them for one with
    # |wd p| and the update well above its bound --, one workgroup's float4 plus one for the second trip, 5 for the scalar tail
    where = {"second trip skipped": (1028, 1, 9, False), "scalar tail skipped": (5, 4096, 9, True), "bc1 taken at step - 1": (64, 4096, 1, False)}
    survivors = []
    for name in orf.MUTANTS_ADAM:
        n, cap, preset, host = where.get(name, (64, 4096, 9, False))
        run = run_host if host else run_dev
        arg = preset + 1 if host else preset
        run(orf.Ratios(), n, arg, hp, 11, cap)                                    # the faithful model passes on this very case
        if not caught(name, lambda: run(orf.Ratios(), n, arg, hp, 11, cap, mut=name)):
            survivors.append(name)
    assert not survivors, survivors


def test_elements_past_the_cap_cannot_be_right_by_being_left_alone():
    """SGD, amp_scale: what the GPU tests put past each kernel's grid cap moves under the step, and exact_bits tells a skipped
    second trip (the input left in place) from the expectation -- as it tells -0.0 from 0.0."""
    for cap, n in ((256, 257), (orf.EW_TRIP, orf.EW_TRIP + 1)):
        p, g = orf.wild(n, n), orf.wild(n, n + 1)
        orf.sensitive_past(cap, n, p, g)
        wp, wg = orf.sgd_expect(p, g, 0.5, 2000.0)
        assert (wp[cap:] != p[cap:]).all() and (wg[cap:] != g[cap:]).all()
        skipped_p, skipped_g = np.where(np.arange(n) < cap, wp, p), np.where(np.arange(n) < cap, wg, g)      # 'second trip skipped'
        assert caught("sgd: second trip skipped", lambda: orf.exact_bits(orf.Ratios(), "sgd", "p'", skipped_p, wp))
        assert caught("sgd: second trip skipped", lambda: orf.exact_bits(orf.Ratios(), "sgd", "g'", skipped_g, wg))
        ws = orf.scale_expect(p, 3.3)
        assert caught("amp_scale: second trip skipped", lambda: orf.exact_bits(orf.Ratios(), "amp_scale", "y", np.where(np.arange(n) < cap, ws, f32(9)), ws))
    orf.exact_bits(orf.Ratios(), "x", "same", [0.0, -0.0], [0.0, -0.0])
    assert caught("sign of zero", lambda: orf.exact_bits(orf.Ratios(), "x", "zero", [0.0], [-0.0]))


def test_every_loss_scaler_mutant_fails_a_check():
    survivors = []
    inv = f32(1) / f32(65536.0)
    where = {"blind to NaN": (8, 4096, 3, np.nan), "blind to -inf": (8, 4096, 3, -np.inf), "blind to the last float4": (8, 4096, 7, np.inf),
             "second trip skipped": (1028, 1, 1024, np.inf)}
    for name in orf.MUTANTS_CHECK:
        n, cap, at, bad = where[name]
        g = orf.finite_gradients(n, 5)
        g[at] = bad

        def go(mut):
            out, raised = orf.unscale_model(g, inv, cap, mut)
            orf.check_unscale(f"{bad} at {at} of {n}", g, inv, [0, 3, 2], out, [int(raised), 3, 2])
        go(None)
        if not caught(name, lambda: go(name)):
            survivors.append(name)
    for name in orf.MUTANTS_UPDATE:
        def walk():
            for seq in orf.AMP_SEQUENCES:
                orf.run_amp_sequence(seq, lambda *a: orf.amp_update_model(*a, mut=name))
        if not caught(name, walk):
            survivors.append(name)
    assert not survivors, survivors
