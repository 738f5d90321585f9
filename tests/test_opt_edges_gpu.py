"""What csrc/heads.hip runs after the heads, over the C ABI, against tests/opt_ref.py: the three Adam entry points, the centers'
SGD step and the f16 loss scaler (scale, unscale-and-check, update) -- at the sizes where a grid-stride kernel can go wrong (empty,
one float4, around one workgroup, one float4 / one element / a scalar tail into the SECOND trip of each kernel's own grid cap)
and at the step counts a restored checkpoint presets.

Adam in two layers: the bias corrections the device publishes in hyper[2..3] against float64 within the measured powf slack;
p, m and v element by element against the float64 step evaluated with those published corrections, the bar on p scaling with
the update.  The scale, unscale and SGD kernels are bit-exact expectations.  The non-finite check is tried with +inf, -inf and
NaN at the first and last element, on both sides of the trip boundary and in the middle of the second trip; refused shapes
return CREID_E_SHAPE before any launch and leave every buffer as it was.

Worst error / bound per family, the powf deviations and the file's run time: profiles/opt_edges.md."""
import numpy as np
import pytest
import torch

import opt_ref as orf

pytestmark = pytest.mark.gpu

f32 = np.float32
E_SHAPE = -4
RATIOS = orf.Ratios()
K_SEEN = {}
BIG_DEV, BIG_HOST = orf.DEV_SIZES[-1], orf.HOST_SIZES[-1]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in sorted(RATIOS.worst):
        print(f"\nopt_edges| {fam}: worst error / bound {RATIOS.worst[fam]:.4g}", end="")
    for k in sorted(K_SEEN):
        print(f"\nopt_edges| implied k_pow, {k}: {K_SEEN[k]:.3f} (K_POW {orf.K_POW})", end="")
    print("\nopt_edges| cases: " + ", ".join(f"{k} {v}" for k, v in sorted(RATIOS.cases.items())))


def L():
    from centroids_reid_amd import _lib
    _lib.lib()
    return _lib


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_INPUTS = {}


def adam_inputs(n, seed=0):
    """the big buffers are drawn once, at the host entry point's size, and sliced (the float64 reference of 4 M elements is the
    expensive part of this file; nothing is gained by fresh draws)"""
    if n < 4096:
        return orf.adam_inputs(n, 1000 * seed + n)
    if "big" not in _INPUTS:
        _INPUTS["big"] = orf.adam_inputs(BIG_HOST, 77)
    return tuple(a[:n].copy() for a in _INPUTS["big"])


def hyper0(lr, preset):
    return np.array([lr, preset, 0.5, 0.25, 0, 0.25, -3.0, 7.0], f32)          # ([2], [3]: stale values the step must overwrite)


def adam_dev(bufs, n, hyper, hp, flags=None):
    l = L()
    a = [l.ptr(b) for b in bufs] + [n, l.ptr(hyper), hp["b1"], hp["b2"], hp["eps"], hp["wd"], hp["gscale"]]
    if flags is None:
        return l.lib().creid_adam_step_dev(*a, l.stream())
    return l.lib().creid_adam_step_dev_amp(*a, l.ptr(flags), l.stream())


def dev_of(bufs):
    return dict(p=host(bufs[0]), m=host(bufs[2]), v=host(bufs[3]))


def note_k(variant, h1, hp, t):
    K_SEEN[variant + " bc1"] = max(K_SEEN.get(variant + " bc1", 0.0), orf.implied_k_pow(h1[2], hp["b1"], t))
    K_SEEN[variant + " bc2s"] = max(K_SEEN.get(variant + " bc2s", 0.0), orf.implied_k_pow(h1[3], hp["b2"], t, root=True))


COMBOS = [(5e-4, 1.0), (0.0, 0.37), (5e-4, 0.37)]        # (weight decay, grad scale); only the last tells fma(wd, p, g * gs) from
BIG_COMBOS = COMBOS[2:]                                   # fma(wd, p, g) * gs: that one reaches the second trip


# ------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("amp", [False, True], ids=["dev", "dev_amp"])
@pytest.mark.parametrize("n", orf.DEV_SIZES)
def test_adam_dev_steps(n, amp):
    variant = "dev_amp" if amp else "dev"
    flags = torch.tensor([0, 3, 2], dtype=torch.int32).cuda() if amp else None
    big = n >= 4096
    for wd, gs in BIG_COMBOS if big else COMBOS:
        hp = orf.hyper_params(wd=wd, gscale=gs)
        for preset in [9] if big else orf.PRESET_STEPS:
            inp = adam_inputs(n, preset)
            bufs = [cu(a) if n else torch.zeros(4, device="cuda") for a in inp]
            h0 = hyper0(hp["lr"], preset)
            hyper = cu(h0)
            assert adam_dev(bufs, n, hyper, hp, flags) == 0
            h1 = host(hyper)
            if big and amp:
                # the same kernel on the same operands: bit-identical to the plain entry point, which the reference judges
                ref = [cu(a) for a in inp]
                hyper_r = cu(h0)
                assert adam_dev(ref, n, hyper_r, hp) == 0
                assert all(bits_equal(a, b) for a, b in zip(bufs, ref)) and bits_equal(hyper, hyper_r)
                continue
            orf.judge_adam_dev(RATIOS, "adam_" + variant, f"{variant} n {n} preset {preset} wd {wd} gscale {gs}", inp, hp, h0,
                               dev_of(bufs) if n else None, h1)
            note_k(variant, h1, hp, preset + 1)
            if n:
                assert np.array_equal(host(bufs[1]), inp[1]), "the gradient buffer was written"
            if amp:
                assert host(flags).tolist() == [0, 3, 2]


@pytest.mark.parametrize("n", orf.HOST_SIZES)
def test_adam_host_scalar_steps(n):
    l = L()
    big = n >= 4096
    for wd, gs in BIG_COMBOS if big else COMBOS:
        hp = orf.hyper_params(wd=wd, gscale=gs)
        for preset in [9] if big else orf.PRESET_STEPS:
            step = preset + 1
            inp = adam_inputs(n, preset)
            bufs = [cu(a) if n else torch.zeros(4, device="cuda") for a in inp]
            rc = l.lib().creid_adam_step(*[l.ptr(b) for b in bufs], n, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], step, hp["gscale"],
                                         l.stream())
            assert rc == 0
            bc1, bc2s = orf.bias_corr32(hp["b1"], hp["b2"], step)      # the host's powf, through the same libm
            orf.check_bias_corr(RATIOS, "adam_host_bc", "host powf", bc1, bc2s, hp["b1"], hp["b2"], step)
            K_SEEN["host bc1"] = max(K_SEEN.get("host bc1", 0.0), orf.implied_k_pow(bc1, hp["b1"], step))
            K_SEEN["host bc2s"] = max(K_SEEN.get("host bc2s", 0.0), orf.implied_k_pow(bc2s, hp["b2"], step, root=True))
            if n:
                orf.check_adam(RATIOS, "adam_host", f"host n {n} step {step} wd {wd} gscale {gs}", inp, hp, bc1, bc2s, dev_of(bufs))
                assert np.array_equal(host(bufs[1]), inp[1]), "the gradient buffer was written"


@pytest.mark.parametrize("amp", [False, True], ids=["dev", "dev_amp"])
def test_ten_steps_back_to_back_advance_the_counter_by_ten(amp):
    """No host synchronisation between the launches: the last workgroup of each publishes {step, bc1, bc2s} and clears the
    ticket before the next launch reads them.  40 workgroups; the result is bit-identical to ten synchronised steps, each of
    which is judged."""
    n = 40 * 1024
    hp = orf.hyper_params(wd=5e-4, gscale=0.37)
    rng = np.random.default_rng(3)
    inp = orf.adam_inputs(n, 5)
    grads = [inp[1]] + [(f32(1e-2) * rng.standard_normal(n)).astype(f32) for _ in range(9)]
    flags = torch.zeros(3, dtype=torch.int32).cuda() if amp else None
    fast = [cu(a) for a in inp]
    gfast = [cu(g) for g in grads]
    hyper = cu(hyper0(hp["lr"], 0))
    for g in gfast:
        assert adam_dev([fast[0], g, fast[2], fast[3]], n, hyper, hp, flags) == 0
    h = host(hyper)
    assert float(h[1]) == 10.0 and int(h.view(np.int32)[4]) == 0, h
    slow = [cu(a) for a in inp]
    hyper_s = cu(hyper0(hp["lr"], 0))
    cur = [a.copy() for a in inp]
    for i, g in enumerate(grads):
        h0 = host(hyper_s)
        assert adam_dev([slow[0], gfast[i], slow[2], slow[3]], n, hyper_s, hp, flags) == 0
        out = dev_of(slow)
        orf.judge_adam_dev(RATIOS, "adam_chain", f"chained step {i + 1}", (cur[0], g, cur[2], cur[3]), hp, h0, out, host(hyper_s))
        cur[0], cur[2], cur[3] = out["p"], out["m"], out["v"]
    assert all(bits_equal(fast[i], slow[i]) for i in (0, 2, 3)) and bits_equal(hyper, hyper_s)


def test_empty_buffer_advances_the_counter_unless_skipped():
    hp = orf.hyper_params()
    z = [torch.zeros(4, device="cuda") for _ in range(4)]
    for flag, want in ((0, 6.0), (1, 5.0)):
        flags = torch.tensor([flag, 3, 2], dtype=torch.int32).cuda()
        h0 = hyper0(hp["lr"], 5)
        hyper = cu(h0)
        assert adam_dev(z, 0, hyper, hp, flags) == 0
        h1 = host(hyper)
        assert float(h1[1]) == want
        if flag:
            assert orf.same_bits(h1, h0)
        else:
            orf.judge_adam_dev(RATIOS, "adam_dev_amp", "empty, not skipped", tuple(np.zeros(0, f32) for _ in range(4)), hp, h0, None, h1)
        assert host(flags).tolist() == [flag, 3, 2]


@pytest.mark.parametrize("n", [1, 2, 3, 1026, 4099])
def test_odd_lengths_are_refused_untouched(n):
    l = L()
    hp = orf.hyper_params()
    inp = orf.adam_inputs(n + 1, n)
    bufs = [cu(a) for a in inp]
    keep = [b.clone() for b in bufs]
    flags = torch.tensor([0, 3, 2], dtype=torch.int32).cuda()
    state = cu(np.array([65536.0, 1.0 / 65536.0], f32))
    for f in (None, flags):
        hyper = cu(hyper0(hp["lr"], 4))
        assert adam_dev(bufs, n, hyper, hp, f) == E_SHAPE
        assert orf.same_bits(host(hyper), hyper0(hp["lr"], 4))
    assert l.lib().creid_amp_unscale_check(l.ptr(bufs[1]), n, l.ptr(state), l.ptr(flags), l.stream()) == E_SHAPE
    assert all(bits_equal(a, b) for a, b in zip(bufs, keep)) and host(flags).tolist() == [0, 3, 2]


# ------------------------------------------------------------------------------------------------ the skip
@pytest.mark.parametrize("n", [0, 4, 1028, 8192])
def test_a_raised_flag_skips_adam_and_sgd_bit_for_bit(n):
    l = L()
    hp = orf.hyper_params()
    inp = orf.adam_inputs(max(n, 4), n + 1)
    bufs = [cu(a) for a in inp]
    keep = [b.clone() for b in bufs]
    flags = torch.tensor([1, 3, 2], dtype=torch.int32).cuda()
    h0 = np.array([hp["lr"], 17, 0.83, 0.13, 0, 1.5, -2.5, 3.5], f32)
    hyper = cu(h0)
    assert adam_dev(bufs, n, hyper, hp, flags) == 0
    assert orf.same_bits(host(hyper), h0), "a skipped step changed hyper"
    assert l.lib().creid_sgd_scaled_step_amp(l.ptr(bufs[0]), l.ptr(bufs[1]), n, 0.5, 2000.0, l.ptr(flags), l.stream()) == 0
    assert all(bits_equal(a, b) for a, b in zip(bufs, keep)) and host(flags).tolist() == [1, 3, 2]


# ------------------------------------------------------------------------------------------------ SGD, scale: bit-exact
@pytest.mark.parametrize("amp", [False, True], ids=["plain", "amp"])
@pytest.mark.parametrize("n", orf.EW_SIZES + [orf.EW_TRIP + 1])
def test_sgd_scaled_step_is_two_rounded_products_and_a_difference(n, amp):
    l = L()
    p, g = orf.wild(n, n), orf.wild(n, n + 1)
    orf.sensitive_past(orf.EW_TRIP, n, p, g)                 # the element of the second trip: p and g of order 1
    p[-1], g[-1] = 1.5, -0.75                                # (and the last element of every size)
    if n > 1:
        g[n // 2] = 0
    for lr, gmul in ((0.5, 2000.0), (0.3, 1.0 / 3)):
        lr, gmul = float(f32(lr)), float(f32(gmul))
        pd, gd = cu(p), cu(g)
        if amp:
            flags = torch.tensor([0, 3, 2], dtype=torch.int32).cuda()
            rc = l.lib().creid_sgd_scaled_step_amp(l.ptr(pd), l.ptr(gd), n, lr, gmul, l.ptr(flags), l.stream())
        else:
            rc = l.lib().creid_sgd_scaled_step(l.ptr(pd), l.ptr(gd), n, lr, gmul, l.stream())
        assert rc == 0
        wp, wg = orf.sgd_expect(p, g, lr, gmul)
        assert wp[-1] != p[-1] and wg[-1] != g[-1], "the last element (the only one of trip two past the cap) must have to move"
        orf.exact_bits(RATIOS, "sgd", f"g' n {n}", host(gd), wg)
        orf.exact_bits(RATIOS, "sgd", f"p' n {n}", host(pd), wp)
    RATIOS.count("sgd")
    assert l.lib().creid_sgd_scaled_step(l.ptr(pd), l.ptr(gd), 0, 0.5, 1.0, l.stream()) == 0


@pytest.mark.parametrize("n", orf.EW_SIZES + [orf.SCALE_TRIP + 1])
def test_amp_scale_is_one_rounded_product(n):
    l = L()
    x = orf.wild(n, n + 7)
    orf.sensitive_past(orf.SCALE_TRIP, n, x)
    x[-1] = 1.5                                              # (and the last element of every size: its product differs from it and from the prefill)
    for s in (65536.0, 1000.0, 1.0, 3.3):
        state = np.array([s, 1.0], f32)
        state[1] = f32(1) / state[0]
        xd, yd = cu(x), torch.full((n,), 9.0, device="cuda")
        assert l.lib().creid_amp_scale(l.ptr(xd), n, l.ptr(cu(state)), l.ptr(yd), l.stream()) == 0
        want = orf.scale_expect(x, state[0])
        assert want[-1] != 9.0 and (s == 1.0 or want[-1] != x[-1])
        orf.exact_bits(RATIOS, "amp_scale", f"n {n} scale {s}", host(yd), want)
        assert np.array_equal(host(xd), x)
    RATIOS.count("amp_scale")


# ------------------------------------------------------------------------------------------------ the non-finite check
STATES = [(65536.0, "scale 2^16"), (1000.0, "scale 1000: 1 / scale is rounded"), (1.0, "check-only {1, 1}")]


@pytest.mark.parametrize("n", [4, 1020, 1024, 1028])
def test_unscale_check_small(n):
    l = L()
    g = orf.finite_gradients(n, n)
    for s, _ in STATES:
        state = np.array([s, 0], f32)
        state[1] = f32(1) / state[0]
        sd = cu(state)
        for at, bad in [(None, None)] + [(at, bad) for at in sorted({0, n // 2, n - 1}) for bad in orf.NONFINITE]:
            gb = g.copy()
            if at is not None:
                gb[at] = bad
            gd, flags = cu(gb), torch.tensor([0, 3, 2], dtype=torch.int32).cuda()
            assert l.lib().creid_amp_unscale_check(l.ptr(gd), n, l.ptr(sd), l.ptr(flags), l.stream()) == 0
            orf.check_unscale(f"n {n} scale {s}: {bad} at {at}", gb, state[1], [0, 3, 2], host(gd), host(flags))
            assert orf.same_bits(host(sd), state)
    RATIOS.count("amp_unscale")
    assert l.lib().creid_amp_unscale_check(l.ptr(gd), 0, l.ptr(sd), l.ptr(flags), l.stream()) == 0


@pytest.mark.parametrize("s,what", STATES, ids=["s65536", "s1000", "check_only"])
def test_unscale_check_one_float4_past_the_cap(s, what):
    """n = 4096 * 1024 + 4.  One bad value at a time from {+inf, -inf, NaN} at index 0, cap - 1, cap (first reached in the second
    trip), n - 1 and in the middle of the second trip: bit 0 of flags[0] and nothing else is raised, every other element is
    fl(g * inv) exactly (compared on the device, bit for bit).  All-finite data with +-3e38 raises nothing."""
    l = L()
    n, cap = BIG_DEV, orf.ADAM_TRIP
    g = orf.finite_gradients(n, 9)
    state = np.array([s, 0], f32)
    state[1] = f32(1) / state[0]
    sd = cu(state)
    want, raised = orf.unscale_model(g, state[1])
    assert not raised
    base, wd = cu(g), cu(want).view(torch.int32)
    work = torch.empty_like(base)
    for at, bad in [(None, None)] + [(at, bad) for at in (0, cap - 1, cap, cap + 2, n - 1) for bad in orf.NONFINITE]:
        work.copy_(base)
        if at is not None:
            work[at] = bad
        flags = torch.tensor([0, 3, 2], dtype=torch.int32).cuda()
        assert l.lib().creid_amp_unscale_check(l.ptr(work), n, l.ptr(sd), l.ptr(flags), l.stream()) == 0
        got = work.view(torch.int32)
        diff = got != wd
        if at is not None:
            v = float(work[at])
            assert (np.isnan(v) if np.isnan(bad) else v == bad), f"{what}: {bad} at {at} became {v}"
            diff[at] = False
        assert not bool(diff.any()), f"{what}: {bad} at {at}: {int(diff.sum())} other elements are not fl(g * inv)"
        assert host(flags).tolist() == [0 if at is None else 1, 3, 2], f"{what}: {bad} at {at}: flags {host(flags).tolist()}"
    RATIOS.count("amp_unscale")


# ------------------------------------------------------------------------------------------------ the scale's state machine
@pytest.mark.parametrize("seq", orf.AMP_SEQUENCES, ids=[s[0].split(":")[0].replace(" ", "_") for s in orf.AMP_SEQUENCES])
def test_amp_update_follows_the_model(seq):
    l = L()

    def update(state, flags, growth, backoff, interval):
        sd, fd = cu(np.array(state, f32)), cu(np.array(flags, np.int32))
        assert l.lib().creid_amp_update(l.ptr(sd), l.ptr(fd), growth, backoff, interval, l.stream()) == 0
        return list(host(sd)), list(host(fd))
    orf.run_amp_sequence(seq, update)


# ------------------------------------------------------------------------------------------------ the powf slack, widely
SWEEP_STEPS = list(range(1, 65)) + [100, 500, 1000, 2000, 5000, 10000, 20000]


@pytest.mark.parametrize("n", [0, 4], ids=["adam_advance_kernel", "adam_dev_kernel"])
def test_published_corrections_hold_their_bar_over_a_sweep_of_steps(n):
    """The steps K_POW was measured over (profiles/opt_edges.md), from both kernels that publish corrections: every bc1 and bc2s
    within pow_bar of float64; the report prints the largest implied k_pow."""
    hp = orf.hyper_params()
    bufs = [torch.zeros(4, device="cuda") for _ in range(4)]
    for t in SWEEP_STEPS:
        hyper = cu(hyper0(hp["lr"], t - 1))
        assert adam_dev(bufs, n, hyper, hp) == 0
        h1 = host(hyper)
        assert float(h1[1]) == t
        orf.check_bias_corr(RATIOS, "bc_sweep", f"n {n}", h1[2], h1[3], hp["b1"], hp["b2"], t)
        note_k(f"sweep n {n}", h1, hp, t)
    RATIOS.count("bc_sweep")
