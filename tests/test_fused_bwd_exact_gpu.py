"""The FUSED backward launches of 16-bit training, pinned exactly against fp64 at ragged and tiny shapes (references, operand
sets and the proofs of exactness: tests/fused_bwd_exact.py).  Every assertion is an exact comparison of values.

  A  creid_conv2d_dgrad_fused_nhwc, bf16 and f16, seven forms per geometry, dx and partial pre-filled with NaN:
       1 sums with bn_act, 2 sums with bn_mask (bn_act = -1 handed in too: it must not be read), 3 sums with neither,
       4 form 2 + full add_src, 5 form 2 + add_src * add_mask, 6 form 2 + compact stride-2 add (even extents), 7 add_mask only.
     dx bit for bit; every partial value written; column sums over all rows exact; partial rows exact against the zero-padded
     128-row tiles (rows beyond M contribute nothing).  The parity-class stride-2 kernel (route " parity=1": stride-2 3 x 3,
     even extents, (M / 4) % 128 == 0, no compact add) enumerates its GEMM rows parity-class major, so its partial row t is NOT
     pixels 128 t .. 128 t + 127: for it the whole-sum check stands alone (form 6 of that geometry runs the plain row order and
     is checked row by row).  Per-image statistics (IBN): B = 3 at 16 x 8 and 32 x 8, mean / invstd [B][C] differing per image.
     fp32: plain, full add, compact add, each carrying a reduce job (which then runs as its own launch first).
  B  creid_conv2d_wgrad_partials (bf16, f16, fp32), then the reduce job in each of its three homes, accumulate 0 and 1, against
     ref_wgrad (+ the initial dw): creid_conv2d_wgrad_reduce_job; carried by a data gradient of ANOTHER geometry (3 x 3 job on a
     1 x 1 carrier and the reverse, the M = 1 carrier, the parity-eligible carrier; BatchNorm sums on and off; the carrier's own
     dx and partials stay exact); creid_bn2d_bwd_finalize_wred next to a finalize whose outputs are exact.
  C  creid_conv2d_wgrad_partials_bnfin: five finalize shapes on a tap-fused, a tile-kernel and an M = 1 weight gradient, with
     CREID_WGRAD_TAPS both ways.
  D  the refusals of conv_dgrad_check / wred_make_job: return code, and outputs untouched.

Which test speaks for which branch (file:line as of this commit):
  conv_igemm.hip:301-306  pre_x / pre_a / pre_m prefetch under rr < g.M .... A forms 1-3 at M = 1, 105, 129, 255 (partial tiles)
  conv_igemm.hip:304      mask byte bnred.mask[off >> 3] ................... A forms 2, 4, 5, 6 (bn_act = -1 must not matter)
  conv_igemm.hip:342      per-image offset tile_m / tiles_per_image ........ test_per_image_statistics (one and two tiles per image)
  conv_igemm.hip:367-373  compact-add address and even-pixel predicate ..... A form 6 (M = 96 and 12348: partial tiles; 256, 1536, 4096)
  conv_igemm.hip:376      add_mask byte g.add_mask[aoff >> 3] .............. A forms 5, 7
  conv_igemm.hip:380      bnred_chunk on the STORED chunk (after the add) .. A forms 4-6
  conv_igemm.hip:383-397  octet sums -> partial row tile_m ................. A row-by-row check; parity: whole sums
  conv_epilogue.hpp:83    add_chunk bit order (2q, 2q + 1) ................. A forms 5, 7
  conv_epilogue.hpp:99    bnred_chunk bit order, a > 0 && bit .............. A forms 1, 2
  conv_igemm.hip:1136-1143 fp32 epilogue: full / compact add ............... test_fp32_forms_carry_a_job (the compact form read the
                          compact tensor at the full-resolution index before this file existed: profiles/fused_bwd_exact.md)
  conv_igemm.hip:1429     reduce job as its own launch first (fp32) ........ test_fp32_forms_carry_a_job, B fp32
  wgrad_reduce.hpp:29-69  1 x 1 flat path, split lanes, 8-unroll + tail .... B 1 x 1 jobs (splits 1, 10, 16, 49; fp32 2 .. 111)
  wgrad_reduce.hpp:71-129 3 x 3 path, 8 / 4 / 1 unroll tails, two lanes .... B 3 x 3 jobs (splits 1, 2, 3, 4, 8, 28, 32; fp32 .. 56)
  bn_fin.hpp:38-49        4-way unrolled row loop and its tail ............. C rows 1, 3, 7, 512, 1024
  bn_fin.hpp:79-84        cw = 4 / cw = 16, C % 16 != 0 .................... C (64, 1024), (256, 512) / (64, 1), (1000, 7), (2048, 3)
  conv_wgrad.hip:1262-1269 finalize rides / own launch after ............... C 16-bit (CREID_WGRAD_TAPS = 1 / 0) / C fp32
  conv_wgrad.hip:1362-1370 wred_bnfin_kernel ............................... B home 3

Counts and run time, measured on one MI355X (profiles/fused_bwd_exact.md): 146 cases -- A 24 + 8 per-image + 12 fp32, B 54, C 45,
D 1, and the two host-side checks of the parameter lists -- 1112 launches, 2890 exact comparisons; the whole file runs in 3.9 s
(the first case 0.85 s: it loads the library; every other case <= 0.16 s)."""
import ctypes as C
import types

import pytest
import torch

import conv_exact as ce
import fused_bwd_exact as fx

pytestmark = pytest.mark.gpu

H16 = ["bf16", "f16"]
FOREIGN = ((32, 512, 512, 3, 1, 16, 8), (1024, 512, 512, 3, 1, 2, 2))       # (layer4's 3 x 3 at B = 32, 256 x 128; same M, N, K, mode)
WIDE_TILE = (1, 512, 64, 1, 1, 98, 126)
GEOMS_A = [
    (1, 64, 64, 3, 1, 1, 1),            # M = 1
    (3, 64, 64, 3, 1, 7, 5),            # M = 105, one partial tile, image borders inside it
    (1, 64, 256, 1, 1, 43, 3),          # M = 129, one row past a tile
    (17, 64, 64, 3, 1, 5, 3),           # M = 255
    (2, 64, 128, 3, 2, 8, 6),           # stride 2, even extents
    (3, 64, 128, 3, 2, 32, 16),         # eligible for the parity-class stride-2 kernel, odd B
    (5, 256, 64, 1, 2, 9, 7),           # 1 x 1 stride 2, odd extents
    (2, 256, 64, 1, 1, 16, 8),          # 256 output columns
    (1, 512, 128, 1, 1, 10, 10),        # 512 output columns
    (2, 512, 64, 3, 1, 3, 3),           # K = 4608
    WIDE_TILE,                          # 97 row tiles x 512 columns: enough workgroups for the 128-COLUMN tile (every other
                                        # geometry here runs 64-column tiles), M = 12348 with a partial last tile, even extents
    FOREIGN[1],                         # a production plan key under a foreign image factorisation (1024 images of 2 x 2)
]
GEOMS_IBN = [(3, 64, 64, 3, 1, 16, 8), (3, 64, 64, 3, 1, 32, 8), (3, 256, 64, 1, 1, 16, 8), (3, 256, 64, 1, 1, 32, 8)]
GEOMS_B = GEOMS_A + [
    (8, 64, 64, 1, 1, 32, 16),          # 1 x 1, 16 splits on two split lanes: the 8-unrolled loop of the flat path
    (5, 64, 64, 1, 1, 32, 16),          # 1 x 1, 10 splits on two split lanes: its tail loop alone
    (8, 64, 64, 3, 1, 32, 16),          # 3 x 3, 32 splits on two lanes: the 8-unrolled loop twice
    (7, 64, 64, 3, 1, 32, 16),          # 3 x 3, 28 splits on two lanes: 8-unrolled, 4-unrolled and two single steps
    (8, 64, 64, 3, 1, 16, 8),           # 3 x 3, 8 splits on two lanes: the 4-unrolled loop alone
    (4, 128, 128, 3, 1, 16, 8),         # 3 x 3, K = 1152: one lane
]
CARRIER_1X1, CARRIER_3X3 = (2, 256, 64, 1, 1, 16, 8), (3, 64, 64, 3, 1, 7, 5)
CARRIER_M1, CARRIER_PARITY = (1, 64, 64, 3, 1, 1, 1), (3, 64, 128, 3, 2, 32, 16)
FORMS_A = ["1_act", "2_mask", "3_plain_sums", "4_mask_add", "5_mask_add_addmask", "6_mask_compact_add", "7_addmask_only"]


def _lib():
    from centroids_reid_amd import _lib as L
    lib = L.lib()
    assert L.N_PLANS == len(ce.PLANS), "the shipped plan file must be registered"
    return L, lib


def _done(fails, what, launches, compared):
    torch.cuda.synchronize()
    print(f"{what}: {launches} launches, {compared} comparisons")
    assert not fails, f"{what}: {len(fails)} failure(s):\n" + "\n".join(fails[:30])


def _even(geom):
    return geom[5] % 2 == 0 and geom[6] % 2 == 0


# ------------------------------------------------------------------------------------ A
def test_geometries_collide_with_no_plan_but_the_foreign_one():
    from centroids_reid_amd.bench_train import conv_plan_keys
    for g in GEOMS_A[:-1] + GEOMS_IBN + GEOMS_B[len(GEOMS_A):]:
        assert not any(k in ce.PLANS for k in ce.plan_keys(*g).values()), g
    prod, foreign = FOREIGN
    prod_keys = [keys for ls in (1, 2) for shape, keys in conv_plan_keys(prod[0], 256, 128, ls) if shape == tuple(prod[1:])]
    assert prod_keys, "the production layer must be a convolution of the B = 32, 256 x 128 workload"
    mine = ce.plan_keys(*foreign)
    for kind in ("dgrad", "wgrad"):
        assert mine[kind] == prod_keys[0][kind] and mine[kind] in ce.PLANS, kind


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("geom", GEOMS_A, ids=fx.gid)
def test_fused_data_gradient_is_exact(geom, dtype):
    L, lib = _lib()
    dt, o = fx.DT[dtype], fx.operands(geom)
    fails, launches, compared, routes = [], 0, 0, set()
    for form in FORMS_A:
        if fx.FORMS[form][0] == "compact" and not _even(geom):
            continue
        text = fx.describe(geom, fx.ROUTE_DGRAD, fx.route_bits(form), dt)
        parity = " parity=1" in text
        key = ce.plan_keys(*geom)["dgrad"]
        h0 = int(lib.creid_tune_count(*key, 0)) if key in ce.PLANS else None
        rc, dx, part, _ = fx.dgrad_fused(o, dt, form)
        launches += 1
        what = f"A {fx.gid(geom)} {dtype} {form}"
        if rc != 0:
            fails.append(f"{what}: rc = {rc}")
            continue
        if h0 is not None and int(lib.creid_tune_count(*key, 0)) != h0 + 1:
            fails.append(f"{what}: the production plan {key} was not looked up")
        compared += fx.check_dgrad(o, dt, form, dx, part, fails, what, row_by_row=not parity)
        routes.add(text.split(" grid=")[0] + (" parity=1" if parity else ""))
    if geom == CARRIER_PARITY:
        assert any("parity=1" in r for r in routes) and any("parity=1" not in r for r in routes), routes
    assert all(("kernel<128, " in r) == (geom == WIDE_TILE) for r in routes), routes     # the one geometry on 128-column tiles
    _done(fails, f"A| {fx.gid(geom)} {dtype} dy in -{o.dy_hi}..{o.dy_hi} routes {sorted(routes)}", launches, compared)


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("geom", GEOMS_IBN, ids=fx.gid)
def test_per_image_statistics(geom, dtype):
    """bn_stat_image_rows = h w: mean / invstd are [B][C] and differ per image, so a wrong image index changes the sums; the
    partial rows (one or two per image) are compared row by row"""
    _lib()
    dt, o = fx.DT[dtype], fx.operands(geom)
    assert not torch.equal(o.mean_img[0], o.mean_img[1]) and not torch.equal(o.invstd_img[1], o.invstd_img[2])
    fails, launches, compared = [], 0, 0
    for form in ("1_act", "2_mask", "3_plain_sums", "5_mask_add_addmask"):
        text = fx.describe(geom, fx.ROUTE_DGRAD, fx.route_bits(form, per_image=True), dt)
        assert "parity" not in text
        rc, dx, part, _ = fx.dgrad_fused(o, dt, form, per_image=True)
        launches += 1
        what = f"IBN {fx.gid(geom)} {dtype} {form}"
        if rc != 0:
            fails.append(f"{what}: rc = {rc}")
            continue
        compared += fx.check_dgrad(o, dt, form, dx, part, fails, what, per_image=True)
    _done(fails, f"A-ibn| {fx.gid(geom)} {dtype}", launches, compared)


def _small_job(dtype, k):
    """a two-split job of the other kernel size than the carrier's"""
    return fx.Job(fx.operands((4, 64, 64, 1, 1, 16, 8) if k == 1 else (2, 64, 64, 3, 1, 16, 8)), dtype)


@pytest.mark.parametrize("geom", GEOMS_A, ids=fx.gid)
def test_fp32_forms_carry_a_job(geom):
    """fp32: plain, full add and compact add, each with a carried reduce job -- the fp32 kernels have no carrier, the job runs as
    its own launch first (route "pre=wred("); dx and dw exact"""
    _lib()
    dt, o = torch.float32, fx.operands(geom)
    job = _small_job(dt, 1 if geom[3] == 3 else 3)
    assert job.rc == 0 and job.o.geom != geom
    blocks = fx.job_shape(job.o.geom, job.splits)[0]
    fails, launches, compared = [], 1, 0
    for i, form in enumerate(("plain", "add", "compact_add")):
        if form == "compact_add" and not _even(geom):
            continue
        text = fx.describe(geom, fx.ROUTE_DGRAD, fx.route_bits(form, job_blocks=blocks), dt)
        assert text.startswith(f"pre=wred({blocks}) ; igemm_f32_kernel<"), text
        rc, dx, _, dw = fx.dgrad_fused(o, dt, form, job=job, accumulate=i & 1)
        launches += 1
        what = f"fp32 {fx.gid(geom)} {form}"
        if rc != 0:
            fails.append(f"{what}: rc = {rc}")
            continue
        compared += fx.check_dgrad(o, dt, form, dx, None, fails, what) + 1
        if not torch.equal(dw.double(), job.want(i & 1)):
            fails.append(f"{what}: carried dw: {int((dw.double() != job.want(i & 1)).sum())} mismatches")
    _done(fails, f"A-fp32| {fx.gid(geom)}", launches, compared)


# ------------------------------------------------------------------------------------ B
def _carriers(i, geom):
    first = CARRIER_1X1 if geom[3] == 3 else CARRIER_3X3
    special = [CARRIER_M1, CARRIER_PARITY][i % 2]
    if special == geom:
        special = [CARRIER_M1, CARRIER_PARITY][(i + 1) % 2]
    return [first, special]


def _carrier_forms(dtype):
    return ("plain", "add") if dtype == "fp32" else ("5_mask_add_addmask", "plain")          # BatchNorm sums on / off


def test_split_counts_and_job_routes_cover_the_reduce_paths():
    """Over the parameter list of test_reduce_job_in_its_three_homes (host-side planner calls only): the split counts reach 1,
    2-3, 4-7, >= 8 on a 3 x 3 job and a 1 x 1 job with more than 8 splits (split_lanes >= 2); the carried jobs both ride
    ("wred=") and run first ("pre=wred(").  A planner change that thins the list out fails here."""
    _lib()
    seen, rides, first = set(), 0, 0
    for dtype in fx.DT:
        for i, geom in enumerate(GEOMS_B):
            s = fx.splits_of(geom, fx.DT[dtype])
            assert s >= 1 and fx.ws_bytes(geom, fx.DT[dtype]) == s * geom[1] * geom[2] * geom[3] ** 2 * 4
            blocks, lanes = fx.job_shape(geom, s)
            seen.add((dtype != "fp32", geom[3], s, lanes))
            for cg in _carriers(i, geom):
                assert cg != geom and (cg[3] != geom[3] or cg in (CARRIER_M1, CARRIER_PARITY))
                for form in _carrier_forms(dtype):
                    text = fx.describe(cg, fx.ROUTE_DGRAD, fx.route_bits(form, job_blocks=blocks), fx.DT[dtype])
                    rides += f" wred={blocks}" in text
                    first += text.startswith(f"pre=wred({blocks}) ; ")
                    assert (f" wred={blocks}" in text) != text.startswith("pre=wred("), text
    print("B| (16-bit, k, splits, split lanes) covered:", sorted(seen), "rides", rides, "first", first)
    for is16 in (True, False):
        mine = [(k, s, sl) for h, k, s, sl in seen if h == is16]
        assert any(s == 1 for _, s, _ in mine) and any(2 <= s <= 3 for _, s, _ in mine) and any(4 <= s <= 7 for _, s, _ in mine), mine
        assert any(k == 3 and s >= 8 for k, s, _ in mine), mine
        assert any(k == 1 and s > 8 and sl >= 2 for k, s, sl in mine), mine
    assert rides > 0 and first > 0


@pytest.mark.parametrize("dtype", list(fx.DT))
@pytest.mark.parametrize("i", range(len(GEOMS_B)), ids=[fx.gid(g) for g in GEOMS_B])
def test_reduce_job_in_its_three_homes(i, dtype):
    L, lib = _lib()
    geom, dt = GEOMS_B[i], fx.DT[dtype]
    o = fx.operands(geom)
    job = fx.Job(o, dt)
    assert job.rc == 0
    blocks = fx.job_shape(geom, job.splits)[0]
    fails, launches, compared = [], 1, 0
    what = f"B {fx.gid(geom)} {dtype} splits {job.splits}"

    def check_dw(dw, acc, home):
        if not torch.equal(dw.double(), job.want(acc)):
            fails.append(f"{what} {home} accumulate {acc}: {int((dw.double() != job.want(acc)).sum())} of {dw.numel()} differ from fp64")
        return 1

    for acc in (0, 1):
        rc, dw = job.reduce_alone(acc)                                 # home 1
        launches += 1
        assert rc == 0
        compared += check_dw(dw, acc, "reduce_job")
    for cg in _carriers(i, geom):                                      # home 2
        co = fx.operands(cg)
        for form in _carrier_forms(dtype):
            text = fx.describe(cg, fx.ROUTE_DGRAD, fx.route_bits(form, job_blocks=blocks), dt)
            for acc in (0, 1):
                rc, dx, part, dw = fx.dgrad_fused(co, dt, form, job=job, accumulate=acc)
                launches += 1
                home = f"carried by {fx.gid(cg)} {form}"
                if rc != 0:
                    fails.append(f"{what} {home}: rc = {rc}")
                    continue
                compared += check_dw(dw, acc, home)
                compared += fx.check_dgrad(co, dt, form, dx, part, fails, f"{what} {home} (the carrier)",
                                           row_by_row=" parity=1" not in text)
    f = fx.fin_operands(64 + 936 * (i % 2), 7 + 505 * (i % 3 == 0), i, "cuda")             # home 3
    for acc in (0, 1):
        rc, dw, out = job.reduce_with_finalize(acc, f)
        launches += 1
        assert rc == 0
        compared += check_dw(dw, acc, "finalize_wred") + fx.check_finalize(f, out, fails, f"{what} finalize_wred")
    _done(fails, f"B| {fx.gid(geom)} {dtype} splits {job.splits}", launches, compared)


# ------------------------------------------------------------------------------------ C
FIN_SHAPES = [(64, 1), (64, 1024), (256, 512), (1000, 7), (2048, 3)]
WGRAD_SHAPES = {"taps": (2, 64, 64, 3, 1, 16, 8), "tile": (1, 64, 256, 1, 1, 43, 3), "m1": (1, 64, 64, 3, 1, 1, 1)}


@pytest.mark.parametrize("dtype", list(fx.DT))
@pytest.mark.parametrize("fin", FIN_SHAPES, ids=lambda f: f"C{f[0]}_rows{f[1]}")
@pytest.mark.parametrize("shape", list(WGRAD_SHAPES))
def test_finalize_carried_by_the_weight_gradient_is_exact(shape, fin, dtype, monkeypatch):
    """16-bit: the finalize rides in the weight-gradient launch's first workgroups (" fin="), in the tap-fused kernel or the tile
    kernel as CREID_WGRAD_TAPS says; fp32: the kernel has no carrier, the finalize job follows as its own launch (" ; post=fin(")"""
    L, lib = _lib()
    geom, dt = WGRAD_SHAPES[shape], fx.DT[dtype]
    o = fx.operands(geom)
    f = fx.fin_operands(fin[0], fin[1], 0, "cuda")
    fails, launches, compared, routes = [], 0, 0, []
    for sw in ("1", "0"):
        monkeypatch.setenv("CREID_WGRAD_TAPS", sw)
        cw = 4 if fin[0] <= 256 and fin[1] >= 512 else 16
        text = fx.describe(geom, fx.ROUTE_WGRAD, fx.R_JOB | (-(-fin[0] // cw) << 16), dt)
        assert ("wgrad_bf16_taps_kernel" in text) == (shape == "taps" and sw == "1" and dtype != "fp32"), text
        assert (" fin=" in text) == (dtype != "fp32") and (" ; post=fin(" in text) == (dtype == "fp32"), text
        routes.append(text.split(" grid=")[0] + (" fin rides" if " fin=" in text else " fin after"))
        n0 = int(lib.creid_wgrad_taps_launches())
        out = fx.fin_outputs(f)
        job = fx.Job(o, dt, bnfin=(f, out))
        assert job.rc == 0
        assert int(lib.creid_wgrad_taps_launches()) - n0 == (1 if "taps_kernel" in text else 0)
        rc, dw = job.reduce_alone(0)
        assert rc == 0
        launches += 2
        what = f"C {shape} {fx.gid(geom)} {dtype} fin {fin} taps {sw}"
        compared += fx.check_finalize(f, out, fails, what) + 1
        if not torch.equal(dw.double(), job.want(0)):
            fails.append(f"{what}: dw: {int((dw.double() != job.want(0)).sum())} of {dw.numel()} differ from fp64")
    _done(fails, f"C| {shape} {dtype} fin {fin} routes {routes}", launches, compared)


# ------------------------------------------------------------------------------------ D
def _untouched(*tensors):
    return all(t is None or bool(torch.isnan(t.float()).all()) for t in tensors)


def test_refusals_leave_the_outputs_untouched():
    """the return codes of conv_dgrad_check (csrc/conv_igemm.hip) and of a job wred_make_job / wgrad_make_reduce_job turn down
    (CREID_E_SHAPE from the carrying calls), before anything is launched: dx and partial keep their NaN fill, dw its start"""
    L, lib = _lib()
    bf, f32 = torch.bfloat16, torch.float32
    even, odd = fx.operands((2, 256, 64, 1, 1, 16, 8)), fx.operands((3, 64, 64, 3, 1, 7, 5))
    cases = [
        ("bn_stat_image_rows % 128 != 0", fx.E_SHAPE, lambda: fx.dgrad_fused(even, bf, "1_act", image_rows=100)),
        ("compact add on odd extents", fx.E_SHAPE, lambda: fx.dgrad_fused(odd, bf, "compact_add")),
        ("compact add without add_src", fx.E_SHAPE, lambda: fx.dgrad_fused(even, bf, "plain", add_stride=2)),
        ("add_mask with add_src_stride 2", fx.E_ARG, lambda: fx.dgrad_fused(even, bf, "compact_add", force_add_mask=True)),
        ("bn_x in fp32", fx.E_DTYPE, lambda: fx.dgrad_fused(even, f32, "1_act")),
        ("add_mask in fp32", fx.E_ARG, lambda: fx.dgrad_fused(even, f32, "7_addmask_only")),
    ]
    n = 0
    for name, want, run in cases:
        rc, dx, part, _ = run()
        torch.cuda.synchronize()
        assert rc == want, (name, rc, want)
        assert _untouched(dx, part), name
        n += 1
    for dt in (bf, f32):
        job = fx.Job(fx.operands((2, 64, 64, 3, 1, 16, 8)), dt)
        assert job.rc == 0
        big = (1, 1024, 64, 3, 1, 2, 2)                                # K = 9216 > 8192: wred_make_job turns the job down
        nbytes = fx.ws_bytes(big, dt)
        assert nbytes >= 64 * 9216 * 4
        big_job = types.SimpleNamespace(d=fx.desc(big), ws=torch.zeros(nbytes // 4, device="cuda"), nbytes=nbytes,
                                        dw_init=lambda: torch.full((64, 1024, 3, 3), 7.0, device="cuda"))
        f = fx.fin_operands(64, 7, 0, "cuda")
        for name, jb, kw in (("job K > 8192", big_job, {}), ("job workspace too small", job, dict(job_bytes=job.nbytes - 4))):
            rc, dx, part, dw = fx.dgrad_fused(even, dt, "plain" if dt == f32 else "2_mask", job=jb, **kw)
            torch.cuda.synchronize()
            assert rc == fx.E_SHAPE, (name, rc)
            assert _untouched(dx, part) and torch.equal(dw, jb.dw_init()), name
            out, dw = fx.fin_outputs(f), jb.dw_init()
            rc = lib.creid_bn2d_bwd_finalize_wred(
                L.ptr(f.partial), 7, 64, f.count, L.ptr(f.mean), L.ptr(f.invstd), L.ptr(f.gamma), L.ptr(out.sums), L.ptr(out.dgamma),
                L.ptr(out.dbeta), C.byref(jb.d), L.ptr(dw), 0, L.ptr(jb.ws), kw.get("job_bytes", jb.nbytes), L._DT[dt], L.stream())
            torch.cuda.synchronize()
            assert rc == fx.E_SHAPE, (name, rc)
            assert _untouched(out.sums) and torch.equal(dw, jb.dw_init()), name
            assert torch.equal(out.dgamma, f.dgamma0) and torch.equal(out.dbeta, f.dbeta0), name
            n += 2
    print(f"D| {n} refusals")
