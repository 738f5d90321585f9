"""The convolution kernels (csrc/conv_igemm.hip, conv_pipe.hip, conv_stream.hip, conv_wgrad.hip and the routing of launch_igemm /
plan_wgrad_route) checked EXACTLY against fp64 (tests/conv_exact.py: operands in {-2..2}, every result an exact integer, 16-bit
outputs the one correctly rounded value) at the geometries where an implicit-GEMM gather usually breaks and that no network of
the benchmark produces: odd extents, stride 2 over odd extents, maps smaller than the 3 x 3 footprint, one-pixel-wide and
one-pixel-high images, M = 1, a 128-row tile that spans many images, M just past a tile boundary.

  A  the built-in routing as shipped (plans registered, no key collides with one): bf16, f16 and fp32;
  B  the special kernels forced with their per-call knobs at the edges of what they cover -- B1 the persistent kernel of
     conv_pipe.hip (three tile forms, default grid and three workgroups), B2 the two persistent 1 x 1 kernels of conv_stream.hip
     (two workgroups walking all the tiles, the last one partial), B3 the 3 x 3 64 -> 64 kernel at its two tilings and at near
     misses that must fall through;
  C  a production plan key under a foreign image factorisation (B = 2048 images of 2 x 2 share M, N, K and mode with the
     B = 64, 16 x 8 layer): the production plan is looked up (counted) and each kernel's own coverage check has to decline or
     gather correctly.

Per geometry: forward with statistics (the last partial tile zero-padded: rows beyond M contribute nothing), folded-affine
forward plain and with residual + ReLU, data gradient with and without add_src, weight gradient plain and accumulating.  Where
the library counts a route (creid_igemm_halo_launches, creid_wgrad_taps_launches) each launch must run it exactly where the
mirrored coverage rule (tests/test_igemm_halo_cpu.py, tests/test_wgrad_taps_cpu.py) says so; the pipe, stream and c64 kernels
have no counter: the exact comparison holds on whichever kernel ran.  Counts and the measured run time:
profiles/conv_edge_sweep.md."""
import pytest
import torch

import conv_exact as ce
import test_igemm_halo_cpu as hc
import test_wgrad_taps_cpu as tc

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "fp32": torch.float32}


def _gid(g):
    B, cin, cout, k, s, h, w = g
    return f"B{B}_{cin}to{cout}_k{k}s{s}_{h}x{w}"


def route_rule(geom, dtype, c64_on=True):
    """f(launch name) -> (halo kernel must run, tap-fused weight gradient must run) for the built-in rules and every shipped plan
    word except the 4-deep 128-column ring at 256 channels (the one (tile, depth) igemm_halo_covers refuses for LDS; no geometry
    of this file that the halo kernel covers has such a plan)."""
    B, cin, cout, k, s, h, w = geom
    oh, ow = ce.out_hw(k, s, h, w)
    is16 = dtype != torch.float32
    fwd_halo = hc.halo_covers(cin, k, s, k // 2, oh, ow, h, w, B * oh * ow, 64, 2, is16)
    # (the transposed gather: rows are input pixels, channels per tap = cout)
    dgrad_halo = hc.halo_covers(cout, k, s, k // 2, h, w, oh, ow, B * h * w, 64, 2, is16)
    taps = tc.covers(cin, cout, k, s, k // 2, oh, ow, h, w, B * oh * ow, is16)
    c64 = c64_on and is16 and (cin, cout, k, s) == (64, 64, 3, 1) and ce.c64_covers(oh, ow)

    def rule(name):
        if name.startswith("wgrad"):
            return False, taps
        if name.startswith("dgrad"):
            return dgrad_halo, False
        if name in ("fwd", "aff_plain") and c64:              # conv3x3_c64_kernel runs ahead of the tile kernels
            return False, False
        return fwd_halo, False
    return rule


def _run(geom, dtype, monkeypatch, route=True, plans_on=True, strict=True, rules_too=False, what=""):
    from centroids_reid_amd import _lib as L
    L.lib()
    assert L.N_PLANS == len(ce.PLANS), "the shipped plan file must be registered"
    B, shape = geom[0], tuple(geom[1:])
    sw = ce.Sweep(dtype, plans_on and dtype != torch.float32, strict=strict, expect_route=route_rule(geom, dtype) if route else None)
    ce.run_geometry(sw, B, shape, None, monkeypatch, rules_too=rules_too)
    ce.assert_clean(sw, f"{what} {_gid(geom)} {dtype}")
    assert sw.compared >= 9
    print(f"{what}| {_gid(geom)} {dtype}: {sw.launches} launches, {sw.compared} comparisons, {sw.routes_confirmed} routes confirmed")
    return sw


# ------------------------------------------------------------------------------------ A: built-in routing
GROUP_A = [
    (1, 64, 64, 3, 1, 1, 1),            # M = 1; eight of nine taps are padding
    (1, 64, 64, 1, 1, 1, 1),            # ... and the 1 x 1 GEMM of one row
    (1, 64, 128, 3, 2, 1, 1),           # stride 2 on a single pixel
    (2, 64, 64, 3, 1, 2, 2),            # a map under the 3 x 3 footprint: no pixel has all nine taps
    (1, 64, 128, 3, 2, 2, 2),           # stride 2 from 2 x 2 to one pixel: the bottom / right taps are read, the top / left are padding
    (3, 64, 64, 3, 1, 7, 5),            # odd extents; M = 105 in one partial tile; image borders inside a tile
    (3, 128, 64, 3, 2, 7, 5),           # stride 2 over odd extents, output 4 x 3
    (2, 64, 128, 3, 2, 8, 6),           # stride 2 over even extents; bottom and right padding never read (the asymmetric case)
    (5, 256, 64, 1, 2, 9, 7),           # 1 x 1 stride 2 on odd extents, M = 100
    (2, 256, 64, 1, 2, 8, 6),           # ... and on even extents: the last input row and column are never read
    (1, 64, 256, 1, 1, 43, 3),          # M = 129, one row past a tile
    (1, 64, 256, 1, 1, 32, 4),          # M = 128, exactly one tile
    (1, 64, 256, 1, 1, 127, 1),         # M = 127, one row short of a tile
    (1, 128, 128, 3, 1, 127, 1),        # one-pixel-wide image; left and right taps all padding
    (1, 128, 128, 3, 1, 1, 130),        # one-pixel-high image
    (2, 512, 64, 3, 1, 3, 3),           # K = 4608 on a 3 x 3 map
    (17, 64, 64, 3, 1, 5, 3),           # M = 255; more than eight images per tile
    (1, 64, 128, 3, 2, 32, 16),         # eligible for the parity-class stride-2 data gradient, H != W
    (3, 64, 128, 3, 2, 32, 16),         # ... odd B
    (1, 64, 128, 3, 2, 34, 16),         # just ineligible: (M / 4) % 128 != 0
    (2, 64, 128, 3, 2, 15, 17),         # just ineligible: odd extents
]


@pytest.mark.parametrize("dtype", list(DT), ids=list(DT))
@pytest.mark.parametrize("geom", GROUP_A, ids=_gid)
def test_built_in_routing_is_exact(geom, dtype, monkeypatch):
    keys = ce.plan_keys(*geom)
    assert not any(k in ce.PLANS for k in keys.values()), "a group A geometry must not collide with a shipped plan"
    sw = _run(geom, DT[dtype], monkeypatch, what="A")
    assert sw.routes_confirmed >= 7          # none of these shapes is covered by the halo or tap-fused kernels: asserted per launch


# ------------------------------------------------------------------------------------ B1: persistent kernel of conv_pipe.hip
def vword(bm, bn, kph, mode):
    return (bm // 128) | ((bn // 128) << 2) | (kph << 4) | (mode << 8)


PIPE_VARIANTS = {"128x128pp": vword(128, 128, 1, 0), "128x256": vword(128, 256, 2, 0), "256x256free": vword(256, 256, 1, 2)}
PIPE_GEOMS = [(3, 64, 256, 3, 1, 7, 5), (3, 128, 256, 3, 2, 7, 5), (5, 256, 256, 1, 2, 9, 7), (1, 64, 256, 1, 1, 43, 3),
              (1, 128, 256, 3, 1, 127, 1)]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("wgs", [0, 3], ids=["grid", "wgs3"])
@pytest.mark.parametrize("variant", list(PIPE_VARIANTS), ids=list(PIPE_VARIANTS))
@pytest.mark.parametrize("geom", PIPE_GEOMS, ids=_gid)
def test_pipe_kernel_is_exact_at_the_edges(geom, variant, wgs, dtype, monkeypatch):
    """CREID_IGEMM_PP = 0x1000 | variant: every 16-bit launch the kernel covers (forward forms at 256 output channels; the data
    gradient where its N = cin divides by the column tile) runs it, the others fall through to the tile kernels."""
    monkeypatch.setenv("CREID_IGEMM_PP", hex(0x1000 | PIPE_VARIANTS[variant]))
    if wgs:
        monkeypatch.setenv("CREID_PP_WGS", str(wgs))
    _run(geom, DT[dtype], monkeypatch, what=f"B1 {variant} wgs {wgs}")


# ------------------------------------------------------------------------------------ B2: persistent 1 x 1 kernels of conv_stream.hip
STREAM_IMAGES = {1: (1, 1, 1), 105: (3, 7, 5), 129: (1, 43, 3), 255: (17, 5, 3)}          # M -> (B, h, w)
STREAM_CHANNELS = [(64, 256), (128, 128), (256, 64), (256, 512)]                          # K -> N: 256-, 128- and 64-column slabs
STREAM_GEOMS = [(b, k, n, 1, 1, h, w) for (k, n) in STREAM_CHANNELS for (b, h, w) in STREAM_IMAGES.values()]


@pytest.mark.parametrize("form", ["stream1x1_bf16", "stream2_bf16", "stream2_f16"])
@pytest.mark.parametrize("geom", STREAM_GEOMS, ids=_gid)
def test_stream_kernels_are_exact_at_the_edges(geom, form, monkeypatch):
    """CREID_STREAM1X1=1 (bf16, statistics / plain epilogue) and CREID_STREAM2=1 (both dtypes, also the folded-affine epilogues
    with and without residual), two workgroups (CREID_STREAM1X1_WGS=2): one workgroup walks several tiles and ends on the partial
    one."""
    knob, dtype = form.rsplit("_", 1)
    monkeypatch.setenv("CREID_STREAM1X1" if knob == "stream1x1" else "CREID_STREAM2", "1")
    monkeypatch.setenv("CREID_STREAM1X1_WGS", "2")
    _run(geom, DT[dtype], monkeypatch, what=f"B2 {form}")


# ------------------------------------------------------------------------------------ B3: the 3 x 3 64 -> 64 kernel
C64_COVERED = [(8, 16), (8, 48), (4, 32), (2, 64), (16, 80)]
C64_NEAR = [(12, 16), (8, 24), (3, 32)]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("wgs", [0, 2], ids=["grid", "wgs2"])
@pytest.mark.parametrize("hw", C64_COVERED + C64_NEAR, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_c64_kernel_is_exact_at_the_edges_of_its_tilings(hw, wgs, dtype, monkeypatch):
    """Three images (image borders between tiles, an odd count) of each covered shape -- 16 x 8 blocks (W % 16 == 0, H % 8 == 0:
    8 x 16, 8 x 48, 16 x 80) and whole 128-pixel row blocks (W = 32, 64: 4 x 32, 2 x 64) -- and of the near misses, which must
    fall through to the tile kernels; with the default grid and with two workgroups walking runs of tiles across the image
    boundaries (CREID_STREAM1X1_WGS=2).  Statistics per image where the c64 kernel runs (its rows are 16 x 8 blocks), per
    128-pixel tile elsewhere; run_geometry also runs the forward forms with CREID_C64_3X3=0."""
    assert ce.c64_covers(*hw) == (hw in C64_COVERED)
    if wgs:
        monkeypatch.setenv("CREID_STREAM1X1_WGS", str(wgs))
    sw = _run((3, 64, 64, 3, 1) + hw, DT[dtype], monkeypatch, what="B3")
    assert sw.routes_confirmed >= 9


# ------------------------------------------------------------------------------------ C: production key, foreign image
FOREIGN_M8192 = [(2048, 2, 2), (8192, 1, 1), (64, 4, 32), (64, 32, 4), (1, 64, 128), (1, 128, 64)]
GROUP_C = ([((64, c, c, 3, 1, 16, 8), (b, c, c, 3, 1, h, w)) for c in (256, 512) for (b, h, w) in FOREIGN_M8192] +
           [((64, 512, 1024, 1, 2, 32, 16), (64, 512, 1024, 1, 2, 31, 15)),
            ((64, 128, 128, 3, 2, 64, 32), (64, 128, 128, 3, 2, 63, 31))])


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("prod,geom", GROUP_C, ids=[_gid(g) for _, g in GROUP_C])
def test_production_key_with_a_foreign_image_is_exact(prod, geom, dtype, monkeypatch):
    """The geometry shares plan keys with a layer of the B = 64, 256 x 128 workload (checked against tuned_plans.json), so its
    launches get that layer's plans: every shared key with a plan must show a counted lookup, applied or declined, and every
    output must still be exact -- with the plans and with the registry cleared."""
    from centroids_reid_amd.bench_train import conv_plan_keys
    prod_keys = [keys for ls in (1, 2) for shape, keys in conv_plan_keys(prod[0], 256, 128, ls) if shape == tuple(prod[1:])]
    assert prod_keys, "the production layer must be a convolution of the B = 64, 256 x 128 workload"
    mine = ce.plan_keys(*geom)
    shared = {k for k in mine.values() if k in prod_keys[0].values() and k in ce.PLANS}
    assert shared, "no key with a shipped plan is shared: this case produces no collision"
    assert geom[1:] != prod[1:] or geom[0] != prod[0]
    sw = _run(geom, DT[dtype], monkeypatch, strict=False, rules_too=True, what="C")
    assert shared <= sw.looked_up, f"plans never looked up: {sorted(shared - sw.looked_up)}"
    assert shared <= (sw.applied | sw.declined)
    print(f"C {_gid(geom)} {dtype}: applied {sorted(sw.applied)} declined {sorted(sw.declined)}")
