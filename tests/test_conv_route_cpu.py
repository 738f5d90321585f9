"""CPU: the convolution dispatch, pinned.  creid_conv_route_describe (csrc/conv_route.hip) runs the route_igemm /
plan_wgrad_route the launchers run and words the result; tests/golden/conv_routes.json holds what the library launched for the
same calls BEFORE the route was a value (recorded with a launch macro that wrote instead of launching: tools/conv_route_dump.py,
profiles/conv_route_refactor.md).  Every geometry x operation x dtype x registry state x knob setting of the sweep must describe
to the recorded kernel instantiation, grid, block, LDS bytes, carried jobs and plan bookkeeping."""
import ctypes as C
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import conv_route_dump as rd  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import centroids_reid_amd._lib as L
    return L.lib()


@pytest.fixture(scope="module")
def gold():
    g = json.load(open(rd.GOLDEN))
    assert g["cases"] == len(rd.cases()) and g["cases_sha1"] == rd.cases_digest(), "the sweep and the recorded table must line up"
    return g


def test_sweep_covers_the_benchmark_network():
    from centroids_reid_amd.bench_train import conv_shapes
    for B, H, W in rd.WORKLOADS:
        for ls in (1, 2):
            assert [g[1:] for g in rd.resnet50_convs(B, H, W, ls)] == conv_shapes(B, H, W, ls)
    geoms = set(rd.geometries())
    assert all((64,) + s in geoms for s in conv_shapes(64, 256, 128)) and all((64,) + s in geoms for s in conv_shapes(64, 320, 320))


def test_recording_has_every_family_and_refusal(gold):
    """what the parent's recording must contain for the comparison to mean something: each kernel family of the forward /
    data-gradient dispatch and of the weight gradient, the 256-row and parity forms, carried and stand-alone jobs, and the
    refusals a public entry point can reach (the N % bn and K % 64 returns of route_igemm are behind check_desc's power-of-two
    channel counts: no descriptor reaches them)"""
    text = "\n".join(gold["shapes"]) + "\n"
    for word in ("conv3x3_c64_kernel<16,", "conv3x3_c64_kernel<32,", "igemm_bf16_pp_kernel<256, 256, 4, 1, 0, 1,", "igemm_bf16_pp_kernel<128, 256,",
                 "igemm1x1_stream_kernel<", "igemm1x1_stream2_kernel<", "igemm_bf16_ws_kernel<128, 3, 256,", "igemm_bf16_ws_kernel<64, 3, 128,",
                 "igemm_bf16_halo_kernel<256,", "igemm_bf16_dma_kernel<64, 5,", "igemm_bf16_kernel<", "igemm_f32_kernel<", " parity=1",
                 " wred=64", "pre=wred(64)", " fin=4", "post=fin(4)", "wgrad_bf16_taps_kernel<8,", "wgrad_bf16_dma_kernel<64, 64, 3, false, 2,",
                 "wgrad_bf16_dma_kernel<128, 128, 2, true, 1,", "wgrad_bf16_kernel<", "wgrad_f32_kernel<", "rc=-1\n", "rc=-2\n", "rc=-4\n"):
        assert word in text, word
    assert any("plan=hit" in v for v in gold["text"].values()) and any("plan=declined" in v for v in gold["text"].values())


def test_default_and_per_call_knob_routes_match_the_recording(lib, gold):
    """the default and every knob that is read per call (CREID_DEBUG_KNOBS=1: tests/conftest.py), in this process"""
    got = {"default": rd.run_setting(rd.load(), {})}
    for s in rd.LIVE:
        got[rd.setting_name(s)] = rd.run_setting(rd.load(), s)
    bad = rd.compare(got, gold)
    assert not bad, f"{len(bad)} groups of routes differ from the recording, first:\n" + "\n".join(bad[:10])
    assert set(rd.shapes(got)) <= set(gold["shapes"])
    moved = json.loads(json.dumps(gold))
    moved["default"]["plans"]["dgrad f16"] = "0" * 12              # (the comparison does see a group that moved)
    assert len(rd.compare({"default": got["default"]}, moved)) == 1


@pytest.mark.parametrize("setting", rd.ONCE, ids=rd.setting_name)
def test_read_once_knob_routes_match_the_recording(lib, gold, setting):
    """a knob that is read once per process: a subprocess of its own, without CREID_DEBUG_KNOBS (production reading)"""
    name = rd.setting_name(setting)
    got = {name: rd.run_once_setting(setting)}
    bad = rd.compare(got, gold)
    assert not bad, f"{len(bad)} groups of routes differ from the recording, first:\n" + "\n".join(bad[:10])
    assert set(rd.shapes(got)) <= set(gold["shapes"])


def test_workspace_bytes_is_the_described_split_count(lib):
    """creid_conv2d_wgrad_workspace_bytes = splits x out_c x K x 4 of the route the weight gradient would take, with the shipped
    plans and without, tap-fused route on and off"""
    h = rd.load()
    n = 0
    try:
        for plans in (True, False):
            rd.register_plans(h, plans)
            for taps in ("1", "0"):
                os.environ["CREID_WGRAD_TAPS"] = taps
                for g in rd.geometries():
                    for dt in rd.DTYPES.values():
                        line = rd.describe(h, g, rd.WGRAD, 0, dt)
                        m = re.search(r" splits=(\d+) ", line)
                        if m is None:
                            assert line.startswith("rc="), line
                            continue
                        d = rd.desc(*g)
                        assert h.creid_conv2d_wgrad_workspace_bytes(C.byref(d), dt) == int(m.group(1)) * g[2] * g[3] * g[3] * g[1] * 4, (g, dt, line)
                        n += 1
    finally:
        os.environ.pop("CREID_WGRAD_TAPS", None)
        rd.register_plans(h, True)
    assert n > 1000


def test_describe_leaves_the_registry_counters_alone(lib):
    h = rd.load()
    rd.register_plans(h, True)
    keys = [(int(e["kind"]), *[int(v) for v in e["key"]]) for e in json.load(open(rd.PLANS))["plans"]]
    count = lambda: [h.creid_tune_count(*k, w) for k in keys for w in (0, 1)]
    before = count()
    assert min(before) >= 0
    lines = [rd.describe(h, g, op, bits, dt) for (_, g, op, bits, dt) in rd.cases()]
    assert sum("plan=hit" in s for s in lines) > 100 and count() == before
