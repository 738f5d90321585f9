"""CPU: every launch plan of centroids-reid_amd/tuned_plans.json belongs to a convolution of the workloads it was measured for.

A plan is looked up by an exact (kind, M, N, K, mode) key; bench_train.conv_plan_keys derives the keys each ResNet50 convolution
looks up.  tests/test_plan_sweep_gpu.py checks the plans bit for bit through exactly those geometries, so an entry no geometry
reaches would ship untested (and a plan the launches never ask for would never run)."""
import json
import os

import pytest

from centroids_reid_amd.bench_train import PLAN_WORKLOADS, conv_plan_keys

PLANS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "centroids-reid_amd", "tuned_plans.json")


def plan_geometries():
    """{(B, H, W, last_stride, shape): keys} over PLAN_WORKLOADS."""
    out = {}
    for (H, W), batches in PLAN_WORKLOADS.items():
        for B in batches:
            for ls in (1, 2):
                for shape, keys in conv_plan_keys(B, H, W, ls):
                    out[(B, H, W, ls, shape)] = keys
    return out


def unreached(entries, geoms):
    reached = {k for keys in geoms.values() for k in keys.values()}
    return [e for e in entries if (e["kind"], *e["key"]) not in reached]


def test_every_shipped_plan_is_reached_by_a_workload_geometry():
    entries = json.load(open(PLANS))["plans"]
    geoms = plan_geometries()
    keys = [(e["kind"], *e["key"]) for e in entries]
    assert len(set(keys)) == len(keys), "duplicate plan keys"
    missing = unreached(entries, geoms)
    assert not missing, f"{len(missing)} plan(s) no workload geometry looks up: {missing[:5]}"
    # the check bites: a plan for a batch size no workload runs is reported
    fake = dict(entries[0], key=[entries[0]["key"][0] + 128] + entries[0]["key"][1:])
    assert unreached(entries + [fake], geoms) == [fake]


@pytest.mark.parametrize("B,H,W,ls", [(64, 256, 128, 1), (56, 320, 320, 2)])
def test_conv_plan_keys_follow_the_launch_geometry(B, H, W, ls):
    """The keys are the GEMMs conv_igemm.hip / conv_wgrad.hip launch: forward rows = output pixels, data-gradient rows = input
    pixels with N = in_c and K = out_c * k^2; mode = transposed | stride << 1 (| 8: eval-mode twin of the forward).
    This restates the derivation on the Python side only; that it matches what the C launches look up is shown on the GPU by
    the registry counters (tests/test_plan_sweep_gpu.py)."""
    for (cin, cout, k, s, h, w), keys in conv_plan_keys(B, H, W, ls):
        oh, ow = (h - 1) // s + 1, (w - 1) // s + 1            # 3x3 pad 1 and 1x1 pad 0 alike
        assert keys["fwd"] == (1, B * oh * ow, cout, cin * k * k, 2 * s)
        assert keys["fwd_eval"] == keys["fwd"][:4] + (2 * s | 8,)
        assert keys["dgrad"] == (1, B * h * w, cin, cout * k * k, 2 * s | 1)
        assert keys["wgrad"] == (0,) + keys["fwd"][1:]
        assert max(keys["fwd"][1], keys["dgrad"][1]) < 1 << 24          # the registry's M is an int on the C side
