"""GPU: the C entry points the backbone engine calls, in order.  tests/golden/backbone_launch_trace.json holds the ordered names
of two training forward + backward rounds (ResNet50 in bf16 / f16 / fp32 / bf16x3, ResNet50-IBN-a and ResNet18 in bf16) and of one
eval forward (ResNet50 in bf16 / fp32 / bf16x3, ResNet50-IBN-a in bf16) at B = 4, 128 x 64, under the default schedule and under
every retained switch at its non-default values -- recorded on an MI355X BEFORE the engine kept its schedule as one value, when
it still carried the side-stream and ablation branches (tools/backbone_schedule_dump.py, profiles/backbone_schedule_refactor.md).
The tests that wrap _wgrad / _dgrad / _bn_bwd pin the Python-level order; this pins what reaches the library."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import backbone_schedule_dump as sd  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(sd.GOLDEN_TRACE) as f:
        doc = json.load(f)
    assert doc["shape"] == [sd.B, sd.H, sd.W]
    yield sd.expand_traces(doc)
    sd._NETS.clear()


def _compare(got, golden):
    for key, t in got.items():
        ref = golden[key]
        if t != ref and "names" in t and "names" in ref:
            i = next((i for i, (a, b) in enumerate(zip(t["names"], ref["names"])) if a != b), min(len(t["names"]), len(ref["names"])))
            raise AssertionError(f"{key}: call {i} is {t['names'][i:i + 3]}, recorded {ref['names'][i:i + 3]} "
                                 f"({len(t['names'])} calls, recorded {len(ref['names'])})")
        assert t == ref, key


IN_PROCESS = [s for s in sd.SETTINGS if sd.group_of(s) == "dma1"]


def test_the_fixture_covers_every_case_of_every_setting(golden):
    n = len(sd.TRAIN_CASES) + len(sd.EVAL_CASES)
    assert len(golden) == n * len(sd.SETTINGS)
    base = {k.split(" | ")[0]: v for k, v in golden.items() if k.endswith("| default")}
    assert len(base) == n and all("names" in v for v in base.values())
    for s in sd.SETTINGS:                  # every setting but the row-block count (an argument, not a route) changes some trace
        if s and set(s) != {"CREID_FIN_APPLY_RB"}:
            assert any(v != base[k.split(" | ")[0]] for k, v in golden.items() if k.endswith("| " + sd.setting_name(s))), s


@pytest.mark.parametrize("setting", IN_PROCESS, ids=[sd.setting_name(s) for s in IN_PROCESS])
def test_launch_trace_equals_the_recorded_one(setting, golden):
    _compare(sd.trace_setting(setting), golden)


def test_launch_traces_on_the_register_staged_kernels(golden):
    """CREID_IGEMM_DMA=0 and its pairs: the library reads that variable once per process, so these run in a child process"""
    env = {k: v for k, v in os.environ.items() if k not in sd.SWITCHES}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "backbone_schedule_dump.py"), "trace", "--group", "dma0"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0
    got = json.loads(r.stdout.splitlines()[-1])
    assert len(got) == (len(sd.SETTINGS) - len(IN_PROCESS)) * (len(sd.TRAIN_CASES) + len(sd.EVAL_CASES))
    _compare(got, golden)
