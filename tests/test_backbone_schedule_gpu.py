"""GPU: the C entry points the backbone engine calls, in order.  tests/golden/backbone_launch_trace.json holds the ordered names
of two training forward + backward rounds (ResNet50 in bf16 / f16 / fp32 / bf16x3, ResNet50-IBN-a and ResNet18 in bf16) and of one
eval forward (ResNet50 in bf16 / fp32 / bf16x3, ResNet50-IBN-a in bf16) at B = 4, 128 x 64, under the default schedule and under
every retained switch at its non-default values -- recorded on an MI355X BEFORE the engine kept its schedule as one value, when
it still carried the side-stream and ablation branches (tools/backbone_schedule_dump.py, profiles/backbone_schedule_refactor.md).
The tests that wrap _wgrad / _dgrad / _bn_bwd pin the Python-level order; this pins what reaches the library.

tests/golden/backbone_launch_args.json holds, for the same runs, what the names cannot show (a pointer that silently became null
keeps every name): per call every scalar argument by value, every convolution descriptor by its fields and every pointer as
null / non-null, and per case an order-independent integer checksum of the features, every parameter gradient and every
BatchNorm running statistic -- in full for the default schedule, as one SHA-256 per case for every other setting.  Recorded
BEFORE the engine kept its saved step state as records, twice in separate processes with byte-identical files
(profiles/backbone_saved_state_refactor.md).  Each setting is traced once; both comparisons read that trace."""
import functools
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


@pytest.fixture(scope="module")
def golden_args():
    with open(sd.GOLDEN_ARGS) as f:
        doc = json.load(f)
    assert doc["shape"] == [sd.B, sd.H, sd.W]
    return sd.expand_args(doc)


@functools.lru_cache(maxsize=None)
def _traced(name):
    """{case: {"names", "args" (sd.digest_case), ...}} of one in-process setting, traced once for the name and the argument test"""
    return sd.trace_setting(next(s for s in IN_PROCESS if sd.setting_name(s) == name), args=True)


@functools.lru_cache(maxsize=None)
def _traced_dma0():
    """CREID_IGEMM_DMA=0 and its pairs: the library reads that variable once per process, so these run in a child process"""
    env = {k: v for k, v in os.environ.items() if k not in sd.SWITCHES}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "backbone_schedule_dump.py"), "trace", "--group", "dma0", "--args"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0
    got = json.loads(r.stdout.splitlines()[-1])
    assert len(got) == (len(sd.SETTINGS) - len(IN_PROCESS)) * (len(sd.TRAIN_CASES) + len(sd.EVAL_CASES))
    return got


def _names_of(traced):
    return {k: {f: v for f, v in t.items() if f != "args"} for k, t in traced.items()}


def _compare_args(traced, golden_args):
    bad = [d for d in (sd.args_difference(k, t["args"], golden_args[k]) for k, t in traced.items()) if d]
    assert not bad, f"{len(bad)} of {len(traced)} cases differ from the recorded arguments / checksums:\n" + "\n".join(bad)


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
    _compare(_names_of(_traced(sd.setting_name(setting))), golden)


def test_launch_traces_on_the_register_staged_kernels(golden):
    _compare(_names_of(_traced_dma0()), golden)


def test_the_argument_fixture_covers_every_case_of_every_setting(golden_args):
    n = len(sd.TRAIN_CASES) + len(sd.EVAL_CASES)
    assert len(golden_args) == n * len(sd.SETTINGS)
    full = {k: v for k, v in golden_args.items() if k.endswith("| default")}
    assert len(full) == n and all(v["calls"] and "feat" in v["sums"] for v in full.values())
    assert all(("sha256" in v) != ("error" in v) for k, v in golden_args.items() if k not in full)
    for kind, arch, dtype in (("train", "resnet50", "bfloat16"), ("train", "resnet50", "float32")):
        sums = full[f"{kind} {arch} {dtype} | default"]["sums"]
        assert sum(k.startswith("grad ") and k.endswith(("conv1.weight", "conv2.weight", "conv3.weight", "downsample.0.weight"))
                   for k in sums) == 53, "every convolution weight gradient is part of the checksums"


@pytest.mark.parametrize("setting", IN_PROCESS, ids=[sd.setting_name(s) for s in IN_PROCESS])
def test_launch_arguments_and_results_equal_the_recorded_ones(setting, golden_args):
    """in a default row a mismatch names the first differing call and argument slot, or the first tensor whose checksum differs"""
    _compare_args(_traced(sd.setting_name(setting)), golden_args)


def test_launch_arguments_and_results_on_the_register_staged_kernels(golden_args):
    _compare_args(_traced_dma0(), golden_args)
