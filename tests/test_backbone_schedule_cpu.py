"""CPU: the backbone engine's schedule as a value.  backbone.resolve_schedule reads every schedule switch once and applies every
rule that ties two of them together; tests/golden/backbone_schedule.json holds what BackboneEngine.__init__ resolved for the same
{dtype} x {arch} x {environment} rows BEFORE the Schedule value existed, when it read the variables inline into loose attributes
(recorded with tools/backbone_schedule_dump.py at that commit: profiles/backbone_schedule_refactor.md)."""
import dataclasses
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import backbone_schedule_dump as sd  # noqa: E402


@pytest.fixture(scope="module")
def bb():
    import __graft_entry__ as ge
    ge.build()
    from centroids_reid_amd import backbone
    return backbone


@pytest.fixture(scope="module")
def golden():
    with open(sd.GOLDEN_RESOLVE) as f:
        doc = json.load(f)
    assert doc["fields"] == list(sd.FIELDS) and doc["settings"] == [sd.setting_name(s) for s in sd.SETTINGS]
    return sd.expand_rows(doc)


def test_engines_resolve_to_the_recorded_schedules(bb, golden):
    """every row through the engine's constructor, the refusals with their text"""
    rows = sd.resolve_rows()
    assert len(rows) == len(golden) == len(sd.SETTINGS) * len(sd.DTYPES) * len(sd.ARCHS)
    for ref, got in zip(golden, rows):
        assert got == ref, (ref, got)
    assert [f.name for f in dataclasses.fields(bb.Schedule)] == list(sd.FIELDS)


def _env_of(name):
    return {} if name == "default" else dict(kv.split("=", 1) for kv in name.split(" "))


class _CountingEnv(dict):
    def __init__(self, *a):
        super().__init__(*a)
        self.reads = []

    def get(self, k, default=None):
        self.reads.append(k)
        return super().get(k, default)


def test_resolve_schedule_takes_the_environment_as_a_value(bb, golden, monkeypatch):
    """the same rows through resolve_schedule(env=...), with the process environment saying the opposite of every default: it must
    not be consulted.  Each variable is read once."""
    for k, (default, vals) in sd.SWITCHES.items():
        monkeypatch.setenv(k, vals[0])
    n = 0
    for row in golden:
        if row["arch"] != "resnet50" or ("error" in row and "float16" not in row["error"]):
            continue                       # (no rule looks at the architecture; the BasicBlock refusal is the constructor's)
        x3 = row["dtype"].startswith("bf16x3")
        dtype = torch.float32 if x3 else getattr(torch, row["dtype"])
        env = _CountingEnv(_env_of(row["env"]))
        if "error" in row:
            from centroids_reid_amd import _lib
            with pytest.raises(_lib.CreidError, match="float16 needs the LDS-DMA"):
                bb.resolve_schedule(dtype, None, False, env=env)
            continue
        s = bb.resolve_schedule(dtype, "bf16x3" if x3 else None, row["dtype"].endswith("-train"), env=env)
        got = {k: sorted(v) if isinstance(v, frozenset) else v for k, v in dataclasses.asdict(s).items()}
        assert got == row["sched"], row
        assert len(env.reads) == len(set(env.reads)), env.reads
        retired = {k for k, _ in bb.RETIRED_SWITCHES}
        assert set(env.reads) - retired <= set(sd.SWITCHES) and retired <= set(env.reads)
        if row["dtype"] == "bfloat16" and row["env"] == "default":
            assert set(env.reads) - retired == set(sd.SWITCHES)          # the retained switches, all of them, and nothing else
        n += 1
    assert n >= 4 * len(sd.SETTINGS)


def test_every_retained_switch_is_covered_at_a_non_default_value(golden):
    """each switch at each of its non-default values is a row of the table, and resolves at least one engine differently from the
    defaults (or refuses it)"""
    default = {(r["dtype"], r["arch"]): r for r in golden if r["env"] == "default"}
    for k, (dflt, vals) in sd.SWITCHES.items():
        assert vals and dflt not in vals, k
        for v in vals:
            rows = [r for r in golden if r["env"] == f"{k}={v}"]
            assert len(rows) == len(sd.DTYPES) * len(sd.ARCHS), (k, v)
            if k == "CREID_C3_AXF" and v == "":
                assert any(r.get("sched", {}).get("c3_axf") == [] for r in rows)
            assert any({a: b for a, b in r.items() if a != "env"} != {a: b for a, b in default[(r["dtype"], r["arch"])].items() if a != "env"}
                       for r in rows), (k, v)


def test_a_retired_switch_raises(bb, monkeypatch):
    from centroids_reid_amd import _lib
    assert len(bb.RETIRED_SWITCHES) == 8
    net = bb.build_backbone("resnet18", 1)
    for name, default in bb.RETIRED_SWITCHES:
        other = "0" if default != "0" else "1"
        with pytest.raises(_lib.CreidError, match=name + r"=.*docs/history/"):
            bb.resolve_schedule(torch.bfloat16, env={name: other})
        bb.resolve_schedule(torch.bfloat16, env={name: default})       # spelled out at its default: nothing was flipped
        monkeypatch.setenv(name, other)
        with pytest.raises(_lib.CreidError, match=name):
            bb.BackboneEngine(net, torch.float32)
        monkeypatch.delenv(name)
    bb.BackboneEngine(net, torch.float32)


def test_the_environment_is_read_in_one_place(bb):
    with open(bb.__file__) as f:
        src = f.read()
    assert src.count("os.environ") == 1 and "env=os.environ" in src
    assert os.path.exists(os.path.join(ROOT, "docs", "history", "backbone_schedule_switches.md"))
