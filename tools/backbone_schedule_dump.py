#!/usr/bin/env python3
"""What the backbone engine decides and what it launches, as tables that a refactor of the engine can be held against.

    python tools/backbone_schedule_dump.py resolve            # compare the resolved schedules with the golden table (no GPU)
    python tools/backbone_schedule_dump.py resolve --write    # ... or write tests/golden/backbone_schedule.json
    python tools/backbone_schedule_dump.py trace              # compare the C-level launch order with the golden (one GPU)
    python tools/backbone_schedule_dump.py trace --write      # ... or write tests/golden/backbone_launch_trace.json
    python tools/backbone_schedule_dump.py trace --args       # compare every call's arguments and the results' checksums (one GPU)
    python tools/backbone_schedule_dump.py trace --args --write   # ... or write tests/golden/backbone_launch_args.json

The tool sets switches through environment variables only, before it constructs a BackboneEngine, and reads only the engine's
schedule attributes (`eng.sched.<field>` where the engine keeps a Schedule value, `eng.<field>` where it keeps loose
attributes) and the names of the C entry points the engine calls.  It therefore runs unchanged on a commit from before the
Schedule value existed: both golden files were written there (profiles/backbone_schedule_refactor.md).

resolve: {bfloat16, float16, float32, "bf16x3", "bf16x3" trainable} x {resnet50, resnet50_ibn_a, resnet18} x SETTINGS, engines
on CPU parameter holders.  A combination the constructor rejects is recorded with the text of the rejection.

trace: one training forward + backward (twice, so the rotating workspaces wrap) or one eval forward at B = 4, 128 x 64 per
TRAIN_CASES / EVAL_CASES x SETTINGS, through a proxy of the library handle that keeps the ordered entry-point names (host-side
size queries included).  The library reads CREID_IGEMM_DMA once per process, so the settings that carry it run in a child
process of their own (`--group dma0`).  Distinct name sequences are stored once, as indices into one name table.

trace --args: the same runs, and per call through the proxy every scalar argument by value (floats by repr), every ConvDesc
passed by reference as its field tuple, every pointer as null / non-null ("p"); per case an integer checksum, computed on the
device, of `feat`, every parameter gradient and every BatchNorm running statistic after the two rounds: the tensor viewed as int32,
widened to int64, summed plainly and weighted by 1-based index (wrap-around integer sums: independent of the reduction order).
The `default` rows are stored in full (distinct calls once, as indices into one call table); every other row as one SHA-256 of
its canonical call list and checksums."""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN_RESOLVE = os.path.join(ROOT, "tests", "golden", "backbone_schedule.json")
GOLDEN_TRACE = os.path.join(ROOT, "tests", "golden", "backbone_launch_trace.json")
GOLDEN_ARGS = os.path.join(ROOT, "tests", "golden", "backbone_launch_args.json")

# every schedule switch the engine keeps: name -> (default, the non-default values the tables cover)
SWITCHES = {
    "CREID_RELU_BITMASK": ("1", ("0",)), "CREID_STEM_FUSE": ("1", ("0",)), "CREID_STEM_POOL": ("1", ("0",)),
    "CREID_PAIR_FUSE": ("1", ("0",)), "CREID_STEM_FUSE_BWD": ("0", ("1",)), "CREID_DROP_GM": ("1", ("0",)),
    "CREID_FUSE_BN_REDUCE": ("1", ("0",)), "CREID_EVAL_FOLD": ("1", ("0",)), "CREID_C3_AXF": ("64,128", ("", "64", "128")),
    "CREID_DS_REDUCE2": ("1", ("0",)), "CREID_DUAL_APPLY": ("1", ("0",)), "CREID_FIN_APPLY": ("64", ("0", "16")),
    "CREID_FIN_APPLY_RB": ("64", ("0", "16")), "CREID_WRED_PIGGYBACK": ("1", ("0",)), "CREID_FIN_CARRIER": ("wgrad", ("wred", "none")),
    "CREID_HEADS_BNRED": ("1", ("0",)), "CREID_IGEMM_DMA": ("1", ("0",)),
}
SETTINGS = ([{}] + [{k: v} for k, (_, vals) in SWITCHES.items() for v in vals] +
            [{"CREID_WRED_PIGGYBACK": "0", "CREID_FIN_CARRIER": v} for v in ("wgrad", "wred", "none")] +
            [{"CREID_IGEMM_DMA": "0", k: v} for k in ("CREID_FUSE_BN_REDUCE", "CREID_EVAL_FOLD") for v in ("0", "1")])
# the schedule fields: what each switch resolves to, and the fields derived from them
FIELDS = ("relu_bitmask", "stem_fuse_pool", "stem_pool_fused", "pair_fused", "stem_fuse_pool_bwd", "drop_gm", "fuse_bn_reduce",
          "eval_fold", "c3_axf", "ds_reduce2", "dual_apply", "fin_apply_rows", "fin_apply_rb", "wred_piggyback", "bnfin_piggyback",
          "fin_with_wred", "wgrad_first", "heads_bnred")
DTYPES = ("bfloat16", "float16", "float32", "bf16x3", "bf16x3-train")
ARCHS = ("resnet50", "resnet50_ibn_a", "resnet18")
TRAIN_CASES = (("resnet50", "bfloat16"), ("resnet50", "float16"), ("resnet50", "float32"), ("resnet50", "bf16x3-train"),
               ("resnet50_ibn_a", "bfloat16"), ("resnet18", "bfloat16"))
EVAL_CASES = (("resnet50", "bfloat16"), ("resnet50", "float32"), ("resnet50", "bf16x3"), ("resnet50_ibn_a", "bfloat16"))
B, H, W = 4, 128, 64


def setting_name(s):
    return " ".join(f"{k}={v}" for k, v in sorted(s.items())) or "default"


def group_of(s):
    return "dma0" if s.get("CREID_IGEMM_DMA", "1") != "1" else "dma1"


class _Env:
    """the environment `setting` on top of an environment with no CREID schedule switch set; restored on exit"""

    def __init__(self, setting):
        self.setting = setting

    def __enter__(self):
        self.old = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
        os.environ.update(self.setting)

    def __exit__(self, *exc):
        for k in self.setting:
            os.environ.pop(k, None)
        os.environ.update(self.old)


def engine(net, dtype):
    import torch
    from centroids_reid_amd import backbone as bb
    if dtype.startswith("bf16x3"):
        return bb.BackboneEngine(net, "bf16x3", trainable=dtype.endswith("-train"))
    return bb.BackboneEngine(net, getattr(torch, dtype))


def schedule_of(eng):
    """every schedule field of an engine as JSON values"""
    s = getattr(eng, "sched", eng)
    out = {}
    for f in FIELDS:
        if f == "heads_bnred" and not hasattr(s, f):      # (an engine without the field reads the variable at every call)
            out[f] = os.environ.get("CREID_HEADS_BNRED", "1") == "1"
            continue
        v = getattr(s, f)
        out[f] = sorted(v) if isinstance(v, (set, frozenset)) else v
    return out


# ------------------------------------------------------------------------------------------ resolve
def resolve_rows():
    """[{"dtype", "arch", "env", "sched" | "error"}]: one row per combination, in a fixed order"""
    from centroids_reid_amd import backbone as bb
    nets = {a: bb.build_backbone(a, 1) for a in ARCHS}
    rows = []
    for s in SETTINGS:
        with _Env(s):
            for dtype in DTYPES:
                for arch in ARCHS:
                    row = {"dtype": dtype, "arch": arch, "env": setting_name(s)}
                    try:
                        row["sched"] = schedule_of(engine(nets[arch], dtype))
                    except Exception as e:           # the constructor's own refusals (CreidError / ValueError)
                        row["error"] = f"{type(e).__name__}: {e}"
                    rows.append(row)
    return rows


def condense_rows(rows):
    scheds, out = [], []
    for r in rows:
        r = dict(r)
        if "sched" in r:
            if r["sched"] not in scheds:
                scheds.append(r["sched"])
            r["sched"] = scheds.index(r["sched"])
        out.append(r)
    return {"fields": list(FIELDS), "settings": [setting_name(s) for s in SETTINGS], "scheds": scheds, "rows": out}


def expand_rows(doc):
    return [dict(r, sched=doc["scheds"][r["sched"]]) if "sched" in r else dict(r) for r in doc["rows"]]


# ------------------------------------------------------------------------------------------ trace
def _arg(v):
    """one argument of a library call as a JSON value: None = null pointer, "p" = non-null pointer, int, repr(float), or the
    field list of a ConvDesc passed by reference"""
    if v is None:
        return None
    if isinstance(v, ctypes.c_void_p):
        return "p" if v.value else None
    if isinstance(v, (bool, int)):
        return int(v)
    if isinstance(v, float):
        return repr(v)
    obj = getattr(v, "_obj", None)                      # ctypes.byref(...)
    if type(obj).__name__ == "ConvDesc":
        return [int(getattr(obj, f)) for f, _ in obj._fields_]
    raise TypeError(f"argument {v!r}: neither a scalar, a pointer nor a ConvDesc by reference")


class _LibProxy:
    def __init__(self, lib, names, calls=None):
        self._lib, self._names, self._calls = lib, names, calls

    def __getattr__(self, name):
        self._names.append(name)
        fn = getattr(self._lib, name)
        if self._calls is None:
            return fn

        def call(*a):
            self._calls.append([name] + [_arg(v) for v in a])
            return fn(*a)
        return call


_NETS = {}


def _net(arch):
    """a fresh copy per engine: an engine hooks itself into its network, which would keep every engine of a group alive"""
    import copy
    if arch not in _NETS:
        import torch
        from centroids_reid_amd import backbone as bb
        torch.manual_seed(11)
        _NETS[arch] = bb.build_backbone(arch, 1).cuda()
    return copy.deepcopy(_NETS[arch])


def _checksums(named):
    """{name: [plain sum, index-weighted sum]} of fp32 device tensors, as wrap-around int64 sums of their int32 bit patterns; one
    copy back"""
    import torch
    rows = []
    for _, t in named:
        v = t.detach().contiguous().view(torch.int32).reshape(-1).to(torch.int64)
        rows.append(torch.stack((v.sum(), (v * torch.arange(1, v.numel() + 1, dtype=torch.int64, device=v.device)).sum())))
    host = torch.stack(rows).cpu().tolist()
    return {n: r for (n, _), r in zip(named, host)}


def trace_case(kind, arch, dtype, args=False):
    """the ordered entry-point names of one case under the current environment: {"names": [...]} (training cases also say whether
    the engine offers the heads the operands of the first BatchNorm backward), or {"error": text}.  args: also "calls" (every
    call with its arguments, _arg) and "sums" (_checksums of the results)"""
    import torch
    from centroids_reid_amd import _lib as L
    real, names, calls = L.lib(), [], ([] if args else None)
    try:
        eng = engine(_net(arch), dtype)
    except Exception as e:
        return {"error": f"{type(e).__name__}: {e}"}
    g = torch.Generator().manual_seed(3)
    x = torch.rand((B, 3, H, W), generator=g).cuda()
    coef = torch.randn((B, eng.cout), generator=g).cuda()
    out = {}
    orig = L.lib
    L.lib = lambda: _LibProxy(real, names, calls)
    try:
        if kind == "eval":
            with torch.no_grad():
                _, feat = eng.forward(x, training=False)
        else:
            for rnd in range(2):
                _, feat = eng.forward(x, training=True)
                if rnd == 0:
                    L.lib = orig                      # (not part of forward / backward: the heads ask for it in a full step)
                    out["heads_bnred_operands"] = eng.first_bn_bwd_operands() is not None
                    L.lib = lambda: _LibProxy(real, names, calls)
                eng.backward(coef)
    finally:
        L.lib = orig
    if args:
        out["calls"] = calls
        out["sums"] = _checksums([("feat", feat)] +
                                 [("grad " + n, p.grad) for n, p in eng.net.named_parameters() if p.grad is not None] +
                                 [(n, b) for n, b in eng.net.named_buffers() if n.endswith(("running_mean", "running_var"))])
    torch.cuda.synchronize()
    for p in eng.net.parameters():
        p.grad = None
    out["names"] = names
    return out


def digest_case(key, t):
    """what the argument record keeps of one traced case: calls and checksums in full for a `default` row, their SHA-256 otherwise"""
    t = dict(t)
    t.pop("names", None)
    if "calls" in t and not key.endswith("| default"):
        canon = json.dumps({"calls": t.pop("calls"), "sums": t.pop("sums")}, sort_keys=True, separators=(",", ":"))
        t["sha256"] = hashlib.sha256(canon.encode()).hexdigest()
    return t


def trace_setting(s, args=False):
    """{case key: trace_case(...)} for every case under the setting `s`.  args: each case carries its names and, under "args",
    its digest_case"""
    out = {}
    with _Env(s):
        for kind, cases in (("train", TRAIN_CASES), ("eval", EVAL_CASES)):
            for arch, dtype in cases:
                key = f"{kind} {arch} {dtype} | {setting_name(s)}"
                t = trace_case(kind, arch, dtype, args)
                if args:
                    t = {k: v for k, v in t.items() if k not in ("calls", "sums")} | {"args": digest_case(key, t)}
                out[key] = t
    return out


def trace_group(group, args=False):
    out = {}
    for s in SETTINGS:
        if group_of(s) == group:
            out.update(trace_setting(s, args))
    return out


def trace_all(args=False):
    """both groups, each in a child process of its own (the parent never opens the GPU)"""
    out = {}
    for group in ("dma1", "dma0"):
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "trace", "--group", group] + (["--args"] if args else []),
                           env=env, cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"trace group {group} failed with exit status {r.returncode}")
        out.update(json.loads(r.stdout.splitlines()[-1]))
    return out


def condense_traces(traces):
    table, seqs, cases = [], [], {}
    for key, t in traces.items():
        t = dict(t)
        if "names" in t:
            for n in t["names"]:
                if n not in table:
                    table.append(n)
            seq = [table.index(n) for n in t.pop("names")]
            if seq not in seqs:
                seqs.append(seq)
            t["seq"] = seqs.index(seq)
        cases[key] = t
    return {"shape": [B, H, W], "names": table, "seqs": seqs, "cases": cases}


def expand_traces(doc):
    out = {}
    for key, t in doc["cases"].items():
        t = dict(t)
        if "seq" in t:
            t["names"] = [doc["names"][i] for i in doc["seqs"][t.pop("seq")]]
        out[key] = t
    return out


def condense_args(digests):
    """{case key: digest_case(...)} -> the stored form: distinct calls once, a default row's calls as indices into that table"""
    table, index, seqs, cases = [], {}, [], {}
    for key, t in digests.items():
        t = dict(t)
        if "calls" in t:
            seq = []
            for c in t.pop("calls"):
                k = json.dumps(c)
                if k not in index:
                    index[k] = len(table)
                    table.append(c)
                seq.append(index[k])
            if seq not in seqs:
                seqs.append(seq)
            t["seq"] = seqs.index(seq)
        cases[key] = t
    return {"shape": [B, H, W], "calls": table, "seqs": seqs, "cases": cases}


def expand_args(doc):
    out = {}
    for key, t in doc["cases"].items():
        t = dict(t)
        if "seq" in t:
            t["calls"] = [doc["calls"][i] for i in doc["seqs"][t.pop("seq")]]
        out[key] = t
    return out


def args_difference(key, got, ref):
    """None if the digest `got` of case `key` equals the recorded `ref`, else one line that says where it differs: in a default
    row the first differing call and argument slot, or the first differing tensor checksum"""
    if got == ref:
        return None
    if "calls" in got and "calls" in ref:
        for i, (a, b) in enumerate(zip(got["calls"], ref["calls"])):
            if a != b:
                if a[0] != b[0] or len(a) != len(b):
                    return f"{key}: call {i} is {a}, recorded {b}"
                j = next(j for j in range(1, len(a)) if a[j] != b[j])
                return f"{key}: call {i} {a[0]}, argument {j - 1} is {a[j]!r}, recorded {b[j]!r}"
        if len(got["calls"]) != len(ref["calls"]):
            return f"{key}: {len(got['calls'])} calls, recorded {len(ref['calls'])}"
        for n in sorted(set(got["sums"]) | set(ref["sums"])):
            if got["sums"].get(n) != ref["sums"].get(n):
                return f"{key}: same calls, checksum of {n} is {got['sums'].get(n)}, recorded {ref['sums'].get(n)}"
    def short(t):                                       # (a non-default row: the hash; any row: the flags, or the refusal)
        return {k: v for k, v in t.items() if k not in ("calls", "sums")}
    return f"{key}: {short(got)}, recorded {short(ref)}"


def _dump(doc, path):
    """one top-level key per line; the long tables one entry per line (diffs stay readable)"""
    def js(v):
        return json.dumps(v, separators=(",", ":"))

    def body(v):
        if isinstance(v, list) and len(v) > 8:
            return "[\n" + ",\n".join(js(x) for x in v) + "]"
        if isinstance(v, dict) and len(v) > 8:
            return "{\n" + ",\n".join(f"{js(k)}:{js(x)}" for k, x in v.items()) + "}"
        return js(v)
    with open(path, "w") as f:
        f.write("{" + ",\n".join(f"{js(k)}:{body(v)}" for k, v in doc.items()) + "}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("resolve", "trace"))
    ap.add_argument("--write", nargs="?", const="", default=None, help="write the table (to PATH, default: the golden file)")
    ap.add_argument("--group", choices=("dma1", "dma0"), help="trace: run one group of settings in this process, print JSON")
    ap.add_argument("--args", action="store_true", help="trace: the argument-level record (backbone_launch_args.json)")
    a = ap.parse_args()
    if a.mode == "trace" and a.group:
        print(json.dumps(trace_group(a.group, a.args), separators=(",", ":")))
        return 0
    if a.mode == "trace" and a.args:
        got = {k: t["args"] for k, t in trace_all(True).items()}
        if a.write is not None:
            _dump(condense_args(got), a.write or GOLDEN_ARGS)
            print(f"wrote {a.write or GOLDEN_ARGS}: {len(got)} cases")
            return 0
        ref = expand_args(json.load(open(GOLDEN_ARGS)))
        bad = [d for d in (args_difference(k, got.get(k, {}), ref.get(k, {})) for k in sorted(set(ref) | set(got))) if d]
        for b in bad[:20]:
            print("DIFFERS:", b)
        print(f"{len(got)} cases, {len(bad)} differ from {os.path.relpath(GOLDEN_ARGS, ROOT)}")
        return 1 if bad else 0
    got = resolve_rows() if a.mode == "resolve" else trace_all()
    golden = GOLDEN_RESOLVE if a.mode == "resolve" else GOLDEN_TRACE
    if a.write is not None:
        _dump(condense_rows(got) if a.mode == "resolve" else condense_traces(got), a.write or golden)
        print(f"wrote {a.write or golden}: {len(got)} {'rows' if a.mode == 'resolve' else 'cases'}")
        return 0
    ref = json.load(open(golden))
    ref = expand_rows(ref) if a.mode == "resolve" else expand_traces(ref)
    if a.mode == "resolve":
        bad = [(r, g) for r, g in zip(ref, got) if r != g]
        bad += [("row count", len(ref), len(got))] if len(ref) != len(got) else []
    else:
        bad = [k for k in sorted(set(ref) | set(got)) if ref.get(k) != got.get(k)]
    for b in bad[:20]:
        print("DIFFERS:", b)
    print(f"{len(got)} {'rows' if a.mode == 'resolve' else 'cases'}, {len(bad)} differ from {os.path.relpath(golden, ROOT)}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
