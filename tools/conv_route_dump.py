#!/usr/bin/env python3
"""Which kernel runs for which convolution call: walk a fixed sweep of geometries x operations x dtypes x registry states x
knob settings and print (or compare) the route of every call.  Needs no GPU.

    python tools/conv_route_dump.py                 # describe the sweep with the built library, compare with the golden
    python tools/conv_route_dump.py --show bf16     # print the default routes of the ResNet50 layers at B = 64, 256 x 128
    python tools/conv_route_dump.py --write PATH    # write the table (only meaningful against a RECORDING library, below)

The routes come from creid_conv_route_describe (include/creid.h), i.e. from the route_igemm / plan_wgrad_route the launchers
run.  tests/golden/conv_routes.json was NOT made that way: it was recorded from the commit before csrc/conv_route.hpp existed,
with a library whose launch macro wrote "<kernel instantiation> grid block lds" into a string instead of launching
(profiles/conv_route_refactor.md); this driver then called the public entry points with dummy pointers.  A library that
exports `creid_rec_take` is such a recording library and is driven that way.

Normalisation (`normalise`, applied to both sides before they are compared):
  * namespace qualifiers and a leading `&` of the kernel name are dropped;
  * a stand-alone `wgrad_reduce_job_kernel` launch of N workgroups in front reads `pre=wred(N)`, a stand-alone
    `bn_bwd_finalize_job_kernel` launch behind reads `post=fin(N)`;
  * the split-reduce launch that the stem's one-call weight gradient appends (`wgrad_reduce_*`) is dropped: the route is the
    partials launch;
  * of the text behind ` | ` only `plan=none|hit|declined` is kept (the recording has the registry's counter deltas, no more).

Without a GPU the CU-count query behind the persistent grids falls back to 256, the MI355X's count."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_routes.json")
PLANS = os.path.join(ROOT, "centroids-reid_amd", "tuned_plans.json")
LIB = os.environ.get("CREID_LIB_PATH") or os.path.join(ROOT, "centroids-reid_amd", "lib", "libcreid_hip.so")

F32, BF16, F16 = 0, 1, 2
DTYPES = {"bf16": BF16, "f16": F16, "f32": F32}
FWD, DGRAD, WGRAD, STEM_FWD, STEM_WGRAD = range(5)
ADD, COMPACT, MASK, STATS, AFFINE, BNRED, PER_IMAGE, JOB = (1 << i for i in range(8))
# (name, op, feat bits)
OPS = [("fwd", FWD, 0), ("fwd_stats", FWD, STATS), ("fwd_affine", FWD, AFFINE), ("fwd_affine_res", FWD, AFFINE | ADD),
       ("dgrad", DGRAD, 0), ("dgrad_add", DGRAD, ADD), ("dgrad_compact", DGRAD, ADD | COMPACT), ("dgrad_masked", DGRAD, ADD | MASK),
       ("dgrad_bnred", DGRAD, BNRED), ("dgrad_bnred_img", DGRAD, BNRED | PER_IMAGE), ("dgrad_job", DGRAD, JOB),
       ("wgrad", WGRAD, 0), ("wgrad_fin", WGRAD, JOB)]
STEM_OPS = [("stem_fwd", STEM_FWD, 0), ("stem_fwd_stats", STEM_FWD, STATS), ("stem_fwd_affine", STEM_FWD, AFFINE),
            ("stem_wgrad", STEM_WGRAD, 0)]
# the carried jobs of the sweep: the split reduction of a 3 x 3, 64 -> 64 weight gradient (one workgroup per output channel) and
# the finalize job of a 64-channel BatchNorm over 8 partial rows (16 channels per workgroup)
WRED_DESC, WRED_NBLOCKS = (2, 64, 64, 3, 1, 8, 8), 64
FIN_ROWS, FIN_C, FIN_NBLOCKS = 8, 64, 4


class ConvDesc(C.Structure):
    _fields_ = [("batch", C.c_int64), ("in_h", C.c_int64), ("in_w", C.c_int64), ("in_c", C.c_int64), ("out_h", C.c_int64),
                ("out_w", C.c_int64), ("out_c", C.c_int64), ("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32),
                ("pad", C.c_int32)]


def desc(B, cin, cout, k, s, h, w):
    p = k // 2
    return ConvDesc(B, h, w, cin, (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1, cout, k, k, s, p)


def resnet50_convs(B, H, W, last_stride=1):
    """(B, cin, cout, k, stride, Hin, Win) of every non-stem convolution of ResNet50: bench_train.conv_shapes (the test checks
    that the two agree; this copy keeps the tool free of the torch import)"""
    shapes, h, w, inpl = [], H // 4, W // 4, 64
    for planes, n, st in zip((64, 128, 256, 512), (3, 4, 6, 3), (1, 2, 2, last_stride)):
        for b in range(n):
            s = st if b == 0 else 1
            shapes.append((B, inpl, planes, 1, 1, h, w))
            shapes.append((B, planes, planes, 3, s, h, w))
            ho, wo = (h + 2 - 3) // s + 1, (w + 2 - 3) // s + 1
            shapes.append((B, planes, planes * 4, 1, 1, ho, wo))
            if b == 0:
                shapes.append((B, inpl, planes * 4, 1, s, h, w))
            inpl, h, w = planes * 4, ho, wo
    return shapes


WORKLOADS = [(64, 256, 128), (128, 256, 128), (256, 256, 128), (64, 320, 320)]
# small shapes: the odd / tiny / ragged geometries of the exact sweeps (tests/test_conv_edge_sweep_gpu.py over tests/conv_exact.py),
# the GPU route test's cases, and CHANNELS x SIZES x BATCHES of tests/test_wgrad_taps_cpu.py
EDGE = [(1, 64, 64, 3, 1, 1, 1), (1, 64, 64, 1, 1, 1, 1), (1, 64, 128, 3, 2, 1, 1), (2, 64, 64, 3, 1, 2, 2), (3, 64, 64, 3, 1, 7, 5),
        (3, 128, 64, 3, 2, 7, 5), (2, 64, 128, 3, 2, 8, 6), (5, 256, 64, 1, 2, 9, 7), (1, 64, 256, 1, 1, 43, 3), (1, 64, 256, 1, 1, 32, 4),
        (1, 64, 256, 1, 1, 127, 1), (1, 128, 128, 3, 1, 127, 1), (2, 512, 64, 3, 1, 3, 3), (17, 64, 64, 3, 1, 5, 3),
        (1, 64, 128, 3, 2, 32, 16), (3, 64, 128, 3, 2, 32, 16), (1, 64, 128, 3, 2, 34, 16), (2, 64, 128, 3, 2, 15, 17),
        (3, 64, 256, 3, 1, 7, 5), (3, 128, 256, 3, 2, 7, 5), (5, 256, 256, 1, 2, 9, 7), (1, 128, 256, 3, 1, 127, 1),
        (3, 128, 128, 1, 1, 7, 5), (1, 256, 64, 1, 1, 43, 3), (17, 256, 512, 1, 1, 5, 3),
        (1, 64, 64, 3, 1, 4, 32), (2, 128, 128, 3, 1, 16, 8), (2, 128, 128, 3, 2, 16, 16), (2, 64, 256, 1, 1, 16, 8), (2, 256, 64, 1, 1, 16, 8),
        (64, 64, 64, 3, 1, 80, 80), (2, 2048, 512, 1, 1, 16, 8)]
TAPS_CHANNELS = [(64, 64), (64, 192), (128, 64), (256, 256), (512, 128)]
TAPS_SIZES = [(16, 8), (8, 16), (4, 32)]
TAPS_BATCHES = [1, 3, 5]
STEMS = [(64, 256, 128), (128, 256, 128), (256, 256, 128), (64, 320, 320), (2, 32, 16), (3, 30, 18)]


def geometries():
    seen, out = set(), []
    for B, H, W in WORKLOADS:
        for ls in (1, 2):
            for g in resnet50_convs(B, H, W, ls):
                if g not in seen:
                    seen.add(g)
                    out.append(g)
    for g in EDGE + [(b, ci, co, 3, 1, h, w) for (ci, co) in TAPS_CHANNELS for (h, w) in TAPS_SIZES for b in TAPS_BATCHES]:
        if g not in seen:
            seen.add(g)
            out.append(g)
    return out


def cases():
    """every call of the sweep: (label, geometry | stem (B, H, W), op, feat bits, dtype code)"""
    out = []
    for g in geometries():
        for name, op, bits in OPS:
            for dn, dt in DTYPES.items():
                out.append((f"{name} {dn} B{g[0]} {g[1]}->{g[2]} k{g[3]} s{g[4]} {g[5]}x{g[6]}", g, op, bits, dt))
    for st in STEMS:
        for name, op, bits in STEM_OPS:
            for dn, dt in DTYPES.items():
                out.append((f"{name} {dn} B{st[0]} {st[1]}x{st[2]}", st, op, bits, dt))
    return out


def cases_digest():
    return hashlib.sha1(json.dumps([c[0] for c in cases()]).encode()).hexdigest()


def vword(bm, bn, kph, mode):
    return (bm // 128) | ((bn // 128) << 2) | (kph << 4) | (mode << 8)


# knob settings, one at a time against the default.  LIVE: read per call under CREID_DEBUG_KNOBS=1, swept inside one process;
# ONCE: read once per process, each in a subprocess of its own.
LIVE = ([{"CREID_C64_3X3": "0"}, {"CREID_IGEMM_PP": "0"}] +
        [{"CREID_IGEMM_PP": hex(0x1000 | vword(bm, bn, 2, 0))} for bm in (128, 256) for bn in (128, 256)] +
        [{"CREID_IGEMM_PP": hex(0x1000 | vword(256, 256, 1, 2))}, {"CREID_IGEMM_PP": hex(0x1000 | vword(128, 256, 1, 2))},
         {"CREID_STREAM1X1": "1"}, {"CREID_STREAM2": "1"}, {"CREID_STREAM2": "1", "CREID_STREAM2_BN": "64"},
         {"CREID_STREAM2": "1", "CREID_STREAM2_BN": "128"}, {"CREID_STREAM2_BN": "64"}, {"CREID_STREAM1X1_WGS": "3"},
         {"CREID_STREAM2": "1", "CREID_STREAM1X1_WGS": "3"}, {"CREID_PP_WGS": "5"},
         {"CREID_IGEMM_PP": hex(0x1000 | vword(128, 128, 2, 0)), "CREID_PP_WGS": "5"},
         {"CREID_IGEMM_BM": "256"}, {"CREID_IGEMM_BM": "128"}, {"CREID_IGEMM_HALO": "0"}, {"CREID_WGRAD_TAPS": "0"},
         {"CREID_WGRAD_TAPS_WGS": "2"}])
ONCE = ([{"CREID_IGEMM_DMA": "0"}, {"CREID_IGEMM_WS": "0"}] +
        [{"CREID_IGEMM_WS": "2", "CREID_IGEMM_WS_STAGES": v} for v in ("2", "3", "4")] +
        [{"CREID_IGEMM_WS": "0", "CREID_IGEMM_STAGES": v} for v in ("3", "4", "5")] +
        [{"CREID_STEM_DMA": "0"}, {"CREID_DGRAD_PARITY": "0"}, {"CREID_WGRAD_DMA": "0"}, {"CREID_WGRAD_WS": "1"}, {"CREID_WGRAD_KG": "2"},
         {"CREID_WGRAD_KG": "2", "CREID_WGRAD_STAGES": "3"}, {"CREID_WGRAD_STAGES": "3"}, {"CREID_WGRAD_STAGES": "4"},
         {"CREID_WGRAD_XCD": "0"}, {"CREID_WGRAD_XCD": "2"}])


def setting_name(s):
    return " ".join(f"{k}={v}" for k, v in sorted(s.items())) or "default"


# ------------------------------------------------------------------------------------ the library
def load(path=LIB):
    h = C.CDLL(path)
    h.creid_tune_set.argtypes = [C.c_int32] + [C.c_int64] * 4 + [C.c_int32] * 3
    h.creid_tune_count.restype = C.c_int64
    h.creid_tune_count.argtypes = [C.c_int32] + [C.c_int64] * 4 + [C.c_int32]
    h.creid_conv2d_wgrad_workspace_bytes.restype = C.c_size_t
    h.creid_conv2d_wgrad_workspace_bytes.argtypes = [C.c_void_p, C.c_int]
    if hasattr(h, "creid_conv_route_describe"):
        h.creid_conv_route_describe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    return h


def register_plans(h, on):
    h.creid_tune_clear()
    if on:
        for e in json.load(open(PLANS))["plans"]:
            h.creid_tune_set(int(e["kind"]), *[int(v) for v in e["key"]], *[int(v) for v in e["plan"]])


_BUF = C.create_string_buffer(1024)


def describe(h, geom, op, bits, dt):
    """the route of one call, as creid_conv_route_describe words it"""
    d = ConvDesc(geom[0], geom[1], geom[2], 3, geom[1] // 2, geom[2] // 2, 64, 7, 7, 2, 3) if op >= STEM_FWD else desc(*geom)
    if bits & JOB:
        bits |= (WRED_NBLOCKS if op == DGRAD else FIN_NBLOCKS) << 16
    rc = h.creid_conv_route_describe(C.byref(d), op, bits, dt, _BUF, len(_BUF))
    assert rc == 0, (rc, geom, op, bits, dt)
    return _BUF.value.decode()


# ---- a recording library (see the module docstring): drive the public entry points with pointers that are never followed
_P = C.c_void_p(0x10000)
_BIG = C.c_size_t(1 << 60)


def record(h, geom, op, bits, dt):
    i64, ci = C.c_int64, C.c_int
    kind = 0 if op in (WGRAD, STEM_WGRAD) else 1
    h.creid_tune_total.restype = C.c_int64
    h0, d0 = h.creid_tune_total(kind, 0), h.creid_tune_total(kind, 1)
    if op >= STEM_FWD:
        B, H, W = (i64(v) for v in geom)
        if op == STEM_WGRAD:
            rc = h.creid_stem_conv_wgrad(B, H, W, _P, _P, _P, ci(0), _P, _BIG, ci(dt), None)
        elif bits & AFFINE:
            rc = h.creid_stem_conv_fwd_affine(B, H, W, _P, _P, _P, _P, ci(1), ci(dt), None)
        else:
            rc = h.creid_stem_conv_fwd(B, H, W, _P, _P, _P, _P if bits & STATS else None, ci(dt), None)
    else:
        d = C.byref(desc(*geom))
        if op == FWD and bits & AFFINE:
            rc = h.creid_conv2d_fwd_affine_nhwc(d, _P, _P, _P, _P, _P if bits & ADD else None, ci(1), ci(dt), None)
        elif op == FWD:
            rc = h.creid_conv2d_fwd_nhwc(d, _P, _P, _P, _P if bits & STATS else None, ci(dt), None)
        elif op == DGRAD:
            bn = _P if bits & BNRED else None
            rows = i64(geom[5] * geom[6] if bits & PER_IMAGE else 0)
            wd = C.byref(desc(*WRED_DESC)) if bits & JOB else None
            rc = h.creid_conv2d_dgrad_fused_nhwc(d, _P, _P, _P, _P if bits & ADD else None, ci(2 if bits & COMPACT else 1),
                                                 _P if bits & MASK else None, bn, bn, None, bn, bn, bn, rows, wd, _P if wd else None,
                                                 ci(0), _P if wd else None, _BIG, ci(dt), None)
        elif bits & JOB:
            rc = h.creid_conv2d_wgrad_partials_bnfin(d, _P, _P, _P, _BIG, ci(dt), _P, i64(FIN_ROWS), i64(FIN_C), i64(FIN_ROWS * 128),
                                                     _P, _P, _P, _P, _P, _P, None)
        else:
            rc = h.creid_conv2d_wgrad_partials(d, _P, _P, _P, _BIG, ci(dt), None)
    h.creid_rec_take.restype = C.c_size_t
    h.creid_rec_take(_BUF, C.c_size_t(len(_BUF)))
    h1, d1 = h.creid_tune_total(kind, 0), h.creid_tune_total(kind, 1)
    plan = "none" if h1 == h0 else ("declined" if d1 != d0 else "hit")
    return (f"rc={rc}" if rc else _BUF.value.decode()) + f" | plan={plan}"


def normalise(line, op):
    body, _, tail = line.partition(" | ")
    launches = [re.sub(r"^&", "", re.sub(r"(\(anonymous namespace\)|\w+)::", "", x.strip())) for x in body.split(" ; ")]
    if op == STEM_WGRAD:
        launches = [x for x in launches if not x.startswith("wgrad_reduce_")]
    m = re.match(r"wgrad_reduce_job_kernel grid=\((\d+),1,1\)", launches[0])
    if m:
        launches[0] = f"pre=wred({m.group(1)})"
    m = re.match(r"bn_bwd_finalize_job_kernel grid=\((\d+),1,1\)", launches[-1])
    if m:
        launches[-1] = f"post=fin({m.group(1)})"
    return " ; ".join(launches) + " | " + re.match(r"plan=\w+", tail).group(0)


def run_setting(h, setting):
    """{"plans": [...], "noplans": [...]}: the normalised route of every case with the shipped plans registered / cleared, under
    the environment `setting` (set here and removed again)"""
    one = record if hasattr(h, "creid_rec_take") else describe
    for k, v in setting.items():
        os.environ[k] = v
    out = {}
    try:
        for state in ("plans", "noplans"):
            register_plans(h, state == "plans")
            out[state] = [normalise(one(h, g, op, bits, dt), op) for (_, g, op, bits, dt) in cases()]
    finally:
        for k in setting:
            del os.environ[k]
        register_plans(h, True)
    return out


def run_once_setting(setting):
    """a read-once knob: a fresh process (production knob reading: CREID_DEBUG_KNOBS unset)"""
    env = {k: v for k, v in os.environ.items() if k != "CREID_DEBUG_KNOBS"}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", json.dumps(setting)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def sweep():
    """name -> run_setting result, for the default and every knob setting"""
    os.environ["CREID_DEBUG_KNOBS"] = "1"                       # before the library reads its first knob
    h = load()
    out = {"default": run_setting(h, {})}
    for s in LIVE:
        out[setting_name(s)] = run_setting(h, s)
    for s in ONCE:
        out[setting_name(s)] = run_once_setting(s)
    return out


# ------------------------------------------------------------------------------------ the golden table.  The sweep is ~580 000
# routes; the table keeps a digest per (setting, registry state, operation, dtype) group -- for a knob setting only where it
# differs from the default's -- plus two readable parts: every distinct route without its launch numbers, and default routes of the
# ResNet50 layers at B = 64, 256 x 128 in bf16.
def groups():
    """group name -> case indices; a group is one operation in one dtype over every geometry"""
    out = {}
    for i, c in enumerate(cases()):
        out.setdefault(" ".join(c[0].split()[:2]), []).append(i)
    return out


def digests(rows):
    return {g: hashlib.sha1("\n".join(rows[i] for i in idx).encode()).hexdigest()[:12] for g, idx in groups().items()}


def shapes(table):
    """every distinct route of the table without its grid, block, LDS bytes and plan word"""
    return sorted({re.sub(r" grid=\S+ block=\d+ lds=\d+| \| plan=\w+", "", s) for res in table.values() for rows in res.values() for s in rows})


def readable(rows):
    """label -> route of the bf16 calls of the B = 64, 256 x 128 layers (every other operation of the sweep's list)"""
    keep, ops = set(resnet50_convs(64, 256, 128)), {o[0] for o in OPS[::2]}
    return {c[0]: rows[i] for i, c in enumerate(cases()) if c[2] < STEM_FWD and c[4] == BF16 and c[1] in keep and c[0].split()[0] in ops}


def pack(table):
    base = {st: digests(table["default"][st]) for st in ("plans", "noplans")}
    knobs = {name: {st: {g: d for g, d in digests(res[st]).items() if d != base[st][g]} for st in ("plans", "noplans")}
             for name, res in table.items() if name != "default"}
    return {"_comment": "Recorded from the commit before csrc/conv_route.hpp: tools/conv_route_dump.py against a library whose launch "
                        "macro wrote the kernel instantiation, grid, block and LDS bytes instead of launching "
                        "(profiles/conv_route_refactor.md).  No GPU: the CU-count query fell back to 256, the MI355X's count.  "
                        "default / knobs: sha1[:12] of the newline-joined normalised routes of each group of conv_route_dump.groups(), "
                        "shipped plans registered / cleared; a knob setting lists the groups that differ from the default.  shapes: "
                        "every distinct route of the sweep without grid, block, LDS bytes and plan word.  text: default routes (plans "
                        "registered) of bf16 calls of the B = 64, 256 x 128 layers.",
            "cases": len(cases()), "cases_sha1": cases_digest(), "default": base, "knobs": knobs, "shapes": shapes(table),
            "text": readable(table["default"]["plans"])}


def compare(got, gold):
    """one line per group of `got` whose routes differ from the recording (with the route itself where the recording has it)"""
    bad = []
    for name, res in got.items():
        for st in ("plans", "noplans"):
            want = dict(gold["default"][st], **(gold["knobs"][name][st] if name != "default" else {}))
            bad += [f"{name} / {st} / {g}: the routes of this group differ from the recording" for g, d in digests(res[st]).items() if d != want[g]]
    if "default" in got:
        for lab, line in readable(got["default"]["plans"]).items():
            if line != gold["text"][lab]:
                bad.append(f"default / plans / {lab}:\n    got  {line}\n    want {gold['text'][lab]}")
    return bad


def main(argv):
    if "--one" in argv:
        print(json.dumps(run_setting(load(), json.loads(argv[argv.index("--one") + 1]))))
        return 0
    if "--show" in argv:
        dt = DTYPES[argv[argv.index("--show") + 1]]
        h = load()
        register_plans(h, True)
        for g in resnet50_convs(64, 256, 128):
            for name, op, bits in OPS:
                print(f"{name:16s} {str(g):36s} {describe(h, g, op, bits, dt)}")
        return 0
    table = sweep()
    if "--write" in argv:
        with open(argv[argv.index("--write") + 1], "w") as f:
            g, c = pack(table), lambda v: json.dumps(v, separators=(",", ":"))
            rows = [f'"{k}":{c(g[k])}' for k in ("_comment", "cases", "cases_sha1", "default")]     # one knob setting / route per line
            for k in ("knobs", "text"):
                rows.append(f'"{k}":{{\n' + ",\n".join(f"{c(a)}:{c(b)}" for a, b in g[k].items()) + "}")
            rows.append('"shapes":[\n' + ",\n".join(c(x) for x in g["shapes"]) + "]")
            f.write("{" + ",\n".join(rows) + "}\n")
        print(f"{len(cases())} cases x {len(table)} settings x 2 registry states recorded")
        return 0
    gold = json.load(open(GOLDEN))
    assert gold["cases_sha1"] == cases_digest(), "the sweep changed: the golden table no longer lines up with cases()"
    bad = compare(table, gold) + [f"a route the recording does not have: {x}" for x in set(shapes(table)) ^ set(gold["shapes"])]
    print("\n".join(bad[:40]))
    print(f"{len(bad)} differences over {len(cases())} cases x {len(table)} settings x 2 registry states")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
