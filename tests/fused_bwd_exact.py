"""Exact references and launch helpers for the FUSED backward launches (shared by tests/test_fused_bwd_exact_gpu.py and
tests/test_fused_bwd_exact_cpu.py; importable without a GPU): creid_conv2d_dgrad_fused_nhwc, creid_conv2d_wgrad_partials with the
three homes of its reduce job, creid_conv2d_wgrad_partials_bnfin and creid_bn2d_bwd_finalize_wred.

Everything is arranged to be exact, so every comparison is bit for bit (as values):
  * convolution operands are small integers as in tests/conv_exact.py; the expected stored dx is rd(acc) for a 16-bit type,
    rd(rd(acc) + a) with an add (the epilogue rounds twice: conv_epilogue.hpp add_chunk on the staged 16-bit tile), acc in fp32;
  * the BatchNorm-backward column sums s1 = sum g [keep], s2 = sum g [keep] (x - mean) invstd take g = the STORED dx (an integer),
    integer x and mean, invstd in {0.5, 1, 2}: every term is a multiple of a power-of-two unit, and `assert_tile_sums_exact`
    proves ON THE REFERENCE that the sum of |terms| of every (128-row tile, channel) stays below 2^24 units -- then every partial
    sum of any subset, in any order, with or without a fused multiply-add, is an exact fp32 value;
  * the finalize's operands (`fin_operands`) are dyadic, and `ref_finalize` proves by an fp32 round trip that every intermediate
    and every result of bn_bwd_finalize_block's expressions is an fp32 value: contraction cannot change an exact result."""
import ctypes as C
import functools
import types
import zlib

import torch
import torch.nn.functional as F

import conv_exact as ce

E_ARG, E_DTYPE, E_WS, E_SHAPE = -1, -2, -3, -4                       # include/creid.h
ROUTE_DGRAD, ROUTE_WGRAD = 1, 2
R_ADD, R_ADD_COMPACT, R_ADD_MASK, R_BNRED, R_BNRED_PER_IMAGE, R_JOB = 1, 2, 4, 32, 64, 128
TILE = 128
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "fp32": torch.float32}
F64 = torch.float64


def gid(g):
    B, cin, cout, k, s, h, w = g
    return f"B{B}_{cin}to{cout}_k{k}s{s}_{h}x{w}"


# ------------------------------------------------------------------------------------ bit masks
def pack_bits(keep):
    """bool [...] -> uint8 [numel / 8]: bit k of byte i = keep.flat[8 i + k] -- for an [M, C] tensor (C % 8 == 0) one byte per
    8 channels, bit c % 8 of byte (pixel * C + c) / 8 (creid_bn2d_apply_mask's layout)"""
    k = keep.reshape(-1, 8).to(torch.int32)
    wgt = (1 << torch.arange(8, device=keep.device, dtype=torch.int32))
    return (k * wgt).sum(1).to(torch.uint8)


def unpack_bits(bits, shape):
    wgt = (1 << torch.arange(8, device=bits.device, dtype=torch.int32))
    return ((bits.to(torch.int32).reshape(-1, 1) & wgt) != 0).reshape(shape)


# ------------------------------------------------------------------------------------ fp64 references
def rd(t, dtype):
    """the stored value of an fp64 tensor: one RNE rounding to a 16-bit type, the plain value in fp32"""
    return ce._rd(t, dtype) if dtype != torch.float32 else t.float().double()


def stored_dx(acc, dtype, add=None):
    """acc fp64 [M, C] (exact integers) -> what the epilogue stores: rd(acc), or rd(rd(acc) + add) (16-bit: two roundings)"""
    e = rd(acc, dtype)
    return e if add is None else rd(e + add, dtype)


def upsample_compact(add_c, h, w):
    """the compact stride-2 add [B, h/2, w/2, C] as its full-resolution tensor: the add on even (y, x), zero elsewhere"""
    B, _, _, c = add_c.shape
    full = torch.zeros((B, h, w, c), dtype=add_c.dtype, device=add_c.device)
    full[:, ::2, ::2] = add_c
    return full


def _tiles(t):
    """[M, C] -> [ceil(M / 128), 128, C], the last tile zero-padded: rows beyond M contribute nothing"""
    return F.pad(t, (0, 0, 0, (-t.shape[0]) % TILE)).view(-1, TILE, t.shape[1])


def assert_tile_sums_exact(terms, what=""):
    """terms fp64 [M, C]: every term is a multiple of one power-of-two unit 2^-k (k <= 24) and, per (128-row tile, channel),
    sum |terms| < 2^24 units -- so every partial sum is an integer count of units below 2^24: exact in fp32 in any order."""
    unit = None
    for k in range(25):
        s = terms * 2.0 ** k
        if bool((s == s.round()).all()):
            unit = 2.0 ** -k
            break
    assert unit is not None, f"{what}: the terms are not multiples of a power-of-two unit >= 2^-24"
    worst = float(_tiles(terms.abs()).sum(1).max()) / unit if terms.numel() else 0.0
    assert worst < 2.0 ** 24, f"{what}: sum |terms| of a tile is {worst:.0f} units of {unit}, not below 2^24: narrow the operands"
    return unit


def ref_bn_partials(g, keep, x, mean, invstd, image_rows=0, what="bn sums"):
    """The fused column reduction in fp64.  g [M, C]: the stored dx; keep [M, C] bool or None; x [M, C]; mean / invstd [C], or
    [B, C] with image_rows = rows of one image (a multiple of 128: a tile then lies in one image).  Returns the partial rows
    [ceil(M / 128), 2, C] of the zero-padded 128-row tiles; their exactness in fp32 is asserted here, on the reference alone."""
    g, x, mean, invstd = g.double(), x.double(), mean.double(), invstd.double()
    if image_rows:
        assert image_rows % TILE == 0 and mean.dim() == 2 and mean.shape[0] * image_rows == g.shape[0]
        mean, invstd = mean.repeat_interleave(image_rows, 0), invstd.repeat_interleave(image_rows, 0)
    t1 = g if keep is None else g * keep.double()
    t2 = t1 * ((x - mean) * invstd)
    assert_tile_sums_exact(t1, what + " s1")
    assert_tile_sums_exact(t2, what + " s2")
    return torch.stack([_tiles(t1).sum(1), _tiles(t2).sum(1)], 1)


def _f32_exact(t, what):
    assert bool((t.float().double() == t).all()) and bool(torch.isfinite(t.float()).all()), f"{what} is not an fp32 value"
    return t


def ref_finalize(partial, count, mean, invstd, gamma, dgamma0, dbeta0):
    """bn_bwd_finalize_block (csrc/bn_fin.hpp) in fp64, every intermediate of its fp32 expressions asserted to be an fp32 value:
    s = fp64 column sums of the partial rows; a = (float) s / count; k1 = gamma invstd;
    sums = [k1, -k1 is a2, -k1 a1 + k1 is a2 mu]; dgamma = dgamma0 + s2; dbeta = dbeta0 + s1."""
    p = partial.double()
    s1, s2 = p[:, 0].sum(0), p[:, 1].sum(0)
    mu, is_, g = mean.double(), invstd.double(), gamma.double()
    inv = _f32_exact(torch.tensor(1.0 / count, dtype=F64), "1 / count")
    _f32_exact(s1, "s1"), _f32_exact(s2, "s2")
    a1, a2 = _f32_exact(s1 * inv, "a1"), _f32_exact(s2 * inv, "a2")
    k1 = _f32_exact(g * is_, "k1")
    c1 = _f32_exact(_f32_exact(-k1 * is_, "k1 is") * a2, "k1 is a2")
    c2 = _f32_exact(_f32_exact(-k1 * a1, "k1 a1") + _f32_exact(-c1 * mu, "k1 is a2 mu"), "the third coefficient")
    return dict(sums=torch.stack([k1, c1, c2]), dgamma=_f32_exact(dgamma0.double() + s2, "dgamma"),
                dbeta=_f32_exact(dbeta0.double() + s1, "dbeta"))


def fin_operands(bn_c, rows, seed, device):
    """partial rows integers in {-8..8}; gamma in {-8..8} / 4, invstd in {0.5, 1, 2}, mean in {-4..4} / 2; dgamma0 / dbeta0
    non-zero integers.  |s| <= 8 rows <= 2^13 (rows <= 1024), so with count = 2^12 every expression of ref_finalize has at most
    4 + 14 + 4 = 22 significant bits."""
    gen = torch.Generator(device=device).manual_seed(zlib.crc32(repr(("fin", bn_c, rows, seed)).encode()))
    ri = lambda lo, hi, *sh: torch.randint(lo, hi + 1, sh, generator=gen, device=device).float()
    nz = lambda t: torch.where(t == 0, torch.ones_like(t), t)
    return types.SimpleNamespace(
        partial=ri(-8, 8, rows, 2, bn_c), count=4096, mean=ri(-4, 4, bn_c) * 0.5, invstd=2.0 ** ri(-1, 1, bn_c),
        gamma=ri(-8, 8, bn_c) * 0.25, dgamma0=nz(ri(-5, 5, bn_c)), dbeta0=nz(ri(-5, 5, bn_c)))


# ------------------------------------------------------------------------------------ operands of one geometry
def _ops_on(geom, dy_hi, device):
    B, cin, cout, k, s, h, w = geom
    oh, ow = ce.out_hw(k, s, h, w)
    gen = torch.Generator(device=device).manual_seed(zlib.crc32(repr(("fused", geom, dy_hi)).encode()))
    ri = lambda lo, hi, *sh: torch.randint(lo, hi + 1, sh, generator=gen, device=device, dtype=torch.int8)
    o = types.SimpleNamespace(geom=geom, oh=oh, ow=ow, M=B * h * w, dy_hi=dy_hi)
    o.x8, o.w8, o.dy8 = ri(-2, 2, B, h, w, cin), ri(-2, 2, cout, cin, k, k), ri(-dy_hi, dy_hi, B, oh, ow, cout)
    o.add8, o.addc8 = ri(-2, 2, B, h, w, cin), ri(-2, 2, B, h // 2, w // 2, cin)
    o.act8 = ri(-2, 2, B, h, w, cin)                                   # positive, zero and negative entries
    o.bn_keep = ri(0, 1, B, h, w, cin).bool()                          # about half the bits
    o.add_keep = ri(0, 1, B, h, w, cin).bool()
    o.mean = ri(-2, 2, cin).float()
    o.invstd = 2.0 ** ri(-1, 1, cin).float()
    o.mean_img = ri(-2, 2, B, cin).float()                             # per-(image, channel) statistics: differ per image
    o.invstd_img = 2.0 ** ri(-1, 1, B, cin).float()
    o.dw0 = ri(-3, 3, cout, cin, k, k).float()
    o.acc = ce.ref_dgrad(o.dy8, o.w8, s, k // 2, h, w, 0, B).reshape(-1, cin)        # fp64, exact integers
    return o


FORMS = {  # name: (add: None | "full" | "compact", add_mask, bn: None | "act" | "mask" | "plain")
    "1_act": (None, False, "act"), "2_mask": (None, False, "mask"), "3_plain_sums": (None, False, "plain"),
    "4_mask_add": ("full", False, "mask"), "5_mask_add_addmask": ("full", True, "mask"),
    "6_mask_compact_add": ("compact", False, "mask"), "7_addmask_only": ("full", True, None),
    "plain": (None, False, None), "add": ("full", False, None), "compact_add": ("compact", False, None)}


def expected(o, dtype, form, per_image=False):
    """(dx [M, cin] fp64, partial rows [ceil(M / 128), 2, cin] fp64 or None) of one form of the fused data gradient"""
    add, add_mask, bn = FORMS[form]
    B, cin, cout, k, s, h, w = o.geom
    a = None
    if add == "full":
        a = o.add8.double() * (o.add_keep.double() if add_mask else 1.0)
    elif add == "compact":
        a = upsample_compact(o.addc8, h, w).double()
    g = stored_dx(o.acc, dtype, None if a is None else a.reshape(-1, cin))
    if bn is None:
        return g, None
    keep = {"act": o.act8 > 0, "mask": o.bn_keep, "plain": None}[bn]
    mean, invstd = (o.mean_img, o.invstd_img) if per_image else (o.mean, o.invstd)
    part = ref_bn_partials(g, None if keep is None else keep.reshape(-1, cin), o.x8.reshape(-1, cin), mean, invstd,
                           h * w if per_image else 0, f"{gid(o.geom)} {form}")
    return g, part


def _sums_hold(o):
    """the exactness condition of every BatchNorm form of this operand set, for both 16-bit types"""
    try:
        for dtype in (torch.bfloat16, torch.float16):
            for form, (_, _, bn) in FORMS.items():
                if bn is not None and (FORMS[form][0] != "compact" or (o.geom[5] % 2 == 0 and o.geom[6] % 2 == 0)):
                    expected(o, dtype, form)
    except AssertionError:
        return False
    return True


@functools.lru_cache(maxsize=None)
def operands(geom, device="cuda"):
    """The operand set of one geometry, built once and never modified: dy in {-2..2}, narrowed to {-1, 0, 1} where the column
    sums of the wider set would not be provably exact (assert_tile_sums_exact); the narrowed set must then hold."""
    o = _ops_on(geom, 2, device)
    if not _sums_hold(o):
        o = _ops_on(geom, 1, device)
        assert _sums_hold(o), f"{gid(geom)}: the column sums are not exact even with dy in {{-1, 0, 1}}"
    return o


# ------------------------------------------------------------------------------------ the library, called directly
def _L():
    from centroids_reid_amd import _lib as L
    return L


def desc(geom):
    from centroids_reid_amd import layers as ly
    B, cin, cout, k, s, h, w = geom
    return ly.conv_desc(B, h, w, cin, cout, k, s, k // 2)[0]


def describe(geom, op, bits, dtype):
    L = _L()
    buf = C.create_string_buffer(512)
    d = desc(geom)
    assert L.lib().creid_conv_route_describe(C.byref(d), op, bits, L._DT[dtype], buf, len(buf)) == 0
    return buf.value.decode()


def ws_bytes(geom, dtype):
    L = _L()
    d = desc(geom)
    return int(L.lib().creid_conv2d_wgrad_workspace_bytes(C.byref(d), L._DT[dtype]))


def splits_of(geom, dtype):
    B, cin, cout, k, s, h, w = geom
    return ws_bytes(geom, dtype) // (cout * cin * k * k * 4)


def job_shape(geom, splits):
    """(workgroups, split lanes) of the reduce job, as wred_make_job (csrc/wgrad_reduce.hpp) sets them"""
    B, cin, cout, k, s, h, w = geom
    if k != 1:
        return cout, 1
    sl = 1
    while sl < 64 and splits > 8 * sl:
        sl *= 2
    per_wg = 512 // sl
    return max(1, min(2048, (cout * cin // 4 + per_wg - 1) // per_wg)), sl


def weights(o, dtype):
    from centroids_reid_amd import layers as ly
    return ly.weight_prep(o.w8.float(), dtype)


class Job:
    """the partial tiles of one weight gradient (creid_conv2d_wgrad_partials), to be reduced by one of the three homes"""
    def __init__(self, o, dtype, bnfin=None):
        L = _L()
        self.o, self.dtype, self.d = o, dtype, desc(o.geom)
        self.nbytes = ws_bytes(o.geom, dtype)
        self.splits = splits_of(o.geom, dtype)
        self.ws = torch.full((max(self.nbytes, 16) // 4,), float("nan"), dtype=torch.float32, device="cuda")
        B, cin, cout, k, s, h, w = o.geom
        self.x, self.dy = o.x8.to(dtype), o.dy8.to(dtype)
        if bnfin is None:
            self.rc = L.lib().creid_conv2d_wgrad_partials(C.byref(self.d), L.ptr(self.x), L.ptr(self.dy), L.ptr(self.ws), self.nbytes,
                                                          L._DT[dtype], L.stream())
        else:
            f, out = bnfin
            self.rc = L.lib().creid_conv2d_wgrad_partials_bnfin(
                C.byref(self.d), L.ptr(self.x), L.ptr(self.dy), L.ptr(self.ws), self.nbytes, L._DT[dtype], L.ptr(f.partial),
                f.partial.shape[0], f.partial.shape[2], f.count, L.ptr(f.mean), L.ptr(f.invstd), L.ptr(f.gamma), L.ptr(out.sums),
                L.ptr(out.dgamma), L.ptr(out.dbeta), L.stream())
        if not hasattr(o, "dw_ref"):                                   # fp64 OIHW, exact integers; once per geometry
            o.dw_ref = ce.ref_wgrad(o.x8, o.dy8, k, s, k // 2)
        self.ref = o.dw_ref

    def dw_init(self):
        return self.o.dw0.clone()

    def want(self, accumulate):
        return self.ref + self.o.dw0.double() if accumulate else self.ref

    def reduce_alone(self, accumulate):
        L = _L()
        dw = self.dw_init()
        rc = L.lib().creid_conv2d_wgrad_reduce_job(C.byref(self.d), L.ptr(dw), accumulate, L.ptr(self.ws), self.nbytes, L._DT[self.dtype],
                                                   L.stream())
        return rc, dw

    def reduce_with_finalize(self, accumulate, f):
        L = _L()
        dw, out = self.dw_init(), fin_outputs(f)
        rc = L.lib().creid_bn2d_bwd_finalize_wred(
            L.ptr(f.partial), f.partial.shape[0], f.partial.shape[2], f.count, L.ptr(f.mean), L.ptr(f.invstd), L.ptr(f.gamma),
            L.ptr(out.sums), L.ptr(out.dgamma), L.ptr(out.dbeta), C.byref(self.d), L.ptr(dw), accumulate, L.ptr(self.ws), self.nbytes,
            L._DT[self.dtype], L.stream())
        return rc, dw, out


def fin_outputs(f):
    """sums pre-filled with NaN; dgamma / dbeta start from the non-zero integers of fin_operands: they accumulate"""
    return types.SimpleNamespace(sums=torch.full((3, f.partial.shape[2]), float("nan"), device=f.partial.device),
                                 dgamma=f.dgamma0.clone(), dbeta=f.dbeta0.clone())


def check_finalize(f, out, fails, what):
    ref = ref_finalize(f.partial, f.count, f.mean, f.invstd, f.gamma, f.dgamma0, f.dbeta0)
    for name in ("sums", "dgamma", "dbeta"):
        got = getattr(out, name).double()
        if not torch.equal(got, ref[name]):
            fails.append(f"{what}: finalize {name}: {int((got != ref[name]).sum())} of {got.numel()} values differ from fp64")
    return 3


def dgrad_fused(o, dtype, form, per_image=False, job=None, accumulate=0, image_rows=None, job_bytes=None, add_stride=None,
                force_add_mask=False):
    """One creid_conv2d_dgrad_fused_nhwc launch of `form` -> (rc, dx, partial or None, dw or None); dx and partial are pre-filled
    with NaN.  job: a Job whose reduction rides (or runs first); image_rows / job_bytes / add_stride / force_add_mask override
    what the form implies (the refusals)."""
    L = _L()
    add, add_mask, bn = FORMS[form]
    B, cin, cout, k, s, h, w = o.geom
    d = desc(o.geom)
    _, crsk = weights(o, dtype)
    dy = o.dy8.to(dtype)
    dx = torch.full((B, h, w, cin), float("nan"), dtype=dtype, device="cuda")
    a = {None: None, "full": o.add8, "compact": o.addc8}[add]
    a = None if a is None else a.to(dtype)
    am = pack_bits(o.add_keep) if add_mask or force_add_mask else None
    bx = act = bm = part = mean = invstd = None
    if bn is not None:
        bx = o.x8.to(dtype)
        part = torch.full((int(L.lib().creid_bn2d_bwd_rows(o.M)), 2, cin), float("nan"), dtype=torch.float32, device="cuda")
        mean, invstd = (o.mean_img, o.invstd_img) if per_image else (o.mean, o.invstd)
        if bn == "act":
            act = o.act8.to(dtype)
        elif bn == "mask":                                             # the header: bn_act is not read when bn_mask is given
            bm, act = pack_bits(o.bn_keep), torch.full((B, h, w, cin), -1.0, dtype=dtype, device="cuda")
    rows = (h * w if per_image else 0) if image_rows is None else image_rows
    dw = None if job is None else job.dw_init()
    rc = L.lib().creid_conv2d_dgrad_fused_nhwc(
        C.byref(d), L.ptr(dy), L.ptr(crsk), L.ptr(dx), L.ptr(a), add_stride or (2 if add == "compact" else 1), L.ptr(am), L.ptr(bx), L.ptr(act), L.ptr(bm),
        L.ptr(mean), L.ptr(invstd), L.ptr(part), rows, C.byref(job.d) if job else None, L.ptr(dw), accumulate,
        L.ptr(job.ws) if job else None, (job.nbytes if job_bytes is None else job_bytes) if job else 0, L._DT[dtype], L.stream())
    return rc, dx, part, dw


def route_bits(form, per_image=False, job_blocks=0):
    add, add_mask, bn = FORMS[form]
    bits = (R_ADD if add else 0) | (R_ADD_COMPACT if add == "compact" else 0) | (R_ADD_MASK if add_mask else 0)
    bits |= (R_BNRED if bn else 0) | (R_BNRED_PER_IMAGE if per_image else 0)
    return bits | ((R_JOB | (job_blocks << 16)) if job_blocks else 0)


def check_dgrad(o, dtype, form, dx, part, fails, what, per_image=False, row_by_row=True):
    """dx bit-exact; every partial value written (finite); the column sums over all rows exact; row by row exact against the
    zero-padded 128-row tiles where the kernel's tile is 128 consecutive pixels (row_by_row).  Returns the comparisons made."""
    cin = o.geom[1]
    edx, epart = expected(o, dtype, form, per_image)
    n = 1
    got = dx.reshape(-1, cin).double()
    if not torch.equal(got, edx):
        bad = (got != edx) | torch.isnan(got)
        i = int(bad.reshape(-1).nonzero()[0])
        fails.append(f"{what}: dx: {int(bad.sum())} mismatches, first at (row, col) {divmod(i, cin)}: got "
                     f"{float(got.reshape(-1)[i])} expected {float(edx.reshape(-1)[i])}")
    if epart is None:
        return n
    p = part.double()
    if not bool(torch.isfinite(p).all()):
        fails.append(f"{what}: {int((~torch.isfinite(p)).sum())} of {p.numel()} partial values were not written")
    if p.shape != epart.shape:
        fails.append(f"{what}: {p.shape[0]} partial rows, expected {epart.shape[0]}")
        return n
    if not torch.equal(p.sum(0), epart.sum(0)):
        fails.append(f"{what}: column sums over all rows: {int((p.sum(0) != epart.sum(0)).sum())} of {2 * cin} differ")
    n += 2
    if row_by_row:
        n += 1
        if not torch.equal(p, epart):
            bad = (p != epart).nonzero()[0].tolist()
            fails.append(f"{what}: partial rows: {int((p != epart).sum())} values differ, first at (row, which, col) {bad}: got "
                         f"{float(p[tuple(bad)])} expected {float(epart[tuple(bad)])}")
    return n
