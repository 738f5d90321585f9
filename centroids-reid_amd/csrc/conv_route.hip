// creid_conv_route_describe: the route of a convolution call as one line of text, from the same route_igemm / plan_wgrad_route
// the launchers run.  Host only: no launch, no device memory, plans are peeked at (the registry's counters do not move), so it
// answers in a process that has no GPU.  tools/conv_route_dump.py walks the sweep that tests/test_conv_route_cpu.py pins.
#include "conv_route.hpp"
#include <stdarg.h>
#include <string>

namespace {

void addf(std::string& o, const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  o += buf;
}

const char* et_name(int dtype) { return dtype == CREID_F16 ? "F16T" : "Bf16T"; }

// the instantiation's name as the compiler spells it
std::string kernel_name(const ConvRoute& r) {
  std::string o;
  const char* et = et_name(r.dtype);
  switch (r.family) {
    case CONV_C64: addf(o, "conv3x3_c64_kernel<%d, %s, %s>", r.tw, et, r.t2d ? "true" : "false"); break;
    case CONV_PP: addf(o, "igemm_bf16_pp_kernel<%d, %d, %d, %d, %d, %d, %s>", r.bm, r.bn, r.wn, r.kph, r.glm, r.epi, et); break;
    case CONV_STREAM1: addf(o, "igemm1x1_stream_kernel<%d, %d, %d>", r.bn, r.kch, r.ns); break;
    case CONV_STREAM2: addf(o, "igemm1x1_stream2_kernel<%d, %d, %d, %s, false>", r.bn, r.kch, r.ns, et); break;
    case CONV_WS: case CONV_WS256: addf(o, "igemm_bf16_ws_kernel<%d, %d, %d, %s>", r.bn, r.ns, r.bm, et); break;
    case CONV_HALO: addf(o, "igemm_bf16_halo_kernel<%d, %d, %d, %s>", r.chan, r.bn, r.ns, et); break;
    case CONV_DMA4: addf(o, "igemm_bf16_dma_kernel<%d, %d, %s>", r.bn, r.ns, et); break;
    case CONV_REG_BF16: addf(o, "igemm_bf16_kernel<%d>", r.bn); break;
    case CONV_F32: addf(o, "igemm_f32_kernel<%d>", r.bn); break;
    default: o = "none"; break;
  }
  return o;
}

const char* plan_word(bool found, bool declined) { return !found ? "none" : (declined ? "declined" : "hit"); }

std::string describe_igemm(const IGemmGeom& g, const ConvFeat& f) {
  const ConvRoute r = route_igemm(g, f, conv_igemm_knobs(), true);
  std::string o;
  if (r.err) { addf(o, "rc=%d | plan=%s", r.err, plan_word(r.have_plan, false)); return o; }
  if (r.wred_first) addf(o, "pre=wred(%d) ; ", f.wred_nblocks);
  o += kernel_name(r);
  addf(o, " grid=(%u,1,1) block=%u lds=%u", r.grid, r.block, r.lds);
  if (r.parity) o += " parity=1";
  if (r.wred_rides) addf(o, " wred=%d", f.wred_nblocks);
  addf(o, " | plan=%s", plan_word(r.have_plan, r.kernel_id != r.planned));
  if (r.have_plan) addf(o, " key=%d planned=%d runs=%d", r.plan_key, r.planned, r.kernel_id);
  return o;
}

std::string describe_wgrad(const IGemmGeom& g, int NCO, int dtype, const WgradShape& sh, int fin_nblocks) {
  std::string o;
  if (!creid_is_storage(dtype) || (dtype == CREID_F16 && !wgrad_dma_env())) return "rc=-2 | plan=none";   // (run_wgrad: before the plan is looked up)
  const WgradPlan p = plan_wgrad_route(g.M, NCO, g.K, dtype, g.stride, sh, fin_nblocks, true);
  const char* plan = plan_word(p.plan_state != 0, p.plan_state == 2);
  if (p.family == WGRAD_NONE) { addf(o, "rc=%d | plan=%s", p.err, plan); return o; }
  const char* et = et_name(dtype);
  if (p.family == WGRAD_TAPS) addf(o, "wgrad_bf16_taps_kernel<%d, %s>", g.OW, et);
  else if (p.family == WGRAD_DMA) addf(o, "wgrad_bf16_dma_kernel<%d, %d, %d, %s, %d, %s>", p.tm, p.tn, p.ns, p.wsk ? "true" : "false", p.kgroups, et);
  else addf(o, "%s<%d, %d>", p.family == WGRAD_REG_BF16 ? "wgrad_bf16_kernel" : "wgrad_f32_kernel", p.tm, p.tn);
  addf(o, " grid=(%u,%u,1) block=%u lds=0", p.gx, p.gy, p.block);
  if (p.fin_rides) addf(o, " fin=%d", fin_nblocks);
  else if (fin_nblocks) addf(o, " ; post=fin(%d)", fin_nblocks);
  addf(o, " | plan=%s splits=%d tiles=%d m_per_split=%d xcd=%d", plan, p.splits, p.tiles, p.m_per_split, p.xcd);
  return o;
}

}  // namespace

extern "C" int creid_conv_route_describe(const creid_conv_desc* d, int op, int feat_bits, int dtype, char* buf, size_t n) {
  CREID_CHECK_ARG(d && buf && n > 0 && op >= CREID_ROUTE_FWD && op <= CREID_ROUTE_STEM_WGRAD);
  ConvFeat f;
  f.dtype = dtype;
  f.add_src = feat_bits & CREID_ROUTE_ADD; f.add_compact = feat_bits & CREID_ROUTE_ADD_COMPACT; f.add_mask = feat_bits & CREID_ROUTE_ADD_MASK;
  f.stats = feat_bits & CREID_ROUTE_STATS; f.affine = feat_bits & CREID_ROUTE_AFFINE; f.bnred = feat_bits & CREID_ROUTE_BNRED;
  const int nblocks = (feat_bits & CREID_ROUTE_JOB) ? (int)((unsigned)feat_bits >> 16) : 0;
  std::string o;
  int rc = 0;
  const bool stem = op == CREID_ROUTE_STEM_FWD || op == CREID_ROUTE_STEM_WGRAD;
  if (stem) rc = stem_check_shape(d->batch, d->in_h, d->in_w);
  else if (op == CREID_ROUTE_WGRAD) rc = (igemm_ilog2(d->in_c) < 0 || d->in_c < 64 || d->out_c % 64 != 0) ? CREID_E_SHAPE : 0;
  else rc = conv_check_desc(d);
  if (!rc && op == CREID_ROUTE_DGRAD) {
    const int64_t rows = (feat_bits & CREID_ROUTE_BNRED_PER_IMAGE) ? d->in_h * d->in_w : 0;
    f.tiles_per_image = (int)(rows / 128);
    f.wred = nblocks > 0; f.wred_nblocks = nblocks;
    rc = creid_is_storage(dtype) ? conv_dgrad_check(d, f, rows, f.add_compact ? 2 : 1) : CREID_E_DTYPE;
  }
  if (rc) addf(o, "rc=%d | plan=none", rc);
  else if (op == CREID_ROUTE_FWD) o = describe_igemm(fwd_geom(d), f);
  else if (op == CREID_ROUTE_DGRAD) o = describe_igemm(dgrad_geom(d), f);
  else if (op == CREID_ROUTE_STEM_FWD) o = describe_igemm(stem_geom(d->batch, d->in_h, d->in_w), f);
  else if (op == CREID_ROUTE_WGRAD) o = describe_wgrad(fwd_geom(d), (int)d->out_c, dtype, wgrad_shape_of(d), nblocks);
  else {
    const IGemmGeom g = stem_geom(d->batch, d->in_h, d->in_w);
    o = describe_wgrad(g, 64, dtype, WgradShape{0, 7, g.pad, 3, g.OH, g.OW, g.SH, g.SW, 32, conv_is_stem_geom(g)}, 0);
  }
  snprintf(buf, n, "%s", o.c_str());
  return o.size() < n ? 0 : CREID_E_WS;
}
