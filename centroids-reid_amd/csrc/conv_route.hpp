// The one place a convolution launch is decided.
//
// Forward / data gradient: route_igemm(geometry, facts of the call, knobs) returns a ConvRoute -- kernel family, template
// arguments, grid, block, what rides in the grid, or the error code -- and launch_route() turns that value into the template
// instantiation without deciding anything.  Weight gradient: plan_wgrad_route() returns a WgradPlan that workspace sizing, the
// carried reduce job and the launchers all read.  Both are pure host code (no launch, no device API except the cached CU-count
// query of conv_pipe.hip), so creid_conv_route_describe (conv_route.hip) can print the route of any call on a machine without
// a GPU, and tests/test_conv_route_cpu.py pins the whole dispatch against a table recorded before this header existed.
#pragma once
#include "conv_common.hpp"
#include "wgrad_reduce.hpp"
#include "bn_fin.hpp"
#include "tune.hpp"

enum ConvFamily {
  CONV_NONE = 0,
  CONV_C64,        // conv3x3_c64_kernel<TW, ET, T2D>                         (conv_stream.hip)
  CONV_PP,         // igemm_bf16_pp_kernel<BM, BN, WN, KPH, GLM, EPI, ET>     (conv_pipe.hip)
  CONV_STREAM1,    // igemm1x1_stream_kernel<BN, KCH, NSA>                    (conv_stream.hip)
  CONV_STREAM2,    // igemm1x1_stream2_kernel<BN, KCH, RT, ET>                (conv_stream.hip)
  CONV_WS,         // igemm_bf16_ws_kernel<BN, NS, 128, ET>                   (conv_igemm.hip, as are the rest)
  CONV_WS256,      // igemm_bf16_ws_kernel<128, NS, 256, ET>
  CONV_HALO,       // igemm_bf16_halo_kernel<C, BN, NS, ET>
  CONV_DMA4,       // igemm_bf16_dma_kernel<BN, NS, ET>
  CONV_REG_BF16,   // igemm_bf16_kernel<BN>
  CONV_F32         // igemm_f32_kernel<BN>
};

// Everything a launch site needs and nothing it must re-derive.
struct ConvRoute {
  int family = CONV_NONE;
  int err = 0;                  // CREID_E_*: no kernel covers the call (family stays CONV_NONE)
  int dtype = 0;                // element type: CREID_BF16 / CREID_F16 -> Bf16T / F16T; CREID_F32
  int bm = 128, bn = 0, ns = 0; // tile rows / columns; ring depth (stream kernels: NSA | RT)
  int wn = 0, kph = 0, glm = 0, epi = 0;   // pp
  int kch = 0;                  // stream: 64-wide k chunks
  int tw = 0, t2d = 0;          // c64
  int chan = 0;                 // halo: channels per tap
  unsigned grid = 0, block = 0, lds = 0;   // lds: dynamic bytes (every family keeps its LDS static: 0)
  int tiles_m = 0, tiles_n = 0; // the tile counts the kernels take as arguments
  int parity = 0;               // parity-class row order (stride-2 3x3 data gradient)
  int abl = 0;                  // the family's timing-ablation / debug word (0 outside the ablation build and the probes)
  bool have_plan = false;       // the registry answered for plan_key
  int plan_key = 0;             // 4th key slot that was looked up: transposed | stride << 1 (| 8: folded epilogue)
  int planned = -1;             // the plan's kernel id once its word passed the checks, else -1
  int kernel_id = -2;           // what runs: plan kinds 0..5, 6 = the c64 kernel, -2 = the rest.  != planned with a plan: declined
  bool wred_rides = false;      // the weight-gradient reduce job is carried by this grid (+ nblocks workgroups) ...
  bool wred_first = false;      // ... or needs its own launch first
};

// The facts of a call that steer routing (the launchers read them off pointers, creid_conv_route_describe off its bits).
struct ConvFeat {
  int dtype = 0;
  bool add_src = false, add_compact = false, add_mask = false;
  bool stats = false;           // BatchNorm statistics partials
  bool affine = false;          // folded eval-mode BatchNorm epilogue
  bool bnred = false;           // fused reduction of the next BatchNorm backward ...
  int tiles_per_image = 0;      // ... per (image, channel) when > 0
  bool wred = false;            // a weight-gradient reduce job comes with the call ...
  int wred_nblocks = 0;         // ... of this many workgroups
};

// Every environment switch the forward / data-gradient dispatch reads (conv_igemm_knobs(), conv_igemm.hip: the one read site).
struct IGemmKnobs {
  int abl;                      // CREID_IGEMM_ABL (ablation build only)
  bool c64_on;                  // CREID_C64_3X3 != 0
  int c64_abl;                  // CREID_C64_ABL (ablation build only)
  bool pp_off; int force_pp;    // CREID_IGEMM_PP: "0" forbids, 0x1000 | variant forces
  int pp_wgs;                   // CREID_PP_WGS (0: one or two workgroups per CU)
  int force_stream1, force_stream2;   // CREID_STREAM1X1, CREID_STREAM2
  int stream2_bn;               // CREID_STREAM2_BN
  int stream_wgs;               // CREID_STREAM1X1_WGS (0: 256)
  int stream1_dbg;              // CREID_STREAM1X1_DBG
  int stream2_abl;              // CREID_STREAM2_ABL (ablation build only)
  int force_bm;                 // CREID_IGEMM_BM
  bool halo_on;                 // CREID_IGEMM_HALO != 0
  int min_wgs, use_dma, use_ws, ws_stages, ws_min_k, parity_on, bm256_min, stages;   // the read-once ones
};
const IGemmKnobs& conv_igemm_knobs();
int conv_stem_dma_env();        // CREID_STEM_DMA (default 1), read once

// The stem on its LDS-DMA kernels: 32-element taps of the pre-padded image, switched by CREID_STEM_DMA.
static inline bool conv_is_stem_geom(const IGemmGeom& g) {
  return g.log2span == 5 && !g.transposed && !g.check_bounds && g.kw == 1 && g.stride == 2 && g.pad == 0 && conv_stem_dma_env() != 0;
}

struct ConvPtrs { const void* src; const void* wgt; void* out; const void* add_src; float* bn_part; };

// persistent grid of the streamed 1x1 kernels: `wgs` workgroups (one per CU) split evenly over the column slabs
static inline unsigned conv_stream_slab_grid(int wgs_knob, int tiles_m, int tiles_n) {
  int groups = (wgs_knob > 0 ? wgs_knob : 256) / tiles_n;
  if (groups < 1) groups = 1;
  if (groups > tiles_m) groups = tiles_m;
  return (unsigned)(groups * tiles_n);
}

// ---- coverage-and-shape of each family (true: its part of r is filled; false: not covered, r untouched) and its launcher
// conv_stream.hip
bool conv3x3_c64_route(const IGemmGeom& g, const ConvFeat& f, const IGemmKnobs& k, ConvRoute& r);
bool stream1_route(const IGemmGeom& g, const IGemmKnobs& k, ConvRoute& r);
bool stream2_route(const IGemmGeom& g, int bn_cap, const IGemmKnobs& k, ConvRoute& r);
void launch_conv3x3_c64(const ConvRoute& r, const IGemmGeom& g, const ConvPtrs& p, hipStream_t s);
void launch_stream1(const ConvRoute& r, const IGemmGeom& g, const ConvPtrs& p, hipStream_t s);
void launch_stream2(const ConvRoute& r, const IGemmGeom& g, const ConvPtrs& p, hipStream_t s);
// conv_pipe.hip: variant = BM / 128 | (BN / 128) << 2 | KPH << 4 | MODE << 8
bool igemm_pp_route(const IGemmGeom& g, const ConvFeat& f, int variant, const IGemmKnobs& k, ConvRoute& r);
void launch_igemm_pp(const ConvRoute& r, const IGemmGeom& g, const ConvPtrs& p, hipStream_t s);
// conv_igemm.hip: the whole precedence; peek = look plans up without counting the hit (creid_conv_route_describe)
ConvRoute route_igemm(const IGemmGeom& g, const ConvFeat& f, const IGemmKnobs& k, bool peek = false);
int conv_dgrad_check(const creid_conv_desc* d, const ConvFeat& f, int64_t bn_stat_image_rows, int add_src_stride);

// ---- weight gradient (conv_wgrad.hip)
enum WgradFamily { WGRAD_NONE = 0, WGRAD_TAPS, WGRAD_DMA, WGRAD_REG_BF16, WGRAD_F32 };

struct WgradShape { int kh, kw, pad, cin, OH, OW, SH, SW; int span; bool stem; };   // span: elements of K per tap; stem: conv_is_stem_geom

struct WgradPlan {
  int tm, tn, tiles, tiles_k, splits, m_per_split, xcd;
  int stages, ws, kg;           // what a measured plan asks for (0: default)
  int taps;                     // wgrad_bf16_taps_kernel
  int family, err;              // WgradFamily; err: why there is none (CREID_E_*)
  int ns, wsk, kgroups;         // WGRAD_DMA template arguments: ring depth, producer/consumer form, k-groups
  unsigned gx, gy, block;       // grid (2-D, or the 1-D XCD form with the finalize job's workgroups in front) and block
  bool fin_rides;               // the BatchNorm-backward finalize job is carried by this grid
  int plan_state;               // registry: 0 no plan, 1 applied, 2 declined
};

static inline WgradShape wgrad_shape_of(const creid_conv_desc* d) {
  return WgradShape{d->kh, d->kw, d->pad, (int)d->in_c, (int)d->out_h, (int)d->out_w, (int)d->in_h, (int)d->in_w, (int)d->in_c, false};
}
// fin_nblocks: workgroups of the finalize job offered to the launch (0: none); peek: as route_igemm
WgradPlan plan_wgrad_route(int M, int NCO, int K, int dtype, int stride, const WgradShape& sh, int fin_nblocks = 0, bool peek = false);
int wgrad_dma_env();            // CREID_WGRAD_DMA (default 1), read once

bool wgrad_make_reduce_job(const creid_conv_desc* d, int dtype, const void* ws, size_t ws_bytes, float* dw, int accumulate,
                           WRedJob& j);
int wgrad_reduce_job_launch(const WRedJob& j, hipStream_t s);
