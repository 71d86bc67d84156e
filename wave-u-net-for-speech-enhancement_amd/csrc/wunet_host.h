// Host side of libwunet_hip.so, shared declarations: the per-shape plan (tilings, workspace layout), the context, and the
// launch helpers the forward / backward / single-op translation units call.  Nothing here is part of the C ABI
// (include/wunet_hip.h); no torch types, no hidden device allocations on the hot path, nothing synchronises the stream.
//   wunet_plan.cpp      shape planning, workspace layout, context life cycle, error text, per-launch profiler
//   wunet_launchers.cpp argument blocks + launches of the GEMM kernels, weight packs, side stream
//   wunet_forward.cpp   wunet_forward
//   wunet_backward.cpp  wunet_backward[_range[_async]], wunet_backward_join
//   wunet_ops.cpp       every other entry point: the losses and metrics (wunet_loss_mean.h, wunet_loss_rows.h, wunet_stft.h, wunet_cspec.h,
//                       wunet_stoi.h, wunet_estoi.h), fused Adam (wunet_adam.h: one kernel pair and one enqueue behind both entries), the
//                       loader ops (wunet_mix.h with the window crops, wunet_reverb.h, wunet_chunks.h, wunet_resample.h), profiler read-out,
//                       single-op entry points (tests / tools)
// Device code the translation units share: wunet_dev.h (vocabulary), wunet_reduce.h (block reductions), wunet_elementwise.h /
// wunet_h3_elem.h / wunet_tiny.h (the network's memory-bound kernels), wunet_kernels.h / wunet_h3*.h (the GEMMs), wunet_lds.h.
#pragma once
#include <cstdarg>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "wunet_kernels.h"
#include "wunet_h3.h"
#include "wunet_h3u.h"
#include "wunet_launch.h"
#include "wunet_hip.h"

namespace wunet_host {

int fail(int code, const char* fmt, ...);
const char* last_error_text();

#define WUNET_CHECK_LAUNCH()                                                                   \
    do {                                                                                       \
        hipError_t e_ = hipGetLastError();                                                     \
        if (e_ != hipSuccess) return wunet_host::fail(WUNET_E_RUNTIME, "%s:%d HIP error: %s", __FILE__, __LINE__, hipGetErrorString(e_)); \
    } while (0)

// ---- optional per-launch profiler (HIP events on the launch stream), used by bench.py's roofline leg
extern bool g_prof_on;
void prof_begin(hipStream_t st, const char* name, double flops, double bytes);
void prof_end(hipStream_t st);
long long prof_collect(char* buf, size_t cap);
extern unsigned long long* g_h3_trace;       // wunet_debug_set_conv_trace

inline int ilog2(long long v) { int r = 0; while ((1LL << r) < v) ++r; return r; }
inline bool is_pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }
inline size_t align64(size_t v) { return (v + 63) & ~(size_t)63; }
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
// blocks of a grid-stride launch: one per per_block elements of n, at most cap
inline unsigned capped_blocks(size_t n, size_t per_block, size_t cap) { const size_t b = (n + per_block - 1) / per_block; return (unsigned)(b < cap ? b : cap); }
inline int kc_of(int taps) { return wunet_lds::conv_mfma(taps, 1).kc; }      // input channels per K chunk of conv_mfma_kernel

// Tiling of one implicit-GEMM conv: rows = output channels of the GEMM, kch = its K channels.
struct ConvCfg { int mrep, nrep, mtiles_p, mblocks, cp, grid_x, ksplit, kcps; };
ConvCfg plan_conv(int B, int L, int rows, int kch, int taps);
ConvArgs make_conv_args(const float* x, int kch, const float* wpk, const float* bias, float* out, float* stats,
                        int B, int rows, int L, int taps, const ConvCfg& c, size_t split_stride);
int launch_conv(int taps, const ConvArgs& a, const ConvCfg& c, hipStream_t st);

struct WgradCfg { int mrep, nw, xit, wsplit, mblocks, nblocks, ksplit, cps, rows; };
WgradCfg plan_wgrad(int B, int L, int cin, int cout, int taps);
WgradArgs make_wgrad_args(const float* x, const float* g, float* part, int B, int Cin, int Cout, int L, int taps, int cps);
int launch_wgrad_any(int taps, const WgradArgs& a, const WgradCfg& w, hipStream_t st);

enum { LK_RAW = 0, LK_DECIM = 1, LK_UPCAT = 2 };

// Every environment switch of the planner, read once by read_plan_switches() when a context is planned (wunet_create, wunet_set_h3)
// or a split single-op entry point is called; nothing else in wunet_plan.cpp reads the environment.
//   variable               effect                                                                            kind
//   WUNET_H3_ORDER         rows-per-wave preference of conv_h3d_kernel, forward GEMM (levels >= 256 samples)  test hook
//   WUNET_H3D_ORDER        ... of the data gradient                                                           test hook
//   WUNET_H3W_ORDER        ... of the split weight gradient                                                   test hook
//   WUNET_H3_NOSPLIT       no split-K on conv_h3d_kernel (the un-split epilogue on small shapes)              test hook
//   WUNET_H3_SPS=<n>       K stages per split (tools/conv_bench.py sweeps it per layer)                       measurement hook
//   WUNET_H3_OLDSPLIT      the split-K rule of rounds 1 - 3                                                   A/B switch
//   WUNET_H3_KTAIL=0       the K tail as one zero-padded chunk everywhere                                     A/B switch
//   WUNET_H3U=<e>[,<t>]    conv_h3u_kernel from <e> samples in eval, <t> in training (one number: both; 0: off) A/B switch
//   WUNET_NO_SKIP_FUSE     the decoder-side operand pass reads the skip itself (eval mode's path)             test hook
//   WUNET_NO_EVOP          no conv writes the next encoder layer's operand                                    A/B switch
//   WUNET_NO_E0            the first layer's weight gradient as a GEMM of its own                             A/B switch
//   WUNET_NO_ENC_GZ        the encoder layers' g written by pass A and read back, not recomputed by gz_split_h3_kernel  A/B switch
//   WUNET_PA_SWAP=0        pass A on the (channels, pieces) grid of rounds 1 - 3                              A/B switch
//   WUNET_UPT=0            no data gradient stores its upsampled half at the producer's resolution            A/B switch
//   WUNET_WGRAD_XCD=0      wgrad_h3d_kernel keeps its 3-D grid                                                A/B switch
//   WUNET_A_CAP=<n>        most pieces of a channel in the gradient-assembly pass (1 .. 256, default 128)     measurement hook
struct PlanSwitches {
    const char *order_f, *order_d, *order_w;      // nullptr: the planner's own order (the text lives in the environment: use it within the call)
    bool no_split, old_split, ktail_off, no_skip_fuse, no_evop, no_e0, no_enc_gz, pa_swap_off, upt_off, wgrad_xcd_off;
    int sps, h3u_eval, h3u_train, a_cap;          // sps < 1: the planner's rule
};
PlanSwitches read_plan_switches();

// Tiling of conv_h3d_kernel for one GEMM (rows x B*L positions, K = kch channels x taps): accumulator rows per wave, padded
// m-tiles, chunks of 32 K channels, K stages per split and the split count, steps of a K tail stage (0: the last chunk is padded to
// 32 channels).  Shared by the network planner and the single-op entry points, so a geometry gets the same kernel instantiation either way.
struct H3ConvPlan { int mrep, mtp, nch, sps, ksplit, ntiles, ntt; };
H3ConvPlan plan_h3_conv(int B, int L, int rows, int kch, int taps, bool transposed, int bf, const PlanSwitches& sw);
// Tiling of the split weight gradient: rows per wave, grid, chunks of tp positions per split, the XCD-aware walk (the blocks of one K
// split on one XCD), and the kernel: dma = wgrad_h3d_kernel (DMA-staged) instead of wgrad_h3_kernel, db = its double-buffered form
struct H3WgradPlan { int mrep, mblocks, nblocks, ksplit, cps, tp, xcd, dma, db; };
H3WgradPlan plan_h3_wgrad(int B, int L, int cin, int cout, int taps, int bf, const PlanSwitches& sw);

// what wunet_create sets: the layer as the model defines it
struct LayerGeom {
    int cin, cout, taps, L, logL, kind;
    int Lt;              // samples of a row that exist: L is the power-of-two row stride, Lt <= L (lengths m*2^n; Lt == L otherwise)
    int src0, src1;      // producer layers (src0 = -1: network input)
    int c0;              // UPCAT: channels from the upsampled branch
};
// what layout_workspace decides and allots: all of it written anew on every planning of the context
struct LayerDecisions {
    ConvCfg f;           // forward conv (rows = cout, K channels = cin)
    ConvCfg d;           // data gradient (rows = cin, K channels = cout)
    WgradCfg w;          // weight gradient
    int f_rows;          // BN statistics partial rows written by the forward conv
    int a_split;         // pass A position splits
    size_t f_wpk, d_wpk; // float offsets inside the forward / backward weight packs
    // workspace (float offsets)
    size_t z, a, s, mean, rstd, xin, g, dx, k1, k2, k3;
    size_t wl1;          // cout absolute row sums of the conv weight (eval mode: the bound conv_h3d_kernel<.., EVOP> scales the next operand by)
    int evop;            // eval mode: this encoder layer's conv also writes the next layer's operand (no prep_h3_kernel<0> for that one)
    // fp16-split path
    int h3f, h3d, h3w;            // forward conv / data gradient use conv_h3d_kernel, the weight gradient wgrad_h3[d]_kernel
    H3ConvPlan hf, hd;            // ... their tilings (the split counts also as f.ksplit / d.ksplit)
    H3WgradPlan hw;
    int first;                    // encoder[0] (Cin = 1): direct fp32 kernel (conv_first_kernel)
    int h3x;                      // the conv input exists only in the split layout (no fp32 xin)
    int skip_from;                // decoder layer: > 0 = its skip half is written by the operand pass of encoder-side layer skip_from
    int h3u, h3u_train;           // conv_h3u_kernel (operand pass fused into the conv's loader waves) runs the eval / also the training forward
    int feeds_h3;                 // the layer's activation is the (or a) source of a conv input that exists in the split layout
    size_t xh, xl, xzp;           // split activated input (float offsets): hi plane, lo plane right behind it, then 16 zero bytes (DMA pad)
    size_t gzh, gzl, gzp;         // split scaled g_z (float offsets), likewise
    size_t h3f_wpk, h3d_wpk;      // half offsets inside the split weight packs
    int upt;                      // a decoder layer whose data gradient stores its upsampled rows at the producer's resolution (conv_h3d_kernel<.., UPT>)
    size_t dxh, usp;              // ... [B][c0][L/2] and the tile-edge terms [2][c0][tiles]
};
struct LayerPlan : LayerGeom, LayerDecisions {};

int h3_stage_count(int kch, int taps, int ntt);
size_t h3w_part_stride(const LayerGeom& g, const H3WgradPlan& w);
// resident blocks per CU the split-K rules of the two weight-gradient planners count on (tools/plan_dump.cpp --check holds the layouts' bytes against them)
int wgrad_blocks_per_cu(const WgradCfg& w, int L, int taps);
int h3w_blocks_per_cu(int taps, int mrep, int L);
bool up_pairs_regular(int Lin);       // the x2 upsample reads the source pairs ((j-1) >> 1, +1) at this length (fp32 coordinates, host check)
unsigned pack_gx();

}  // namespace wunet_host

struct wunet_ctx {
    int n, ci, B, T, NL;
    int Tt = 0;                   // the caller's frame length (T: rounded up to a power of two, the row stride of every level)
    bool padded = false;          // Tt < T
    size_t pad_in = 0, pad_out = 0, pad_gout = 0;      // padded copies of noisy / enhanced / grad_enhanced (float offsets; padded only)
    std::vector<wunet_host::LayerPlan> ly;
    size_t stats_off, wpkf_off, spart_off, fwd_floats;
    size_t bmax_off, bound_off;   // pass A maxima / per-channel |g_z| bounds (fp16-split scale)
    size_t bpart_off, wgpart_off, wpkb_off, gh_off, hpart_off, hpart2_off, e0part_off, total_floats;
    int e0 = 1;                   // the first layer's weight gradient from pass A's sums (pass_a_kernel<.., E0>); WUNET_NO_E0=1, read when the context is planned: off
    int enc_gz = 1;               // gz_split_h3_kernel recomputes the encoder layers' g (GZ_ENC) instead of reading it back; WUNET_NO_ENC_GZ=1, likewise: off
    int pa_swap = 1;              // pass A on the (pieces, channels) grid; WUNET_PA_SWAP=0, likewise: off
    int head_blocks;
    int h3 = 0;                   // fp16-split GEMMs: 0 off, 1 where the planner wants them, 2 wherever they can run
    int bf = 0;                   // the split kernels run their bf16 mode (one bf16 word per operand value, one MFMA pass)
    // wunet_set_bn_frozen: per-layer BatchNorm on the running statistics (nn.BatchNorm1d in eval mode) inside a training forward and
    // its backward; all zero = every layer on batch statistics (the default).  Host state only: read when a call enqueues its launches.
    std::vector<unsigned char> frozen;
    bool any_frozen = false;
    size_t h3_wf_hi, h3_wf_lo, h3_wb_hi, h3_wb_lo, h3_slot;   // float offsets
    size_t fslot_off, wmax_off;   // forward segment: WUNET_SLOT_FLOATS per layer (x / weight scales, activation bound), partial max |W|
    size_t h3_wf_halfs, h3_wb_halfs;
    // side stream for the weight-gradient GEMMs (off the backward's critical chain): one per device the ctx is used on, created
    // lazily under the lock and never replaced, so replicas of one shape on several devices (or threads) do not disturb each other.
    // Everything else in the ctx is immutable after wunet_create / wunet_set_h3 / wunet_set_bn_frozen.
    struct Side {
        hipStream_t stream = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_pack = nullptr, ev_fpack = nullptr, ev_fpack2 = nullptr;
        const void* packed_ws = nullptr;      // the workspace whose backward weight packs the last training forward enqueued on `stream`
    };
    std::map<int, Side> side;
    std::mutex side_lock;
};

namespace wunet_host {

void layout_workspace(wunet_ctx* c);
int launch_split(const float* x, wunet_half* hi, wunet_half* lo, const float* sc, const float* xb0, const float* xb1, float* xsc,
                 int B, int C, int L, hipStream_t st, int bf = 0);
// the per-layer scale slots of the split kernels inside the workspace: {scale, 1 / scale} of the conv operand and of the weight, the
// bound of the layer's activation (forward segment, WUNET_SLOT_FLOATS per layer), {scale, 1 / scale} of g_z (backward segment)
float* x_scale_slot(const wunet_ctx* c, float* ws, int layer);
float* w_scale_slot(const wunet_ctx* c, float* ws, int layer);
float* act_bound_slot(const wunet_ctx* c, float* ws, int layer);
float* gz_scale_slot(const wunet_ctx* c, float* ws, int layer);
// (op: eval mode, the conv also writes the next encoder layer's operand - ConvH3Args::op_*, conv_h3d_kernel<.., EVOP>)
struct ConvH3OpOut { wunet_half* h; wunet_half* l; const float* wl1; const float* xmax; float* xsc; int C8; };
// (upt: training backward of a decoder layer, the rows < c0 stored pulled back through the upsample - ConvH3Args::uh_*, conv_h3d_kernel<.., UPT>)
struct ConvH3Upt { int c0; float up_scale; float* uh_out; float* uh_spill; };
// one launch of conv_h3d_kernel; a caller fills what it uses, the rest stays zero
struct ConvH3Launch {
    int taps, mrep, mtiles_p, sps, nch, ntt;         // the tiling (plan_h3_conv)
    int B, rows, kch, L, bf;                         // the GEMM: rows x B*L positions, K = kch channels x taps
    const wunet_half *xh, *xl, *wh, *wl;             // split operand and weight pack
    const void* zpad;                                // the operand's zero pad (DMA)
    const float *bias, *sc, *sc2;                    // sc / sc2: {scale, 1 / scale} of the operand / of the weight
    float *out, *stats;
    const float *ev_a, *ev_s; float* xrows;          // eval: BatchNorm scale / shift, the activation bound the epilogue folds its maxima into
    const ConvH3OpOut* op;
    const ConvH3Upt* upt;
};
int launch_conv_h3(const ConvH3Launch& k, hipStream_t st);
int launch_conv_h3u(const ConvH3uArgs& a, int mrep, int mtiles_p, int kch, hipStream_t st);
int launch_wgrad_h3(const LayerGeom& g, const H3WgradPlan& w, const wunet_half* xh, const wunet_half* xl, const wunet_half* gh, const wunet_half* gl,
                    const float* sc, const float* sc2, float* part, int B, hipStream_t st, int bf = 0);
int launch_backward_packs(wunet_ctx* c, const float* const* params, float* ws, hipStream_t st);
// the side stream + fork / join events of the CURRENT device (nullptr + error text on failure)
wunet_ctx::Side* side_for_current_device(wunet_ctx* c);
bool side_stream_off();     // WUNET_NO_SIDE_STREAM is set (read once per process)

}  // namespace wunet_host
