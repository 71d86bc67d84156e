// wunet_backward[_range[_async]] / wunet_backward_join: the backward of the network, whole or by layer ranges (see wunet_host.h).
#include "wunet_host.h"
#include "wunet_elementwise.h"
#include "wunet_tiny.h"
#include "wunet_h3_elem.h"
#include "wunet_input_grad.h"

using namespace wunet_host;

namespace {
// ---- measurement hook (WUNET_STAMP=1; bench.py prints the slots): one-thread kernels that write the device's 100 MHz wall clock into a slot, enqueued
// beside the backward's launches - in FRONT of a layer's data gradient on the caller's stream (slot 2 i), in FRONT of its weight gradient on
// the side stream (slot 2 i + 1), at the join (slots 126, 127).  They are captured into a step graph like any launch, so a REPLAY can be asked
// when its two chains really ran - a tracer changes how a graph is submitted.  Off: no launches, no allocation.  (The buffer is allocated by
// the first backward that runs with the switch on: an eager warm-up step, never inside a capture.)
#ifndef WUNET_EMU
__global__ void stamp_kernel(unsigned long long* p) { *p = wall_clock64(); }
unsigned long long* g_stamps = nullptr;
bool stamps_on()
{
    static const bool on = getenv("WUNET_STAMP") != nullptr;
    if (on && !g_stamps && (hipMalloc(&g_stamps, 128 * sizeof(unsigned long long)) != hipSuccess || hipMemset(g_stamps, 0, 128 * sizeof(unsigned long long)) != hipSuccess)) g_stamps = nullptr;
    return on && g_stamps;
}
#define WUNET_STAMP(stream_, slot_) { if (stamps_on()) hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(1), 0, stream_, g_stamps + (slot_)); }
#else
#define WUNET_STAMP(stream_, slot_) {}
#endif

// dx of an encoder-side layer i (1 <= i <= n: encoder 1 .. middle) has ONE reader, pass A of layer i - 1, the next kernel on the
// stream: a split-K data gradient leaves its partials in the scratch and that pass adds them itself, in split order (same bits), instead
// of a split_sum_kernel launch in between.  (A decoder layer's dx is read again much later - its skip half by the encoder side - and is
// summed as before.)
bool dx_stays_split(const wunet_ctx* c, int i)
{
    if (i < 1 || i > c->n) return false;
    const LayerPlan& l = c->ly[i];
    return l.d.ksplit > 1 && l.L >= 4 && c->ly[i - 1].L >= 4;       // (neither end on the scalar kernels of the 1-2-sample levels)
}

// a level of < 4 samples: the scalar kernels (g_z written in place of g)
bool bwd_tiny(const wunet_ctx* c, int i) { return c->ly[i].L < 4; }
// a whole channel in one pass of one block (the levels of <= 16 samples at batch 64)
bool bwd_one_block(const wunet_ctx* c, int i) { return c->ly[i].a_split == 1 && (size_t)c->B * c->ly[i].L <= 4 * WUNET_THREADS; }
// ... with the BatchNorm-backward finalize and g_z inside pass A - two launches of ~5 us (latency, not bandwidth) less per such level
bool bwd_fuse(const wunet_ctx* c, int i) { return !bwd_tiny(c, i) && i < c->NL - 1 && !(i > 0 && c->ly[i].h3d) && bwd_one_block(c, i); }

// The UPT hand-off (planned by layout_workspace, LayerPlan::upt) is ONE decision read by both of its ends: decoder layer q's data
// gradient stores the rows of its upsampled half at the producer's resolution (conv_h3d_kernel<.., UPT>: dxh, usp) if and only if pass A
// and gz_split_h3_kernel of layer q - 1 read them there (pass_a_kernel<A_UPH>, GZ_UPH) - the producer's gradient assembly is then
// elementwise.  Were the two ends decided apart and ever disagreed, pass_a_kernel<A_UP> would read stale rows of dx.
bool upt_handoff(const wunet_ctx* c, int q) { return q > c->n && q < c->NL && c->ly[q].upt; }
// what both ends rely on at run time: the data gradient un-split on the split kernels, its upsampled half produced by layer q - 1, that
// layer's g_z on the split kernels (neither the scalar kernels nor the finalize inside pass A)
bool upt_handoff_sound(const wunet_ctx* c, int q)
{
    const LayerPlan& l = c->ly[q];
    return l.src0 == q - 1 && l.h3d && l.d.ksplit == 1 && c->ly[q - 1].h3d && !bwd_tiny(c, q - 1) && !bwd_fuse(c, q - 1);
}

// How the backward runs layer i: which kernels, who reads what, and so where its g_z ends up.  The one place where these decisions are
// made - a function of the context and the layer alone (the frozen mask is run-time state and not part of it; the A/B switches were read when
// the context was planned) - for the stages of
// backward_range_impl and for wunet_backward_input, which reads the first layer's g_z in whatever form that backward left it
// (first_layer_gz_source).
enum { DG_NONE = 0, DG_H3 = 1, DG_SCALAR = 2, DG_FP32 = 3 };
struct BwdLayerPlan {
    bool tiny;          // bwd_tiny
    bool fuse;          // bwd_fuse: finalize and g_z inside pass A (g_z written in place of g)
    bool gz_h3;         // g_z on the split kernels: pass A also takes the maxima, gz_split_h3_kernel scales and splits
    bool gz_in_wgrad;   // the first layer: g stored, its weight gradient forms g_z while it stages its chunks
    bool e0;            // ... and its weight gradient's sums are taken by pass A instead: nothing written
    // pass A: its source of dL/d(activation) (A_HEAD / A_UPH / A_UP / A_ENC), the bytes per element it reads there, whether it stores g
    // (no: gz_split_h3_kernel forms g again from the same source - its HEAD / ENC / UPH modes - or, E0, nobody reads it)
    int pa_mode;
    const char* pa_name;
    double g_src_bytes;
    bool stores_g;
    bool swap;          // grid (pieces, channels) instead of (channels, pieces)
    bool g1_split;      // A_ENC: the next encoder layer's data gradient arrives as split-K partials (dx_stays_split)
    bool fin_in_gz;     // the finalize runs in the prologue of gz_split_h3_kernel's blocks
    int gz_mode;        // gz_split_h3_kernel's source of g: GZ_G, or pass A's source again
    // the data gradient: family, split-K partials summed by split_sum_kernel or left to the reader (dx_stays_split), UPT hand-off
    int dgrad;
    bool dx_split, dx_sum;
    bool upt;           // upt_handoff(c, i): this layer's data gradient writes the half-resolution rows
    // algorithmic bytes per element of the gradient assembly (HBM-bound): z + the source of g read, g written where it is stored
    double pa_bytes() const { return 4.0 + g_src_bytes + (stores_g ? 4.0 : 0.0); }
    // ... and of gz_split_h3_kernel, without its output: z + g, or g's source again
    double gz_bytes() const { return 4.0 + (gz_mode == GZ_G ? 4.0 : g_src_bytes); }
};
BwdLayerPlan bwd_layer_plan(const wunet_ctx* c, int i)
{
    const LayerPlan& l = c->ly[i];
    const int NL = c->NL, n = c->n;
    BwdLayerPlan q{};
    q.tiny = bwd_tiny(c, i);
    q.fuse = bwd_fuse(c, i);
    q.gz_h3 = i > 0 && l.h3d;
    // the first layer's g_z has one reader: its weight gradient forms it while it stages its chunks (not where pass A finishes g_z itself)
    q.gz_in_wgrad = i == 0 && !q.tiny && !l.h3d && !l.h3w && l.w.wsplit && !bwd_one_block(c, i);
    // the first layer (Cin = 1, 15 taps): its weight gradient's sums are taken by pass A and finished by the finalize - no g written, no
    // weight-gradient GEMM, no split reduce (the last 66 us of the backward, alone on the chip; WUNET_NO_E0=1 when the context is planned: A/B switch)
    q.e0 = c->e0 && q.gz_in_wgrad && !q.fuse && l.cin == 1 && l.taps == 15 && l.L >= 16 && !dx_stays_split(c, 1) && n >= 1;
    const bool recompute = q.gz_h3 && !q.fuse && !q.tiny;      // gz_split_h3_kernel can form g itself
    q.stores_g = true;
    if (i == NL - 1) {
        // the last layer on the split kernels: its g is recomputed from the head gradient by gz_split_h3_kernel (HEAD mode), not stored
        q.pa_mode = A_HEAD; q.pa_name = "pass_a_kernel<HEAD>"; q.g_src_bytes = 0.0; q.gz_mode = GZ_HEAD;
        q.stores_g = !recompute;
    } else if (i >= n && upt_handoff(c, i + 1)) {
        // a layer behind an upsample whose consumer's data gradient arrives at this layer's resolution: g is not stored
        q.pa_mode = A_UPH; q.pa_name = "pass_a_kernel<UPH>"; q.g_src_bytes = 4.0; q.gz_mode = GZ_UPH;
        q.stores_g = false;
    } else if (i >= n) {
        q.pa_mode = A_UP; q.pa_name = q.tiny ? "pass_a_scalar_kernel<UP>" : "pass_a_kernel<UP>"; q.g_src_bytes = 8.0; q.gz_mode = GZ_G;
    } else {
        // an encoder layer on the split kernels whose two data gradients are whole tensors: g is recomputed by gz_split_h3_kernel (ENC
        // mode) from them instead of written here and read back (WUNET_NO_ENC_GZ=1: A/B switch)
        q.g1_split = dx_stays_split(c, i + 1);
        q.pa_mode = A_ENC; q.pa_name = q.e0 ? "pass_a_kernel<ENC, e0>" : q.tiny ? "pass_a_scalar_kernel<ENC>" : "pass_a_kernel<ENC>"; q.g_src_bytes = 6.0; q.gz_mode = GZ_ENC;
        q.stores_g = !(c->enc_gz && recompute && !q.g1_split) && !q.e0;
    }
    if (q.stores_g) q.gz_mode = GZ_G;
    // grid (pieces, channels): consecutive blocks walk consecutive pieces of ONE channel row (rounds 1 - 3 had (channels, pieces):
    // neighbours 4 L bytes apart; 5.156 -> 5.139 ms per step; WUNET_PA_SWAP=0: A/B switch)
    q.swap = c->pa_swap && l.a_split > 1 && !q.tiny;        // (pass_a_scalar_kernel reads its channel from blockIdx.x)
    // (short levels on the split kernels: the finalize runs in the prologue of gz_split_h3_kernel's blocks instead of a launch of its own)
    q.fin_in_gz = !q.fuse && q.gz_h3 && l.a_split * l.cout <= WUNET_GZ_FIN_LOADS && l.cout <= WUNET_GZ_FIN_C;
    q.dgrad = i == 0 ? DG_NONE : l.h3d ? DG_H3 : q.tiny ? DG_SCALAR : DG_FP32;      // (not needed for the first layer)
    q.dx_split = q.dgrad != DG_NONE && q.dgrad != DG_SCALAR && l.d.ksplit > 1;
    q.dx_sum = q.dx_split && !dx_stays_split(c, i);
    q.upt = upt_handoff(c, i);
    return q;
}

// input_grad_kernel's mode: the first layer's g_z rebuilt from its consumers' data gradients (E0 wrote nothing), formed from the stored g,
// or read as stored (gz_materialize_kernel in place, pass A's fused finalize, the scalar kernels)
int first_layer_gz_source(const wunet_ctx* c)
{
    const BwdLayerPlan q = bwd_layer_plan(c, 0);
    return q.e0 ? IG_ENC : q.gz_in_wgrad ? IG_G : IG_GZ;
}

// the source of encoder layer i's g (0 <= i < n): the skip rows of its decoder partner's data gradient, the next encoder layer's data gradient -
// for pass A, gz_split_h3_kernel's ENC mode and input_grad_kernel<IG_ENC> alike
WunetEncSrc enc_grad_source(const wunet_ctx* c, float* ws, int i)
{
    const LayerPlan& dc = c->ly[2 * c->n - i];
    return WunetEncSrc{ws + dc.dx, ws + c->ly[i + 1].dx, dc.cin, dc.c0};
}

// what every stage of one backward call shares
struct BwdCall {
    wunet_ctx* c; float* ws; const float* const* params; float* const* grads; const float* noisy;
    hipStream_t st, sd;           // the caller's stream (the critical chain), the weight gradients' stream (== st: one stream)
    wunet_ctx::Side* side;
};

// ---- the backward's weight packs and the head: gh = gout * tanh', d wh, d bh
int head_backward(const BwdCall& k, void* workspace, const float* enhanced, const float* grad_enhanced)
{
    wunet_ctx* c = k.c; float* ws = k.ws; const hipStream_t st = k.st;
    // flipped/transposed weights for every data gradient: already enqueued on the side stream by the training forward of this
    // workspace (they only depend on the weights: off the critical path), else packed here
    if (k.side->packed_ws == workspace && k.sd != st) {
        k.side->packed_ws = nullptr;
        if (hipStreamWaitEvent(st, k.side->ev_pack, 0) != hipSuccess) return fail(WUNET_E_RUNTIME, "waiting for the weight packs failed");
    } else {
        k.side->packed_ws = nullptr;
        const int rc = launch_backward_packs(c, k.params, ws, st);
        if (rc) return rc;
    }
    const LayerPlan& l = c->ly[c->NL - 1];
    HeadBwdArgs h{};
    h.z = ws + l.z; h.a = ws + l.a; h.s = ws + l.s; h.in = k.noisy; h.out = enhanced; h.gout = grad_enhanced;
    h.gh = ws + c->gh_off; h.part = ws + c->hpart_off; h.B = c->B; h.C = c->ci; h.T = c->T; h.logT = ilog2(c->T);
    WUNET_LAUNCH(head_bwd_kernel, dim3(c->head_blocks), dim3(WUNET_THREADS), 0, st, h);
    WUNET_CHECK_LAUNCH();
    // (d(weight of the input channel), d bias and the ci per-channel head-weight gradients - sums of head_bwd_kernel's and of the last layer's
    //  pass A's partial rows - are parameter gradients nothing on the chain reads: they are taken on the weight-gradient stream, weight_gradient)
    return WUNET_OK;
}

// ---- pass A: assemble dL/d(BN output), LeakyReLU', BN-backward partial sums
// (fz: the layer is frozen by wunet_set_bn_frozen - running statistics in the forward: every finalize emits g_z = a g (k2 = k3 = 0) and the
//  conv bias's gradient a sum g)
int pass_a(const BwdCall& k, int i, const BwdLayerPlan& q, int fz)
{
    wunet_ctx* c = k.c; float* ws = k.ws; const hipStream_t st = k.st;
    const int NL = c->NL;
    const LayerPlan& l = c->ly[i];
    PassAArgs p{};
    p.z = ws + l.z; p.a = ws + l.a; p.s = ws + l.s; p.mean = ws + l.mean; p.rstd = ws + l.rstd;
    p.gpre = q.stores_g ? ws + l.g : nullptr; p.part = ws + c->bpart_off; p.pmax = q.gz_h3 ? ws + c->bmax_off : nullptr;
    p.B = c->B; p.C = l.cout; p.L = l.L; p.logL = l.logL; p.Lt = l.Lt;
    p.swap = q.swap ? 1 : 0;
    const dim3 ga(p.swap ? l.a_split : l.cout, p.swap ? l.cout : l.a_split);
    if (q.fuse) {
        p.gamma = k.params[4 * i + 2]; p.dgamma = k.grads[4 * i + 2]; p.dbeta = k.grads[4 * i + 3]; p.dbias = k.grads[4 * i + 1];
        p.k1 = ws + l.k1; p.k2 = ws + l.k2; p.k3 = ws + l.k3; p.count = (double)c->B * l.Lt; p.frozen = fz;
    }
    prof_begin(st, q.pa_name, 0.0, (double)c->B * l.cout * l.L * q.pa_bytes() + (q.pa_mode == A_HEAD ? 4.0 * c->B * l.L : 0.0));
    if (q.pa_mode == A_HEAD) {
        p.g0 = ws + c->gh_off; p.g1 = k.params[4 * NL]; p.hpart = ws + c->hpart2_off;
        WUNET_LAUNCH(pass_a_kernel<A_HEAD>, ga, dim3(WUNET_THREADS), 0, st, p);      // (the last layer has T >= 4 samples)
    } else if (q.pa_mode == A_UPH) {
        // the next decoder layer's data gradient arrived at THIS resolution (conv_h3d_kernel<.., UPT>): elementwise; g is not stored -
        // gz_split_h3_kernel forms it again from the same two arrays (UPH mode)
        const LayerPlan& nx = c->ly[i + 1];
        p.g0 = ws + nx.dxh; p.sp = ws + nx.usp; p.ntiles = (int)(((size_t)c->B * nx.L + 255) / 256); p.tpr = l.L >> 7;
        WUNET_LAUNCH(pass_a_kernel<A_UPH>, ga, dim3(WUNET_THREADS), 0, st, p);
    } else if (q.pa_mode == A_UP) {
        const LayerPlan& nx = c->ly[i + 1];
        p.g0 = ws + nx.dx; p.Cg0 = nx.cin;
        p.up_scale = (float)(l.Lt - 1) / (float)(2 * l.Lt - 1);
        if (q.tiny) WUNET_LAUNCH(pass_a_scalar_kernel<A_UP>, ga, dim3(WUNET_THREADS), 0, st, p);
        else if (q.fuse) WUNET_LAUNCH((pass_a_kernel<A_UP, true>), ga, dim3(WUNET_THREADS), 0, st, p);
        else WUNET_LAUNCH(pass_a_kernel<A_UP>, ga, dim3(WUNET_THREADS), 0, st, p);
    } else {
        const LayerPlan& nx = c->ly[i + 1];
        p.enc = enc_grad_source(c, ws, i);
        if (q.g1_split) {
            p.enc.ge = ws + c->spart_off; p.g1_splits = nx.d.ksplit; p.g1_stride = (size_t)c->B * nx.cin * nx.L;
        }
        if (q.e0) { p.x0 = k.noisy; p.e0rows = ws + c->e0part_off; }
        if (q.tiny) WUNET_LAUNCH(pass_a_scalar_kernel<A_ENC>, ga, dim3(WUNET_THREADS), 0, st, p);
        else if (q.e0) WUNET_LAUNCH((pass_a_kernel<A_ENC, false, false, true>), ga, dim3(WUNET_THREADS), 0, st, p);
        else if (q.fuse && p.g1_splits > 1) WUNET_LAUNCH((pass_a_kernel<A_ENC, true, true>), ga, dim3(WUNET_THREADS), 0, st, p);
        else if (q.fuse) WUNET_LAUNCH((pass_a_kernel<A_ENC, true>), ga, dim3(WUNET_THREADS), 0, st, p);
        else if (p.g1_splits > 1) WUNET_LAUNCH((pass_a_kernel<A_ENC, false, true>), ga, dim3(WUNET_THREADS), 0, st, p);
        else WUNET_LAUNCH(pass_a_kernel<A_ENC>, ga, dim3(WUNET_THREADS), 0, st, p);
    }
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

// ---- BatchNorm-backward finalize, then g_z = k1*g + k2*z + k3, materialised once for both gradient GEMMs (fp32 in place, or scaled
// hi/lo halves).  (Not for a fused layer: pass A did both.)
int finalize_and_gz(const BwdCall& k, int i, const BwdLayerPlan& q, int fz)
{
    wunet_ctx* c = k.c; float* ws = k.ws; const hipStream_t st = k.st;
    const LayerPlan& l = c->ly[i];
    BnBwdArgs b{};
    b.part = ws + c->bpart_off; b.rows = l.a_split; b.gamma = k.params[4 * i + 2]; b.mean = ws + l.mean; b.rstd = ws + l.rstd;
    b.dgamma = k.grads[4 * i + 2]; b.dbeta = k.grads[4 * i + 3]; b.dbias = k.grads[4 * i + 1]; b.k1 = ws + l.k1; b.k2 = ws + l.k2; b.k3 = ws + l.k3;
    b.C = l.cout; b.count = (double)c->B * l.Lt; b.frozen = fz;
    b.pmax = q.gz_h3 ? ws + c->bmax_off : nullptr; b.bound = ws + c->bound_off;
    if (q.e0) { b.e0rows = ws + c->e0part_off; b.dw0 = k.grads[0]; }
    if (!q.fin_in_gz) {
        WUNET_LAUNCH(bn_finalize_bwd_kernel, dim3(l.cout), dim3(WUNET_THREADS), 0, st, b);
        WUNET_CHECK_LAUNCH();
    }
    const size_t n4 = (size_t)c->B * l.cout * l.L / 4;
    if (q.gz_h3) {
        const int c8 = (l.cout + 7) / 8;
        const size_t nt = (size_t)c->B * c8 * (l.L / 4);
        const unsigned hb = capped_blocks(nt, WUNET_THREADS, 8192);
        prof_begin(st, "gz_split_h3_kernel", 0.0, (double)c->B * l.cout * l.L * (q.gz_bytes() + (c->bf ? 2.0 : 4.0)));
        GzHeadArgs hd{};
        if (q.gz_mode != GZ_G) { hd.a = ws + l.a; hd.s = ws + l.s; }
        if (q.gz_mode == GZ_HEAD) { hd.gh = ws + c->gh_off; hd.wh = k.params[4 * c->NL]; }
        if (q.gz_mode == GZ_UPH) hd.gq = ws + c->ly[i + 1].dxh;
        if (q.gz_mode == GZ_ENC) hd.enc = enc_grad_source(c, ws, i);
        // (the source of g is a compile-time mode of the kernel: every load of a thread is issued before its first use)
#define WUNET_GZ_LAUNCH(FIN_, GM_, BF_)                                                                                                               \
    WUNET_LAUNCH((gz_split_h3_kernel<FIN_, GM_, BF_>), dim3(hb), dim3(WUNET_THREADS), 0, st, (const float*)(ws + l.g), (const float*)(ws + l.z), \
                 (const float*)(ws + l.k1), (const float*)(ws + l.k2), (const float*)(ws + l.k3), (const float*)(ws + c->bound_off),                 \
                 gz_scale_slot(c, ws, i), reinterpret_cast<wunet_half*>(ws + l.gzh), reinterpret_cast<wunet_half*>(ws + l.gzl),                      \
                 c->B, l.cout, c8, l.L, l.logL, l.Lt, b, hd)
#define WUNET_GZ_MODE(GM_)                                                                                                                            \
    case GM_:                                                                                                                                         \
        if (q.fin_in_gz) { if (c->bf) WUNET_GZ_LAUNCH(true, GM_, true); else WUNET_GZ_LAUNCH(true, GM_, false); }                                     \
        else { if (c->bf) WUNET_GZ_LAUNCH(false, GM_, true); else WUNET_GZ_LAUNCH(false, GM_, false); }                                               \
        break;
        switch (q.gz_mode) { WUNET_GZ_MODE(GZ_G) WUNET_GZ_MODE(GZ_HEAD) WUNET_GZ_MODE(GZ_ENC) WUNET_GZ_MODE(GZ_UPH) }
#undef WUNET_GZ_MODE
#undef WUNET_GZ_LAUNCH
        prof_end(st);
    } else if (q.tiny) {
        prof_begin(st, "gz_scalar_kernel", 0.0, 12.0 * c->B * l.cout * l.L);
        WUNET_LAUNCH(gz_scalar_kernel, dim3((unsigned)((n4 * 4 + WUNET_THREADS - 1) / WUNET_THREADS) + 1), dim3(WUNET_THREADS), 0, st, (const float*)(ws + l.g),
                     (const float*)(ws + l.z), (const float*)(ws + l.k1), (const float*)(ws + l.k2), (const float*)(ws + l.k3), l.cout, l.logL,
                     (size_t)c->B * l.cout * l.L, ws + l.g);
        prof_end(st);
    } else if (!q.gz_in_wgrad) {
        WUNET_LAUNCH(gz_materialize_kernel, dim3(capped_blocks(n4, WUNET_THREADS, 8192)), dim3(WUNET_THREADS), 0, st, (const float*)(ws + l.g), (const float*)(ws + l.z),
                     (const float*)(ws + l.k1), (const float*)(ws + l.k2), (const float*)(ws + l.k3), l.cout, l.logL, n4, ws + l.g, l.Lt);   // in place
    }
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

// the partials of a split-K data gradient summed into dx, in split order
int sum_dx_splits(const BwdCall& k, const LayerPlan& l)
{
    const size_t nd = (size_t)k.c->B * l.cin * l.L;
    WUNET_LAUNCH(split_sum_kernel, dim3(capped_blocks(nd, WUNET_THREADS, 2048)), dim3(WUNET_THREADS), 0, k.st, (const float*)(k.ws + k.c->spart_off), l.d.ksplit, nd, k.ws + l.dx, (const float*)nullptr, 1, 0);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

// ---- data gradient: the same conv kernel on the flipped/transposed pack
int data_gradient(const BwdCall& k, int i, const BwdLayerPlan& q)
{
    wunet_ctx* c = k.c; float* ws = k.ws; const hipStream_t st = k.st;
    const LayerPlan& l = c->ly[i];
    float* const dx = q.dx_split ? ws + c->spart_off : ws + l.dx;
    if (q.dgrad == DG_H3) {
        // fp16-split data gradient: scale g_z by a power of two into fp16's range, split, 3 MFMA passes, un-scale
        // (UPT: the rows of the upsampled half leave at the producer's resolution - upt_handoff)
        ConvH3Upt up{};
        if (q.upt) {
            up.c0 = l.c0; up.up_scale = (float)(l.Lt / 2 - 1) / (float)(l.Lt - 1);
            up.uh_out = ws + l.dxh; up.uh_spill = ws + l.usp;
        }
        ConvH3Launch h{};
        h.taps = l.taps; h.mrep = l.hd.mrep; h.mtiles_p = l.hd.mtp; h.sps = l.hd.sps; h.nch = l.hd.nch; h.ntt = l.hd.ntt;
        h.B = c->B; h.rows = l.cin; h.kch = l.cout; h.L = l.L; h.bf = c->bf;
        h.xh = reinterpret_cast<wunet_half*>(ws + l.gzh); h.xl = reinterpret_cast<wunet_half*>(ws + l.gzl); h.zpad = ws + l.gzp;
        h.wh = reinterpret_cast<const wunet_half*>(ws + c->h3_wb_hi) + l.h3d_wpk; h.wl = reinterpret_cast<const wunet_half*>(ws + c->h3_wb_lo) + l.h3d_wpk;
        h.sc = gz_scale_slot(c, ws, i); h.sc2 = w_scale_slot(c, ws, i); h.out = dx;
        h.upt = q.upt ? &up : nullptr;
        const int rc = launch_conv_h3(h, st);
        if (rc) return rc;
        WUNET_CHECK_LAUNCH();
    } else if (q.dgrad == DG_SCALAR) {
        const size_t nd = (size_t)c->B * l.cin * l.L;
        WUNET_LAUNCH(tiny_conv_kernel, dim3((unsigned)((nd + WUNET_THREADS - 1) / WUNET_THREADS)), dim3(WUNET_THREADS), 0, st,
                     (const float*)(ws + l.g), k.params[4 * i], ws + l.dx, c->B, l.cout, l.cin, l.L, l.logL, l.taps, 1);
        WUNET_CHECK_LAUNCH();
    } else if (q.dgrad == DG_FP32) {
        const ConvArgs a = make_conv_args(ws + l.g, l.cout, ws + c->wpkb_off + l.d_wpk, nullptr, dx, nullptr, c->B, l.cin, l.L, l.taps, l.d,
                                          (size_t)c->B * l.cin * l.L);
        const int rc = launch_conv(l.taps, a, l.d, st);
        if (rc) return rc;
        WUNET_CHECK_LAUNCH();
    }
    return q.dx_sum ? sum_dx_splits(k, l) : WUNET_OK;
}

// ---- weight gradient on the side stream: GEMM over positions on the materialised operands, split-K partials + deterministic reduce
int weight_gradient(const BwdCall& k, int i, const BwdLayerPlan& q)
{
    wunet_ctx* c = k.c; float* ws = k.ws; const hipStream_t sd = k.sd;
    const int NL = c->NL;
    const LayerPlan& l = c->ly[i];
    if (sd != k.st && hipStreamWaitEvent(sd, k.side->ev_fork, 0) != hipSuccess) return fail(WUNET_E_RUNTIME, "fork onto the weight-gradient stream failed");
    WUNET_STAMP(sd, 2 * i + 1)
    if (i == NL - 1) {
        // the head's parameter gradients (rounds 1 - 6: two 4.7 us launches between the kernels of the main chain, which never reads them):
        // d(weight of the input channel), d bias from head_bwd_kernel's rows; the ci per-channel weight gradients from pass A's
        WUNET_LAUNCH(rows_sum_kernel, dim3(2), dim3(WUNET_THREADS), 0, sd,
                     (const float*)(ws + c->hpart_off), c->head_blocks, 2, k.grads[4 * NL] + c->ci, 1, k.grads[4 * NL + 1]);
        WUNET_CHECK_LAUNCH();
        WUNET_LAUNCH(rows_sum_kernel, dim3(c->ci), dim3(WUNET_THREADS), 0, sd,
                     (const float*)(ws + c->hpart2_off), l.a_split, c->ci, k.grads[4 * NL], c->ci, k.grads[4 * NL + 1]);
        WUNET_CHECK_LAUNCH();
    }
    if (q.e0) return WUNET_OK;                          // (finished by bn_finalize_bwd_kernel from pass A's sums)
    const float* xin = i == 0 ? k.noisy : ws + l.xin;
    const size_t nw = (size_t)l.cout * l.cin * l.taps;
    if (q.tiny) {
        prof_begin(sd, "tiny_wgrad_kernel", 2.0 * c->B * l.L * nw, 4.0 * c->B * l.L * (l.cout + l.cin));
        WUNET_LAUNCH(tiny_wgrad_kernel, dim3((unsigned)((nw + WUNET_THREADS - 1) / WUNET_THREADS)), dim3(WUNET_THREADS), 0, sd,
                     (const float*)(ws + l.g), xin, k.grads[4 * i], c->B, l.cin, l.cout, l.L, l.taps);
        prof_end(sd);
        WUNET_CHECK_LAUNCH();
        return WUNET_OK;
    }
    int rc;
    if (l.h3w)
        rc = launch_wgrad_h3(l, l.hw, reinterpret_cast<const wunet_half*>(ws + l.xh), reinterpret_cast<const wunet_half*>(ws + l.xl),
                             reinterpret_cast<const wunet_half*>(ws + l.gzh), reinterpret_cast<const wunet_half*>(ws + l.gzl),
                             gz_scale_slot(c, ws, i), x_scale_slot(c, ws, i),
                             ws + c->wgpart_off, c->B, sd, c->bf);
    else {
        WgradArgs w = make_wgrad_args(xin, ws + l.g, ws + c->wgpart_off, c->B, l.cin, l.cout, l.L, l.taps, l.w.cps);
        if (q.gz_in_wgrad) {
            w.z = ws + l.z; w.k1 = ws + l.k1; w.k2 = ws + l.k2; w.k3 = ws + l.k3; w.Lt = l.Lt;
        }
        rc = launch_wgrad_any(l.taps, w, l.w, sd);
    }
    if (rc) return rc;
    WUNET_CHECK_LAUNCH();
    if (l.h3w) {
        WgradH3ReduceArgs ra{};
        ra.part = ws + c->wgpart_off; ra.part_stride = h3w_part_stride(l, l.hw); ra.splits = l.hw.ksplit; ra.dw = k.grads[4 * i];
        ra.Cout = l.cout; ra.Cin = l.cin; ra.taps = l.taps; ra.mrep = l.hw.mrep; ra.tw = l.taps == 15 ? 8 : 5;
        ra.nblocks = l.hw.nblocks; ra.mblocks = l.hw.mblocks; ra.cib = l.taps == 15 ? 32 : 64;
        // few splits over many outputs: the barrier-free serial form (64, 8192: 6.19 -> 6.13 ms per step in round 1).
        // Emulator-build test hook WUNET_REDUCE_SERIAL = "<max splits>,<min float4 outputs>": tiny shapes reach that kernel
        int serial_max = 64; long long serial_min_n4 = 8192;
#ifdef WUNET_EMU
        if (const char* e = getenv("WUNET_REDUCE_SERIAL")) sscanf(e, "%d,%lld", &serial_max, &serial_min_n4);
#endif
        const size_t n4 = ra.part_stride / 4;
        const bool serial = ra.splits <= serial_max && (long long)n4 >= serial_min_n4;
        prof_begin(sd, serial ? "wgrad_h3_reduce_serial_kernel" : "wgrad_h3_reduce_kernel", 0.0, 4.0 * ra.part_stride * (ra.splits + 1.0));
        if (serial) {
            WUNET_LAUNCH(wgrad_h3_reduce_serial_kernel, dim3(capped_blocks(n4, WUNET_THREADS, 4096)), dim3(WUNET_THREADS), 0, sd, ra);
        } else {
            WUNET_LAUNCH(wgrad_h3_reduce_kernel, dim3(capped_blocks(n4, 16, 4096)), dim3(WUNET_THREADS), 0, sd, ra);
        }
        prof_end(sd);
    } else {
        const unsigned blocks = capped_blocks(nw / 4, 16, 4096);                   // 16 float4 groups of outputs per block
        WUNET_LAUNCH(wgrad_reduce_kernel, dim3(blocks < 1 ? 1 : blocks), dim3(WUNET_THREADS), 0, sd,
                     (const float*)(ws + c->wgpart_off), l.w.rows, nw, k.grads[4 * i]);
    }
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

int backward_range_impl(wunet_ctx* c, const float* noisy, const float* const* params, const float* enhanced,
                        const float* grad_enhanced, void* workspace, float* const* grads,
                        int layer_begin, int layer_end, void* stream, bool join)
{
    if (!c || !noisy || !params || !enhanced || !grad_enhanced || !workspace || !grads) return fail(WUNET_E_ARG, "null argument");
    if (layer_begin < 0 || layer_end > c->NL || layer_begin >= layer_end) return fail(WUNET_E_ARG, "bad layer range");
    // (both ends of a UPT hand-off read LayerPlan::upt; a plan that sets it where they cannot run is refused before anything is launched)
    for (int q = c->n + 1; q < c->NL; ++q)
        if (upt_handoff(c, q) && !upt_handoff_sound(c, q)) return fail(WUNET_E_ARG, "layer %d: UPT planned where the data gradient or its producer cannot run it", q);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const int NL = c->NL;
    // weight gradients run on a side stream: they only depend on g_z and x of their own layer, so the HBM-bound
    // gradient-assembly kernels of the next layers overlap with them instead of idling the matrix cores
    wunet_ctx::Side* side = side_for_current_device(c);
    if (!side) return WUNET_E_RUNTIME;
    hipStream_t sd = (g_prof_on || side_stream_off()) ? st : side->stream;  // the per-kernel profiler serialises everything on one stream
    if (c->padded) {
        // the forward's zero-padded copies of the input and of the result are still in the workspace; the incoming gradient is
        // padded with zeros here (the head's backward then gives the row padding a zero gradient)
        if (layer_end == NL &&
            (hipMemsetAsync(ws + c->pad_gout, 0, (size_t)c->B * c->T * sizeof(float), st) != hipSuccess ||
             hipMemcpy2DAsync(ws + c->pad_gout, (size_t)c->T * sizeof(float), grad_enhanced, (size_t)c->Tt * sizeof(float),
                              (size_t)c->Tt * sizeof(float), (size_t)c->B, hipMemcpyDeviceToDevice, st) != hipSuccess))
            return fail(WUNET_E_RUNTIME, "padding the output gradient failed");
        noisy = ws + c->pad_in; enhanced = ws + c->pad_out; grad_enhanced = ws + c->pad_gout;
    }
    const BwdCall k{c, ws, params, grads, noisy, st, sd, side};
    if (layer_end == NL) { const int rc = head_backward(k, workspace, enhanced, grad_enhanced); if (rc) return rc; }

    for (int i = layer_end - 1; i >= layer_begin; --i) {
        const BwdLayerPlan q = bwd_layer_plan(c, i);
        const int fz = (c->any_frozen && c->frozen[i]) ? 1 : 0;      // (run-time state: wunet_set_bn_frozen may change it between calls)
        int rc = pass_a(k, i, q, fz);
        if (rc) return rc;
        if (!q.fuse && (rc = finalize_and_gz(k, i, q, fz)) != 0) return rc;
        // The weight gradient's fork EVENT is recorded here, right behind g_z; the side stream's launches are issued after the data gradient's, so
        // that the kernel of the critical chain is enqueued - and, in a captured graph, created - FIRST: its persistent blocks take the
        // CUs and the weight gradient fills in behind it and beside the next layer's memory-bound passes.  Eager launches got that order
        // anyway (the event wait costs the side stream ~6 us); a captured graph released both kernels at once, the weight gradient
        // won the race (data gradient 204 us instead of 110) and the replay was 10 % slower than the eager step (5.93 -> 5.25 ms with
        // this order, eager 5.26: profiles/r4_graph_vs_eager.txt).
        if (sd != st && hipEventRecord(side->ev_fork, st) != hipSuccess) return fail(WUNET_E_RUNTIME, "fork onto the weight-gradient stream failed");
        WUNET_STAMP(st, 2 * i)
        if ((rc = data_gradient(k, i, q)) != 0) return rc;
        if ((rc = weight_gradient(k, i, q)) != 0) return rc;
    }
    // join: the caller's stream sees every weight gradient.  An un-joined range (wunet_backward_range_async) leaves them to
    // wunet_backward_join - except the range that ends the backward, which always joins: the next forward overwrites the
    // operands the side stream is still reading.
    if (sd != st && (join || layer_begin == 0)) {
        WUNET_STAMP(st, 126)
        WUNET_STAMP(sd, 127)
        if (hipEventRecord(side->ev_join, sd) != hipSuccess || hipStreamWaitEvent(st, side->ev_join, 0) != hipSuccess)
            return fail(WUNET_E_RUNTIME, "join of the weight-gradient stream failed");
    }
    return WUNET_OK;
}
}  // namespace

extern "C" {

int wunet_backward_range(wunet_ctx* c, const float* noisy, const float* const* params, const float* enhanced,
                         const float* grad_enhanced, void* workspace, float* const* grads,
                         int layer_begin, int layer_end, void* stream)
{
    return backward_range_impl(c, noisy, params, enhanced, grad_enhanced, workspace, grads, layer_begin, layer_end, stream, true);
}

int wunet_backward_range_async(wunet_ctx* c, const float* noisy, const float* const* params, const float* enhanced,
                               const float* grad_enhanced, void* workspace, float* const* grads,
                               int layer_begin, int layer_end, void* stream)
{
    return backward_range_impl(c, noisy, params, enhanced, grad_enhanced, workspace, grads, layer_begin, layer_end, stream, false);
}

// measurement hook: the stamps of the last backward (WUNET_STAMP=1), 128 device wall-clock values (100 MHz; 0 = slot not written)
int wunet_debug_stamps(unsigned long long* out, int n)
{
#ifndef WUNET_EMU
    if (!out || n < 0 || n > 128 || !g_stamps) return fail(WUNET_E_ARG, "no stamps (WUNET_STAMP unset, or no backward ran)");
    return hipMemcpy(out, g_stamps, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? WUNET_OK : fail(WUNET_E_RUNTIME, "copy of the stamps failed");
#else
    (void)out; (void)n; return fail(WUNET_E_ARG, "no stamps in the emulator build");
#endif
}

int wunet_backward_join(wunet_ctx* c, void* stream)
{
    if (!c) return fail(WUNET_E_ARG, "null ctx");
    wunet_ctx::Side* side = side_for_current_device(c);
    if (!side) return WUNET_E_RUNTIME;
    if (g_prof_on || side_stream_off()) return WUNET_OK;                   // the weight gradients ran on the caller's stream
    if (hipEventRecord(side->ev_join, side->stream) != hipSuccess ||
        hipStreamWaitEvent((hipStream_t)stream, side->ev_join, 0) != hipSuccess)
        return fail(WUNET_E_RUNTIME, "join of the weight-gradient stream failed");
    return WUNET_OK;
}

int wunet_backward(wunet_ctx* c, const float* noisy, const float* const* params, const float* enhanced,
                   const float* grad_enhanced, void* workspace, float* const* grads, void* stream)
{
    if (!c) return fail(WUNET_E_ARG, "null ctx");
    return backward_range_impl(c, noisy, params, enhanced, grad_enhanced, workspace, grads, 0, c->NL, stream, true);
}

int wunet_backward_input(wunet_ctx* c, const float* noisy, const float* const* params, void* workspace, float* grad_noisy, void* stream)
{
    // (noisy is not read: the input enters the network linearly - the head's input channel and encoder.0's conv)
    if (!c || !noisy || !params || !workspace || !grad_noisy) return fail(WUNET_E_ARG, "null argument");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const LayerPlan& l = c->ly[0];
    const int src = first_layer_gz_source(c);
    InputGradArgs A{};
    A.z = ws + l.z; A.k1 = ws + l.k1; A.k2 = ws + l.k2; A.k3 = ws + l.k3;
    A.w0 = params[0]; A.wh = params[4 * c->NL]; A.gh = ws + c->gh_off; A.dx = grad_noisy;
    A.B = c->B; A.C = l.cout; A.L = l.L; A.Lt = l.Lt; A.Tt = c->Tt;
    A.vec = (reinterpret_cast<size_t>(grad_noisy) & 15) == 0 && (c->Tt & 3) == 0;
    if (src == IG_ENC) {
        A.a = ws + l.a; A.s = ws + l.s; A.enc = enc_grad_source(c, ws, 0);
    } else {
        A.g = ws + l.g;
    }
    const dim3 grid((unsigned)((l.L + WUNET_IG_TP - 1) / WUNET_IG_TP), (unsigned)c->B);
    // algorithmic bytes: z + the rebuilt gradient's sources (IG_ENC: skip rows, half-length encoder.1 rows), g or g_z; gh read, the result written
    const double pe = (double)c->B * l.cout * l.L;
    prof_begin(st, src == IG_ENC ? "input_grad_kernel<ENC>" : src == IG_G ? "input_grad_kernel<G>" : "input_grad_kernel<GZ>",
               2.0 * 15.0 * pe, pe * (src == IG_ENC ? 10.0 : src == IG_G ? 8.0 : 4.0) + 4.0 * c->B * ((double)l.L + c->Tt));
    if (src == IG_ENC) WUNET_LAUNCH(input_grad_kernel<IG_ENC>, grid, dim3(WUNET_THREADS), 0, st, A);
    else if (src == IG_G) WUNET_LAUNCH(input_grad_kernel<IG_G>, grid, dim3(WUNET_THREADS), 0, st, A);
    else WUNET_LAUNCH(input_grad_kernel<IG_GZ>, grid, dim3(WUNET_THREADS), 0, st, A);
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

}  // extern "C"
