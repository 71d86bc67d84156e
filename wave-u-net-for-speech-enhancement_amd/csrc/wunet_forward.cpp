// wunet_forward: the training / eval forward of the network as one enqueue (see wunet_host.h).
#include "wunet_host.h"
#include "wunet_elementwise.h"
#include "wunet_tiny.h"
#include "wunet_h3_elem.h"

using namespace wunet_host;

namespace {
// The mode of one forward call: everything fwd_layer_plan's decisions depend on besides the context.
// wunet_set_bn_frozen: a frozen layer of a training forward normalises with the running statistics (scale / shift, mean / rstd
// ahead of the chain, no statistics partials, running statistics untouched) and, as nothing bounds its activation then, its
// consumers' operand scale comes from the measured maximum, as in eval mode.  With no layer frozen nothing changes.
struct FwdMode {
    bool training, save;              // save: a backward follows (save_for_backward)
    const unsigned char* frozen;      // the frozen mask where it applies (a training forward of a context with a frozen layer), else nullptr
    bool is_frozen(int i) const { return frozen && i >= 0 && frozen[i] != 0; }
};

// The two hand-offs between layers of a forward are ONE decision each, read by both of their ends (as upt_handoff is in the backward).
// Skip half (training): the operand pass of encoder-side layer skip_from (prep_h3_kernel<1>) also writes the skip half of decoder
// layer d's operand if and only if d's own pass only writes the upsampled half (prep_h3_kernel<3>).  Only when d's x scale is known
// that early: training mode (data-independent activation bounds) with neither source frozen; in eval mode the decoder-side pass
// reads the skip itself.  Not where conv_h3u_kernel builds d's whole operand.  Were the two ends decided apart and ever disagreed,
// d's conv would read a skip half nobody wrote.
bool skip_handoff(const wunet_ctx* c, int d, const FwdMode& m)
{
    if (!m.training || d <= c->n || d >= c->NL) return false;
    const LayerPlan& dl = c->ly[d];
    return dl.skip_from > 0 && !dl.h3u_train && !m.is_frozen(dl.src0) && !m.is_frozen(dl.src1);
}
// EVOP (eval): encoder layer p's conv writes layer p + 1's operand in its epilogue (conv_h3d_kernel<.., EVOP>) if and only if layer
// p + 1 runs no operand pass.
bool evop_handoff(const wunet_ctx* c, int p, const FwdMode& m) { return !m.training && p >= 0 && p < c->NL && c->ly[p].evop; }

// How the forward runs layer i in this mode: which kernels, who writes the conv's operand, who takes the activation bound, how
// BatchNorm is finished.  The one place where these decisions are made - a pure function of the context, the layer and the mode -
// for the stages of wunet_forward.
enum { OP_NONE = 0, OP_IN_CONV, OP_BY_PRODUCER, OP_PREP_H3, OP_SCALAR, OP_DECIM, OP_UPCAT };
enum { CV_FIRST = 0, CV_H3U, CV_H3, CV_TINY, CV_FP32 };
enum { BOUND_NONE = 0, BOUND_EPILOGUE, BOUND_REDUCE, BOUND_ACT_MAX };
struct FwdLayerPlan {
    bool bstats;        // this layer's BatchNorm takes batch statistics
    // the conv's operand: none (the network input), built inside the conv (conv_h3u_kernel, wunet_h3u.h), written by the producing
    // encoder conv's epilogue (evop_handoff), or materialised by a pass: BN scale / shift + LeakyReLU + decimation, or + x2 upsample +
    // skip concat - prep_h3_kernel<op_mode> into the split layout, else an fp32 pass (and launch_split where the conv is a split one)
    int operand;
    int op_mode;        // prep_h3_kernel: 0 decimation, 1 ... + the skip half of decoder layer skip_to, 2 upsample + concat, 3 the upsampled half only
    int skip_to;        // (-1: none)
    bool split_pass;
    const char* op_name;        // profiler name of the operand pass (nullptr: not profiled) and its algorithmic bytes per (row, sample)
    double op_bytes;            // position (HBM-bound): fp32 sources read once, 2 + 2 (bf16: 2) bytes per value written
    int conv;           // the conv family
    bool split;         // the result goes bias-free through the split buffer (split-K, the scalar kernels, a padded length)
    bool save_operand;  // conv_h3u_kernel writes its operand out: the weight gradient reads the split operand
    // A layer whose activation feeds split operands and has no bound from batch statistics (eval mode, a frozen layer): its
    // consumers' operand scale comes from the measured maximum of |a z + s|.  The large producers (conv_first_kernel, un-split
    // conv_h3d_kernel) take it in their epilogue - the BatchNorm coefficients only depend on the running statistics, so they are
    // finalised BEFORE the conv; a split layer's conv_reduce_bn_kernel takes it; the small ones get a pass of act_max_kernel over z.
    // (a frozen layer: a / s are there from the launch ahead of the chain; its bound is measured behind the conv)
    int bound;
    bool evop;          // evop_handoff(c, i): this layer's conv writes the next layer's operand
    int reduce_rows;    // > 0: conv_reduce_bn_kernel sums the z-slices (+ bias -> z) and reduces the BN statistics in that many rows
    bool finalize;      // bn_finalize_fwd_kernel runs (eval: a / s of every layer are already there, bn_eval_all_kernel)
};
FwdLayerPlan fwd_layer_plan(const wunet_ctx* c, int i, const FwdMode& m)
{
    const LayerPlan& l = c->ly[i];
    FwdLayerPlan q{};
    const bool fz = m.is_frozen(i);
    q.bstats = m.training && !fz;
    const bool use_u = i > 0 && (m.training ? l.h3u_train : l.h3u);
    q.conv = l.first ? CV_FIRST : use_u ? CV_H3U : l.h3f ? CV_H3 : l.L < 4 ? CV_TINY : CV_FP32;
    q.split = l.f.ksplit > 1 || l.L < 4 || (c->padded && !l.first);
    q.save_operand = q.conv == CV_H3U && m.training && m.save;
    q.skip_to = -1;
    if (i == 0) q.operand = OP_NONE;
    else if (use_u) q.operand = OP_IN_CONV;
    else if (l.kind == LK_DECIM && evop_handoff(c, l.src0, m)) q.operand = OP_BY_PRODUCER;
    else if (l.h3x) {
        static const char* const pn[4] = {"prep_h3_kernel<0>", "prep_h3_kernel<1>", "prep_h3_kernel<2>", "prep_h3_kernel<3>"};
        const int dj = 2 * c->n - i + 1;             // the decoder layer that concatenates this pass's producer
        q.operand = OP_PREP_H3;
        if (l.kind == LK_UPCAT) q.op_mode = skip_handoff(c, i, m) ? 3 : 2;
        else if (l.kind == LK_DECIM && dj < c->NL && c->ly[dj].skip_from == i && skip_handoff(c, dj, m)) { q.op_mode = 1; q.skip_to = dj; }
        const double ob = c->bf ? 2.0 : 4.0, C0 = l.c0, C1 = l.cin - l.c0;
        q.op_name = pn[q.op_mode];
        q.op_bytes = q.op_mode == 0 ? l.cin * (8.0 + ob) : q.op_mode == 1 ? l.cin * (8.0 + 3.0 * ob)
                   : q.op_mode == 2 ? C0 * 2.0 + C1 * 4.0 + l.cin * ob : C0 * (2.0 + ob);
    } else q.operand = l.L < 4 ? OP_SCALAR : l.kind == LK_DECIM ? OP_DECIM : OP_UPCAT;
    q.split_pass = q.conv == CV_H3 && !l.h3x;
    const bool ev_need = (!m.training || fz) && c->h3 && l.feeds_h3;
    const bool ev_epi = ev_need && !m.training && (l.first || (l.h3f && !q.split));
    q.bound = !ev_need ? BOUND_NONE : ev_epi ? BOUND_EPILOGUE : q.split ? BOUND_REDUCE : BOUND_ACT_MAX;
    q.evop = q.conv == CV_H3 && evop_handoff(c, i, m);
    if (q.split) {       // (never with ev_epi: that conv's epilogue folds the bound into the xb slot and nothing is launched)
        // (eval: every block ends in a block-wide maximum and an atomic on one address - half as many blocks: eval forward 1.470 -> 1.445 ms,
        //  one block per channel the same, twice as many 1.53 -> 1.57; training 2048 / 4096 / 8192 positions per block: 5.166 / 5.152 /
        //  5.148 ms, within the noise and another summation order - left alone; profiles/r5_small_ab.txt)
        const long long rs = (long long)c->B * l.L / (q.bstats ? 2048 : 4096);
        q.reduce_rows = rs < 1 ? 1 : rs > 64 ? 64 : (int)rs;
        q.finalize = q.reduce_rows > 1 && q.bstats;     // (short levels finish BN in the reduce launch)
    } else q.finalize = q.bstats;       // (ev_epi: eval mode, no batch statistics)
    return q;
}

// Both ends of a hand-off read one predicate; a plan that sets one where an end cannot run it in this mode and mask is refused
// before anything is launched (the counterpart of upt_handoff_sound).
int fwd_handoffs_sound(const wunet_ctx* c, const FwdMode& m)
{
    for (int p = 0; p + 1 < c->NL; ++p) {
        if (!evop_handoff(c, p, m)) continue;
        const LayerPlan& nx = c->ly[p + 1];
        const FwdLayerPlan q = fwd_layer_plan(c, p, m), qn = fwd_layer_plan(c, p + 1, m);
        // the producer un-split on conv_h3d_kernel with the bound in its epilogue; the consumer a decimation of it that lives in the split layout
        if (!q.evop || q.split || q.bound != BOUND_EPILOGUE || nx.src0 != p || qn.operand != OP_BY_PRODUCER || qn.conv != CV_H3 || !nx.h3x)
            return fail(WUNET_E_ARG, "layer %d: EVOP planned where the conv or its consumer cannot run it", p);
    }
    for (int d = c->n + 1; d < c->NL; ++d) {
        if (!skip_handoff(c, d, m)) continue;
        const LayerPlan& dl = c->ly[d];
        const int e = dl.skip_from;
        // both passes prep_h3_kernel, the encoder-side one a decimation of the activation layer d concatenates, whole channel groups
        if (e < 1 || e > c->n || fwd_layer_plan(c, e, m).skip_to != d || fwd_layer_plan(c, d, m).op_mode != 3 || dl.src1 != c->ly[e].src0 || dl.c0 % 8 != 0)
            return fail(WUNET_E_ARG, "layer %d: skip half planned where its operand pass or the encoder-side pass cannot write it", d);
    }
    return WUNET_OK;
}

// what every stage of one forward call shares
struct FwdCall {
    wunet_ctx* c; float* ws; const float* const* params; float* const* running; long long* const* nbt;
    const float* noisy;           // the network input (the zero-padded copy of the caller's when padded)
    hipStream_t st;
    FwdMode m;
};
// the side stream(s) a forward's packs went to (nullptr: the caller's stream)
struct FwdSides { wunet_ctx::Side* fwd = nullptr; wunet_ctx::Side* bwd = nullptr; };

int fork_side(wunet_ctx::Side* side, hipStream_t st)
{
    if (hipEventRecord(side->ev_fork, st) != hipSuccess || hipStreamWaitEvent(side->stream, side->ev_fork, 0) != hipSuccess)
        return fail(WUNET_E_RUNTIME, "fork onto the side stream failed");
    return WUNET_OK;
}

// the fp32 fragment packs of the layers on the fp32 kernels
int pack_fp32(const FwdCall& k, hipStream_t pst)
{
    wunet_ctx* c = k.c;
    PackTable tab{};
    int nd = 0;
    for (int i = 0; i < c->NL; ++i) {
        const LayerPlan& l = c->ly[i];
        if (l.h3f || l.first) continue;            // those layers do not read the fp32 pack
        PackDesc& d = tab.d[nd++];
        d.w = k.params[4 * i]; d.dst = k.ws + c->wpkf_off + l.f_wpk;
        d.Cout = l.cout; d.Cin = l.cin; d.taps = l.taps; d.M = l.cout; d.CP = l.f.cp; d.mtiles = l.f.mtiles_p; d.transposed = 0;
    }
    if (nd > 0) {
        WUNET_LAUNCH(pack_weights_kernel, dim3(pack_gx(), nd), dim3(WUNET_THREADS), 0, pst, tab);
        WUNET_CHECK_LAUNCH();
    }
    return WUNET_OK;
}

// the split path's scales, split weight pack and (eval) weight row sums
int pack_split(const FwdCall& k, hipStream_t pst)
{
    wunet_ctx* c = k.c; float* ws = k.ws;
    const bool training = k.m.training;
    // power-of-two scales of the split operands (wunet_h3_elem.h): partial max |W| of every layer with a split pack, and
    // the activation bounds the x scales derive from (training: from gamma / beta; eval: cleared here, measured per layer)
    {
        ScaleTable T{};
        bool any = false;
        for (int i = 0; i < c->NL; ++i) {
            const LayerPlan& l = c->ly[i];
            ScaleDesc& d = T.d[i];
            d.w = (l.h3f || l.h3d) ? k.params[4 * i] : nullptr; d.wn = (unsigned)((size_t)l.cout * l.cin * l.taps);
            d.gamma = k.params[4 * i + 2]; d.beta = k.params[4 * i + 3]; d.C = l.cout;
            d.sqrtn = sqrtf((float)((double)c->B * l.Lt));
            d.frozen = k.m.is_frozen(i) ? 1 : 0;
            d.zp0 = l.h3f ? ws + l.xzp : nullptr;
            d.zp1 = (l.h3d && training && k.m.save) ? ws + l.gzp : nullptr;      // (the backward segment only exists then)
            any = any || l.h3f;
        }
        T.wmax = ws + c->wmax_off; T.slots = x_scale_slot(c, ws, 0); T.training = training ? 1 : 0;
        if (any) {
            WUNET_LAUNCH(h3_scales_kernel, dim3(WUNET_WMAX_PARTS, c->NL), dim3(WUNET_THREADS), 0, pst, T);
            WUNET_CHECK_LAUNCH();
        }
    }
    PackH3Table tab{};
    int nd = 0;
    wunet_half* wh = reinterpret_cast<wunet_half*>(ws + c->h3_wf_hi);
    wunet_half* wl = reinterpret_cast<wunet_half*>(ws + c->h3_wf_lo);
    for (int i = 0; i < c->NL; ++i) {
        const LayerPlan& l = c->ly[i];
        if (!l.h3f) continue;
        PackH3Desc& d = tab.d[nd++];
        d.w = k.params[4 * i]; d.hi = wh + l.h3f_wpk; d.lo = wl + l.h3f_wpk;
        d.Cout = l.cout; d.Cin = l.cin; d.taps = l.taps; d.rows = l.cout; d.kch = l.cin; d.mtiles = l.hf.mtp; d.nch = l.hf.nch; d.transposed = 0;
        // (conv_h3u_kernel walks whole chunks: the layers it runs in this mode get a pack without K tail - never longer than the one with)
        d.ntt = (training ? l.h3u_train : l.h3u) ? 0 : l.hf.ntt; d.nfull = ((l.cin + 7) / 8) / 4; d.ns = h3_stage_count(l.cin, l.taps, d.ntt);
        d.wmax = ws + c->wmax_off + (size_t)WUNET_WMAX_PARTS * i; d.wsc = w_scale_slot(c, ws, i);
        d.bf = c->bf;
    }
    if (nd > 0) {
        WUNET_LAUNCH(pack_h3_kernel, dim3(pack_gx(), nd), dim3(WUNET_THREADS), 0, pst, tab);
        WUNET_CHECK_LAUNCH();
    }
    if (!training) {
        RowL1Table rt{};
        int nr = 0;
        for (int i = 0; i < c->NL; ++i) {
            const LayerPlan& l = c->ly[i];
            if (!l.evop) continue;
            RowL1Desc& d = rt.d[nr++];
            d.w = k.params[4 * i]; d.dst = ws + l.wl1; d.rows = l.cout; d.rowlen = l.cin * l.taps;
        }
        if (nr > 0) {
            WUNET_LAUNCH(w_rowl1_kernel, dim3(8, nr), dim3(WUNET_THREADS), 0, pst, rt);
            WUNET_CHECK_LAUNCH();
        }
    }
    return WUNET_OK;
}

// ---- 1. pack all forward weights into MFMA-fragment order (one launch each for the fp32 and the split packs).  A training forward
// whose first layer runs conv_first_kernel (it reads the raw weights) enqueues them - and the operand scales - on the side stream:
// conv_first and its BatchNorm finalize run beside them instead of behind three launches that only read the weights.
// Order on the side stream: scales, split pack (first needed by layer 1), fp32 pack (the
// levels of <= 8 samples), then the backward's packs.
// (packs_valid - eval mode, the caller's workspace still holds this ctx's packs of these weights: nothing to pack)
int forward_packs(const FwdCall& k, bool packs_valid, void* workspace, FwdSides& sides)
{
    wunet_ctx* c = k.c; float* ws = k.ws; const hipStream_t st = k.st;
    const bool training = k.m.training;
    int rc;
    if (training && c->NL > 1 && c->ly[0].first && !g_prof_on && !k.m.is_frozen(0)) {      // (a frozen first layer measures its bound before layer 1)
        if (!side_stream_off()) sides.fwd = side_for_current_device(c);
        if (sides.fwd && (rc = fork_side(sides.fwd, st)) != 0) return rc;
    }
    const hipStream_t pst = sides.fwd ? sides.fwd->stream : st;
    if (!sides.fwd && !packs_valid && (rc = pack_fp32(k, pst)) != 0) return rc;
    if (c->h3 && packs_valid) {
        ScaleTable T{};
        for (int i = 0; i < c->NL; ++i) T.d[i].zp0 = c->ly[i].h3f ? ws + c->ly[i].xzp : nullptr;
        T.slots = x_scale_slot(c, ws, 0);
        WUNET_LAUNCH(h3_slots_clear_kernel, dim3(1), dim3(WUNET_THREADS), 0, st, T, c->NL);
        WUNET_CHECK_LAUNCH();
    } else if (c->h3 && (rc = pack_split(k, pst)) != 0) return rc;
    if (sides.fwd) {
        if (hipEventRecord(sides.fwd->ev_fpack, pst) != hipSuccess) return fail(WUNET_E_RUNTIME, "recording the pack event failed");
        if ((rc = pack_fp32(k, pst)) != 0) return rc;
        if (hipEventRecord(sides.fwd->ev_fpack2, pst) != hipSuccess) return fail(WUNET_E_RUNTIME, "recording the pack event failed");
    }
    // The backward's flipped / transposed weight packs only depend on the weights (and on the maxima h3_scales_kernel has just
    // taken): a training forward that will be followed by a backward enqueues them on the side stream now, beside the first convs,
    // instead of leaving two launches at the head of the backward's critical path.
    if (training && k.m.save && c->NL > 1) {
        wunet_ctx::Side* side = (side_stream_off() || g_prof_on) ? nullptr : side_for_current_device(c);
        if (side) {
            // (behind the forward's packs on the side stream when they are there: no second fork)
            if (side != sides.fwd && (rc = fork_side(side, st)) != 0) return rc;
            if ((rc = launch_backward_packs(c, k.params, ws, side->stream)) != 0) return rc;
            if (hipEventRecord(side->ev_pack, side->stream) != hipSuccess) return fail(WUNET_E_RUNTIME, "recording the pack event failed");
            side->packed_ws = workspace;
            sides.bwd = side;          // the side stream holds this forward's backward packs
        }
    }
    return WUNET_OK;
}

// ---- BatchNorm scale / shift from the running statistics, one launch ahead of the chain: every layer in eval mode; in training mode
// the frozen layers, with the backward's mean / rstd
int bn_tables(const FwdCall& k)
{
    wunet_ctx* c = k.c; float* ws = k.ws;
    const bool training = k.m.training;
    if (training && !k.m.frozen) return WUNET_OK;
    BnEvalTable T{};
    int nd = 0, maxc = 1;
    for (int i = 0; i < c->NL; ++i) {
        if (training && !k.m.is_frozen(i)) continue;
        const LayerPlan& l = c->ly[i];
        BnEvalDesc& d = T.d[nd++];
        d.gamma = k.params[4 * i + 2]; d.beta = k.params[4 * i + 3]; d.running_mean = k.running[2 * i]; d.running_var = k.running[2 * i + 1];
        d.a = ws + l.a; d.s = ws + l.s; d.C = l.cout;
        if (training) { d.mean = ws + l.mean; d.rstd = ws + l.rstd; }
        if (l.cout > maxc) maxc = l.cout;
    }
    if (nd > 0) {
        WUNET_LAUNCH(bn_eval_all_kernel, dim3((unsigned)((maxc + WUNET_THREADS - 1) / WUNET_THREADS), (unsigned)nd), dim3(WUNET_THREADS), 0, k.st, T);
        WUNET_CHECK_LAUNCH();
    }
    return WUNET_OK;
}

// ---- 2a. materialise the conv input (FwdLayerPlan::operand)
// The skip half of each decoder input only depends on an encoder level and could run on a side stream during
// the encoder phase; measured on MI355X that is SLOWER (forward 4.24 vs 3.99 ms: the elementwise kernel steals
// L2/HBM bandwidth and CU slots from the encoder GEMMs), so it stays on the caller's stream.
int operand_pass(const FwdCall& k, int i, const FwdLayerPlan& q)
{
    wunet_ctx* c = k.c; float* ws = k.ws; const hipStream_t st = k.st;
    const LayerPlan& l = c->ly[i];
    if (q.operand == OP_NONE || q.operand == OP_IN_CONV || q.operand == OP_BY_PRODUCER) return WUNET_OK;
    const LayerPlan& p = c->ly[l.src0];
    const bool upcat = l.kind == LK_UPCAT;
    if (q.operand == OP_PREP_H3) {
        PrepH3Args ph{};
        ph.z0 = ws + p.z; ph.a0 = ws + p.a; ph.s0 = ws + p.s;
        ph.xh = reinterpret_cast<wunet_half*>(ws + l.xh); ph.xl = reinterpret_cast<wunet_half*>(ws + l.xl);
        ph.B = c->B; ph.C0 = l.c0; ph.C1 = l.cin - l.c0; ph.C8 = (l.cin + 7) / 8; ph.L = l.L; ph.logL = l.logL; ph.Lt = l.Lt;
        ph.kind = upcat ? 1 : 0;
        ph.up_only = q.op_mode == 3 ? 1 : 0;
        ph.xb0 = act_bound_slot(c, ws, l.src0);
        ph.xb1 = upcat ? act_bound_slot(c, ws, l.src1) : nullptr;
        ph.xsc = x_scale_slot(c, ws, i);
        ph.bf = c->bf;
        if (q.skip_to >= 0) {
            const LayerPlan& dl = c->ly[q.skip_to];
            ph.sh = reinterpret_cast<wunet_half*>(ws + dl.xh); ph.sl = reinterpret_cast<wunet_half*>(ws + dl.xl);
            ph.SC8 = (dl.cin + 7) / 8; ph.sc8off = dl.c0 / 8;
            ph.ssb0 = act_bound_slot(c, ws, dl.src0);
            ph.ssb1 = act_bound_slot(c, ws, dl.src1);
        }
        if (upcat) {
            const LayerPlan& s = c->ly[l.src1];
            ph.z1 = ws + s.z; ph.a1 = ws + s.a; ph.s1 = ws + s.s;
            ph.up_scale = (float)(l.Lt / 2 - 1) / (float)(l.Lt - 1);
        }
        const size_t nt = (size_t)c->B * (ph.up_only ? ph.C0 / 8 : ph.C8) * (l.L / 4);
        const dim3 g1(capped_blocks(nt * 4, WUNET_THREADS, 65536)), t1(WUNET_THREADS);            // one thread per sample and channel group
        prof_begin(st, q.op_name, 0.0, (double)c->B * l.L * q.op_bytes);
        if (q.op_mode == 3) WUNET_LAUNCH((prep_h3_kernel<3>), g1, t1, 0, st, ph);
        else if (q.op_mode == 2) WUNET_LAUNCH((prep_h3_kernel<2>), g1, t1, 0, st, ph);
        else if (q.op_mode == 1) WUNET_LAUNCH((prep_h3_kernel<1>), g1, t1, 0, st, ph);
        else WUNET_LAUNCH((prep_h3_kernel<0>), g1, t1, 0, st, ph);
        prof_end(st);
        WUNET_CHECK_LAUNCH();
        return WUNET_OK;
    }
    PrepArgs pa{};
    pa.z0 = ws + p.z; pa.a0 = ws + p.a; pa.s0 = ws + p.s; pa.x = ws + l.xin;
    pa.B = c->B; pa.C0 = l.c0; pa.C1 = l.cin - l.c0; pa.L = l.L; pa.logL = l.logL; pa.Lt = l.Lt;
    if (upcat) {
        const LayerPlan& s = c->ly[l.src1];
        pa.z1 = ws + s.z; pa.a1 = ws + s.a; pa.s1 = ws + s.s;
        pa.up_scale = l.Lt > 1 ? (float)(l.Lt / 2 - 1) / (float)(l.Lt - 1) : 0.f;
    }
    const size_t ne = (size_t)c->B * l.cin * l.L;
    const dim3 grid(capped_blocks(ne / 4, WUNET_THREADS, 8192));
    if (q.operand == OP_SCALAR)
        WUNET_LAUNCH(prep_scalar_kernel, dim3((unsigned)((ne + WUNET_THREADS - 1) / WUNET_THREADS)), dim3(WUNET_THREADS), 0, st, pa, upcat ? 1 : 0);
    else if (q.operand == OP_DECIM) WUNET_LAUNCH(prep_decim_kernel, grid, dim3(WUNET_THREADS), 0, st, pa);
    else WUNET_LAUNCH(prep_upcat_kernel, grid, dim3(WUNET_THREADS), 0, st, pa, 0, l.cin);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

// ---- 2b. conv (+ bias, + per-wave BN statistics partials) on the matrix cores
int conv(const FwdCall& k, int i, const FwdLayerPlan& q)
{
    wunet_ctx* c = k.c; float* ws = k.ws; const hipStream_t st = k.st;
    const LayerPlan& l = c->ly[i];
    const float* const xin = i == 0 ? k.noisy : ws + l.xin;
    // (a result that goes through conv_reduce_bn_kernel gets its bias THERE: an un-split launch into the split buffer - a padded
    //  length - added it twice; invisible behind training-mode BatchNorm, 0.03 off in eval mode)
    const float* const bias = q.split ? nullptr : k.params[4 * i + 1];
    float* const out = q.split ? ws + c->spart_off : ws + l.z;
    float* const stats = (q.bstats && !q.split) ? ws + c->stats_off : nullptr;
    // the bound in the epilogue: the blocks fold their maxima into the layer's xb slot (cleared by h3_scales_kernel)
    const bool epi = q.bound == BOUND_EPILOGUE;
    const float* const ev_a = epi ? ws + l.a : nullptr;
    const float* const ev_s = epi ? ws + l.s : nullptr;
    float* const xrows = epi ? act_bound_slot(c, ws, i) : nullptr;
    const wunet_half* const wh = reinterpret_cast<const wunet_half*>(ws + c->h3_wf_hi) + l.h3f_wpk;
    int rc = 0;
    if (q.conv == CV_FIRST) {
        prof_begin(st, "conv_first_kernel<15>", 2.0 * c->B * l.L * l.cout * 15.0, 4.0 * c->B * l.L * (1.0 + l.cout));
        WUNET_LAUNCH(conv_first_kernel<15>, dim3((unsigned)l.f.grid_x), dim3(WUNET_THREADS), 0, st, xin, k.params[4 * i], k.params[4 * i + 1],
                     ws + l.z, stats, c->B, l.cout, l.L, l.logL, ev_a, ev_s, xrows, l.Lt);
        prof_end(st);
    } else if (q.conv == CV_H3U) {
        const LayerPlan& p = c->ly[l.src0];
        const LayerPlan& s = c->ly[l.src1];
        ConvH3uArgs u{};
        u.z0 = ws + p.z; u.a0 = ws + p.a; u.s0 = ws + p.s; u.z1 = ws + s.z; u.a1 = ws + s.a; u.s1 = ws + s.s;
        u.xb0 = act_bound_slot(c, ws, l.src0); u.xb1 = act_bound_slot(c, ws, l.src1);
        u.xsc = x_scale_slot(c, ws, i);
        u.up_scale = (float)(l.Lt / 2 - 1) / (float)(l.Lt - 1); u.Lt = l.Lt; u.C0 = l.c0; u.C1 = l.cin - l.c0;
        u.wh = wh;
        u.wdelta = (unsigned)((const char*)(ws + c->h3_wf_lo) - (const char*)(ws + c->h3_wf_hi));
        u.bias = k.params[4 * i + 1]; u.sc2 = w_scale_slot(c, ws, i);
        u.out = ws + l.z; u.stats = stats;
        u.ev_a = ev_a; u.ev_s = ev_s; u.xrows = xrows;
        if (q.save_operand) {
            u.oxh = reinterpret_cast<wunet_half*>(ws + l.xh); u.oxl = reinterpret_cast<wunet_half*>(ws + l.xl);
        }
        u.B = c->B; u.Cout = l.cout; u.L = l.L;
        rc = launch_conv_h3u(u, l.hf.mrep, l.hf.mtp, l.cin, st);
    } else if (q.conv == CV_H3) {
        // fp16-split GEMM: split the materialised input, then 3 MFMA passes on the 2.5 PF pipe
        wunet_half* xh = reinterpret_cast<wunet_half*>(ws + l.xh);
        wunet_half* xl = reinterpret_cast<wunet_half*>(ws + l.xl);
        if (q.split_pass) {
            launch_split(xin, xh, xl, nullptr, act_bound_slot(c, ws, l.src0), l.kind == LK_UPCAT ? act_bound_slot(c, ws, l.src1) : nullptr,
                         x_scale_slot(c, ws, i), c->B, l.cin, l.L, st, c->bf);
            WUNET_CHECK_LAUNCH();
        }
        ConvH3OpOut opo{};
        if (q.evop) {
            const LayerPlan& nx = c->ly[i + 1];
            opo.h = reinterpret_cast<wunet_half*>(ws + nx.xh); opo.l = reinterpret_cast<wunet_half*>(ws + nx.xl);
            opo.wl1 = ws + l.wl1; opo.xmax = act_bound_slot(c, ws, l.src0);
            opo.xsc = x_scale_slot(c, ws, i + 1); opo.C8 = (nx.cin + 7) / 8;
        }
        ConvH3Launch h{};
        h.taps = l.taps; h.mrep = l.hf.mrep; h.mtiles_p = l.hf.mtp; h.sps = l.hf.sps; h.nch = l.hf.nch; h.ntt = l.hf.ntt;
        h.B = c->B; h.rows = l.cout; h.kch = l.cin; h.L = l.L; h.bf = c->bf;
        h.xh = xh; h.xl = xl; h.wh = wh; h.wl = reinterpret_cast<const wunet_half*>(ws + c->h3_wf_lo) + l.h3f_wpk; h.zpad = ws + l.xzp;
        h.bias = bias; h.sc = x_scale_slot(c, ws, i); h.sc2 = w_scale_slot(c, ws, i); h.out = out; h.stats = stats;
        h.ev_a = ev_a; h.ev_s = ev_s; h.xrows = xrows;
        h.op = q.evop ? &opo : nullptr;
        rc = launch_conv_h3(h, st);
    } else if (q.conv == CV_TINY) {
        const size_t no = (size_t)c->B * l.cout * l.L;
        WUNET_LAUNCH(tiny_conv_kernel, dim3((unsigned)((no + WUNET_THREADS - 1) / WUNET_THREADS)), dim3(WUNET_THREADS), 0, st,
                     xin, k.params[4 * i], ws + c->spart_off, c->B, l.cin, l.cout, l.L, l.logL, l.taps, 0);
    } else {
        const ConvArgs a = make_conv_args(xin, l.cin, ws + c->wpkf_off + l.f_wpk, bias, out, stats, c->B, l.cout, l.L, l.taps, l.f, (size_t)c->B * l.cout * l.L);
        rc = launch_conv(l.taps, a, l.f, st);
    }
    if (rc) return rc;
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

// ---- 2c. BatchNorm statistics -> scale/shift for the consumers (+ running stats), and the activation bound where no conv epilogue took it
int bn_finish(const FwdCall& k, int i, const FwdLayerPlan& q)
{
    wunet_ctx* c = k.c; float* ws = k.ws; const hipStream_t st = k.st;
    const LayerPlan& l = c->ly[i];
    BnFwdArgs b{};
    b.stats = ws + c->stats_off; b.rows = l.f_rows; b.bias = k.params[4 * i + 1];
    b.gamma = k.params[4 * i + 2]; b.beta = k.params[4 * i + 3];
    b.running_mean = k.running[2 * i]; b.running_var = k.running[2 * i + 1]; b.nbt = k.nbt[i];
    b.a = ws + l.a; b.s = ws + l.s; b.mean = ws + l.mean; b.rstd = ws + l.rstd;
    b.C = l.cout; b.count = (double)c->B * l.Lt; b.training = q.bstats ? 1 : 0;
    if (q.reduce_rows) {
        b.rows = q.reduce_rows;
        WUNET_LAUNCH(conv_reduce_bn_kernel, dim3(l.cout, q.reduce_rows), dim3(WUNET_THREADS), 0, st, b, (const float*)(ws + c->spart_off),
                     q.conv == CV_TINY ? 1 : l.f.ksplit, (size_t)c->B * l.cout * l.L, ws + l.z, c->B, l.L, l.logL, ws + c->stats_off, l.Lt,
                     q.bound == BOUND_REDUCE ? act_bound_slot(c, ws, i) : (float*)nullptr);
        WUNET_CHECK_LAUNCH();
    }
    if (q.finalize) {
        WUNET_LAUNCH(bn_finalize_fwd_kernel, dim3(l.cout), dim3(WUNET_THREADS), 0, st, b);
        WUNET_CHECK_LAUNCH();
    }
    if (q.bound == BOUND_ACT_MAX) {
        const size_t n4 = (size_t)c->B * l.cout * l.L / 4;
        const unsigned blocks = capped_blocks(n4, WUNET_THREADS * 4, 2048);
        WUNET_LAUNCH(act_max_kernel, dim3(blocks < 1 ? 1 : blocks), dim3(WUNET_THREADS), 0, st, (const float*)(ws + l.z), (const float*)(ws + l.a),
                     (const float*)(ws + l.s), l.cout, l.logL, n4, act_bound_slot(c, ws, i));
        WUNET_CHECK_LAUNCH();
    }
    return WUNET_OK;
}

// ---- 3. head
int head_forward(const FwdCall& k, float* enhanced)
{
    wunet_ctx* c = k.c; float* ws = k.ws; const hipStream_t st = k.st;
    const LayerPlan& l = c->ly[c->NL - 1];
    HeadFwdArgs h{};
    h.z = ws + l.z; h.a = ws + l.a; h.s = ws + l.s; h.in = k.noisy;
    h.wh = k.params[4 * c->NL]; h.bh = k.params[4 * c->NL + 1]; h.out = enhanced;
    h.B = c->B; h.C = c->ci; h.T = c->T; h.logT = ilog2(c->T);
    prof_begin(st, "head_fwd_kernel", 2.0 * c->B * c->T * (c->ci + 1.0), 4.0 * c->B * c->T * (c->ci + 2.0));
    WUNET_LAUNCH(head_fwd_kernel, dim3(capped_blocks((size_t)c->B * c->T / 4, WUNET_THREADS, 4096)), dim3(WUNET_THREADS), 0, st, h);      // four samples per thread
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}
}  // namespace

extern "C" {

int wunet_forward(wunet_ctx* c, const float* noisy, const float* const* params, float* const* running,
                  long long* const* nbt, int training, int save_for_backward, void* workspace, float* enhanced, void* stream)
{
    if (!c || !noisy || !params || !running || !nbt || !workspace || !enhanced) return fail(WUNET_E_ARG, "null argument");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const bool packs_valid = !training && (save_for_backward & WUNET_FWD_PACKS_VALID) != 0;
    const FwdMode m{training != 0, (save_for_backward & WUNET_FWD_SAVE) != 0, (training && c->any_frozen) ? c->frozen.data() : nullptr};
    int rc = fwd_handoffs_sound(c, m);
    if (rc) return rc;
    float* const enhanced_user = enhanced;
    if (c->padded) {
        // the caller's [B][1][Tt] rows into zero-padded rows of T floats; the result is cropped back at the end
        if (hipMemsetAsync(ws + c->pad_in, 0, (size_t)c->B * c->T * sizeof(float), st) != hipSuccess ||
            hipMemcpy2DAsync(ws + c->pad_in, (size_t)c->T * sizeof(float), noisy, (size_t)c->Tt * sizeof(float), (size_t)c->Tt * sizeof(float),
                             (size_t)c->B, hipMemcpyDeviceToDevice, st) != hipSuccess)
            return fail(WUNET_E_RUNTIME, "padding the input failed");
        noisy = ws + c->pad_in;
        enhanced = ws + c->pad_out;
    }
    const FwdCall k{c, ws, params, running, nbt, noisy, st, m};
    FwdSides sides;
    if ((rc = forward_packs(k, packs_valid, workspace, sides)) != 0) return rc;
    if ((rc = bn_tables(k)) != 0) return rc;
    // (packs on the side stream: the operand scales and the split pack are first read by layer 1, the fp32 pack by the first
    // layer on the fp32 kernels)
    bool fpack_joined = sides.fwd == nullptr, fpack2_joined = sides.fwd == nullptr;
    for (int i = 0; i < c->NL; ++i) {
        if (!fpack_joined && i >= 1) {
            if (hipStreamWaitEvent(st, sides.fwd->ev_fpack, 0) != hipSuccess) return fail(WUNET_E_RUNTIME, "waiting for the weight packs failed");
            fpack_joined = true;
        }
        if (!fpack2_joined && i >= 1 && !c->ly[i].h3f) {
            if (hipStreamWaitEvent(st, sides.fwd->ev_fpack2, 0) != hipSuccess) return fail(WUNET_E_RUNTIME, "waiting for the weight packs failed");
            fpack2_joined = true;
        }
        const FwdLayerPlan q = fwd_layer_plan(c, i, m);
        if ((rc = operand_pass(k, i, q)) != 0 || (rc = conv(k, i, q)) != 0 || (rc = bn_finish(k, i, q)) != 0) return rc;
    }
    if (!fpack_joined && hipStreamWaitEvent(st, sides.fwd->ev_fpack, 0) != hipSuccess) return fail(WUNET_E_RUNTIME, "waiting for the weight packs failed");
    if (!fpack2_joined && hipStreamWaitEvent(st, sides.fwd->ev_fpack2, 0) != hipSuccess) return fail(WUNET_E_RUNTIME, "waiting for the weight packs failed");
    if ((rc = head_forward(k, enhanced)) != 0) return rc;
    // The backward packs were written into the caller's workspace from the side stream: the caller's stream joins them here (they
    // finished long ago - the wait costs nothing), so a forward whose backward never runs (loss discarded, an exception) leaves no
    // write in flight on a stream the owner of the workspace does not know about when it frees or re-uses the block.
    if (sides.bwd && hipStreamWaitEvent(st, sides.bwd->ev_pack, 0) != hipSuccess) return fail(WUNET_E_RUNTIME, "waiting for the weight packs failed");
    if (c->padded && hipMemcpy2DAsync(enhanced_user, (size_t)c->Tt * sizeof(float), ws + c->pad_out, (size_t)c->T * sizeof(float),
                                      (size_t)c->Tt * sizeof(float), (size_t)c->B, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return fail(WUNET_E_RUNTIME, "cropping the output failed");
    return WUNET_OK;
}

}  // extern "C"
