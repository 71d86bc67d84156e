// plan_dump: what the planner (csrc/wunet_plan.cpp) decides, as text, without a device.  A stand-alone host program built against
// the emulator headers (make -C tests/emu plan_dump).  For every context of a sweep - shape x wunet_set_h3 0..4 x planner switch
// set - one "ctx" line with every offset and size of wunet_ctx and one "layer" line per layer with every planned field as
// name=value.  Two builds of the planner agree if and only if their dumps are the same bytes (a refactor's check).
//
//     plan_dump [--check] [--n-layers LO HI] [--shape N CI B T]...
//
// Without --shape: n_layers 1..16 (or LO..HI) x channels_interval {4, 8, 12, 16, 20, 24, 32} x batch {1, 2, 3, 4, 6, 16, 32, 64} x
// length m * 2^n_layers * 2^j (m in {1, 3}, j in {0, 2, 4}, at most 65536); what wunet_create refuses is skipped.  Switches set in
// the caller's environment stay set under every switch set of the table below (how a per-process switch is swept).
// --check prints nothing and asserts per context: the forward segment inside the workspace; every offset, in allotment order,
// non-decreasing, 64-aligned and below its segment's end; a replanned context equal to a fresh one; skip_from, evop, upt, h3u,
// h3u_train and h3w only on layers that meet what their readers rely on (fwd_handoffs_sound / upt_handoff_sound, restated from
// plan fields); for every kernel a layer may run, the bytes of dynamic LDS its launch requests (csrc/wunet_lds.h) times the resident
// blocks per CU its planner counted on within the CU's LDS.  Exit status 1 on a violation.
#include "wunet_host.h"

using namespace wunet_host;

// ---- accessors: the only lines that know how the structs name the tilings
static const H3ConvPlan& HF(const LayerPlan& l) { return l.hf; }
static const H3ConvPlan& HD(const LayerPlan& l) { return l.hd; }
static H3WgradPlan HW(const wunet_ctx*, const LayerPlan& l) { return l.hw; }
// ----

static const char* const kSwitchSets[] = {
    "", "WUNET_H3_NOSPLIT=1", "WUNET_H3_SPS=1", "WUNET_H3_SPS=2", "WUNET_H3_OLDSPLIT=1", "WUNET_H3_KTAIL=0", "WUNET_H3_ORDER=432",
    "WUNET_H3D_ORDER=432", "WUNET_H3W_ORDER=432", "WUNET_H3_ORDER=432 WUNET_H3D_ORDER=432 WUNET_H3W_ORDER=432", "WUNET_H3U=0",
    "WUNET_H3U=256,256", "WUNET_H3U=512", "WUNET_NO_SKIP_FUSE=1", "WUNET_NO_EVOP=1", "WUNET_NO_E0=1", "WUNET_UPT=0",
    "WUNET_NO_ENC_GZ=1", "WUNET_PA_SWAP=0",
};

// sets (on) or clears the variables of one switch set ("NAME=VALUE NAME=VALUE")
static void apply_switches(const char* set, bool on)
{
    std::string s(set);
    for (size_t at = 0; at < s.size();) {
        size_t end = s.find(' ', at);
        if (end == std::string::npos) end = s.size();
        const std::string kv = s.substr(at, end - at), name = kv.substr(0, kv.find('='));
        if (on) setenv(name.c_str(), kv.substr(name.size() + 1).c_str(), 1);
        else unsetenv(name.c_str());
        at = end + 1;
    }
}

struct Off { std::string name; size_t at; };
// every workspace offset in the order layout_workspace allots it; `split`: how many of them lie in the forward segment
static std::vector<Off> offsets_in_order(const wunet_ctx* c, size_t* split)
{
    std::vector<Off> v;
    const auto L = [&](int i, const char* f, size_t at) { v.push_back({std::string(f) + "[" + std::to_string(i) + "]", at}); };
    const auto C = [&](const char* f, size_t at) { v.push_back({f, at}); };
    for (int i = 0; i < c->NL; ++i) {
        const LayerPlan& l = c->ly[i];
        L(i, "z", l.z); L(i, "a", l.a); L(i, "s", l.s); L(i, "mean", l.mean); L(i, "rstd", l.rstd); L(i, "wl1", l.wl1); L(i, "xin", l.xin);
    }
    C("stats_off", c->stats_off); C("wpkf_off", c->wpkf_off); C("spart_off", c->spart_off);
    for (int i = 0; i < c->NL; ++i) {
        const LayerPlan& l = c->ly[i];
        if (l.h3f) { L(i, "xh", l.xh); L(i, "xl", l.xl); L(i, "xzp", l.xzp); }
    }
    C("h3_wf_hi", c->h3_wf_hi); C("h3_wf_lo", c->h3_wf_lo); C("fslot_off", c->fslot_off); C("wmax_off", c->wmax_off);
    if (c->padded) { C("pad_in", c->pad_in); C("pad_out", c->pad_out); }
    *split = v.size();
    for (int i = 0; i < c->NL; ++i) {
        const LayerPlan& l = c->ly[i];
        L(i, "g", l.g); L(i, "dx", l.dx); L(i, "k1", l.k1); L(i, "k2", l.k2); L(i, "k3", l.k3);
    }
    C("bpart_off", c->bpart_off); C("bmax_off", c->bmax_off); C("bound_off", c->bound_off); C("wgpart_off", c->wgpart_off);
    C("wpkb_off", c->wpkb_off); C("gh_off", c->gh_off); C("hpart_off", c->hpart_off); C("hpart2_off", c->hpart2_off); C("e0part_off", c->e0part_off);
    for (int i = 0; i < c->NL; ++i) {
        const LayerPlan& l = c->ly[i];
        if (l.h3d) { L(i, "gzh", l.gzh); L(i, "gzl", l.gzl); L(i, "gzp", l.gzp); }
    }
    for (int i = 0; i < c->NL; ++i) {
        const LayerPlan& l = c->ly[i];
        if (l.upt) { L(i, "dxh", l.dxh); L(i, "usp", l.usp); }
    }
    C("h3_wb_hi", c->h3_wb_hi); C("h3_wb_lo", c->h3_wb_lo); C("h3_slot", c->h3_slot);
    if (c->padded) C("pad_gout", c->pad_gout);
    return v;
}

static std::string conv_cfg(const char* p, const ConvCfg& k)
{
    char b[256];
    snprintf(b, sizeof b, " %s.mrep=%d %s.nrep=%d %s.mtiles_p=%d %s.mblocks=%d %s.cp=%d %s.grid_x=%d %s.ksplit=%d %s.kcps=%d", p, k.mrep, p, k.nrep,
             p, k.mtiles_p, p, k.mblocks, p, k.cp, p, k.grid_x, p, k.ksplit, p, k.kcps);
    return b;
}
static std::string h3_cfg(const char* p, int on, const H3ConvPlan& k)
{
    char b[160];
    snprintf(b, sizeof b, " %s.mrep=%d %s.mtp=%d %s.nch=%d %s.sps=%d %s.ntt=%d", p, on ? k.mrep : 0, p, on ? k.mtp : 0, p, on ? k.nch : 0,
             p, on ? k.sps : 0, p, on ? k.ntt : 0);
    return b;
}

// the whole plan of a context as text: the "ctx" line, then one "layer" line per layer
static std::string dump(const wunet_ctx* c, int length, int h3, const char* set)
{
    char b[1024];
    std::string out;
    snprintf(b, sizeof b, "ctx n_layers=%d channels_interval=%d batch=%d length=%d set_h3=%d switches=[%s] T=%d padded=%d h3=%d bf=%d e0=%d head_blocks=%d"
             " fwd_floats=%zu total_floats=%zu h3_wf_halfs=%zu h3_wb_halfs=%zu", c->n, c->ci, c->B, length, h3, set, c->T, (int)c->padded, c->h3, c->bf,
             c->e0, c->head_blocks, c->fwd_floats, c->total_floats, c->h3_wf_halfs, c->h3_wb_halfs);
    out += b;
    // (the backward's two A/B switches where one is off: a dump from before they were planner switches has neither field)
    if (!c->enc_gz || !c->pa_swap) out += " enc_gz=" + std::to_string(c->enc_gz) + " pa_swap=" + std::to_string(c->pa_swap);
    size_t split = 0;
    for (const Off& o : offsets_in_order(c, &split))
        if (o.name.find('[') == std::string::npos) out += " " + o.name + "=" + std::to_string(o.at);
    out += "\n";
    for (int i = 0; i < c->NL; ++i) {
        const LayerPlan& l = c->ly[i];
        const H3WgradPlan w = l.h3w ? HW(c, l) : H3WgradPlan{};
        snprintf(b, sizeof b, "layer %d cin=%d cout=%d taps=%d L=%d Lt=%d kind=%d src0=%d src1=%d c0=%d first=%d h3f=%d h3d=%d h3w=%d h3x=%d h3u=%d h3u_train=%d"
                 " skip_from=%d evop=%d feeds_h3=%d upt=%d f_rows=%d a_split=%d", i, l.cin, l.cout, l.taps, l.L, l.Lt, l.kind, l.src0, l.src1, l.c0, l.first,
                 l.h3f, l.h3d, l.h3w, l.h3x, l.h3u, l.h3u_train, l.skip_from, l.evop, l.feeds_h3, l.upt, l.f_rows, l.a_split);
        out += b;
        out += conv_cfg("f", l.f) + conv_cfg("d", l.d);
        snprintf(b, sizeof b, " w.mrep=%d w.nw=%d w.xit=%d w.wsplit=%d w.mblocks=%d w.nblocks=%d w.ksplit=%d w.cps=%d w.rows=%d", l.w.mrep, l.w.nw, l.w.xit,
                 l.w.wsplit, l.w.mblocks, l.w.nblocks, l.w.ksplit, l.w.cps, l.w.rows);
        out += b;
        out += h3_cfg("hf", l.h3f, HF(l)) + h3_cfg("hd", l.h3d, HD(l));
        snprintf(b, sizeof b, " hw.mrep=%d hw.mblocks=%d hw.nblocks=%d hw.ksplit=%d hw.cps=%d hw.tp=%d hw.xcd=%d hw.dma=%d hw.db=%d", w.mrep, w.mblocks, w.nblocks,
                 w.ksplit, w.cps, w.tp, w.xcd, w.dma, w.db);
        out += b;
        snprintf(b, sizeof b, " f_wpk=%zu d_wpk=%zu h3f_wpk=%zu h3d_wpk=%zu z=%zu a=%zu s=%zu mean=%zu rstd=%zu wl1=%zu xin=%zu g=%zu dx=%zu k1=%zu k2=%zu k3=%zu"
                 " xh=%zu xl=%zu xzp=%zu gzh=%zu gzl=%zu gzp=%zu dxh=%zu usp=%zu\n", l.f_wpk, l.d_wpk, l.h3f ? l.h3f_wpk : 0, l.h3d ? l.h3d_wpk : 0, l.z, l.a, l.s,
                 l.mean, l.rstd, l.wl1, l.xin, l.g, l.dx, l.k1, l.k2, l.k3, l.h3f ? l.xh : 0, l.h3f ? l.xl : 0, l.h3f ? l.xzp : 0, l.h3d ? l.gzh : 0,
                 l.h3d ? l.gzl : 0, l.h3d ? l.gzp : 0, l.upt ? l.dxh : 0, l.upt ? l.usp : 0);
        out += b;
    }
    return out;
}

static long g_bad = 0, g_overcounted = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++g_bad; fprintf(stderr, "plan_dump: " __VA_ARGS__); fprintf(stderr, "  [%s]\n", #cond); } } while (0)

// the LDS budget of layer i: per kernel it may run, bytes of one block x blocks per CU the planner assumed <= WUNET_LDS_PER_CU
static void check_lds(const wunet_ctx* c, int i, const char* what)
{
    const LayerPlan& l = c->ly[i];
    const auto fits = [&](const char* kernel, size_t bytes, int blocks) {
        EXPECT(bytes * blocks <= WUNET_LDS_PER_CU, "%s: layer %d %s: %d block(s) of %zu bytes of LDS per CU\n", what, i, kernel, blocks, bytes);
    };
    const bool bf = c->bf != 0;
    if (l.L >= 4) {         // the fp32 GEMMs (a level of 1-2 samples runs the scalar kernels)
        if (!l.h3f && !l.first) fits("conv_mfma_kernel, forward", wunet_lds::conv_mfma(l.taps, l.f.mrep).bytes(wunet_lds::conv_mfma_rowp(l.L, l.f.nrep)), 1);
        if (!l.h3d && i > 0) fits("conv_mfma_kernel, data gradient", wunet_lds::conv_mfma(l.taps, l.d.mrep).bytes(wunet_lds::conv_mfma_rowp(l.L, l.d.nrep)), 1);
        if (!l.h3w) fits("wgrad_mfma_kernel", wunet_lds::wgrad_mfma(l.taps, l.w.mrep, l.w.nw, l.w.wsplit != 0).bytes(wunet_lds::wgrad_mfma_rowp(l.taps, l.L)),
                         wgrad_blocks_per_cu(l.w, l.L, l.taps));
    }
    const int nseg = l.L >= 256 ? 1 : 256 / l.L;
    if (l.h3f) {            // training, and eval with the table of constants where launch_conv_h3 keeps it (EVOP: the same layout)
        const wunet_lds::ConvH3d y = wunet_lds::conv_h3d(HF(l).mrep, nseg, bf, false);
        const int er = HF(l).mtp * 16;
        fits("conv_h3d_kernel, forward", y.bytes(er, 0), y.blocks_per_cu());
        fits("conv_h3d_kernel, eval forward", y.bytes(er, y.eval_table_fits(er) ? 1 : 0), y.blocks_per_cu());
        if (l.h3u || l.h3u_train) fits("conv_h3u_kernel", wunet_lds::conv_h3u(HF(l).mrep).bytes((l.cin + 7) / 8, er), 1);
    }
    if (l.h3d) {
        const wunet_lds::ConvH3d y = wunet_lds::conv_h3d(HD(l).mrep, nseg, bf, l.upt != 0);
        fits("conv_h3d_kernel, data gradient", y.bytes(HD(l).mtp * 16, 0), wunet_lds::conv_h3d(HD(l).mrep, nseg, bf, false).blocks_per_cu());
    }
    if (l.h3w) {
        const H3WgradPlan w = HW(c, l);
        const int blocks = h3w_blocks_per_cu(l.taps, w.mrep, l.L);
        if (w.dma) fits(w.db ? "wgrad_h3d_kernel, double buffered" : "wgrad_h3d_kernel", wunet_lds::wgrad_h3d(l.taps, w.mrep, w.db != 0, bf, w.tp).bytes(), blocks);
        else {
            // KNOWN over-count, reported and not a violation while plans must stay as they are: plan_h3_wgrad's slots rule counts two
            // resident blocks of wgrad_h3_kernel with 2 m-tiles (its launch bounds) at every length, but at 5 taps and 16 samples the
            // halo rows of the chunk's 8 items make the block 83584 bytes, so one fits a CU and the split-K sized for 512 slots takes two
            // rounds.  Each block is held to the CU's LDS; every other plan is held to the blocks its planner counted on
            const size_t bytes = wunet_lds::wgrad_h3(l.taps, w.mrep, l.L >= w.tp ? 1 : w.tp / l.L, w.tp, bf).bytes();
            const bool known = l.taps == 5 && l.L == 16 && w.mrep == 2 && !bf && blocks == 2 && bytes * 2 > WUNET_LDS_PER_CU;
            if (known) ++g_overcounted;
            fits("wgrad_h3_kernel", bytes, known ? 1 : blocks);
        }
    }
}

static void check(const wunet_ctx* c, const char* what)
{
    EXPECT(c->fwd_floats <= c->total_floats, "%s: forward segment past the workspace\n", what);
    size_t split = 0, prev = 0;
    const std::vector<Off> v = offsets_in_order(c, &split);
    for (size_t k = 0; k < v.size(); ++k) {
        const size_t end = k < split ? c->fwd_floats : c->total_floats;
        if (k == split) EXPECT(v[k].at >= c->fwd_floats, "%s: %s inside the forward segment\n", what, v[k].name.c_str());
        EXPECT(v[k].at >= prev && v[k].at % 64 == 0 && v[k].at < end, "%s: offset %s=%zu (before it %zu, segment end %zu)\n", what, v[k].name.c_str(), v[k].at, prev, end);
        prev = v[k].at;
    }
    const int n = c->n, NL = c->NL;
    for (int i = 0; i < NL; ++i) {
        const LayerPlan& l = c->ly[i];
        const bool fsplit = l.f.ksplit > 1 || l.L < 4 || (c->padded && !l.first);      // fwd_layer_plan's `split`
        if (l.skip_from) {      // both operand passes prep_h3_kernel, the encoder-side one a decimation of the activation this layer concatenates
            const int e = l.skip_from;
            EXPECT(i > n && e >= 1 && e <= n && e == 2 * n - i + 1, "%s: layer %d skip_from=%d out of place\n", what, i, e);
            if (e >= 1 && e <= n)
                EXPECT(l.kind == LK_UPCAT && l.h3x && c->ly[e].kind == LK_DECIM && c->ly[e].h3x && l.src1 == c->ly[e].src0 && l.c0 % 8 == 0,
                       "%s: layer %d skip_from=%d unsound\n", what, i, e);
        }
        if (l.evop) {           // un-split on conv_h3d_kernel with the bound in its epilogue; the consumer a decimation of it in the split layout
            EXPECT(i >= 1 && i < n && l.h3f && !l.first && !fsplit && l.feeds_h3 && !c->bf, "%s: layer %d evop unsound\n", what, i);
            if (i + 1 < NL) {
                const LayerPlan& q = c->ly[i + 1];
                EXPECT(q.src0 == i && q.kind == LK_DECIM && q.h3f && q.h3x && !q.h3u && !q.h3u_train, "%s: layer %d evop, consumer unsound\n", what, i);
            }
        }
        if (l.upt)              // the data gradient un-split on the split kernels, the producer's g_z on them too (neither scalar nor fused into pass A)
            EXPECT(i > n && l.src0 == i - 1 && l.kind == LK_UPCAT && l.h3d && l.d.ksplit == 1 && c->ly[i - 1].h3d && c->ly[i - 1].L >= 4 && !c->bf && !c->padded,
                   "%s: layer %d upt unsound\n", what, i);
        if (l.h3u || l.h3u_train)
            EXPECT(l.h3f && l.h3x && l.kind == LK_UPCAT && l.taps == 5 && l.L >= 256 && l.c0 % 8 == 0 && l.cin % 8 == 0 && HF(l).mrep <= 4 && !fsplit && !c->bf,
                   "%s: layer %d conv_h3u_kernel unsound\n", what, i);
        if (l.h3w) {
            const H3WgradPlan w = HW(c, l);
            const long long chunks = ((long long)c->B * l.L + w.tp - 1) / w.tp;
            EXPECT(l.h3d && l.h3x && i > 0 && l.cin >= 16 && l.L >= 16 && w.mrep >= 2 && w.ksplit >= 1 && (long long)w.ksplit * w.cps >= chunks &&
                   (long long)(w.ksplit - 1) * w.cps < chunks && (!w.dma || l.L >= w.tp), "%s: layer %d split weight gradient unsound\n", what, i);
        }
        if (l.h3d) EXPECT(l.h3f && i > 0, "%s: layer %d data gradient on the split kernels without the forward\n", what, i);
        check_lds(c, i, what);
    }
}

int main(int argc, char** argv)
{
    bool checking = false;
    int lo = 1, hi = 16;
    std::vector<std::vector<int>> shapes;
    for (int a = 1; a < argc; ++a) {
        const std::string o = argv[a];
        if (o == "--check") checking = true;
        else if (o == "--n-layers" && a + 2 < argc) { lo = atoi(argv[a + 1]); hi = atoi(argv[a + 2]); a += 2; }
        else if (o == "--shape" && a + 4 < argc) { shapes.push_back({atoi(argv[a + 1]), atoi(argv[a + 2]), atoi(argv[a + 3]), atoi(argv[a + 4])}); a += 4; }
        else { fprintf(stderr, "usage: plan_dump [--check] [--n-layers LO HI] [--shape N CI B T]...\n"); return 2; }
    }
    if (shapes.empty()) {
        const int cis[] = {4, 8, 12, 16, 20, 24, 32}, bs[] = {1, 2, 3, 4, 6, 16, 32, 64};
        for (int n = lo; n <= hi; ++n)
            for (int ci : cis)
                for (int B : bs)
                    for (int m : {1, 3})
                        for (int j : {0, 2, 4})
                            if (((long long)m << (n + j)) <= 65536) shapes.push_back({n, ci, B, m << (n + j)});
    }
    long contexts = 0, lines = 0;
    for (const char* set : kSwitchSets) {
        apply_switches(set, true);
        for (const std::vector<int>& s : shapes) {
            wunet_ctx* replanned = nullptr;
            if (wunet_create(s[0], s[1], s[2], s[3], &replanned) != WUNET_OK) continue;      // refused: not part of the sweep
            for (int h3 = 4; h3 >= 0; --h3) {
                wunet_ctx* c = nullptr;
                wunet_create(s[0], s[1], s[2], s[3], &c);
                wunet_set_h3(c, h3);
                const std::string text = dump(c, s[3], h3, set);
                ++contexts; lines += 1 + c->NL;
                if (checking) {
                    char what[160];
                    snprintf(what, sizeof what, "(%d, %d, %d, %d) set_h3=%d [%s]", s[0], s[1], s[2], s[3], h3, set);
                    check(c, what);
                    wunet_set_h3(replanned, h3);
                    EXPECT(dump(replanned, s[3], h3, set) == text, "%s: a replanned context differs from a fresh one\n", what);
                } else fputs(text.c_str(), stdout);
                wunet_destroy(c);
            }
            wunet_destroy(replanned);
        }
        apply_switches(set, false);
    }
    fprintf(stderr, "plan_dump: %ld contexts, %ld lines, %ld violations", contexts, lines, g_bad);
    if (g_overcounted) fprintf(stderr, " (%ld plans of wgrad_h3_kernel at 5 taps, 16 samples count two blocks per CU where the LDS holds one: known)", g_overcounted);
    fprintf(stderr, "\n");
    return g_bad ? 1 : 0;
}
