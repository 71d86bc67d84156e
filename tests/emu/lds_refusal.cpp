// TEST INFRASTRUCTURE ONLY: every dispatcher of the kernels with a hand-carved LDS layout (csrc/*_inst.cpp), built against the emulator,
// refuses a request of dynamic LDS one byte short of its instantiation's layout (csrc/wunet_lds.h) with WUNET_LAUNCH_E_LDS, leaves the
// bytes it needed in wunet_lds_needed and launches nothing; at exactly the layout's bytes it launches (an empty grid: no block runs).
// Stand-alone host program (make -C tests/emu lds_refusal; tests/test_lds_refusal.py runs it).  Exit status 1 on a failure.
#include <cstdio>
#include "wunet_h3d.h"
#include "wunet_h3u.h"
#include "wunet_launch.h"

static int g_bad = 0;

template <class Call>
static void expect_refusal(const char* what, size_t need, Call call)
{
    const long before = emu::launch_count();
    wunet_lds_needed = 0;
    const int short_rc = call(need - 1);
    const long after_short = emu::launch_count() - before;
    const bool refused = short_rc == WUNET_LAUNCH_E_LDS && wunet_lds_needed == need && after_short == 0;
    const int exact_rc = call(need);
    const long after_exact = emu::launch_count() - before;
    const bool launched = exact_rc == 0 && after_exact == 1;
    printf("%-32s needs %6zu bytes: one short -> rc %d, %ld launches; exact -> rc %d, %ld launch(es)  %s\n", what, need, short_rc, after_short,
           exact_rc, after_exact, refused && launched ? "ok" : "FAILED");
    if (!refused || !launched) ++g_bad;
}

int main()
{
    const dim3 none(0, 1, 1);      // a launch that gets past the check runs no block
    const hipStream_t st = nullptr;
    {
        ConvArgs a{};
        a.rowp = wunet_lds::conv_mfma_rowp(256, 4);
        expect_refusal("conv_mfma_kernel<15, 3, 4>", wunet_lds::conv_mfma(15, 3).bytes(a.rowp), [&](size_t smem) { return wunet_launch_conv_15(a, 3, 4, none, smem, st); });
        a.rowp = wunet_lds::conv_mfma_rowp(16, 1);
        expect_refusal("conv_mfma_kernel<5, 2, 1>", wunet_lds::conv_mfma(5, 2).bytes(a.rowp), [&](size_t smem) { return wunet_launch_conv_5(a, 2, 1, none, smem, st); });
    }
    {
        WgradArgs a{};
        a.rowp = wunet_lds::wgrad_mfma_rowp(15, 64);
        expect_refusal("wgrad_mfma_kernel<15, 4, 6>", wunet_lds::wgrad_mfma(15, 4, 6, false).bytes(a.rowp),
                       [&](size_t smem) { return wunet_launch_wgrad_15(a, 4, 6, 2, 0, none, smem, st); });
        a.rowp = wunet_lds::wgrad_mfma_rowp(5, 32);
        expect_refusal("wgrad_mfma_kernel<5, 6, 2>", wunet_lds::wgrad_mfma(5, 6, 2, false).bytes(a.rowp),
                       [&](size_t smem) { return wunet_launch_wgrad_5(a, 6, 2, 8, 0, none, smem, st); });
    }
    {
        WgradH3Args a{};
        expect_refusal("wgrad_h3_kernel<15, 2, 4>", wunet_lds::wgrad_h3(15, 2, 4, 128, false).bytes(),
                       [&](size_t smem) { return wunet_launch_wgrad_h3(a, 15, 2, 4, 128, none, smem, st, false); });
        WgradH3dArgs d{};
        expect_refusal("wgrad_h3d_kernel<5, 3>", wunet_lds::wgrad_h3d(5, 3, false, false, 128).bytes(),
                       [&](size_t smem) { return wunet_launch_wgrad_h3d(d, 5, 3, false, none, smem, st, false, 128); });
        expect_refusal("wgrad_h3d_kernel<15, 5, db, bf>", wunet_lds::wgrad_h3d(15, 5, true, true, 128).bytes(),
                       [&](size_t smem) { return wunet_launch_wgrad_h3d(d, 15, 5, true, none, smem, st, true, 128); });
    }
    {
        ConvH3Args a{};
        a.mblocks = 5; a.NS = a.NFS = 1;
        a.epi_eval = 1;
        expect_refusal("conv_h3d_kernel<15, 3, 1> eval", wunet_lds::conv_h3d(3, 1, false, false).bytes(5 * 3 * 16, 1),
                       [&](size_t smem) { return wunet_launch_conv_h3d(a, 15, 3, 1, none, smem, st, false); });
        expect_refusal("conv_h3d_kernel<.., evop>", wunet_lds::conv_h3d(3, 1, false, false).bytes(5 * 3 * 16, 1),
                       [&](size_t smem) { return wunet_launch_conv_h3d(a, 15, 3, 1, none, smem, st, false, true); });
        a.epi_eval = 0;
        expect_refusal("conv_h3d_kernel<5, 2, 16, bf>", wunet_lds::conv_h3d(2, 16, true, false).bytes(5 * 2 * 16, 0),
                       [&](size_t smem) { return wunet_launch_conv_h3d(a, 5, 2, 16, none, smem, st, true); });
        expect_refusal("conv_h3d_kernel<.., upt>", wunet_lds::conv_h3d(4, 1, false, true).bytes(5 * 4 * 16, 0),
                       [&](size_t smem) { return wunet_launch_conv_h3d(a, 5, 4, 1, none, smem, st, false, false, true); });
    }
    {
        ConvH3uArgs a{};
        a.C8 = 9; a.mblocks = 2;
        expect_refusal("conv_h3u_kernel<4>", wunet_lds::conv_h3u(4).bytes(9, 2 * 4 * 16), [&](size_t smem) { return wunet_launch_conv_h3u(a, 4, none, smem, st); });
        wunet_half copy[8];
        a.oxh = copy;
        expect_refusal("conv_h3u_kernel<2, copy>", wunet_lds::conv_h3u(2).bytes(9, 2 * 2 * 16), [&](size_t smem) { return wunet_launch_conv_h3u(a, 2, none, smem, st); });
    }
    printf("lds_refusal: %d failed\n", g_bad);
    return g_bad ? 1 : 0;
}
