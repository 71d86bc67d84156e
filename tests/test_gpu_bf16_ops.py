"""-m gpu: the bf16 instantiations of the GEMM kernels (conv_h3d_kernel<.., bf16>, wgrad_h3d_kernel / wgrad_h3_kernel<.., bf16>) one op at
a time on the MI355X, through wunet_op_conv1d_bf16 / _dgrad_bf16 / _wgrad_bf16, and the per-layer forward of forced-bf16 networks
(Engine(h3=4)) - what tests/test_emu_bf16_ops.py runs on the CPU emulator, on the hardware: the one-plane LDS layout the DMA pieces
fill, v_mfma_f32_16x16x32_bf16, the store guards and the split-K plans of this mode's own LDS budget.

Reference (tests/bf16_ref.py): the float64 conv of the bf16-ROUNDED operands.  The operand scales are powers of two, wunet_f2b is
round to nearest even and a product of two bf16 values is exact in fp32, so only fp32 accumulation separates a correct kernel from
it: the bar is the 1e-5 (tensor-relative and relative to the tensor's largest entry, every element; outputs pre-filled with NaN)
that tests/test_gpu_split_ops_ragged.py and test_split_ops_at_baseline_geometries hold the fp16-split instantiations of the same
kernels to.  The whole-network tests of this mode (tests/test_bf16_mode.py, tests/test_gpu_parity.py) have to allow the bf16 noise
itself, 1.8e-2 on the output: a tile-edge, K-tail, split-K or store-guard error that moves a few percent of one layer passes them.

Figures on the MI355X (tensor-relative norm / largest difference over the largest |ref|; the CPU emulator's in brackets):
  15 table cases, tie set, ten 16-level geometries
    conv   4.2e-8 .. 9.0e-8 / <= 1.7e-7   [4.7e-8 .. 9.6e-8 / <= 1.8e-7]
    dgrad  4.8e-8 .. 1.2e-7 / <= 2.0e-7   [5.7e-8 .. 1.4e-7 / <= 3.2e-7]
    wgrad  6.3e-8 .. 7.4e-8 / <= 1.5e-7   [7.1e-8 .. 8.3e-8 / <= 2.1e-7]
  K tail on / off (4 cases, conv and dgrad): 6.3e-8 .. 9.2e-8 / <= 1.9e-7, the two arms not the same bits in any case
  kernels (all with the bf16 tag; conv + dgrad, their split-K counts where split_sum_kernel ran, the weight gradient) - the same
  tilings and split counts as the fp16-split run of the same case, printed beside them, in every case but the one marked *:
    B1-24x40-L256-k15   conv_h3d<15, 3, 1> + <15, 2, 1>, splits 3 + 4, wgrad_h3d<15, 2>     B2-20x24-L512-k5 (and ties)  conv_h3d<5, 2, 1> x 2, no split, wgrad_h3d<5, 2>
    B3-48x24-L128-k5    conv_h3d<5, 2, 2> + <5, 3, 2>, splits 2, wgrad_h3d<5, 2>            B5-16x56-L64-k15    conv_h3d<15, 2, 4> x 2, splits 2 + 6, wgrad_h3<15, 2>
    B9-72x40-L32-k5     conv_h3d<5, 3, 8> x 2, splits 2 + 3, wgrad_h3<5, 3>                 B17-40x72-L16-k15   conv_h3d<15, 3, 16> x 2, splits 6 + 9, wgrad_h3<15, 2>
    B2-72x80-L512-k15   conv_h3d<15, 3, 1> x 2, splits 7 + 8, wgrad_h3d<15, 3>              B3-104x24-L256-k5   conv_h3d<5, 2, 1> x 2, splits 4, wgrad_h3d<5, 2>
    B16-16x16-L16-k5    conv_h3d<5, 2, 16> x 2, no split, wgrad_h3<5, 2>                    B33-24x24-L16-k5    conv_h3d<5, 2, 16> x 2, no split, wgrad_h3<5, 2>
    B7-60x20-L64-k5     conv_h3d<5, 2, 4> x 2, splits 2, wgrad_h3<5, 2>                     B5-100x60-L128-k15  conv_h3d<15, 2, 2> x 2, splits 6 + 10, wgrad_h3d<15, 2>
    B1-20x24-L256-k15   conv_h3d<15, 2, 1> x 2, splits 3 + 3, wgrad_h3d<15, 2>              B3-20x40-L1024-k5   conv_h3d<5, 3, 1> + <5, 2, 1>, splits 2, wgrad_h3d<5, 3>
    B2-28x36-L2048-k15  conv_h3d<15, 3, 1> + <15, 2, 1>, splits 3 + 4, wgrad_h3d<15, 3>
    B4-192x216-L256-k15 conv_h3d<15, 3, 1> + <15, 2, 1>, splits 18 + 21, wgrad_h3d<15, 2>   B4-216x240-L128-k15 conv_h3d<15, 3, 2> + <15, 2, 2>, splits 21 + 23, wgrad_h3d<15, 2>
    B4-240x264-L64-k15  conv_h3d<15, 3, 4> x 2, splits 23 + 25, wgrad_h3<15, 2>             B8-264x288-L32-k15  conv_h3d<15, 3, 8> x 2, splits 25 + 27, wgrad_h3<15, 2>
  * B16-288x312-L16-k15 conv_h3d<15, 3, 16> + <15, 2, 16>, splits 27 + 15 (fp16-split: 15 + 14: one resident block of the 16-segment tile per CU, not two), wgrad_h3<15, 2>
    B16-648x312-L16-k5  conv_h3d<5, 3, 16> + <5, 2, 16>, splits 10 + 21, wgrad_h3<5, 2>     B8-600x288-L32-k5   conv_h3d<5, 3, 8> + <5, 2, 8>, splits 9 + 19, wgrad_h3<5, 3>
    B4-552x264-L64-k5   conv_h3d<5, 3, 4> x 2, splits 9 + 18, wgrad_h3<5, 3>                B4-504x240-L128-k5  conv_h3d<5, 3, 2> + <5, 2, 2>, splits 8 + 16, wgrad_h3d<5, 3>
    B4-456x216-L256-k5  conv_h3d<5, 3, 1> + <5, 2, 1>, splits 7 + 15, wgrad_h3d<5, 2>
  per-layer forward (no output outside its tolerance anywhere; worst error / tolerance, largest share of a layer's outputs beyond
  the base part, largest tolerance over the layer's scale, layer 0, head; training | eval; per-layer shares are printed):
    n3-ci20-B3-T2048  0.68, 2.2e-3, 7.6e-4, 1.5e-7, 2.0e-7 | 0.89, 4.1e-3, 2.7e-4, 1.5e-7, 2.8e-8
    n2-ci28-B1-T1024  0.33, 0,      6.6e-4, 1.4e-7, 1.9e-7 | 0.23, 0,      2.0e-4, 1.4e-7, 3.1e-8
    n3-ci16-B2-T768   0.92, 9.9e-3, 3.4e-4, 1.2e-7, 2.6e-7 | 0.42, 0,      5.1e-4, 1.2e-7, 8.7e-8
    n3-ci16-B3-T1024  0.92, 1.5e-3, 5.5e-4, 1.7e-7, 2.1e-7 | 0.93, 2.5e-3, 5.1e-4, 1.7e-7, 9.6e-8
    n4-ci16-B5-T1024  0.98, 9.1e-3, 5.2e-4, 1.9e-7, 2.8e-7 | 0.96, 6.9e-3, 2.8e-4, 1.9e-7, 8.3e-8
    shares are 0 on 44 of the 60 layers, at most 9.9e-3 (emulator: at most 2.0e-2); a ratio near 1 is an input that did round to the other
    bf16 neighbour (the allowance is one ulp times |w|, exact in kind).  Every conv but the first ran conv_h3d_kernel<.., bf16>, 2 n launches.
"""
import importlib

import numpy as np
import pytest
import torch

import bf16_ref as R
import split_op_cases as C
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
BAR = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def engine():
    return importlib.import_module(PKG_NAME + ".engine").default_engine()


def _nan(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def _check(what, got, ref):
    got = got.cpu().numpy()
    assert np.isfinite(got).all(), (what, int((~np.isfinite(got)).sum()))
    rel, err = C.errors(got, ref)
    print(f"{what}: rel {rel:.2e} max {err:.2e}")
    assert rel < BAR and err < BAR, (what, rel, err)
    return got


def _run(lib, dev, case, suffix, ops=("conv", "dgrad", "wgrad")):
    """(z, dx, dw) of one case on the `_bf16` or `_split` entry points (device tensors, pre-filled with NaN) and the kernels that ran."""
    B, Cin, Cout, L, K = case[:5]
    x, w, b, gz = (torch.tensor(a).to(dev) for a in R.operands(case))
    z, dx, dw = _nan((B, Cout, L), dev), _nan((B, Cin, L), dev), _nan((Cout, Cin, K), dev)
    fn = {op: getattr(lib, "wunet_op_conv1d" + ("" if op == "conv" else "_" + op) + suffix) for op in ops}

    def run():
        if "conv" in ops:
            assert fn["conv"](x.data_ptr(), w.data_ptr(), b.data_ptr(), z.data_ptr(), B, Cin, Cout, L, K, None) == 0, lib.wunet_last_error()
        if "dgrad" in ops:
            assert fn["dgrad"](gz.data_ptr(), w.data_ptr(), dx.data_ptr(), B, Cin, Cout, L, K, None) == 0, lib.wunet_last_error()
        if "wgrad" in ops:
            assert fn["wgrad"](gz.data_ptr(), x.data_ptr(), dw.data_ptr(), B, Cin, Cout, L, K, None) == 0, lib.wunet_last_error()
    names = C.profiled(lib, run)
    torch.cuda.synchronize()
    return (z, dx, dw), names


def _one_case(lib, dev, case, deep):
    got, names = _run(lib, dev, case, "_bf16")
    _, split_names = _run(lib, dev, case, "_split")
    print(R.kernels_side_by_side(case, names, split_names))
    R.check_kernel_names(case, names, deep=deep)
    assert R.plans_differ(names, split_names) == (C.case_id(tuple(case[:7])) in R.PLAN_DIVERGENCE), (names, split_names)
    for what, g, r in zip(("conv", "dgrad", "wgrad"), got, R.reference(case)):
        _check(f"{R.case_id(case)} {what}", g, r)


@pytest.mark.parametrize("case", C.CASES + [R.TIE_CASE], ids=R.case_id)
def test_bf16_ops_at_ragged_geometries(engine, dev, case):
    """conv, data gradient and weight gradient of one case of the split table (and of the set with planted rounding ties), every
    element, and the kernels: two conv_h3* launches (conv_h3d_kernel from 256 samples on) and one wgrad_h3* launch - wgrad_h3d_kernel
    from 128 samples on - all of them bf16 instantiations, planned as the emulator module records."""
    _one_case(engine.lib, dev, case, deep=False)


@pytest.mark.parametrize("case", R.DEEP16_CASES, ids=R.case_id)
def test_bf16_ops_at_16_level_geometries(engine, dev, case):
    """The 16 .. 256-sample layers of the 16-level net (bench.py's deep16_bf16 extra): 192 .. 312 rows, up to 648 K channels, 14 .. 27
    K splits.  The table's wgrad_h3d / wgrad_h3 rule is not asserted here (it holds up to 80 output channels)."""
    _one_case(engine.lib, dev, case, deep=True)


@pytest.mark.parametrize("case", C.KTAIL_CASES, ids=C.case_id)
def test_bf16_k_tail(engine, dev, monkeypatch, case):
    """The cases with left-over channel groups: conv_h3d_kernel<.., bf16>'s K tail (WUNET_H3_KTAIL=1, the default) and the zero-padded
    last chunk (= 0; read when the op plans its tiling) both meet the bar on every element, and are not the same numbers."""
    zr, dxr, _ = R.reference(case)
    got = {}
    for kt in ("0", "1"):
        monkeypatch.setenv("WUNET_H3_KTAIL", kt)
        (z, dx, _), _ = _run(engine.lib, dev, case, "_bf16", ops=("conv", "dgrad"))
        got[kt] = (_check(f"{C.case_id(case)} ktail={kt} conv", z, zr), _check(f"{C.case_id(case)} ktail={kt} dgrad", dx, dxr))
    assert not (np.array_equal(got["0"][0], got["1"][0]) and np.array_equal(got["0"][1], got["1"][1]))


@pytest.mark.parametrize("net", R.NETS, ids=C.net_id)
def test_bf16_layer_forward_teacher_forced(dev, net):
    """R.measure_layer_forward on the hardware, training and eval: every layer i >= 1 of a forced-bf16 network against the float64 conv
    of the rounded input formed from the DEVICE's previous raw output(s) - no output outside its tolerance (1e-5 of the layer's scale
    plus one bf16 ulp times |w| for every input that the device's fp32 activation may round the other way), at most 5e-2 of a layer's
    outputs beyond the first part alone; layer 0 (conv_first_kernel, fp32) at 2e-5 against the plain float64 conv, the head
    (head_fwd_kernel, fp32: no bf16 GEMM) at 1e-5 against tanh of the 1x1 conv of the device's last activation and the input; behind
    the true end of a padded row exactly the bias; every conv but the first on a conv_h3*_kernel<.., bf16>."""
    eng = importlib.import_module(PKG_NAME + ".engine").Engine(h3=4)
    n = net[0]
    for training in (True, False):
        res = {}

        def run():
            res.update(R.measure_layer_forward(eng, dev, net, training))
        ran = C.profiled(eng.lib, run)
        outside, ratio, share, tol = R.layer_forward_summary(res)
        convs = {k: v for k, v in ran.items() if k.startswith("conv_")}
        print(f"bf16 layer forward {C.net_id(net)} {'train' if training else 'eval'}: outside {outside}, worst err/tol {ratio:.2f}, "
              f"share beyond base {share:.1e}, largest tol {tol:.1e}, first {res['first']:.1e}, head {res['head']:.1e}; per layer share "
              + " ".join(f"{l['share']:.0e}" for l in res["layers"]) + f"; {convs}")
        assert res["first"] < 2e-5 and res["head"] < 1e-5, (res["first"], res["head"])
        for l in res["layers"]:
            assert l["outside"] == 0, l
            assert l["share"] <= 5e-2, l
            assert l["pad_exact"] in (None, True), l
        h3 = {k: v for k, v in ran.items() if k.startswith("conv_h3")}
        assert h3 and all(k.endswith(", bf16>") for k in h3) and sum(h3.values()) == 2 * n, ran
        if net[3] & (net[3] - 1):
            assert all(l["pad_exact"] is True for l in res["layers"]), res["layers"]
