"""The bf16 instantiations of the GEMM kernels (conv_h3d_kernel<.., bf16>, wgrad_h3d_kernel / wgrad_h3_kernel<.., bf16>) one op at a
time, through wunet_op_conv1d_bf16 / _dgrad_bf16 / _wgrad_bf16 on the CPU fiber emulator, and the per-layer forward of forced-bf16
networks - against references from which the bf16 rounding itself has been taken out (tests/bf16_ref.py): the float64 conv of the
bf16-ROUNDED operands.  What is left is fp32 accumulation, so the bars are those of the fp16-split kernels (tests/test_emu_split_ops.py:
2e-6, 4e-6 on the weight gradient's largest entry) - four orders of magnitude below the bf16 noise that the whole-network tests of this
mode (tests/test_bf16_mode.py) have to allow.  tests/test_gpu_bf16_ops.py runs the same cases on the hardware.

Measured here (tensor-relative norm / largest difference over the largest |ref|) over the 15 cases of tests/split_op_cases.py, the
tie set and the ten 16-level geometries:
  conv   4.7e-8 .. 9.6e-8 / <= 1.8e-7     dgrad  5.7e-8 .. 1.4e-7 / <= 3.2e-7     wgrad  7.1e-8 .. 8.3e-8 / <= 2.1e-7
Against the plain float64 conv of the unrounded operands the same results are 1.5e-3 .. 2.5e-3 away.

Plan divergence (the planner does not depend on the device; every case prints the kernels of its bf16 run and of the fp16-split run
of the same geometry side by side, the split-K reduce named by its split count).  The tilings - rows per wave, items per tile, the
weight-gradient kernel - are the same in all 26 cases; ONE case gets other split counts, B16-288x312-L16-k15 of the 16-level
geometries: 27 splits forward and 15 in the data gradient against 15 and 14, because one operand plane of the 16-segment tile is
48 KB of LDS instead of 96 and a CU then holds two blocks of it (wunet_lds.h: ConvH3d::blocks_per_cu), so one round of resident blocks takes twice the
splits.  The table of tests/split_op_cases.py has no such case (its 16-sample cases have too few K stages to split further).
bf16_ref.PLAN_DIVERGENCE names the cases; each test holds it to what the planner does."""
import importlib

import numpy as np
import pytest
import torch

import bf16_ref as R
import emu_lib
import split_op_cases as C
from conftest import PKG_NAME
from oracle import c_oracle

REL, MAX, MAX_WGRAD = 2e-6, 2e-6, 4e-6


def _run(case, suffix):
    """(z, dx, dw) of one case on the `_bf16` or `_split` entry points and the kernels that ran."""
    x, w, b, gz = R.operands(case)
    conv, dgrad, wgrad = (getattr(emu_lib, f + suffix) for f in ("op_conv1d", "op_dgrad", "op_wgrad"))
    got = {}

    def run():
        got["r"] = (conv(x, w, b), dgrad(gz, w, x.shape[1]), wgrad(gz, x, w.shape[2]))
    names = C.profiled(emu_lib.lib(), run)
    return got["r"], names


def _check(case, got):
    for what, g, r, bar in zip(("conv", "dgrad", "wgrad"), got, R.reference(case), (MAX, MAX, MAX_WGRAD)):
        assert np.isfinite(g).all(), (what, int((~np.isfinite(g)).sum()))
        rel, err = C.errors(g, r)
        print(f"emu bf16 {R.case_id(case)} {what}: rel {rel:.2e} max {err:.2e}")
        assert rel < REL and err < bar, (what, rel, err)


def _check_plan(case, names):
    """The kernels of the bf16 run beside those of the fp16-split run of the same operands (printed), and whether they differ beyond
    the bf16 tag - which they do exactly for the cases of R.PLAN_DIVERGENCE."""
    _, split_names = _run(case, "_split")
    print(R.kernels_side_by_side(case, names, split_names))
    assert R.plans_differ(names, split_names) == (C.case_id(tuple(case[:7])) in R.PLAN_DIVERGENCE), (names, split_names)


def test_round_bf16_is_round_to_nearest_even():
    """R.round_bf16 (the bit arithmetic of wunet_f2b) against torch's float32 -> bfloat16 conversion, bit for bit: random values over
    the whole exponent range, exact ties above bf16 words of both parities (down to the even one, up from the odd one), +-0,
    subnormals (also the ties among them), the largest finite values (which round to inf) and +-inf; a NaN stays a NaN with its sign
    and gets the quiet bit."""
    rng = np.random.default_rng(7)
    words = rng.integers(0, 0x7f80, 4096, dtype=np.uint32)                    # finite bf16 words, subnormal ones included
    ties = ((words << np.uint32(16)) | np.uint32(0x8000)).view(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, 9.18e-41, 1.17549435e-38, 3.4028235e38, -3.4028235e38,
                        3.3895314e38, 1.0, 1.00390625, 1.01171875], np.float32)
    a = np.concatenate([rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32).view(np.float32),
                        (rng.standard_normal(1 << 14) * 10.0 ** rng.uniform(-30, 30, 1 << 14)).astype(np.float32), ties, -ties, special])
    a = a[~np.isnan(a)]
    want = torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()
    got = R.round_bf16(a)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not (got.view(np.uint32) & np.uint32(0xffff)).any()
    low = (words >> np.uint32(0)) & np.uint32(1)                              # ties: to the even word, whichever side it lies on
    assert np.array_equal(R.round_bf16(ties).view(np.uint32) >> np.uint32(16), words + low)
    nans = np.array([0x7f800001, 0xff800001, 0x7fc00000, 0xffffffff, 0x7f80ffff], np.uint32)
    r = R.round_bf16(nans.view(np.float32)).view(np.uint32)
    assert np.isnan(r.view(np.float32)).all() and np.array_equal(r, ((nans >> np.uint32(16)) | np.uint32(0x40)) << np.uint32(16))


@pytest.mark.parametrize("case", C.CASES + [R.TIE_CASE], ids=R.case_id)
def test_bf16_ops_vs_conv_of_rounded_operands(case):
    """conv, data gradient and weight gradient of one case, every element (outputs pre-filled with NaN), and the kernels: two
    conv_h3* launches and one wgrad_h3* launch, all of them bf16 instantiations."""
    got, names = _run(case, "_bf16")
    R.check_kernel_names(case, names)
    _check(case, got)
    _check_plan(case, names)


def test_rounding_matters_at_this_bar():
    """The reference really is the conv of ROUNDED operands: against the plain float64 conv the same output is 1e-3 away (so a mode
    switch that silently ran the fp16-split kernels would not pass for bf16 either: the names are asserted above), and the planted
    ties decide products the bar can see - rounding them half away from zero moves the reference by more than the bar."""
    case = R.TIE_CASE
    x, w, b, _ = R.operands(case)
    z = emu_lib.op_conv1d_bf16(x, w, b)
    rel_plain, _ = C.errors(z, c_oracle.conv1d_fwd(x, w, b))
    assert rel_plain > 5e-4, rel_plain

    def half_away(a):             # the wrong rule: ties away from zero
        u = a.view(np.uint32).astype(np.uint64)
        return (((u + 0x8000) >> 16) << 16).astype(np.uint32).view(np.float32).reshape(a.shape)
    rel_wrong, _ = C.errors(c_oracle.conv1d_fwd(half_away(x), half_away(w), b), R.reference(case)[0])
    print(f"plain conv {rel_plain:.2e}, ties rounded away from zero {rel_wrong:.2e}")
    assert rel_wrong > 10 * REL, rel_wrong


@pytest.mark.parametrize("case", C.KTAIL_CASES, ids=C.case_id)
def test_bf16_k_tail(case, monkeypatch):
    """The cases with left-over channel groups: the K tail of conv_h3d_kernel<.., bf16> (WUNET_H3_KTAIL=1, the default) and the
    zero-padded last chunk (= 0) both meet the bar on every element, and are not the same bits."""
    x, w, b, gz = R.operands(case)
    zr, dxr, _ = R.reference(case)
    got = {}
    for kt in ("0", "1"):
        monkeypatch.setenv("WUNET_H3_KTAIL", kt)
        z, dx = emu_lib.op_conv1d_bf16(x, w, b), emu_lib.op_dgrad_bf16(gz, w, x.shape[1])
        for what, g, r in (("conv", z, zr), ("dgrad", dx, dxr)):
            assert np.isfinite(g).all(), what
            rel, err = C.errors(g, r)
            print(f"emu bf16 {C.case_id(case)} ktail={kt} {what}: rel {rel:.2e} max {err:.2e}")
            assert rel < REL and err < MAX, (what, kt, rel, err)
        got[kt] = (z, dx)
    assert not (np.array_equal(got["0"][0], got["1"][0]) and np.array_equal(got["0"][1], got["1"][1]))


@pytest.mark.parametrize("case", R.DEEP16_CASES, ids=R.case_id)
def test_bf16_ops_at_16_level_geometries(case):
    """The 16 .. 256-sample layers of the 16-level net (bench.py's deep16_bf16 extra): 192 .. 312 rows and up to 648 K channels, which
    the table does not reach.  Same bars; the table's wgrad_h3d / wgrad_h3 rule is not asserted (it holds up to 80 output channels)."""
    got, names = _run(case, "_bf16")
    R.check_kernel_names(case, names, deep=True)
    _check(case, got)
    _check_plan(case, names)


def test_some_case_plans_differently_in_bf16():
    """ConvH3d::blocks_per_cu (wunet_lds.h) gives the bf16 mode other split-K plans: at least one geometry of this module must run one."""
    assert R.PLAN_DIVERGENCE and R.PLAN_DIVERGENCE <= {C.case_id(c) for c in C.CASES + R.DEEP16_CASES}


def _engine():
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    return eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True, h3=4)


@pytest.mark.parametrize("net", R.NETS, ids=C.net_id)
def test_bf16_layer_forward_teacher_forced(net):
    """Every layer of a forced-bf16 network (prep_h3_kernel / split_act_kernel with bf set, the statistics epilogue, padded rows, the
    planner's own layer set) against the float64 conv of the rounded input formed from the DEVICE's previous raw output(s)
    (R.measure_layer_forward), training and eval.  Measured here over the five nets and both modes (60 layers): no output outside its
    tolerance, worst error / tolerance 0.98 (an input that did round the other way: the allowance is one bf16 ulp times |w|, exact in
    kind), share of a layer's outputs beyond the base part of the tolerance <= 2.0e-2 (0 on most layers), largest tolerance 7.0e-4
    of the layer's scale; layer 0 <= 1.9e-7, head <= 2.7e-7."""
    eng = _engine()
    n = net[0]
    for training in (True, False):
        res = {}

        def run():
            res.update(R.measure_layer_forward(eng, "cpu", net, training))
        ran = C.profiled(eng.lib, run)
        outside, ratio, share, tol = R.layer_forward_summary(res)
        print(f"emu bf16 layer forward {C.net_id(net)} {'train' if training else 'eval'}: outside {outside}, worst err/tol {ratio:.2f}, "
              f"share beyond base {share:.1e}, largest tol {tol:.1e}, first {res['first']:.1e}, head {res['head']:.1e}; per layer share "
              + " ".join(f"{l['share']:.0e}" for l in res["layers"]))
        assert res["first"] < 2e-5 and res["head"] < 1e-5, (res["first"], res["head"])
        for l in res["layers"]:
            assert l["outside"] == 0, l
            assert l["share"] <= 5e-2, l
            assert l["pad_exact"] in (None, True), l
        convs = {k: v for k, v in ran.items() if k.startswith("conv_h3")}
        assert convs and all(k.endswith(", bf16>") for k in convs) and sum(convs.values()) == 2 * n, ran
        if net[3] & (net[3] - 1):
            assert all(l["pad_exact"] is True for l in res["layers"]), res["layers"]
