"""-m gpu: the backward pass on the MI355X against the float64 arbiter linearised at the device's own forward point - the case table,
the reference and the assertions of tests/linearised_ref.py (shared with tests/test_emu_backward_linearised.py): every parameter
gradient and the input gradient within 2 x (fp32 MFMA path) / 4 x (fp16-split path) d_ref of the arbiter, d_ref being the distance
of the reference's own float32 ATen arithmetic at the same point, measured on the CPU at test time; at most 4 ambiguous slopes.

Measured on the MI355X (profiles/backward_linearised.txt): d_ref 6.0e-7 .. 3.1e-6, the device's worst tensor at 0.40 .. 2.06 x d_ref (the
worst: encoder.1's BatchNorm-bias gradient of the unsplit-encoder case at 2.06 x, bar 4 x; fp32 path at most 1.26 x, bar 2 x), at
most 2 ambiguous slopes in a case, none of them taken the other way."""
import importlib

import pytest
import torch

import linearised_ref as lr
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
SWITCHES = ("WUNET_H3_NOSPLIT", "WUNET_NO_E0", "WUNET_REDUCE_SERIAL", "WUNET_NO_ENC_GZ", "WUNET_PA_SWAP", "WUNET_UPT")


@pytest.mark.parametrize("case", lr.CASES, ids=lr.case_id)
def test_backward_matches_the_arbiter_at_the_devices_forward_point(monkeypatch, case):
    for k in SWITCHES:                           # (planner switches, read when a context is planned: only the case's own are set)
        monkeypatch.delenv(k, raising=False)
    for k, v in case[5].items():
        monkeypatch.setenv(k, v)
    eng = importlib.import_module(PKG_NAME + ".engine").Engine(h3=case[0])
    lr.check(case, lr.device_run(eng, torch.device("cuda:0"), case), "MI355X")
