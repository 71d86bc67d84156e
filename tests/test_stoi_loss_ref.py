"""-m "not gpu": the yardstick of the STOI loss tests itself (tests/stoi_loss_ref.py).  Its float64 scores are those of the numpy / scipy
oracle (tests/stoi_ref.py: oracle64) to 1e-12, and its autograd gradient agrees with a central finite difference of its own loss
along a random direction.  The finite difference's bar: with step h = 1e-5 along a unit-variance direction v the rounding part is about
2^-52 |loss| / h = 2e-11 and the truncation part h^2 |f'''| / 6 - both far below 1e-5 of |g . v| (about 2 here) unless an item
crosses the kink of the clip, which the kink margin of the inputs (>= 1e-4, asserted) excludes for a perturbation of 1e-5 on signals of
amplitude 0.1.  Measured: 6 - 7 digits agree."""
import numpy as np
import pytest
import torch

import stoi_loss_cases as LC
import stoi_loss_ref as L


@pytest.mark.parametrize("name", ("a", "b", "e"))
def test_the_torch_port_reproduces_the_float64_oracle(name):
    ref = LC.check_inputs(name)
    d = np.abs(ref["scores64"] - ref["score"]).max()
    print(f"case {name}: max |port - oracle64| {d:.2e}")
    assert d <= 1e-12 and abs(ref["loss"] + ref["score"].mean()) <= 1e-12


@pytest.mark.parametrize("name, row", (("a", 0), ("b", 1)))
def test_the_autograd_gradient_matches_a_central_finite_difference(name, row):
    fs = LC.CASES[name][2]
    ref = LC.check_inputs(name)
    c, e = ref["c"][row:row + 1].double(), ref["e"][row:row + 1].double()
    v = torch.from_numpy(np.random.default_rng(7).standard_normal(e.shape))
    g = L.oracle64_grad(c, e, fs)[2]
    h = 1e-5
    fd = (L.oracle64_grad(c, e + h * v, fs)[0] - L.oracle64_grad(c, e - h * v, fs)[0]) / (2.0 * h)
    gv = float((g * v.numpy()).sum())
    print(f"case {name} row {row}: g . v {gv:.9e}  finite difference {fd:.9e}  relative {abs(fd - gv) / abs(gv):.2e}")
    assert abs(gv) > 1e-3 and abs(fd - gv) <= 1e-5 * abs(gv)
    # one row of a batch of `rows` rows carries 1 / rows of it
    assert np.abs(ref["g64"][row] * LC.CASES[name][0] - g[0]).max() <= 1e-12 * np.abs(g[0]).max()
