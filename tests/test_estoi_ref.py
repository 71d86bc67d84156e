"""-m "not gpu": the float64 yardstick of the ESTOI tests (tests/estoi_ref.py) checked on its own - properties of the score, the
float64 figures of the six cases, the positive norms the derivative rests on - and, where pystoi is installed, against
pystoi.stoi(..., extended=True) itself (1e-9: the bar the STOI oracle has against pystoi; it absorbs pystoi's EPS * randn dither)."""
import numpy as np
import pytest

import estoi_cases as EC
import estoi_ref as E


def test_a_signal_against_itself_scores_one_scale_is_ignored_and_noise_lowers_the_score():
    rows, T, fs, _ = EC.CASES["a"]
    ref = EC.check_inputs("a")
    c = ref["c"].double().numpy()
    same, _ = E.oracle64(c, c, fs)
    assert (same >= 0.999).all()
    base, _ = E.oracle64(c, ref["e"].double().numpy(), fs)
    tripled, _ = E.oracle64(3.0 * c, ref["e"].double().numpy(), fs)
    assert np.abs(tripled - base).max() <= 1e-12 and np.abs(E.oracle64(3.0 * c, c, fs)[0] - same).max() <= 1e-12
    noise = np.random.default_rng(1).standard_normal((rows, T))
    light, _ = E.oracle64(c, c + 0.01 * noise, fs)
    heavy, _ = E.oracle64(c, c + 0.1 * noise, fs)
    assert (heavy < light).all() and (light < same).all()


@pytest.mark.parametrize("name", sorted(EC.CASES))
def test_the_cases_keep_their_float64_figures_and_positive_norms(name):
    ref = EC.check_inputs(name)
    quoted = {"a": (0.27077, 0.00580), "b": (0.28195, 0.00163, 0.00585), "c": (1e-5,), "d": (0.33527, 0.03111), "e": (0.17305, 0.06422),
              "f": (0.27077, 1e-5)}
    assert np.abs(ref["score"] - np.array(quoted[name])).max() < 1e-5
    assert {"a": [33, 33], "b": [36, 36, 36], "c": [16], "d": [66, 67], "e": [66, 66], "f": [33, 27]}[name] == list(ref["frames"])


def test_the_extended_score_is_not_the_plain_one():
    import stoi_ref as R
    ref = EC.check_inputs("d")
    plain = R.case_reference(*EC.CASES["d"])["score"]
    assert (np.abs(ref["score"] - plain) > 0.1).all()


def test_the_torch_restatement_of_the_loss_is_the_numpy_score():
    """estoi_ref.loss_and_grad (torch, the direct resampler) and estoi_ref.oracle64 (numpy, scipy's) are two statements of one
    definition: their float64 scores agree to 1e-9, and the loss is minus their mean."""
    ref = E.loss_reference(*EC.CASES["b"])
    assert np.abs(ref["scores64"] - ref["score"]).max() <= 1e-9 and abs(ref["loss"] + ref["scores64"].mean()) <= 1e-15
    assert all(np.abs(ref["g64"][r]).max() > 0.0 for r in ref["scoring"]) and np.isfinite(ref["g64"]).all()


@pytest.mark.parametrize("name", ("a", "b", "e"))
def test_oracle64_is_pystoi_extended(name):
    pystoi = pytest.importorskip("pystoi")
    rows, T, fs, _ = EC.CASES[name]
    ref = EC.check_inputs(name)
    for r in range(rows):
        want = pystoi.stoi(ref["c"][r].double().numpy(), ref["e"][r].double().numpy(), fs, extended=True)
        assert abs(ref["score"][r] - want) <= 1e-9
