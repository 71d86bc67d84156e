"""-m "not gpu": the float64 yardstick of the STOI tests (tests/stoi_ref.py) checked on its own - the resampler against the polyphase
sum as written, the band edges against the published list, two properties of the score - and, where pystoi is installed, against
pystoi itself."""
import numpy as np
import pytest

import stoi_cases as C
import stoi_ref as R


@pytest.mark.parametrize("fs", (16000, 8000))
def test_the_oracles_resampler_is_the_direct_polyphase_sum(fs):
    c, _ = R.pair(1, 3001, fs)
    x = c[0].double().numpy()
    a, b = R.resample_scipy(x, fs), R.resample_direct(x, fs)
    p, q = R.pq(fs)
    assert len(a) == len(b) == -(-3001 * p // q)
    assert np.abs(a - b).max() <= 1e-12
    assert {16000: (5, 8, 290), 8000: (5, 4, 182)}[fs] == R.taps(fs)[:3] and len(R.taps(fs)[3]) == 2 * R.taps(fs)[2] + 1


def test_band_edges_from_the_formula():
    assert list(R.band_edges()) == [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87),
                                    (87, 109), (109, 138), (138, 174), (174, 219)]


def test_a_signal_against_itself_scores_one_and_noise_lowers_the_score():
    rows, T, fs, _ = C.CASES["a"]
    ref = C.check_inputs("a")
    same, _ = R.oracle64(ref["c"], ref["c"], fs)
    assert (same >= 0.999).all()
    rng = np.random.default_rng(1)
    noise = rng.standard_normal((rows, T))
    c = ref["c"].double().numpy()
    light, _ = R.oracle64(c, c + 0.01 * noise, fs)
    heavy, _ = R.oracle64(c, c + 0.1 * noise, fs)
    assert (heavy < light).all() and (light < same).all()


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_the_cases_keep_their_margin_and_their_float64_figures(name):
    ref = C.check_inputs(name)
    quoted = {"a": (0.7026, 0.6232), "b": (0.7440, 0.6718, 0.5531), "c": (1e-5,), "d": (0.7116, 0.6974), "e": (0.6411, 0.5561), "f": (0.7026, 1e-5)}
    assert np.abs(ref["score"] - np.array(quoted[name])).max() < 5e-5
    assert {"a": [33, 33], "b": [36, 36, 36], "c": [16], "d": [66, 67], "e": [66, 66], "f": [33, 27]}[name] == list(ref["frames"])


@pytest.mark.parametrize("name", ("a", "b", "e"))
def test_oracle64_is_pystoi(name):
    pystoi = pytest.importorskip("pystoi")
    rows, T, fs, _ = C.CASES[name]
    ref = C.check_inputs(name)
    for r in range(rows):
        want = pystoi.stoi(ref["c"][r].double().numpy(), ref["e"][r].double().numpy(), fs, extended=False)
        assert abs(ref["score"][r] - want) <= 1e-9
