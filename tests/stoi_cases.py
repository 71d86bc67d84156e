"""The case table of the STOI metric, shared by tests/test_stoi_emu.py (CPU emulator) and tests/test_gpu_stoi.py (MI355X): what runs,
on which tensors, and the checks against tests/stoi_ref.py.  `engine` None = the product's default engine."""
import importlib

import numpy as np
import torch

import stoi_ref as R
from conftest import PKG_NAME

# name -> (rows, T, fs, gap lengths per row or None): the smallest shapes at which every stage can go wrong
CASES = {
    "a": (2, 5000, 10000, None),             # no resampling; 38 frames, 34 kept, 33 spectral: just above the 30-frame limit, 4 segments
    "b": (3, 9000, 16000, None),             # 5 / 8 resampling, odd length; 42 frames, 37 kept
    "c": (1, 4000, 16000, None),             # 16 spectral frames: the score is 1e-5 exactly
    "d": (2, 16384, 16000, None),            # the product's chunk; 78 frames, 67 and 68 kept: different counts, more than one 64-frame tile
    "e": (2, 8000, 8000, None),              # p > q: upsampling 5 / 4, L = 182; 77 frames, 67 kept
    "f": (2, 5000, 10000, (0.15, 0.30)),     # row 1's gap widened: it keeps 28 frames and returns 1e-5 beside a row that scores
}
EMU_CASES = ("a", "b", "c", "d", "e", "f")      # (the emulator runs all six in about two seconds)
MARGIN_DB = 0.05


def metrics():
    return importlib.import_module(PKG_NAME + ".metrics")


def check_inputs(name):
    """The one condition the bars rest on: every clean frame's energy lies at least 0.05 dB from its row's threshold max - 40 (nearer
    than that any float32 computation may flip a frame).  Case f also asserts its split: one row scores, its neighbour is short."""
    ref = R.case_reference(*CASES[name])
    print(f"case {name}: least energy margin {ref['margin']:.3f} dB; float64 scores {ref['score']}, frames {ref['frames']}")
    assert ref["margin"] >= MARGIN_DB
    if name == "f":
        assert ref["frames"][0] >= R.SEG > ref["frames"][1] and ref["score"][0] > 0.5 and ref["score"][1] == R.SHORT
    if name == "c":
        assert list(ref["frames"]) == [16] and ref["score"][0] == R.SHORT
    return ref


def run(engine, device, name, c=None, e=None):
    rows, T, fs, _ = CASES[name]
    ref = R.case_reference(*CASES[name])
    c = ref["c"].to(device) if c is None else c
    e = ref["e"].to(device) if e is None else e
    return metrics().stoi(c, e, sample_rate=fs, return_frames=True, engine=engine)


def check_case(name, engine, device, c=None, e=None):
    """Scores and frame counts of one case against the float64 oracle: frames exactly, |score - oracle64| <= 4 d_ref + 2^-23 per row.
    c / e: the case's inputs at another address (the unaligned test).  Returns (scores, frames)."""
    rows = CASES[name][0]
    ref = check_inputs(name)
    bar = R.bar(ref)
    score, frames = run(engine, device, name, c, e)
    assert score.shape == (rows,) and score.dtype == torch.float32 and score.device.type == device.type
    assert frames.shape == (rows,) and frames.dtype == torch.int32 and frames.device.type == device.type
    d = np.abs(score.double().cpu().numpy() - ref["score"])
    print(f"case {name}: scores {score.cpu().numpy()}  d {d.max():.2e} (d_ref {ref['d_ref']:.2e}: restate32 {ref['d_restate']:.2e}, "
          f"fft32 {ref['d_fft']:.2e}; bar {bar:.2e})  frames {frames.cpu().numpy()}")
    assert list(frames.cpu().numpy()) == list(ref["frames"]), (name, frames, ref["frames"])
    assert (d <= bar).all(), (name, d, bar)
    short = ref["frames"] < R.SEG
    assert (score.cpu().numpy()[short] == np.float32(R.SHORT)).all()
    return score, frames
