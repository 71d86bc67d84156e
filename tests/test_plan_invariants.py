"""The planner's invariants on the CPU: tools/plan_dump.cpp (host code only, built by tests/emu/Makefile's plan_dump target) plans
each shape below under wunet_set_h3 0..4 and every planner switch set and asserts, per context, that the forward segment lies
inside the workspace, that every offset in allotment order is non-decreasing, 64-aligned and below its segment's end, that a
replanned context equals a fresh one, and that skip_from / evop / upt / h3u / h3u_train / h3w are only set on layers that meet what
their readers rely on."""
import fcntl
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")

SHAPES = [
    (12, 24, 64, 16384),        # the benchmark's
    (16, 24, 32, 65536),        # BASELINE configs[4]: 16 levels, batch 32
    (12, 24, 2, 12288),         # a padded length
    # tools/emu_lib_ab.py's shapes
    (2, 4, 2, 32), (3, 8, 3, 64), (2, 24, 1, 1024), (3, 8, 2, 16), (4, 4, 2, 16),
    (3, 24, 3, 2048), (4, 16, 3, 4096), (3, 8, 2, 96), (3, 16, 3, 768), (2, 24, 3, 1536),
]


def test_plan_invariants():
    with open(os.path.join(_EMU, ".build.lock"), "w") as lk:      # (the lock of tests/emu_lib.py: one make at a time in that directory)
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", _EMU, "-s", "plan_dump"], check=True)
    cmd = [os.path.join(_EMU, "plan_dump"), "--check"]
    for s in SHAPES:
        cmd += ["--shape"] + [str(v) for v in s]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout == ""
    # 5 settings of wunet_set_h3 x 19 switch sets per shape (WUNET_NO_ENC_GZ and WUNET_PA_SWAP are planner switches too), none refused
    assert f"{len(SHAPES) * 5 * 19} contexts" in r.stderr and " 0 violations" in r.stderr, r.stderr[-400:]
    # the backward's two A/B switches reach the planned context (the dump names them where one is off) and nothing else sets them
    r = subprocess.run([os.path.join(_EMU, "plan_dump"), "--shape", "3", "24", "3", "2048", "--shape", "4", "16", "3", "4096"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    ctx = [ln for ln in r.stdout.splitlines() if ln.startswith("ctx ")]
    assert len(ctx) == 2 * 5 * 19
    for ln in ctx:
        want = {"switches=[WUNET_NO_ENC_GZ=1]": " enc_gz=0 pa_swap=1", "switches=[WUNET_PA_SWAP=0]": " enc_gz=1 pa_swap=0"}
        hit = [v for k, v in want.items() if k in ln]
        assert (hit[0] in ln) if hit else ("enc_gz=" not in ln and "pa_swap=" not in ln), ln[:200]
