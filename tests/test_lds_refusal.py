"""A dispatcher refuses a launch whose dynamic-LDS request is smaller than its instantiation's layout (csrc/wunet_lds.h): the stand-alone
host program tests/emu/lds_refusal.cpp (built against the emulator by tests/emu/Makefile) hands every instantiation unit's dispatcher
a request one byte short - WUNET_LAUNCH_E_LDS, nothing launched - and then exactly the layout's bytes, which launches."""
import fcntl
import os
import subprocess

_EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


def test_dispatchers_refuse_an_undersized_lds_request():
    with open(os.path.join(_EMU, ".build.lock"), "w") as lk:      # (the lock of tests/emu_lib.py: one make at a time in that directory)
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", _EMU, "-s", "lds_refusal"], check=True)
    r = subprocess.run([os.path.join(_EMU, "lds_refusal")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    # two tap counts of conv_inst and of wgrad_inst, both kernels of h3_inst, the four forms of h3d_inst, both of h3u_inst
    assert len(lines) == 14 and lines[-1] == "lds_refusal: 0 failed" and all(ln.endswith("  ok") for ln in lines[:-1]), r.stdout
