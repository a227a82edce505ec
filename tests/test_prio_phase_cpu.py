"""The priority rotation of the register/LDS-resident step kernels is keyed on time: bbx_prio_phase (bbx_common.h) maps the
100 MHz clock's low 32 bits and a wave's rank on its SIMD to the s_setprio operand, one statement shared by the kernel and
this check.  tests/prio_phase_check.cpp — built here with -fsanitize=address,undefined, run on its own — sweeps it tick by
tick: the value stays in 0..3, the four ranks hold four different priorities at every tick, over a whole cycle of four slots
every rank holds every priority for exactly one slot, and the 32-bit wrap of the clock is an ordinary slot boundary.  Built
once more with every slot length the header admits at its ends and with those that were measured (13, 14, 15)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = 5                                                  # the program's sweeps: three cycles of four slots each


def _report(tmp_path, shift):
    exe = str(tmp_path / ("prio_phase_check_%s" % shift))
    csrc = os.path.join(ROOT, "deepgroebner_amd", "csrc")
    define = [] if shift is None else ["-DBBX_PRIO_TICK_SHIFT=%d" % shift]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                          + define + ["-I", csrc, os.path.join(ROOT, "tests", "prio_phase_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    return {ln.split()[0]: [int(v) for v in ln.split()[2::2]] for ln in p.stdout.splitlines() if "cases" in ln}


@pytest.mark.parametrize("shift", [None, 0, 5, 13, 14, 15])
def test_rotation_over_the_clock(tmp_path, shift):
    rep = _report(tmp_path, shift)
    s = rep["shift"][0]
    assert s == (shift if shift is not None else s) and 0 <= s <= 30
    ticks = WINDOWS * 3 * (4 << s)
    assert rep["range"] == [4 * ticks, 0], rep
    assert rep["distinct"] == [ticks, 0], rep
    assert rep["share"] == [WINDOWS * 16, 0], rep
    assert rep["wrap"] == [8, 0], rep


def test_shipped_slot_fits_a_launch():
    """The slot is at least two looks long (a wave looks once per 64 steps, about 10.5 k ticks at 1.65 us per step: a shorter
    slot is over before every wave has seen it) and a 1024-step launch (about 170 k ticks of steps) holds at least one whole
    cycle of four slots (in less, the ranks' shares of a launch cannot be equal)."""
    import re
    text = open(os.path.join(ROOT, "deepgroebner_amd", "csrc", "bbx_common.h")).read()
    s = int(re.search(r"#define BBX_PRIO_TICK_SHIFT (\d+)", text).group(1))
    assert (1 << s) >= 2 * 10500 and (4 << s) <= 170000, s
