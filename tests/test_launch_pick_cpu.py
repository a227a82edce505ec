"""bbx_pick (deepgroebner_amd/csrc/bbx_pick.h) is the one way a launcher turns a run-time shape number into a template argument:
the constant handed to the callback is the value itself, and a value that is not listed launches nothing and returns the
"no such instantiation" code.  tests/launch_pick_check.cpp checks that on the host for every value list the library uses —
built here with -fsanitize=address,undefined as a program of its own."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_pick") / "launch_pick_check")
    csrc = os.path.join(ROOT, "deepgroebner_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, os.path.join(ROOT, "tests", "launch_pick_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    return {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^(\w+) cases (\d+) failed (\d+)$", p.stdout, re.M)}


def test_every_list_every_cell_and_every_refusal(report):
    assert set(report) == {"lists", "nested", "refusal"}, report
    assert all(failed == 0 for _, failed in report.values()), report
    # the counts are cumulative: six lists (19 listed values x 2 returns x 3 checks, 35 unlisted x 4), 20 cells x 2 + 1 and
    # 6 unlisted x 3, 6 refusal cells x 2 and 2 booleans x 2
    assert report["lists"][0] == 19 * 2 * 3 + 35 * 4
    assert report["nested"][0] - report["lists"][0] == 20 * 2 + 1 + 6 * 3
    assert report["refusal"][0] - report["nested"][0] == 6 * 2 + 2 * 2
