"""The episode step limit (bbx_episode_limit), the parts that need no GPU: the pinned seeds of tests/episode_limit_cases.py show
the situations the GPU tests rely on (asserted on the oracle alone); the rule's helpers of bbx_common.h and the fast class's
t_lim arithmetic against a plain restatement (tests/episode_limit_check.cpp, built with -fsanitize=address,undefined and run on
its own); the two new symbols, their ctypes prototypes, the refusal of a negative limit and the size of the record header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.episode_limit_cases import CASES, EXACT_END, K, PIECE, case_walks, limited_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepgroebner_amd", "csrc")


@pytest.mark.parametrize("name", sorted(CASES))
def test_pinned_seeds_show_the_situations(name):
    c = CASES[name]
    mid = c["limits"][-2] if len(c["limits"]) > 1 else c["limits"][0]
    ws = case_walks(name, mid)
    ends = np.concatenate([w["end"] for w in ws])
    assert (ends == 2).any(), (name, "no episode is cut at limit", mid)
    assert (ends == 1).any(), (name, "no ordinary end at limit", mid)
    for w in ws:                                              # an episode never has more steps than the limit
        assert (w["episode_len"] <= mid).all() and len(w["done"]) == c["steps"]
        assert w["episodes"] == int((w["end"] != 0).sum()) and w["truncations"] == int((w["end"] == 2).sum())
    if name in EXACT_END:                                     # an ordinary end on exactly the limit-th step of an episode
        exact = sum(int(l == mid and e == 1) for w in ws for l, e in zip(w["episode_len"], w["end"][w["end"] != 0]))
        assert exact >= 1, (name, mid)
    # launches of PIECE steps begin inside episodes, and a cut falls on a launch's last step or its first
    cuts = np.concatenate([np.flatnonzero(w["end"] == 2) for w in ws])
    assert len(cuts) and c["steps"] % PIECE != 0
    if len(c["limits"]) > 1:
        big = c["limits"][-1]
        free, zero = case_walks(name, big), case_walks(name, 0)
        assert not any((w["end"] == 2).any() for w in free), (name, "the largest limit cuts an episode")
        for a, b in zip(free, zero):                          # ... and changes nothing
            for key in a:
                assert np.array_equal(a[key], b[key]), (name, key)
        assert c["limits"][:2] == (1, 2)
        one = case_walks(name, 1)                             # limit 1: every step ends an episode
        assert all((w["done"] == 1).all() and w["episodes"] == c["steps"] for w in one)


def test_walk_without_limit_is_run_trace():
    """The limited walk with the limit off is oracle/trace.py's run_trace, field for field."""
    from oracle import ffi
    from oracle.trace import run_trace
    c = CASES["fast"]
    seed = c["seeds"][0]
    o = ffi.load("bo").env(c["dist"]); o.seed(seed)
    want = run_trace(o, K, c["steps"], "hash", agent_seed=seed - 2993)
    got = limited_walk(c["dist"], seed, seed - 2993, 0, c["steps"])
    for key in ("action", "reward", "nP", "nG", "done", "obs_hash", "pairs_hash", "newpoly_hash", "final_pairs", "final_order", "final_basis", "final_obs"):
        assert np.array_equal(got[key], want[key]), key


def test_rule_and_t_lim_arithmetic(tmp_path):
    exe = str(tmp_path / "episode_limit_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "episode_limit_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    rep = {ln.split()[0]: (int(ln.split()[2]), int(ln.split()[4])) for ln in p.stdout.splitlines() if " cases " in ln}
    assert set(rep) == {"end", "walk", "off"}, p.stdout[-3000:]
    for name, (cases, failures) in rep.items():
        assert cases > 1000 and failures == 0, (name, cases, failures)


def test_abi():
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    for name, proto in (("bbx_episode_limit", (C.c_int, [C.c_void_p, C.c_int])), ("bbx_episode_counts", (C.c_int, [C.c_void_p] * 3))):
        assert hasattr(lib, name) and _ffi.SIGNATURES[name] == proto, name
    assert lib.bbx_episode_limit(None, 3) == -1 and b"null argument" in lib.bbx_last_error()
    assert lib.bbx_episode_limit(None, -1) == -1 and b">= 0" in lib.bbx_last_error()      # a negative limit is refused
    assert lib.bbx_episode_counts(None, None, None) == -1
    text = open(os.path.join(ROOT, "include", "bbx.h")).read()
    assert "int bbx_episode_limit(bbx_batch* b, int limit);" in text and "int bbx_episode_counts(bbx_batch* b, int64_t* episodes, int64_t* truncations);" in text


def test_header_stays_128_bytes(tmp_path):
    """sizeof(BbxHdr) == 128 with the truncation counter in what was reserved, and the counter sits where reserved[0] was."""
    src = tmp_path / "hdr.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "bbx_common.h"\n'
                   'int main() { printf("%zu %zu %zu\\n", sizeof(BbxHdr), offsetof(BbxHdr, truncations), offsetof(BbxHdr, episode_steps)); return 0; }\n')
    exe = str(tmp_path / "hdr")
    subprocess.check_call(["g++", "-std=c++17", "-Wno-invalid-offsetof", "-I", CSRC, str(src), "-o", exe])
    assert subprocess.check_output([exe], text=True).split() == ["128", "116", "28"]
