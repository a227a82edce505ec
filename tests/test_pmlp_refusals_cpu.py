"""What the PMLP training calls refuse, and which refusal wins when two apply: the 24 entry points
{bbx_pmlp, bbx_pmlp2} x {logprob, grad, ppo_grad, value, value_grad, value_fit} x {plain, _at} and the 8 workspace queries of
include/bbx.h.  Refused calls only: no case reaches a launcher, so nothing here needs a device — every non-null pointer is the
address of one small host buffer, which a refused call never reads.

The faults, by class:
  shape   cols 0 and 65; hidden 0 and 257 (one layer); hidden1 / hidden2 0 and 129 (two layers)
  rows    obs_rows 2049 (BBX_POLICY_MAX_ROWS + 1)
  bad     obs_rows 0, n -1
  index   n_src -1, a null index with n > 0 (the _at forms)
  null    each required pointer null, one at a time (bbx_pmlp[2]_value: both value outputs)
  pool    pool -1 and 3
  ppo     mode -1 and 3, eps -1 and NaN
  epi     the epilogue's arrays: d_old_logprobs, d_advantages, d_coef, d_stats (PPO); d_targets, d_coef, d_stats (fit)
          (bbx_pmlp2_value_fit[_at] accepts a null d_stats — no statistics wanted —, so it is no fault there)
Each fault alone, and every pair of faults of two different classes that do not set the same argument.

The expected return code and message of every case are tests/golden/pmlp_refusals.json, written by running this file as a
program (python tests/test_pmlp_refusals_cpu.py) against a build of the commit before the calls were given one body for both
depths; the program refuses to write a table in which a case is not a refusal."""
import ctypes as C
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pmlp_refusals.json")
BBX_E_ARG, BBX_E_UNSUPPORTED = -1, -5
FAMILIES = ("logprob", "grad", "ppo_grad", "value", "value_grad", "value_fit")
POLICY = ("logprob", "grad", "ppo_grad")


def _params(two, family, at):
    """The parameter names of an entry point, in the order of include/bbx.h."""
    p = ["d_obs", "d_rows"] + (["d_actions"] if family in POLICY else []) + (["n_src", "d_index"] if at else [])
    p += ["n", "obs_rows", "cols", "d_prepared"] + (["hidden1", "hidden2"] if two else ["hidden"])
    grads = ["d_workspace", "d_gw1", "d_gb1", "d_gw2", "d_gb2"] + (["d_gw3", "d_gb3"] if two else [])
    p += {"logprob": ["d_logprobs", "d_entropy"],
          "grad": ["d_glogp", "d_gent"] + grads,
          "ppo_grad": ["d_old_logprobs", "d_advantages", "mode", "scale", "eps", "ent_coef", "c_kl", "d_logprobs", "d_entropy", "d_coef",
                       "d_stats"] + grads,
          "value": ["pool", "d_values", "d_values64"],
          "value_grad": ["pool", "d_gvalue"] + grads,
          "value_fit": ["pool", "d_targets", "scale", "d_values", "d_coef", "d_stats"] + grads}[family]
    return p + ["stream"]


def _faults(two, family, at, query=False):
    """[(class, label, {argument: value})] of an entry point (query: of a workspace query)."""
    f = [("shape", "cols=0", {"cols": 0}), ("shape", "cols=65", {"cols": 65})]
    for name, over in ((("hidden1", 129), ("hidden2", 129)) if two else (("hidden", 257),)):
        f += [("shape", "%s=0" % name, {name: 0}), ("shape", "%s=%d" % (name, over), {name: over})]
    f += [("rows", "obs_rows=2049", {"obs_rows": 2049}), ("bad", "obs_rows=0", {"obs_rows": 0}), ("bad", "n=-1", {"n": -1})]
    if query:
        return f
    if at:
        f += [("index", "n_src=-1", {"n_src": -1}), ("index", "d_index=null", {"d_index": None})]
    grads = ["d_workspace", "d_gw1", "d_gb1", "d_gw2", "d_gb2"] + (["d_gw3", "d_gb3"] if two else [])
    required = ["d_obs", "d_rows"] + (["d_actions"] if family in POLICY else []) + ["d_prepared"]
    required += {"logprob": ["d_logprobs"], "grad": ["d_glogp"] + grads, "ppo_grad": grads, "value": [], "value_grad": ["d_gvalue"] + grads,
                 "value_fit": grads}[family]
    f += [("null", "%s=null" % a, {a: None}) for a in required]
    if family == "value":
        f += [("null", "d_values=d_values64=null", {"d_values": None, "d_values64": None})]
    if family in ("value", "value_grad", "value_fit"):
        f += [("pool", "pool=-1", {"pool": -1}), ("pool", "pool=3", {"pool": 3})]
    if family == "ppo_grad":
        f += [("ppo", "mode=-1", {"mode": -1}), ("ppo", "mode=3", {"mode": 3}), ("ppo", "eps=-1", {"eps": -1.0}), ("ppo", "eps=nan", {"eps": float("nan")})]
        f += [("epi", "%s=null" % a, {a: None}) for a in ("d_old_logprobs", "d_advantages", "d_coef", "d_stats")]
    if family == "value_fit":
        f += [("epi", "%s=null" % a, {a: None}) for a in ("d_targets", "d_coef") + (() if two else ("d_stats",))]
    return f


def _calls():
    """{entry point: (parameter names, faults)}: the 24 training calls and the 8 workspace queries."""
    out = {}
    for two in (False, True):
        stem = "bbx_pmlp2_" if two else "bbx_pmlp_"
        for family in FAMILIES:
            for at in (False, True):
                out[stem + family + ("_at" if at else "")] = (_params(two, family, at), _faults(two, family, at))
        for q in ("grad", "ppo", "value_grad", "value_fit"):
            out[stem + q + "_workspace_floats"] = (["n", "obs_rows", "cols"] + (["hidden1", "hidden2"] if two else ["hidden"]),
                                                  _faults(two, None, False, query=True))
    return out


CALLS = _calls()
_HOST = (C.c_double * 64)()                                 # what every non-null pointer points to: a refused call reads none of it
VALID = {"n": 3, "n_src": 3, "obs_rows": 2, "cols": 6, "hidden": 33, "hidden1": 8, "hidden2": 8, "pool": 0, "mode": 1, "scale": 1.0,
         "eps": 0.2, "ent_coef": 0.01, "c_kl": 1.0, "stream": None}


def _cases(faults):
    """[(label, {argument: value})]: every fault alone, then every pair of two classes on different arguments."""
    out = [(label, dict(args)) for _, label, args in faults]
    for i, (ci, li, ai) in enumerate(faults):
        for cj, lj, aj in faults[i + 1:]:
            if ci != cj and not set(ai) & set(aj):
                out.append((li + " + " + lj, {**ai, **aj}))
    return out


def _outcomes(ffi, name):
    """{case label: [return code, message]} of one entry point."""
    dll = ffi.lib()
    fn = getattr(dll, name)
    params, faults = CALLS[name]
    assert len(params) == len(ffi.SIGNATURES[name][1]), name
    for p, t in zip(params, ffi.SIGNATURES[name][1]):
        assert (p.startswith("d_") or p == "stream") == (t is C.c_void_p), (name, p)
    got = {}
    for label, changed in _cases(faults):
        args = [changed[p] if p in changed else VALID[p] if p in VALID else C.addressof(_HOST) for p in params]
        rc = fn(*args)
        got[label] = [rc, dll.bbx_last_error().decode()]
    return got


@pytest.fixture(scope="module")
def ffi_():
    import __graft_entry__ as graft
    graft.build()
    from deepgroebner_amd import _ffi
    return _ffi


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _refused(rc, msg):
    return rc in (BBX_E_ARG, BBX_E_UNSUPPORTED) and msg and "launch failed" not in msg and "LDS" not in msg


def _unpack(golden, name):
    return {label: golden["outcomes"][i] for label, i in zip(golden["calls"][name]["cases"], golden["calls"][name]["outcome"])}


def test_the_table_covers_every_call_and_case(golden):
    assert len(CALLS) == 32 and sorted(golden["calls"]) == sorted(CALLS)
    for name, (_, faults) in CALLS.items():
        assert golden["calls"][name]["cases"] == [label for label, _ in _cases(faults)], name
        assert len(golden["calls"][name]["outcome"]) == len(golden["calls"][name]["cases"]), name
    for rc, msg in golden["outcomes"]:
        assert _refused(rc, msg), (rc, msg)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_refusals_and_their_precedence(ffi_, golden, name):
    want = _unpack(golden, name)
    got = _outcomes(ffi_, name)
    assert sorted(got) == sorted(want)
    wrong = []
    for label, (rc, msg) in got.items():
        assert _refused(rc, msg), "%s(%s) was not refused: %d %r" % (name, label, rc, msg)
        if [rc, msg] != want[label]:
            wrong.append("%s(%s): %d %r, expected %d %r" % (name, label, rc, msg, want[label][0], want[label][1]))
    assert not wrong, "%d of %d cases differ:\n%s" % (len(wrong), len(got), "\n".join(wrong[:20]))


if __name__ == "__main__":                                  # write the table from the library this tree has built
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from deepgroebner_amd import _ffi
    outcomes, calls = [], {}
    for name_ in sorted(CALLS):
        res = _outcomes(_ffi, name_)
        for label_, (rc_, msg_) in res.items():
            if not _refused(rc_, msg_):
                sys.exit("%s(%s) is no refusal: %d %r" % (name_, label_, rc_, msg_))
            if [rc_, msg_] not in outcomes:
                outcomes.append([rc_, msg_])
        calls[name_] = {"cases": list(res), "outcome": [outcomes.index(v) for v in res.values()]}
    with open(GOLDEN, "w") as f_:
        json.dump({"outcomes": outcomes, "calls": calls}, f_, separators=(",", ":"))
        f_.write("\n")
    print("%d calls, %d cases, %d distinct outcomes -> %s" % (len(calls), sum(len(c["cases"]) for c in calls.values()), len(outcomes), GOLDEN))
