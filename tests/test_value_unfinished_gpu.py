"""The synchronous value calls' side of the protocol all value calls share for a clone that did not finish:
the word pair the collect folds, read by one classifier.  Hard limits: the error names an environment — one the asynchronous
form leaves NaN, never a clone index.  Growth: bbx_values, bbx_values_device and bbx_action_values enlarge the records of
equal handles alike and return what a handle with room to spare returns."""
import re

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import action_value_cases as A
from tests import test_values_device as VD
from tests.fast_harness import same_doubles, stream

pytestmark = pytest.mark.gpu

DIST, B, SEED = "3-20-10-weighted", 64, 500
HARD = {"max_basis": 48, "max_pairs": 128, "lds_max_basis": -1}       # (test_value_rollouts_that_outgrow_hard_limits_are_an_error_and_nan)
# every Degree rollout from these states fits 80 basis elements, some seeded Random rollouts of "sample" do not (the test asserts both)
SAMPLE_HARD = {"max_basis": 80, "max_pairs": 4096, "lds_max_basis": -1}


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def _named(err):
    from deepgroebner_amd import _ffi
    assert isinstance(err, _ffi.BbxError) and err.code == -3, err
    m = re.search(r"environment (\d+)", str(err))
    assert m, str(err)
    return int(m.group(1))


@pytest.fixture(scope="module")
def hard():
    """(a no_growth handle, what values_device("degree") leaves on a copy of it, the entries of that which are NaN)."""
    import torch
    from deepgroebner_amd import _ffi
    ref = VD._make(DIST, B, HARD, seed=SEED, walk=0)
    ref.values("degree", 0.99)
    assert ref.capacities()["grown"] > 0                           # some rollout outgrows these capacities
    env = VD._make(DIST, B, dict(HARD, no_growth=1), seed=SEED, walk=0)
    twin = env.copy()
    out = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    twin.values_device(out, "degree", 0.99, None, stream())
    with pytest.raises(_ffi.BbxError):
        twin.sync()
    got = out.cpu().numpy()
    nan = np.flatnonzero(np.isnan(got))
    assert 0 < len(nan) < B
    return env, got, nan


def test_hard_limits_name_an_environment_the_asynchronous_form_leaves_nan(hard):
    from deepgroebner_amd import _ffi
    env, device_values, nan = hard
    before = (env.capacities(), env.stats().copy(), env.observations(VD.OBS_ROWS).copy())
    seen = []
    for _ in range(2):                                             # (the handle stays usable: the same error again)
        with pytest.raises(_ffi.BbxError) as ei:
            env.values("degree", 0.99)
        named = _named(ei.value)
        print("values('degree') under hard limits:", str(ei.value), "| NaN entries of values_device:", nan.tolist())
        assert 0 <= named < B and named in nan
        seen.append((ei.value.code, str(ei.value)))
    assert seen[0] == seen[1]
    assert env.capacities() == before[0] and np.array_equal(env.stats(), before[1]) and np.array_equal(env.observations(VD.OBS_ROWS), before[2])
    # one environment alone is clone 0 of its call: the message still names the environment
    e = int(nan[-1])
    with pytest.raises(_ffi.BbxError) as ei:
        env.value(e, "degree", 0.99)
    assert _named(ei.value) == e, str(ei.value)
    # usable afterwards: rollouts that fit are not reported as unfinished by what the failed calls left behind
    for e_ok in np.flatnonzero(~np.isnan(device_values))[[0, -1]]:
        assert env.value(int(e_ok), "degree", 0.99) == device_values[e_ok], e_ok


def test_hard_limits_under_sample_on_the_same_handle(hard):
    """(here the Degree pass in front of the 100 Random rollouts per environment already fails: the next test reaches those)"""
    from deepgroebner_amd import _ffi
    env = hard[0]
    with pytest.raises(_ffi.BbxError) as ei:
        env.values("sample", 0.99, seeds=np.random.default_rng(5).integers(0, 2 ** 31 - 1, size=(B, 100)))
    assert 0 <= _named(ei.value) < B


def test_hard_limits_under_sample_name_an_environment_never_a_clone():
    """The failure comes from the pass of 100 clones per environment: the Degree pass in front of it succeeds.  Clone
    100 k + i runs Random from seeds[k][i], as values("random", seeds[:, i]) runs environment k (one clone per environment,
    the mapping the test above checks): the environment "sample" names is the largest any of the 100 columns names."""
    from deepgroebner_amd import _ffi
    env = VD._make(DIST, B, dict(SAMPLE_HARD, no_growth=1), seed=SEED, walk=0)
    want_degree = env.values("degree", 0.99)                       # the Degree rollouts fit
    seeds = np.random.default_rng(5).integers(0, 2 ** 31 - 1, size=(B, 100))
    with pytest.raises(_ffi.BbxError) as ei:
        env.values("sample", 0.99, seeds=seeds)
    named = _named(ei.value)
    by_column = []
    for i in range(100):
        try:
            env.values("random", 0.99, seeds=seeds[:, i])
        except _ffi.BbxError as e:
            by_column.append(_named(e))
    print("values('sample') under hard limits:", str(ei.value), "|", len(by_column), "of 100 columns fail, naming", sorted(set(by_column)))
    assert by_column and 0 <= named < B and named == max(by_column)
    assert np.array_equal(env.values("degree", 0.99), want_degree)  # usable afterwards, and a shorter call reads its own word


@pytest.mark.parametrize("caps", VD.GROWTH)
def test_all_three_calls_enlarge_the_records_and_return_what_room_to_spare_returns(caps):
    import torch
    ref = VD._make(DIST, B, dict(caps, max_basis=0, max_pairs=0), seed=SEED, walk=0)   # (0: the default capacities)
    tight = [VD._make(DIST, B, caps, seed=SEED, walk=0)]
    tight += [tight[0].copy(), tight[0].copy()]
    before = tight[0].capacities()
    assert ref.capacities()["max_basis"] > before["max_basis"] and np.array_equal(ref.rows, tight[0].rows)
    R = int(ref.rows.max())
    want = ref.values("normal", 0.99)
    want_q = A.twin_action_values(ref, "normal", 0.99, R)
    assert ref.capacities()["grown"] == 0 and not np.isnan(want).any()

    got_sync = tight[0].values("normal", 0.99)
    out = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    tight[1].values_device(out, "normal", 0.99, None, stream())
    tight[1].sync()
    got_q = A.call(tight[2], "normal", 0.99, R)
    after = [t.capacities() for t in tight]
    print("capacities", before, "->", after)
    assert all(a["grown"] > before["grown"] for a in after)        # every form outgrew these capacities: none passes by not growing
    assert same_doubles(got_sync, want) and same_doubles(out.cpu().numpy(), want)
    assert after[0] == after[1]
    assert got_q[0] == 0 and np.array_equal(got_q[4], want_q[3])
    assert A.same_block(got_q[1], want_q[0]) and A.same_block(got_q[2], want_q[1]) and np.array_equal(got_q[3], want_q[2])
