"""The headline shape through rollout_device on the seeds of tests/test_pair_compaction_cpu.py: every seed shows a situation
the two-part compaction of an insertion must get right (the first 64 old pairs from the register copy without a loop, the
rest from LDS): dropped pairs in front of the next selection, new pairs behind the survivors, nothing appended, lists beyond
64 pairs, across 64 and back.  Persistent sessions and one kernel per launch; rewards, dones, rows, the observation block,
final states and counters against the oracle, exactly — and once more with the class capped at 16 basis elements, where
environments leave for the HBM-resident pass at the capacity test in front of a step."""
import pytest

from tests.test_pair_compaction_cpu import all_seeds
from tests.test_step_prefetch_cpu import LEAVE_CAP
from tests.test_step_prefetch_gpu import _run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("persistent", [True, False], ids=["session", "launches"])
def test_case_seeds_chained_launches(persistent):
    """Launches of 1, 2, 63, 64, 65 and 125 steps; in a session the calls are queued behind each other, with joins behind
    calls 2 and 4."""
    env = _run(all_seeds(), None, persistent, joins=(2, 4))
    if persistent:
        assert env.session_stats()["sessions"] >= 1, env.session_stats()


@pytest.mark.parametrize("persistent", [True, False], ids=["session", "launches"])
def test_case_seeds_leaving_the_class(persistent):
    """caps={"lds_max_basis": 16}: an environment leaves at the capacity test in front of a step; the HBM-resident pass
    continues from the record the class wrote back, so any difference shows in what is compared."""
    _run(all_seeds(), {"lds_max_basis": LEAVE_CAP}, persistent, joins=(2, 4))
