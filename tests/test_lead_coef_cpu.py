"""The fast class reads 1/LC of every new basis element from the GF(32003) inverse table without asking whether LC is 1
(add_poly in bbx_fast.h: the read is issued with no control flow around it and waited for where the inverse is used).  So the
table's entry 1 must be 1, and the one input that takes another path than before is a new element whose lead coefficient is 1.
This file asserts, without a device, the table's contents and that the seeds tests/test_lead_coef_gpu.py runs really insert
such elements — and elements with lead coefficient -1 = 32002, the other end of the table — which a later step then uses
(found by a search over ideal seeds 5000..9999 with agent seed = ideal seed - 4000, fixed here)."""
import ctypes as C
import functools

import numpy as np

import __graft_entry__ as graft
from tests import oracle_walk as ow

DIST, K, T, P = "3-20-10-weighted", 2, 128, 32003
# (ideal seed, agent seed): an element with the lead coefficient named enters the basis within T steps and is later a member
# of a selected pair of the same episode
LC_ONE = ((5781, 1781), (6048, 2048), (6549, 2549), (6960, 2960))
LC_MINUS_ONE = ((7694, 3694), (8077, 4077), (8711, 4711), (9694, 5694))
SEEDS = LC_ONE + LC_MINUS_ONE


class Insertions:
    """walk()'s observer: the elements the current episode has inserted (live, by basis index), moved to `inserted` when
    the episode ends — the after hook sees o.nP == 0 before the reset — and by flush() behind the last step."""

    def __init__(self):
        self.inserted, self.live = [], {}

    def before(self, o, t, action):
        for g in o.pairs()[action]:
            if int(g) in self.live and self.live[int(g)][3] is None:
                self.live[int(g)][3] = t
        self.nG0 = o.nG

    def after(self, o, t, action, reward):
        if o.nG > self.nG0:
            self.live[self.nG0] = [t, self.nG0, int(o.poly(self.nG0)[0][0]), None]
        if o.nP == 0:
            self.flush()

    def flush(self):
        self.inserted += [tuple(v) for v in self.live.values()]
        self.live = {}


@functools.lru_cache(maxsize=None)
def walk(seed, aseed, nsteps=T):
    """T steps of the hash agent with auto-reset on the oracle: (the environment as it stands afterwards, per-step rewards and
    done flags, the insertions as (step, basis index, lead coefficient, step of its first later selection in the episode or None))."""
    seen = Insertions()
    o, rewards, dones, _ = ow.walk(DIST, seed, aseed, nsteps, seen)
    seen.flush()
    return o, rewards, dones, seen.inserted


def test_inverse_table_of_the_host():
    graft.build()
    from deepgroebner_amd import _ffi
    tab = np.zeros(P, dtype=np.uint16)
    _ffi.lib().bbx_internal_inv_table(tab.ctypes.data_as(C.c_void_p))
    assert tab[1] == 1 and tab[0] == 0
    c = np.arange(1, P, dtype=np.int64)
    assert ((tab[1:].astype(np.int64) * c) % P == 1).all()
    assert tab[P - 1] == P - 1


def test_seeds_insert_the_lead_coefficients_and_use_the_elements():
    assert len(SEEDS) == len(set(SEEDS)) == 8
    for want, group in ((1, LC_ONE), (P - 1, LC_MINUS_ONE)):
        assert len(group) >= 4
        for seed, aseed in group:
            ins = walk(seed, aseed)[3]
            used = [v for v in ins if v[2] == want and v[3] is not None]
            assert used, (seed, aseed, want)
            assert all(v[0] < v[3] < T for v in used)
    # the batch as a whole is ordinary otherwise: most insertions have other lead coefficients, episodes end inside the run
    every = [v for s in SEEDS for v in walk(*s)[3]]
    assert sum(v[2] not in (1, P - 1) for v in every) > 10 * len(SEEDS)
    assert sum(walk(*s)[2].sum() for s in SEEDS) >= len(SEEDS)
