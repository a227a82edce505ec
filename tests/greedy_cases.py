"""What the greedy-policy tests share (tests/test_greedy_cpu.py, tests/test_greedy_gpu.py): the parity cases of the *_act_greedy
kernels against the float64 reference of tests/policy_cases.py, and a scalar restatement of bbx_episodes_device.  Plain numpy,
importable without a GPU.

A greedy pick `a` of a state with reference logits z and tolerance tol (Ref.tol(): the project's C_L bound on a logit's fp32
error) passes iff  z[a] >= max_r z[r] - 2 tol: a kernel whose logits are each within tol of the reference cannot put a row that
is more than 2 tol behind in front.  A state in which exactly ONE row passes is decided: there the pick must be the reference
argmax.  The share of decided states is what keeps the check from being vacuous (SHARE_MIN)."""
import functools

import numpy as np

from tests import policy_cases as pc

B, R = 96, 70
LIVE = (1, 2, 63, 64, 65, 70)                              # both sides of the lane stride of 64
SEEDS = (7, 8)
SHAPES = [(12, (128,)), (64, (256,)), (12, (64, 64)), (20, (128, 128)), (12, (64, 64, 64))]
LOGPROB_SHAPES = [s for s in SHAPES if len(s[1]) <= 2]     # the depths that have a log-probability kernel
SHARE_MIN = {1: 0.9, 2: 0.9, 3: 0.7}                       # per depth: decided states among all


class ParityCase:
    def __init__(self, cols, hidden, seed):
        # three layers of 64 at 0.3 x default init score every row nearly alike: the larger scale separates them
        self.weights = pc.make_weights(cols, hidden, seed, scale=0.5 if len(hidden) == 3 else 0.3)
        self.rows = np.resize(np.array(LIVE, dtype=np.int32), B)
        self.obs = pc.fill_padding(pc.random_blocks(B, R, cols, seed + 1), self.rows, False)
        self.ref = pc.reference(self.weights, self.obs, self.rows)
        lg = np.where(np.isnan(self.ref.logits), -np.inf, self.ref.logits)
        self.passing = lg >= (lg.max(axis=1) - 2.0 * self.ref.tol())[:, None]          # [B, R]: rows a pick may be
        self.decided = self.passing.sum(axis=1) == 1
        self.argmax = lg.argmax(axis=1)
        self.share = float(self.decided.mean())


@functools.lru_cache(maxsize=None)
def parity_case(cols, hidden, seed):
    """Computed once per process, shared by the tests that need it, never modified."""
    return ParityCase(cols, hidden, seed)


def episodes_scalar(rewards, dones, carry_return=None, carry_len=None, count=None):
    """bbx_episodes_device restated one environment and one step at a time in IEEE double: returns (ep_return, ep_len,
    carry_return, carry_len, count) as new arrays."""
    T, nb = rewards.shape
    ep_ret = np.zeros((T, nb)); ep_len = np.zeros((T, nb), dtype=np.int32)
    cr = np.zeros(nb) if carry_return is None else np.array(carry_return, dtype=np.float64)
    cl = np.zeros(nb, dtype=np.int32) if carry_len is None else np.array(carry_len, dtype=np.int32)
    cn = np.zeros(nb, dtype=np.int32) if count is None else np.array(count, dtype=np.int32)
    for b in range(nb):
        acc, ln = np.float64(cr[b]), int(cl[b])
        for t in range(T):
            acc = acc + np.float64(rewards[t, b]); ln += 1
            if dones[t, b]:
                ep_ret[t, b] = acc; ep_len[t, b] = ln; cn[b] += 1
                acc, ln = np.float64(0.0), 0
        cr[b] = acc; cl[b] = ln
    return ep_ret, ep_len, cr, cl, cn


def random_episode_block(T, nb, seed, p_done=0.15):
    rng = np.random.default_rng(seed)
    r = -(rng.integers(1, 400, size=(T, nb)).astype(np.float64) + rng.random((T, nb)))   # (fractions: the order of the adds shows)
    d = rng.random((T, nb)) < p_done
    return r, d
