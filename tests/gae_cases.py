"""Cases and an exact reference for the bootstrapped GAE scan (bbx_gae_bootstrap_device, DeviceTrajectoryBuffer.finish() with
last_values), shared by test_gae_bootstrap_cpu.py and test_gae_bootstrap_gpu.py.

The definition, per environment e, scanning t = T - 1 .. 0:

    start      nret = nval = last[e], nadv = 0, complete      (last given)
               nret = nval = nadv = 0, not complete           (last None)
    step t     done[t]: nret = nval = nadv = 0, complete
               ret[t] = r[t] + gam nret
               adv[t] = r[t] - v[t] + gam nval + gam lam nadv
               lam_ret[t] = adv[t] + v[t]
               nret, nadv, nval = ret[t], adv[t], v[t]

reference() evaluates it in fractions.Fraction: no rounding anywhere (gam, lam and the inputs are taken as the doubles they are).
An entry of `last` behind a done last step is never read, whatever it holds.

Two kinds of case:
    exact_case    rewards integers in [-8, -1], values and last values multiples of 1/4 in [-16, 0], gam = lam = 1/2, T <= 20:
                  every intermediate of the scan is a multiple of 2^-41 (adv gains two binary places per step from 1/8) below 2^6
                  in magnitude (|delta| <= 24, |adv| <= 24 / (1 - 1/4)) — 47 bits — so every operation is exact in double, in whatever order the products and sums are rounded, and kernel and torch loop must equal the
                  reference with ==.
    general_case  the doubles of _filled_buffer in test_values_device.py (rewards -U{0..399} * U[0, 1), values -300 U[0, 1), done
                  with probability 0.06 and at the first and the last step), plus last values -300 U[0, 1)."""
import collections
from fractions import Fraction

import numpy as np

Case = collections.namedtuple("Case", ["rewards", "values", "dones", "last", "gam", "lam"])


def exact_case(T, B, p_done, seed):
    assert T <= 20
    rng = np.random.default_rng(seed)
    r = -rng.integers(1, 9, size=(T, B)).astype(np.float64)
    v = -rng.integers(0, 65, size=(T, B)) / 4.0
    last = -rng.integers(0, 65, size=B) / 4.0
    d = rng.random((T, B)) < p_done
    return Case(r, v, d, last, 0.5, 0.5)


def general_case(T, B, seed):
    rng = np.random.default_rng(seed)
    d = rng.random((T, B)) < 0.06
    d[0, 0] = True; d[T - 1, B - 1] = True
    r = -rng.integers(0, 400, size=(T, B)) * rng.random((T, B))
    v = -rng.random((T, B)) * 300.0
    last = -rng.random(B) * 300.0
    return Case(r, v, d, last, 0.99, 0.97)


def reference(case, bootstrap=True):
    """(ret, adv, lam_ret) as [T][B] nested lists of Fraction, complete as a bool array."""
    r, v, d = case.rewards, case.values, case.dones
    T, B = r.shape
    g, l = Fraction(case.gam), Fraction(case.lam)
    ret = [[None] * B for _ in range(T)]; adv = [[None] * B for _ in range(T)]; lret = [[None] * B for _ in range(T)]
    comp = np.zeros((T, B), dtype=bool)
    for e in range(B):
        nret = nadv = nval = Fraction(0)
        c = bool(bootstrap)
        if bootstrap and not d[T - 1, e]:                    # (behind a done flag the entry is never read)
            nret = nval = Fraction(float(case.last[e]))
        for t in range(T - 1, -1, -1):
            if d[t, e]:
                nret = nadv = nval = Fraction(0)
                c = True
            rr, vv = Fraction(float(r[t, e])), Fraction(float(v[t, e]))
            ret[t][e] = rr + g * nret
            adv[t][e] = rr - vv + g * nval + g * l * nadv
            lret[t][e] = adv[t][e] + vv
            comp[t, e] = c
            nret, nadv, nval = ret[t][e], adv[t][e], vv
    return ret, adv, lret, comp


def equals_exactly(got, want):
    """A float64 [T, B] array against nested Fractions, with == (Fraction(x) of a double is exact; NaN equals nothing)."""
    got = np.asarray(got)
    return all(Fraction(float(got[t, e])) == want[t][e] if np.isfinite(got[t, e]) else False
               for t in range(got.shape[0]) for e in range(got.shape[1]))


def worst_error(got, want, scale):
    """max over entries of |got - want| / scale[e], in exact arithmetic until the last division."""
    got = np.asarray(got)
    worst = 0.0
    for t in range(got.shape[0]):
        for e in range(got.shape[1]):
            if not np.isfinite(got[t, e]):
                return float("inf")
            worst = max(worst, float(abs(Fraction(float(got[t, e])) - want[t][e]) / Fraction(float(scale[e]))))
    return worst


def scale_of(case):
    """S per environment: sum |r| + 2 max |v| + |last| — what bounds every quantity the scan rounds."""
    return np.abs(case.rewards).sum(axis=0) + 2.0 * np.abs(case.values).max(axis=0) + np.abs(case.last)


def fill(buf, case, seed=0, bootstrap=True):
    """The case in a DeviceTrajectoryBuffer of its shape (on whatever device the buffer is), with rows in [1, 8], actions and
    log-probabilities from `seed`; last_values set (bootstrap) or None."""
    import torch
    T, B = case.rewards.shape
    rng = np.random.default_rng(seed)
    dev = buf.rewards.device
    buf.rewards.copy_(torch.from_numpy(case.rewards)); buf.values.copy_(torch.from_numpy(case.values))
    buf.dones.copy_(torch.from_numpy(case.dones))
    buf.rows.copy_(torch.from_numpy(rng.integers(1, 9, size=(T, B)).astype(np.int32)))
    buf.actions.copy_(torch.from_numpy(rng.integers(0, 9, size=(T, B)).astype(np.int32)))
    buf.logprobs.copy_(torch.from_numpy(-rng.random((T, B)).astype(np.float32)))
    buf.t = T
    buf.last_values = torch.from_numpy(case.last.copy()).to(dev) if bootstrap else None
    buf.returns = buf.advantages = buf.complete = buf.lambda_returns = None
    return buf


def new_buffer(case, device, **kw):
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer
    T, B = case.rewards.shape
    return fill(DeviceTrajectoryBuffer(T, B, gam=case.gam, lam=case.lam, device=device), case, **kw)
