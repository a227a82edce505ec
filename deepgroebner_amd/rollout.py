"""The consumer side of the batched environment: trajectory buffer, rollout loops and update loops, all on the
device, replacing the per-step host round trip of the reference's agents.  The policy and the critic they drive (PMLPPolicy,
PMLPValue) and the kernel calls behind them are deepgroebner_amd.pmlp's; both names are importable from here as well.

    discount_rewards, compute_advantages                              pg.py:20-76
    DeviceTrajectoryBuffer     TrajectoryBuffer (store/finish/get)    pg.py:79-240
    get_index + PMLPPolicy.evaluate_at   the update's minibatches as slices of an index list over the buffer: the training
                               kernels read the recorded states where the rollout left them (bbx_pmlp_logprob_at / bbx_pmlp_grad_at)
    ppo_update                 the epochs of the policy update around PMLPPolicy.ppo_step_at          pg.py _fit_policy_model
    action_value_targets, imitation_update   imitation: env.action_values() as target rows (DeviceTrajectoryBuffer(targets=True)), the epochs
                               of cross-entropy minibatches around PMLPPolicy.xent_step_at over every stored state
    fill_values, value_update  a learned baseline (--value_model mlp, pg.py _fit_value_model): one launch for a whole buffer's values
                               after the rollout (PMLPValue.values), the epochs of the squared-error fit around PMLPValue.fit_step_at;
                               run_rollout_fused(critic=...)
    run_rollout                PGAgent.run_episode(s)                 pg.py:451-503   (one library call per vector step)
    run_rollout_fused          the same with the policy INSIDE the step kernel, 256 vector steps per launch
    run_rollout(value_strategy=...)   env.value(strategy, gamma) before every step as the baseline   pg.py:461-465
                               (bbx_values_device: written on the device beside the steps); finish(): one GAE kernel
    run_rollout / run_rollout_fused (bootstrap=True)   buffer.last_values: the value of the state the rollout stops in, where finish()
                               starts its scan (bbx_gae_bootstrap_device) — episodes the buffer's end cuts are kept, not dropped
    act / run_rollout / run_rollout_fused (greedy=True)   the highest-probability pair at every step   pg.py run_episodes(greedy=True)
    episode_returns            one return and one length per episode from a rollout's rewards and dones (bbx_episodes_device)
    evaluate_policy            the first K episodes of every environment under a policy   scripts/eval.py

PyTorch is the plumbing here (device memory, autograd for training); the policy evaluation + sampling runs in hand-written
HIP (deepgroebner_amd.pmlp has which network takes which kernel), in front of the step in the same launch
(bbx_policy_step_device) or inside the step loop (bbx_policy_rollout_device, bbx_policy2_rollout_device) where the network
allows.  Actions never visit the host.
"""
import collections
import contextlib
import ctypes as C
import functools
import gc

import numpy as np
import torch

from . import _ffi
from .pmlp import PMLPPolicy, PMLPValue  # noqa: F401


@contextlib.contextmanager
def _gc_paused():
    """The step loops below enqueue a few kernels per iteration and must not fall behind the device: a generation-2 pass of
    Python's cyclic collector over a process that has torch loaded takes ~40 ms (measured: one in ~900 iterations, +40 us per
    vector step averaged over a 1000-step rollout), so collection is paused for the duration of a rollout."""
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def _with_gc_paused(fn):
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        with _gc_paused():
            return fn(*args, **kwargs)
    return wrapper


def discount_rewards(rewards, gam):
    """Discounted rewards-to-go (pg.py:20-47), float64."""
    out = np.zeros(len(rewards), dtype=np.float64)
    c = 0.0
    for i in reversed(range(len(rewards))):
        c = rewards[i] + gam * c
        out[i] = c
    return out


def compute_advantages(rewards, values, gam, lam):
    """Generalized advantage estimates of one complete trajectory (pg.py:50-76), float64."""
    rewards = np.array(rewards, dtype=np.float64)
    values = np.array(values, dtype=np.float64)
    delta = rewards - values
    delta[:-1] += gam * values[1:]
    return discount_rewards(delta, gam * lam)


class DeviceTrajectoryBuffer:
    """TrajectoryBuffer (pg.py:79-240) for a batch of environments stepping in lockstep, kept on the device: per step the
    -1-padded state block [B, R, cols] (optional), action, reward, log-probability, value and done flag of every
    environment.  finish() turns rewards into discounted rewards-to-go and values into GAE advantages per EPISODE
    (episodes end where done is set; an episode still running at the end of the buffer is incomplete and left out, like
    the reference's `[:self.start]`); get() returns the training tensors with the reference's filtering (states with a
    single row are dropped) and advantage normalisation.
    last_values (None, or float64 [B] on the buffer's device: the value of the state every environment was in BEHIND the last
    stored step; the rollout functions set it with bootstrap=True and clear it otherwise): finish() starts its scan there
    instead of at zero (truncated-horizon GAE), nothing is incomplete, and get() returns the steps of the cut episodes too.
    targets=True: the buffer also keeps `targets`, float32 [T, B, R] — a target distribution over the rows of every stored state,
    filled by store(..., target=) and trained towards by imitation_update; without it the buffer is what it was."""

    def __init__(self, nsteps, batch, gam=0.99, lam=0.97, obs_shape=None, device="cuda", targets=False):
        self.T, self.B, self.gam, self.lam = nsteps, batch, gam, lam
        if targets and not obs_shape:
            raise ValueError("DeviceTrajectoryBuffer: targets=True needs obs_shape=(rows, cols)")
        self.targets = torch.zeros((nsteps, batch, obs_shape[0]), dtype=torch.float32, device=device) if targets else None
        self.actions = torch.zeros((nsteps, batch), dtype=torch.int32, device=device)
        self.rewards = torch.zeros((nsteps, batch), dtype=torch.float64, device=device)
        self.logprobs = torch.zeros((nsteps, batch), dtype=torch.float32, device=device)
        self.values = torch.zeros((nsteps, batch), dtype=torch.float64, device=device)
        self.dones = torch.zeros((nsteps, batch), dtype=torch.bool, device=device)
        self.rows = torch.zeros((nsteps, batch), dtype=torch.int32, device=device)
        self.states = torch.empty((nsteps, batch) + tuple(obs_shape), dtype=torch.int32, device=device) if obs_shape else None
        self.t = 0
        self.last_values = None
        self.returns = self.advantages = self.complete = self.lambda_returns = None

    def store(self, state, rows, action, reward, logprob, value, done, target=None):
        t = self.t
        if self.states is not None:
            self.states[t].copy_(state)
        if target is not None:
            if self.targets is None:
                raise ValueError("store: the buffer keeps no targets (DeviceTrajectoryBuffer(..., targets=True))")
            self.targets[t].copy_(target)
        self.rows[t].copy_(rows); self.actions[t].copy_(action); self.rewards[t].copy_(reward)
        self.logprobs[t].copy_(logprob); self.dones[t].copy_(done.to(torch.bool))
        if value is not None:
            self.values[t].copy_(value)
        self.t += 1

    def fill_values(self, critic, t0=0, t1=None):
        """self.values[t0:t1] (t1 None: the steps stored so far) <- the critic's values of the stored states, float64: a learned
        baseline for GAE after a rollout that recorded none (run_rollout_fused).  On the device one bbx_pmlp_value call over the
        block in place (PMLPValue.values with out64); CPU buffers take the critic's torch path.  returns / advantages / complete /
        lambda_returns are cleared, so that the next get_index() finishes again.  A buffer that keeps no states: ValueError."""
        if self.states is None:
            raise ValueError("fill_values: the buffer keeps no states (DeviceTrajectoryBuffer(..., obs_shape=(rows, cols)))")
        t1 = self.t if t1 is None else t1
        if not 0 <= t0 <= t1 <= self.T:
            raise IndexError("fill_values: steps [%d, %d) of a buffer of %d" % (t0, t1, self.T))
        if t1 > t0:
            critic.values(self.states[t0:t1], self.rows[t0:t1], out64=self.values[t0:t1])
        self.returns = self.advantages = self.complete = self.lambda_returns = None

    def finish(self):
        """Reverse scan over time with episode boundaries: ret_t = r_t + gam ret_{t+1}; delta_t = r_t - v_t + gam v_{t+1};
        adv_t = delta_t + gam lam adv_{t+1}; nothing crosses a done flag (pg.py:20-76 per trajectory).  With self.last_values
        the scan starts from that value of the state behind the last step (ret = v = last_values, adv = 0) and every step is
        complete; an environment whose last step is done never reads its entry.  self.lambda_returns = adv + v, the TD(lambda)
        target of a value fit.  Tensors on the GPU: one kernel (bbx_gae_bootstrap_device, one thread per environment); on the
        CPU: the torch loop (_finish_torch), whose results the kernel reproduces bit for bit."""
        T = self.t
        r, v, d = self.rewards[:T], self.values[:T], self.dones[:T]
        if not r.is_cuda:
            return self._finish_torch()
        last = self._last_values()
        ret = torch.empty_like(r); adv = torch.empty_like(r); comp = torch.empty_like(d); lret = torch.empty_like(r)
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        with torch.cuda.device(r.device):
            _ffi.check(_ffi.lib().bbx_gae_bootstrap_device(p(r), p(v), p(d), T, self.B, float(self.gam), float(self.lam), p(last), p(ret), p(adv),
                                                           p(comp), p(lret), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.returns, self.advantages, self.complete, self.lambda_returns = ret, adv, comp, lret
        return ret, adv, comp

    def _last_values(self):
        """self.last_values as the scans read it: None, or a contiguous float64 [B] tensor on the buffer's device (anything else:
        ValueError — the kernel reads B doubles behind a raw pointer)."""
        last = self.last_values
        if last is None:
            return None
        if not torch.is_tensor(last) or last.dtype != torch.float64 or tuple(last.shape) != (self.B,) or last.device != self.rewards.device:
            raise ValueError("last_values: None or a float64 tensor of shape (%d,) on %s" % (self.B, self.rewards.device))
        return last.contiguous()

    def _finish_torch(self):
        """finish() with torch ops, about ten launches per step: CPU tensors, and the reference of the kernel."""
        T = self.t
        r, v, d = self.rewards[:T], self.values[:T], self.dones[:T]
        boot = self._last_values()
        ret = torch.zeros_like(r); adv = torch.zeros_like(r); comp = torch.zeros_like(d); lret = torch.zeros_like(r)
        nret = torch.zeros(self.B, dtype=torch.float64, device=r.device); nadv = torch.zeros_like(nret)
        nval = torch.zeros_like(nret); ncomp = torch.zeros(self.B, dtype=torch.bool, device=r.device)
        if boot is not None:                                         # the state behind step T - 1 is worth boot, and nothing is cut
            nret = boot.clone(); nval = boot.clone(); ncomp = torch.ones_like(ncomp)
        for t in range(T - 1, -1, -1):
            last = d[t]                                              # step t ends its episode: nothing follows it
            nret = torch.where(last, torch.zeros_like(nret), nret); nadv = torch.where(last, torch.zeros_like(nadv), nadv)
            nval = torch.where(last, torch.zeros_like(nval), nval); ncomp = ncomp | last
            ret[t] = r[t] + self.gam * nret
            adv[t] = (r[t] - v[t] + self.gam * nval) + self.gam * self.lam * nadv
            comp[t] = ncomp
            lret[t] = adv[t] + v[t]
            nret, nadv, nval = ret[t], adv[t], v[t]
        self.returns, self.advantages, self.complete, self.lambda_returns = ret, adv, comp, lret
        return ret, adv, comp

    def get_index(self, batch_size=None, normalize_advantages=True, sort=False, drop_remainder=False, with_rows=False, targets="returns"):
        """get() without the state blocks: the same selection, order, advantage normalisation and batching, but the first element
        of every tuple is an int32 tensor of flat step numbers t * B + b — positions in self.states.view(-1, R, cols),
        self.rows.view(-1) and self.actions.view(-1) — for PMLPPolicy.evaluate_at, which reads the states where the rollout
        left them.  With batch_size the tuples hold slices of ONE index tensor (a shuffle of the epoch is a permutation of it);
        nothing of the size of a state block is allocated, nothing waits for the device per batch, and a buffer without states
        gives the same indices.  targets: what the fifth element holds — "returns" (the discounted returns) or "lambda"
        (lambda_returns, adv + v before normalisation); anything else: ValueError."""
        if targets not in ("returns", "lambda"):
            raise ValueError("targets: \"returns\" or \"lambda\" (got %r)" % (targets,))
        if self.returns is None:
            self.finish()
        T = self.t
        em = lambda x: x[:T].transpose(0, 1)                        # [B, T, ...]: trajectory after trajectory
        comp = em(self.complete)
        adv = em(self.advantages)[comp].to(torch.float32)
        if normalize_advantages and adv.numel():
            adv = (adv - adv.mean()) / adv.std(unbiased=False)
        rows = em(self.rows)[comp]
        keep = rows != 1
        dev = self.rows.device
        step = torch.arange(T, dtype=torch.int32, device=dev)[None, :] * self.B + torch.arange(self.B, dtype=torch.int32, device=dev)[:, None]
        idx, adv, rows = step[comp][keep], adv[keep], rows[keep]
        if sort:
            order = torch.argsort(rows, stable=True)
            idx, adv, rows = idx[order], adv[order], rows[order]
        j = idx.to(torch.int64)
        at = lambda x: x[:T].reshape(-1)[j]
        out = [idx, at(self.actions), at(self.logprobs), adv, at(self.returns if targets == "returns" else self.lambda_returns).to(torch.float32)]
        if with_rows:
            out.append(rows)
        if batch_size is None:
            return tuple(out)
        n = int(idx.numel())
        batches = []
        for i in range(0, n, batch_size):
            k = min(i + batch_size, n)
            if drop_remainder and k - i < batch_size:
                break
            batches.append(tuple(x[i:k] for x in out))
        return batches

    def get(self, batch_size=None, normalize_advantages=True, sort=False, drop_remainder=False, with_rows=False, targets="returns"):
        """Training data of all complete-episode steps whose state had more than one row (pg.py:162-240): (states or None,
        actions, logprobs, advantages, values-to-fit), advantages normalised by their mean and population std over the
        complete steps (pg.py:176-178: before the single-row filter, like the reference), steps ordered trajectory after
        trajectory (environment-major).  batch_size=None: one tuple of whole tensors.  Otherwise the reference's
        padded_batch: a list of such tuples of at most batch_size steps each, the state block of a batch cut to the most
        rows any of its states has (-1 padding beyond a state's own rows, as stored); sort=True orders the steps by their
        number of rows first (less padding); drop_remainder=True leaves a short last batch out.  with_rows=True: every tuple
        carries the states' row counts (int32) as a sixth element (what PMLPPolicy.evaluate takes as `rows`).
        targets: "returns" or "lambda", the values-to-fit as in get_index.
        The selection is get_index's; the states are gathered here, once."""
        whole = self.get_index(None, normalize_advantages, sort, False, True, targets)
        rows = whole[5]
        st = self.states[:self.t].reshape((-1,) + tuple(self.states.shape[2:]))[whole[0].to(torch.int64)] if self.states is not None else None
        out = [st] + list(whole[1:6 if with_rows else 5])
        if batch_size is None:
            return tuple(out)
        n = int(rows.numel())
        batches = []
        for i in range(0, n, batch_size):
            j = min(i + batch_size, n)
            if drop_remainder and j - i < batch_size:
                break
            mr = int(rows[i:j].max()) if self.states is not None else 0
            batches.append(tuple(None if x is None else (x[i:j, :mr] if k == 0 else x[i:j]) for k, x in enumerate(out)))
        return batches


def _epochs(name, buffer, columns, optimizer, epochs, batch_size, shuffle, generator, step, targets="returns", index=None):
    """The epoch loop of ppo_update, value_update and imitation_update, one epoch per iteration: ONE permutation of buffer.get_index()'s
    steps (shuffle; from `generator`), then per minibatch of batch_size step(index slice, the same slice of each of get_index's
    `columns`) — which returns the minibatch's six statistics on the device —, optimizer.step() and optimizer.zero_grad().  index
    (int32 flat step numbers; None: get_index's): the steps to run over instead, with no columns — nothing is finished or filtered.
    Yields (the minibatches' stacked statistics float64 [minibatches, 6] — the epoch's one host read —, their sum, the counted
    positions or 1)."""
    if buffer.states is None:
        raise ValueError("%s: the buffer keeps no states (DeviceTrajectoryBuffer(..., obs_shape=(rows, cols)))" % name)
    if index is None:
        whole = buffer.get_index(None, targets=targets)
        cols = [whole[0]] + [whole[c] for c in columns]
    else:
        cols = [index]
    n = int(cols[0].numel())
    optimizer.zero_grad()
    for _ in range(epochs):
        if shuffle:
            perm = torch.randperm(n, device=cols[0].device, generator=generator)
            e = [x[perm] for x in cols]
        else:
            e = cols
        stats = []
        for i in range(0, n, batch_size):
            k = min(i + batch_size, n)
            stats.append(step(*[x[i:k] for x in e]))
            optimizer.step()
            optimizer.zero_grad()
        st = torch.stack(stats).cpu().numpy() if stats else np.zeros((0, 6))
        tot = st.sum(axis=0) if len(st) else np.zeros(6)
        yield st, tot, max(tot[0], 1.0)


def ppo_update(policy, buffer, optimizer, epochs, batch_size, clip=0.2, ent_coef=0.0, kld_limit=None, mode="clip", shuffle=True, generator=None,
               c_kl=0.0):
    """The policy update of the reference (pg.py _fit_policy_model) over a finished DeviceTrajectoryBuffer with states: `epochs`
    passes over buffer.get_index()'s steps in minibatches of batch_size — per epoch ONE permutation of the index list (shuffle; from
    `generator`, which lives on the buffer's device), per minibatch one policy.ppo_step_at on the buffers as the rollout left them,
    then optimizer.step() and optimizer.zero_grad(); the optimiser is the caller's.  One host read per epoch: the minibatches'
    stacked statistics.  With kld_limit the update stops after an epoch whose mean old - new log-probability exceeds it.
    Returns one dict per epoch run: "stats" (float64 [minibatches, 6], ppo_step_at's), and over the epoch's counted positions
    "loss", "entropy", "kl" (mean old - new) and "clip_frac"."""
    step = lambda i, o, a: policy.ppo_step_at(buffer.states, buffer.actions, buffer.rows, i, o, a, clip=clip, ent_coef=ent_coef, mode=mode, c_kl=c_kl)[0]
    out = []
    for st, tot, cnt in _epochs("ppo_update", buffer, (2, 3), optimizer, epochs, batch_size, shuffle, generator, step):
        out.append({"stats": st, "loss": -(tot[1] + ent_coef * tot[2]) / cnt, "entropy": tot[2] / cnt, "kl": tot[3] / cnt, "clip_frac": tot[4] / cnt})
        if kld_limit is not None and out[-1]["kl"] > kld_limit:
            break
    return out


def value_update(critic, buffer, optimizer, epochs, batch_size, shuffle=True, generator=None, targets="returns"):
    """The counterpart of ppo_update for a PMLPValue critic (pg.py _fit_value_model): `epochs` passes over buffer.get_index()'s steps
    in minibatches of batch_size, the targets its fifth element (get_index(targets=...): the discounted returns, or with "lambda"
    the TD(lambda) targets adv + v) — per epoch ONE permutation of the index
    list (shuffle; from `generator`, which lives on the buffer's device), per minibatch one critic.fit_step_at on the buffers as the
    rollout left them, then optimizer.step() and optimizer.zero_grad(); the optimiser is the caller's.  One host read per epoch: the
    minibatches' stacked statistics.  Returns one dict per epoch: "stats" (float64 [minibatches, 6], fit_step_at's), and over the
    epoch's counted positions "loss" (1/2 mean (V - target)^2, each minibatch under the weights it saw) and "explained_variance"
    (1 - mean (V - target)^2 / var(target); NaN where the targets do not vary)."""
    step = lambda i, r: critic.fit_step_at(buffer.states, buffer.rows, i, r)[0]
    out = []
    for st, tot, cnt in _epochs("value_update", buffer, (4,), optimizer, epochs, batch_size, shuffle, generator, step, targets):
        var = tot[4] / cnt - (tot[3] / cnt) ** 2
        out.append({"stats": st, "loss": 0.5 * tot[1] / cnt, "explained_variance": 1.0 - (tot[1] / cnt) / var if var > 0 else float("nan")})
    return out


def action_value_targets(q, rows, obs_rows, temperature=1.0, out=None):
    """env.action_values()'s q — float64 [B, R], NaN beyond every environment's pairs — as target rows for PMLPPolicy.xent_step[_at] and
    DeviceTrajectoryBuffer.store(target=): float32 [B, obs_rows] (into `out` if given), zero beyond the live rows
    n = clamp(rows, 0, min(R, obs_rows)); columns beyond min(R, obs_rows) are dropped before normalising.
        temperature > 0    the softmax of q / temperature over the live rows (formed in float64)
        temperature == 0   a one-hot row at the first maximum
    An environment without pairs gets a zero row (which trains nothing).  A NaN among the live q (a clone that did not run to the
    end) leaves a NaN row with temperature > 0, which the cross-entropy does not count."""
    if temperature < 0:
        raise ValueError("action_value_targets: temperature >= 0 (got %r)" % (temperature,))
    q = torch.as_tensor(q)
    B, R = q.shape
    m = min(R, obs_rows)
    n = torch.clamp(torch.as_tensor(rows, device=q.device).to(torch.int64), 0, m)
    live = torch.arange(m, device=q.device)[None, :] < n[:, None]
    x = q[:, :m].to(torch.float64)
    neg = torch.full_like(x, float("-inf"))
    zero = torch.zeros_like(x)
    some = (n > 0)[:, None]
    if temperature > 0:
        y = torch.where(live, x / temperature, neg)
        mx = torch.where(some, y.max(dim=1, keepdim=True).values, torch.zeros_like(y[:, :1]))
        e = torch.where(live, torch.exp(y - mx), zero)
        t = torch.where(some, e / e.sum(dim=1, keepdim=True), zero)
    else:
        y = torch.where(live, x, neg)
        top = y.max(dim=1, keepdim=True).values
        first = ((y == top) & live).to(torch.int64).argmax(dim=1)     # (0 / 1 flags: argmax returns the first 1)
        t = torch.where(some & (torch.arange(m, device=q.device)[None, :] == first[:, None]), torch.ones_like(x), zero)
    if out is None:
        out = torch.zeros((B, obs_rows), dtype=torch.float32, device=q.device)
    else:
        out.zero_()
    out[:, :m].copy_(t)
    return out


def imitation_update(policy, buffer, optimizer, epochs, batch_size, shuffle=True, generator=None):
    """Imitation towards the target rows of a DeviceTrajectoryBuffer(..., targets=True): `epochs` passes over EVERY stored state of the
    buffer (no finish(), no rewards, no filter on complete episodes) in minibatches of batch_size — per epoch ONE permutation of
    the steps (shuffle; from `generator`, which lives on the buffer's device), per minibatch one policy.xent_step_at on the buffers as
    the rollout left them (the mean cross-entropy of the minibatch), then optimizer.step() and optimizer.zero_grad(); the optimiser is
    the caller's.  One host read per epoch: the minibatches' stacked statistics.  Returns one dict per epoch: "stats" (float64
    [minibatches, 6], xent_step_at's), "loss" (sum w l / sum w over the epoch) and "entropy" (the mean over the counted positions)."""
    if buffer.targets is None:
        raise ValueError("imitation_update: the buffer keeps no targets (DeviceTrajectoryBuffer(..., targets=True))")
    index = torch.arange(buffer.t * buffer.B, dtype=torch.int32, device=buffer.rows.device)
    step = lambda i: policy.xent_step_at(buffer.states, buffer.rows, i, buffer.targets)[0]
    out = []
    for st, tot, cnt in _epochs("imitation_update", buffer, (), optimizer, epochs, batch_size, shuffle, generator, step, index=index):
        out.append({"stats": st, "loss": tot[1] / tot[4] if tot[4] != 0 else float("nan"), "entropy": tot[3] / cnt})
    return out


def _set_last_values(buffer, last):
    """A rollout's last word on its buffer: the bootstrap of the cut tails (None: there is none), and whatever an earlier
    finish() left is cleared — it knows neither the new steps nor the new tail."""
    buffer.last_values = last
    buffer.returns = buffer.advantages = buffer.complete = buffer.lambda_returns = None


def _critic_last_values(env, critic, obs_rows, stream):
    """The critic's values of the states the environments are in now, float64 [B]: a zero-step launch writes the padded
    observation block and the row counts (it steps nothing and draws nothing), one critic.values call reads them."""
    B, dev = env.batch, torch.device("cuda", torch.cuda.current_device())
    obs = torch.empty((B, obs_rows, env.cols), dtype=torch.int32, device=dev)
    rew = torch.zeros(B, dtype=torch.float64, device=dev); done = torch.zeros(B, dtype=torch.uint8, device=dev)
    rows = torch.zeros(B, dtype=torch.int32, device=dev)
    env.rollout_device("first", 0, False, stream.cuda_stream, rew, done, rows, obs, obs_rows, True, False)
    env.sync()
    last = torch.empty(B, dtype=torch.float64, device=dev)
    critic.values(obs, rows, out64=last)
    return last


@contextlib.contextmanager
def _episode_limit(env, max_episode_length):
    """env.episode_limit(max_episode_length) for the duration of a call, restored afterwards (as `greedy` is)."""
    before = env.episode_limit(max_episode_length)
    try:
        yield
    finally:
        env.episode_limit(before)


@_with_gc_paused
@torch.no_grad()
def run_rollout_fused(env, policy, nsteps, buffer=None, obs_rows=256, generator=None, chunk=256, greedy=False, critic=None, bootstrap=False,
                      max_episode_length=None):
    """run_rollout with the policy INSIDE the step kernel: `chunk` vector steps per launch, environments never wait for each
    other between steps.  One hidden layer: bbx_policy_rollout_device; two hidden layers of at most 128 units:
    bbx_policy2_rollout_device (weights from policy._deep_weights(), refilled in place after optimiser steps); any other
    depth or width raises BbxError (BBX_E_UNSUPPORTED) before anything is prepared or queued.  Per-step outputs land in the
    trajectory buffer's own arrays (no copies).  Raises BbxError (BBX_E_UNSUPPORTED) where the batch's kernel class has no
    built-in policy — callers fall back to run_rollout.  There is no value_strategy here (run_rollout has it): baseline
    values inside the T-step policy kernels would need a rollout to completion nested in the kernels' step loop — a different
    piece of work; a LEARNED baseline is what `critic` is for.  Returns (total reward per environment, finished episodes) like
    run_rollout.  The rollout kernels are the lean ones (no algorithmic-byte accounting): the handle's accounting is switched
    off here.
    greedy=True: the highest-probability pair at every step (env.policy_greedy for the duration of the call, restored
    afterwards); no uniforms are drawn.
    critic (a PMLPValue; needs a buffer that keeps states): after the last chunk buffer.fill_values(critic, ...) writes the
    critic's values of the steps recorded here into buffer.values — one launch over the recorded block, nothing per step; the
    rollout itself is the one without a critic, draw for draw.  None: buffer.values is left as it is.  A critic without a
    state-keeping buffer: ValueError before anything is queued.
    bootstrap=True (needs a critic): behind fill_values one zero-step launch writes the observation block the environments
    stopped in, and the critic's values of it become buffer.last_values — finish() then bootstraps the episodes the end of the
    buffer cut instead of dropping them (truncated-horizon GAE).  The environments are not touched by it.  Every call with a
    buffer sets buffer.last_values (None without bootstrap) and clears what an earlier finish() left.  bootstrap=True without a
    critic: ValueError before anything is queued.
    max_episode_length=L: the reference's cap on episode length (env.episode_limit(L) for the duration of the call, restored
    afterwards): an episode that has taken L steps and still has pairs is cut inside the kernels — done is set, the next episode
    begins.  GAE treats the cut as terminal, as the reference's loop does.  None: the handle's own limit, whatever it is."""
    if max_episode_length is not None:
        with _episode_limit(env, max_episode_length):
            return run_rollout_fused(env, policy, nsteps, buffer, obs_rows, generator, chunk, greedy, critic, bootstrap)
    if critic is not None and (buffer is None or buffer.states is None):
        raise ValueError("run_rollout_fused: a critic reads the recorded states (buffer=DeviceTrajectoryBuffer(..., obs_shape=(rows, cols)))")
    if bootstrap and critic is None:
        raise ValueError("run_rollout_fused: bootstrap=True takes the value of the state the rollout stops in from a critic (critic=PMLPValue(...))")
    B, cols = env.batch, env.cols
    depth = len(policy.embedding)
    if not (depth == 1 or (depth == 2 and policy.deep_ok(cols))):
        raise _ffi.BbxError(-5, "run_rollout_fused: policies with one hidden layer, or two of at most 128 units, run inside the step kernels "
                                "(this one: %s); use run_rollout" % [l.out_features for l in policy.embedding])
    env.accounting(False)
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream()
    if depth == 1:
        w = policy._fused_weights()
        rollout = lambda *a: env.policy_rollout_device(w["prepared"], w["hidden"], *a)
    else:
        w = policy._deep_weights()
        rollout = lambda *a: env.policy2_rollout_device(w["prepared"], w["hidden"][0], w["hidden"][1], *a)
    keep_states = buffer is not None and buffer.states is not None
    if keep_states:
        obs_rows = buffer.states.shape[2]
    if buffer is None:
        act = torch.empty((chunk, B), dtype=torch.int32, device=dev); logp = torch.empty((chunk, B), dtype=torch.float32, device=dev)
    obs1 = None if keep_states else torch.empty((B, obs_rows, cols), dtype=torch.int32, device=dev)
    st0 = env.stats()
    if buffer is not None:
        # the kernel writes n x B elements behind raw pointers into the buffer's arrays: a short slice would be overrun
        if buffer.t + nsteps > buffer.T:
            raise IndexError("trajectory buffer holds %d steps, %d are stored already: no room for %d more" % (buffer.T, buffer.t, nsteps))
        if keep_states and tuple(buffer.states.shape[2:]) != (obs_rows, cols):
            raise ValueError("buffer.states has blocks of %s, the environment writes (%d, %d)" % (tuple(buffer.states.shape[2:]), obs_rows, cols))
    t_start = buffer.t if buffer is not None else 0
    was_greedy = env.policy_greedy(greedy)
    try:
        for t0 in range(0, nsteps, chunk):
            n = min(chunk, nsteps - t0)
            u = None if greedy else torch.rand((n, B), device=dev, generator=generator)
            if buffer is not None:
                t = buffer.t
                obs = buffer.states[t:t + n] if keep_states else obs1
                if keep_states:
                    obs.fill_(-1)                       # the kernel writes the live rows only; the rest is the reference's padding
                rollout(n, u, buffer.actions[t:t + n], buffer.logprobs[t:t + n], buffer.rewards[t:t + n], buffer.dones[t:t + n], buffer.rows[t:t + n],
                        obs, obs_rows, B * obs_rows * cols if keep_states else 0, stream.cuda_stream)
                buffer.t += n
            else:
                rollout(n, u, act, logp, None, None, None, obs1, obs_rows, 0, stream.cuda_stream)
            env.sync()
    finally:
        env.policy_greedy(was_greedy)
    if critic is not None:
        buffer.fill_values(critic, t_start, buffer.t)
    last = None
    if bootstrap:
        last = _critic_last_values(env, critic, obs_rows, stream)
    if buffer is not None:
        _set_last_values(buffer, last)
    d = env.stats() - st0
    total = torch.tensor(-d[:, 1].astype(np.float64), device=dev)
    episodes = torch.tensor(d[:, 2], device=dev)
    return total, episodes


@_with_gc_paused
@torch.no_grad()
def run_rollout(env, policy, nsteps, buffer=None, obs_rows=256, generator=None, sync_every=64, graph=False,
                value_strategy=None, value_gamma=None, greedy=False, critic=None, bootstrap=False, max_episode_length=None):
    """nsteps vector steps of `env` (a VecLeadMonomialsEnv already reset) under `policy`, everything on the device
    (obs_rows: rows of the observation block per environment — a pair set with more rows makes env.sync() raise
    BBX_E_CAPACITY, it is never cut silently; 256 is what the register/LDS-resident class holds):
    observation block -> policy.act (log-softmax + inverse-CDF draw) -> bbx_step_device_autoreset -> next block.  The
    host only enqueues kernels; it waits (env.sync: errors, environments that outgrew a kernel class) every
    `sync_every` steps and at the end.  Returns (total reward per environment float64 [B] — for `additions` rewards —,
    finished episodes int64 [B]).
    graph=True (policies without a fused kernel, i.e. more than one hidden layer; no buffer): the vector step — the
    policy's torch ops and the step kernels — is recorded once into a HIP graph (kept on `env`) and replayed, one graph
    launch per step instead of ~25 kernel launches from Python; same draws, same results.
    value_strategy (with a buffer): buffer.values[t] receives env.value(value_strategy, value_gamma) of the state the policy is
    about to see at step t (pg.py:451-475 with --value_model: value, then action, then step; after an auto-reset it is the
    new episode's first state), written on the device by env.values_device straight into the buffer's row, its rollouts
    overlapping the steps that follow; value_gamma defaults to buffer.gam.  No extra host wait.  None: no values, call for call
    what it was.  With graph=True: ValueError.
    greedy=True: the highest-probability pair at every step (policy.act(greedy=True); env.policy_greedy for the duration of the
    call, restored afterwards); no uniforms are drawn.
    critic (a PMLPValue; needs a buffer that keeps states; not together with value_strategy): behind the loop
    buffer.fill_values(critic, ...) writes the critic's values of the steps recorded here into buffer.values, as
    run_rollout_fused does.
    bootstrap=True (needs a buffer and a value_strategy or a critic): buffer.last_values receives the value of the state the
    rollout stops in — one more env.values_device before the final wait, or the critic's values of the observation block the
    loop ends with — and finish() bootstraps the episodes the end of the buffer cut instead of dropping them.  The
    environments are not touched by it.  Every call with a buffer sets buffer.last_values (None without bootstrap) and clears
    what an earlier finish() left.  All refusals are ValueError before anything is queued.
    max_episode_length=L: as in run_rollout_fused (env.episode_limit(L) for the duration of the call; a recorded graph is kept
    per limit).  The values of value_strategy are those of the whole computation: the value calls ignore the limit."""
    if max_episode_length is not None:
        with _episode_limit(env, max_episode_length):
            return run_rollout(env, policy, nsteps, buffer, obs_rows, generator, sync_every, graph, value_strategy, value_gamma, greedy,
                               critic, bootstrap)
    if value_strategy is not None and graph:
        raise ValueError("run_rollout: value_strategy cannot be recorded into a graph (bbx_values_device keeps host bookkeeping)")
    if value_strategy is not None and buffer is None:
        raise ValueError("run_rollout: value_strategy needs a buffer to write the values to")
    if critic is not None and value_strategy is not None:
        raise ValueError("run_rollout: one baseline per rollout, a critic or a value_strategy")
    if critic is not None and (buffer is None or buffer.states is None):
        raise ValueError("run_rollout: a critic reads the recorded states (buffer=DeviceTrajectoryBuffer(..., obs_shape=(rows, cols)))")
    if bootstrap and buffer is None:
        raise ValueError("run_rollout: bootstrap=True needs a buffer to bootstrap")
    if bootstrap and critic is None and value_strategy is None:
        raise ValueError("run_rollout: bootstrap=True takes the value of the state the rollout stops in from a critic or a value_strategy")
    if value_strategy is not None and value_gamma is None:
        value_gamma = buffer.gam
    B, cols = env.batch, env.cols
    dev = torch.device("cuda", torch.cuda.current_device())
    one_call = len(policy.embedding) == 1 and policy.fused_ok(cols, policy.embedding[0].out_features) and hasattr(env, "policy_step_device")
    if graph and not one_call and buffer is None:
        return _run_rollout_graph(env, policy, nsteps, obs_rows, generator, sync_every, greedy)
    stream = torch.cuda.current_stream()
    obs = torch.empty((B, obs_rows, cols), dtype=torch.int32, device=dev)
    rew = torch.zeros(B, dtype=torch.float64, device=dev); done = torch.zeros(B, dtype=torch.uint8, device=dev)
    rows = torch.zeros(B, dtype=torch.int32, device=dev); act = torch.zeros(B, dtype=torch.int32, device=dev)
    logp = torch.zeros(B, dtype=torch.float32, device=dev)
    st0 = env.stats()
    # the current observation: a zero-step launch writes the padded block and the row counts
    env.rollout_device("first", 0, False, stream.cuda_stream, rew, done, rows, obs, obs_rows, True, False)
    env.sync()
    keep_states = buffer is not None and buffer.states is not None
    t_start = buffer.t if buffer is not None else 0
    by_strategy, last = bootstrap and value_strategy is not None, None
    w = policy._fused_weights() if one_call else None
    nsync = 0
    was_greedy = env.policy_greedy(greedy) if one_call else None
    try:
        for t0 in range(0, nsteps, sync_every):
            n = min(sync_every, nsteps - t0)
            u_all = None if greedy else torch.rand((n, B), device=dev, generator=generator)   # one generator launch per chunk of steps
            for i in range(n):
                u = None if greedy else u_all[i]
                if buffer is not None:                  # what the policy is about to see
                    t = buffer.t
                    if keep_states:
                        buffer.states[t].copy_(obs)
                    buffer.rows[t].copy_(rows)
                    if value_strategy is not None:      # value, then action, then step (pg.py:461-465)
                        env.values_device(buffer.values[t], value_strategy, value_gamma, None, stream.cuda_stream)
                if one_call:                            # policy + step: one library call (one kernel where the class has it)
                    env.policy_step_device(w["prepared"], w["hidden"], u, act, logp, rew, done, rows, obs, obs_rows, 2, stream.cuda_stream)   # (2: incremental padding)
                else:
                    policy.act(obs, rows, u, act, logp, stream, greedy=greedy)
                    env.step_device(act, rew, done, rows, obs, obs_rows, 2, stream.cuda_stream, auto_reset=True)
                if buffer is not None:
                    buffer.actions[t].copy_(act); buffer.logprobs[t].copy_(logp)
                    buffer.rewards[t].copy_(rew); buffer.dones[t].copy_(done)
                    buffer.t += 1
            if by_strategy and t0 + n == nsteps:        # the value of the state the rollout stops in, ahead of the last wait
                last = torch.empty(B, dtype=torch.float64, device=dev)
                env.values_device(last, value_strategy, value_gamma, None, stream.cuda_stream)
            env.sync()
            nsync += 1
    finally:
        if one_call:
            env.policy_greedy(was_greedy)
    if by_strategy and last is None:                    # (a rollout of no steps: the state it started in)
        last = torch.empty(B, dtype=torch.float64, device=dev)
        env.values_device(last, value_strategy, value_gamma, None, stream.cuda_stream)
        env.sync()
    if critic is not None:
        buffer.fill_values(critic, t_start, buffer.t)
        if bootstrap:                                   # obs / rows: the block the loop ends with
            last = torch.empty(B, dtype=torch.float64, device=dev)
            critic.values(obs, rows, out64=last)
    if buffer is not None:
        _set_last_values(buffer, last)
    # totals from the environments' own counters (additions rewards: reward = -additions, buchberger.cpp:328)
    d = env.stats() - st0
    total = torch.tensor(-d[:, 1].astype(np.float64), device=dev)
    episodes = torch.tensor(d[:, 2], device=dev)
    return total, episodes


def _run_rollout_graph(env, policy, nsteps, obs_rows, generator, sync_every, greedy=False):
    """run_rollout with the vector step replayed from a HIP graph (see there).  The graph and its buffers live on `env`
    (one per policy object and block height) and are reused by later calls; the policy's parameters are read in place, so
    optimiser steps between calls are seen."""
    B, cols = env.batch, env.cols
    dev = torch.device("cuda", torch.cuda.current_device())
    cache = env.__dict__.setdefault("_step_graphs", {})
    key = (id(policy), obs_rows, sync_every, bool(greedy), getattr(env, "_episode_limit", None))   # (a recording keeps the mode and the episode limit it was captured with)
    c = cache.get(key)
    if c is None:
        c = {"obs": torch.empty((B, obs_rows, cols), dtype=torch.int32, device=dev),
             "rew": torch.zeros(B, dtype=torch.float64, device=dev), "done": torch.zeros(B, dtype=torch.uint8, device=dev),
             "rows": torch.ones(B, dtype=torch.int32, device=dev), "act": torch.zeros(B, dtype=torch.int32, device=dev),
             "logp": torch.zeros(B, dtype=torch.float32, device=dev),
             "u": torch.zeros((sync_every, B), dtype=torch.float32, device=dev), "i": torch.zeros(1, dtype=torch.int64, device=dev),
             "policy": policy}
        c["obs"].fill_(-1)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                  # the library GEMMs pick their workspaces outside the capture
            for _ in range(3):
                policy.act(c["obs"], c["rows"], c["u"][0], c["act"], c["logp"], side, greedy=greedy)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        env.sync()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cs = torch.cuda.current_stream()
            u = c["u"].index_select(0, c["i"]).squeeze(0)
            policy.act(c["obs"], c["rows"], u, c["act"], c["logp"], cs, greedy=greedy)
            env.step_device(c["act"], c["rew"], c["done"], c["rows"], c["obs"], obs_rows, 2, cs.cuda_stream, auto_reset=True)
            c["i"].add_(1)
        c["graph"] = g
        cache[key] = c
    stream = torch.cuda.current_stream()
    if policy.deep_ok(cols) and obs_rows <= policy.deep_max_rows():
        policy._deep_weights()                       # (weights changed since the recording: the prepared copy is refilled in place)
    st0 = env.stats()
    env.rollout_device("first", 0, False, stream.cuda_stream, c["rew"], c["done"], c["rows"], c["obs"], obs_rows, True, False)
    env.sync()
    for t0 in range(0, nsteps, sync_every):
        n = min(sync_every, nsteps - t0)
        if not greedy:
            c["u"][:n].copy_(torch.rand((n, B), device=dev, generator=generator))
        c["i"].zero_()
        for _ in range(n):
            c["graph"].replay()
        try:
            env.graph_replayed(stream.cuda_stream)
            env.sync()                                 # (records that were enlarged inside the replays are reported here)
        except _ffi.BbxError:
            # the records live at a new address now, or an environment sat out part of the chain: the recording steps a
            # retired copy from here on — dropped, the next call records again
            cache.pop(key, None)
            raise
    d = env.stats() - st0
    return torch.tensor(-d[:, 1].astype(np.float64), device=dev), torch.tensor(d[:, 2], device=dev)


def episode_returns(rewards, dones, carry=None):
    """Per-episode returns and lengths from the [T, B] rewards (float64) and done flags (bool / uint8) of a rollout: one
    return and one length per episode, what run_episodes logs (pg.py).  Per environment b, in step order: acc += r[t, b]
    (a plain double add), len += 1; where dones[t, b] is set, ep_return[t, b] = acc, ep_len[t, b] = len and both start again
    from zero; every other entry is 0.  Returns (ep_return float64 [T, B], ep_len int32 [T, B]).
    carry: None (every environment starts a new episode at t = 0, what is left over at the end is dropped) or a tuple
    (carry_return float64 [B], carry_len int32 [B], ep_count int32 [B] or None) of tensors on the device of `rewards`, updated
    in place: an episode that spans calls is finished by a later one, ep_count gains the episodes finished here — a long
    evaluation is a chain of chunks.
    Tensors on the GPU: one kernel (bbx_episodes_device, one thread per environment).  CPU tensors (or numpy arrays): the
    torch loop below, whose results the kernel reproduces exactly."""
    rewards = torch.as_tensor(rewards)
    dones = torch.as_tensor(dones)
    if rewards.dim() != 2 or tuple(dones.shape) != tuple(rewards.shape):
        raise ValueError("episode_returns: rewards and dones are [T, B] arrays of one shape (got %s and %s)" % (tuple(rewards.shape), tuple(dones.shape)))
    T, B = rewards.shape
    r = rewards.to(torch.float64).contiguous()
    d = (dones if dones.dtype in (torch.bool, torch.uint8) else dones != 0).contiguous()
    cret, clen, count = carry if carry is not None else (None, None, None)
    ep_ret = torch.zeros((T, B), dtype=torch.float64, device=r.device)
    ep_len = torch.zeros((T, B), dtype=torch.int32, device=r.device)
    if r.is_cuda:
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        with torch.cuda.device(r.device):
            _ffi.check(_ffi.lib().bbx_episodes_device(p(r), p(d), T, B, p(cret), p(clen), p(count), p(ep_ret), p(ep_len),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return ep_ret, ep_len
    acc = cret.clone() if cret is not None else torch.zeros(B, dtype=torch.float64)
    ln = clen.clone() if clen is not None else torch.zeros(B, dtype=torch.int32)
    for t in range(T):
        acc = acc + r[t]
        ln = ln + 1
        dd = d[t].to(torch.bool)
        ep_ret[t] = torch.where(dd, acc, torch.zeros_like(acc))
        ep_len[t] = torch.where(dd, ln, torch.zeros_like(ln))
        acc = torch.where(dd, torch.zeros_like(acc), acc)
        ln = torch.where(dd, torch.zeros_like(ln), ln)
        if count is not None:
            count += dd.to(count.dtype)
    if cret is not None:
        cret.copy_(acc)
    if clen is not None:
        clen.copy_(ln)
    return ep_ret, ep_len


Evaluation = collections.namedtuple("Evaluation", ["returns", "lengths", "complete", "steps"])


def evaluate_policy(env, policy, episodes, greedy=True, obs_rows=256, chunk=64, max_steps=None, generator=None, max_episode_length=None):
    """The first `episodes` episodes of every environment of `env` under `policy` (run_episodes(..., greedy=True) and
    scripts/eval.py of the reference, for a whole batch): env.reset(), then chunks of `chunk` vector steps — the fused rollout
    (run_rollout_fused) where the handle's kernel class has the policy built in, run_rollout's per-step path where it raises
    BbxError -5; decided once, at the first chunk, before anything is stepped.  The environments simply keep stepping (auto-reset);
    after each chunk bbx_episodes_device (episode_returns, with carries) turns the chunk's rewards and dones into per-episode
    returns and lengths, and every finished episode whose ordinal within its environment is below `episodes` is scattered, on the
    device, into
        returns  float64 [B, episodes]      lengths  int32 [B, episodes].
    Later episodes of faster environments are ignored: that is what keeps a batch stepping in lockstep from over-weighting short
    episodes.  One host read per chunk (the smallest episode count); the loop ends when it reaches `episodes`, or at `max_steps`
    vector steps — the result then has complete=False, with NaN / -1 in the entries no episode reached.
    greedy=True takes the highest-probability pair at every step (no uniforms drawn); False samples (generator: torch's).
    On a handle built from a LIST of ideals (environment e takes ideals e, e + B, e + 2B, ... in turn), returns[e, j] belongs to
    ideal (e + j * B) % nideals.
    max_episode_length=L (eval.py's cap): env.episode_limit(L) for the duration of the call, restored afterwards — an episode cut
    at L steps is an episode of length L with the return it has collected; no length exceeds L.
    Returns Evaluation(returns, lengths, complete, steps)."""
    if episodes < 1 or chunk < 1:
        raise ValueError("evaluate_policy: episodes and chunk must be positive")
    if max_episode_length is not None:
        with _episode_limit(env, max_episode_length):
            return evaluate_policy(env, policy, episodes, greedy, obs_rows, chunk, max_steps, generator)
    B = env.batch
    dev = torch.device("cuda", torch.cuda.current_device())
    env.reset()
    buf = DeviceTrajectoryBuffer(chunk, B, device=dev)
    # one spare column: where every entry that is not one of the first `episodes` finished episodes lands
    returns = torch.full((B, episodes + 1), float("nan"), dtype=torch.float64, device=dev)
    lengths = torch.full((B, episodes + 1), -1, dtype=torch.int32, device=dev)
    cret = torch.zeros(B, dtype=torch.float64, device=dev)
    clen = torch.zeros(B, dtype=torch.int32, device=dev)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    fused = None
    steps, finished = 0, 0
    while finished < episodes and (max_steps is None or steps < max_steps):
        n = chunk if max_steps is None else min(chunk, max_steps - steps)
        buf.t = 0
        if fused is None:
            try:
                run_rollout_fused(env, policy, n, buffer=buf, obs_rows=obs_rows, generator=generator, chunk=n, greedy=greedy)
                fused = True
            except _ffi.BbxError as ex:                 # (refused before anything was queued: the class has no policy path)
                if ex.code != -5:
                    raise
                fused = False
                buf.t = 0
                run_rollout(env, policy, n, buffer=buf, obs_rows=obs_rows, generator=generator, sync_every=n, greedy=greedy)
        elif fused:
            run_rollout_fused(env, policy, n, buffer=buf, obs_rows=obs_rows, generator=generator, chunk=n, greedy=greedy)
        else:
            run_rollout(env, policy, n, buffer=buf, obs_rows=obs_rows, generator=generator, sync_every=n, greedy=greedy)
        d = buf.dones[:n]
        before = count.clone()
        ep_ret, ep_len = episode_returns(buf.rewards[:n], d, (cret, clen, count))
        ordinal = before.to(torch.int64)[None, :] + torch.cumsum(d.to(torch.int64), dim=0) - 1
        col = torch.where(d & (ordinal < episodes), ordinal, torch.full_like(ordinal, episodes)).t().contiguous()   # [B, n]
        returns.scatter_(1, col, ep_ret.t().contiguous())
        lengths.scatter_(1, col, ep_len.t().contiguous())
        steps += n
        finished = int(count.min())                     # the one host read of the chunk
    return Evaluation(returns[:, :episodes].contiguous(), lengths[:, :episodes].contiguous(), finished >= episodes, steps)
