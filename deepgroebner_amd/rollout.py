"""The consumer side of the batched environment: policy, trajectory buffer and rollout loop, all on the
device, replacing the per-step host round trip of the reference's agents.

    PMLPPolicy                 ParallelMultilayerPerceptron           networks.py:522-571 (:49-95, :414-460)
    discount_rewards, compute_advantages                              pg.py:20-76
    DeviceTrajectoryBuffer     TrajectoryBuffer (store/finish/get)    pg.py:79-240
    get_index + PMLPPolicy.evaluate_at   the update's minibatches as slices of an index list over the buffer: the training
                               kernels read the recorded states where the rollout left them (bbx_pmlp_logprob_at / bbx_pmlp_grad_at)
    PMLPPolicy.ppo_step_at, ppo_update   one minibatch of the update — forward, PPO loss, statistics, weight gradients — in one library
                               call (bbx_pmlp_ppo_grad_at / bbx_pmlp2_ppo_grad_at), and the epochs around it     pg.py _fit_policy_model
    PMLPValue, fill_values, value_update   a learned baseline (--value_model mlp, pg.py _fit_value_model): a critic over the recorded
                               state blocks — one launch for a whole buffer's values after the rollout (bbx_pmlp_value), one library
                               call per minibatch of the squared-error fit (bbx_pmlp_value_fit_at); run_rollout_fused(critic=...)
    run_rollout                PGAgent.run_episode(s)                 pg.py:451-503   (one library call per vector step)
    run_rollout_fused          the same with the policy INSIDE the step kernel, 256 vector steps per launch
    run_rollout(value_strategy=...)   env.value(strategy, gamma) before every step as the baseline   pg.py:461-465
                               (bbx_values_device: written on the device beside the steps); finish(): one GAE kernel
    act / run_rollout / run_rollout_fused (greedy=True)   the highest-probability pair at every step   pg.py run_episodes(greedy=True)
    episode_returns            one return and one length per episode from a rollout's rewards and dones (bbx_episodes_device)
    evaluate_policy            the first K episodes of every environment under a policy   scripts/eval.py

PyTorch is the plumbing here (device memory, autograd for training); the policy evaluation + sampling of the default
one-hidden-layer network runs in hand-written HIP: on the matrix cores, either as a kernel of its own fed by the padded
observation block (bbx_pmlp_act), in front of the step in the same launch (bbx_policy_step_device), or inside the step
loop (bbx_policy_rollout_device).  Two hidden layers of at most 128 units run inside the step loop too
(bbx_policy2_rollout_device) or as a kernel of their own (bbx_pmlp2_act), three as a kernel of their own (bbx_pmlp3_act); deeper
or wider networks take the torch path.  Actions never visit the host.
"""
import collections
import contextlib
import ctypes as C
import functools
import gc

import numpy as np
import torch

from . import _ffi


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


class _PMLPEvaluate(torch.autograd.Function):
    """log pi(a | s) and the entropy of pi(. | s) of a one-hidden-layer PMLPPolicy through bbx_pmlp_logprob, differentiable
    with respect to the four parameter tensors through bbx_pmlp_grad (the hidden activations are recomputed there: nothing of
    size [N, R, hidden] is kept between forward and backward).  No gradient for states, actions or rows.
    index (int32 [n], optional): the call is about the recorded states index[k] of states [..., R, cols], rows and actions, which
    are then whole buffers read in place (bbx_pmlp_logprob_at / bbx_pmlp_grad_at); the outputs have length n."""

    @staticmethod
    def forward(ctx, policy, states, rows, actions, w1, b1, w2, b2, index=None):
        R, cols = states.shape[-2:]
        S = rows.numel()
        N = S if index is None else index.numel()
        w = policy._fused_weights()
        logp = torch.empty(N, dtype=torch.float32, device=states.device)
        ent = torch.empty(N, dtype=torch.float32, device=states.device)
        p = lambda x: C.c_void_p(x.data_ptr())
        with torch.cuda.device(states.device):
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if index is None:
                _ffi.check(_ffi.lib().bbx_pmlp_logprob(p(states), p(rows), p(actions), N, R, cols, w["prepared"], w["hidden"], p(logp), p(ent), s))
            else:
                _ffi.check(_ffi.lib().bbx_pmlp_logprob_at(p(states), p(rows), p(actions), S, p(index), N, R, cols, w["prepared"], w["hidden"],
                                                          p(logp), p(ent), s))
        ctx.policy, ctx.prep, ctx.hidden = policy, w["keep"], w["hidden"]     # (the prepared weights of THIS forward pass)
        ctx.save_for_backward(states, rows, actions, w1, b1, w2, b2, index)
        return logp, ent

    @staticmethod
    def backward(ctx, glogp, gent):
        states, rows, actions, w1, b1, w2, b2, index = ctx.saved_tensors
        R, cols = states.shape[-2:]
        S = rows.numel()
        N = S if index is None else index.numel()
        hidden = ctx.hidden
        dev = states.device
        glogp = glogp.contiguous().float(); gent = gent.contiguous().float()
        gw1 = torch.empty((cols, hidden), dtype=torch.float32, device=dev)
        gb1 = torch.empty(hidden, dtype=torch.float32, device=dev)
        gw2 = torch.empty(hidden, dtype=torch.float32, device=dev)
        gb2 = torch.empty(1, dtype=torch.float32, device=dev)
        p = lambda x: C.c_void_p(x.data_ptr())
        with torch.cuda.device(dev):
            ws = ctx.policy._grad_workspace(N, R, cols, hidden, dev)
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if index is None:
                _ffi.check(_ffi.lib().bbx_pmlp_grad(p(states), p(rows), p(actions), N, R, cols, p(ctx.prep), hidden, p(glogp), p(gent), p(ws),
                                                    p(gw1), p(gb1), p(gw2), p(gb2), s))
            else:
                _ffi.check(_ffi.lib().bbx_pmlp_grad_at(p(states), p(rows), p(actions), S, p(index), N, R, cols, p(ctx.prep), hidden, p(glogp),
                                                       p(gent), p(ws), p(gw1), p(gb1), p(gw2), p(gb2), s))
        return None, None, None, None, gw1.t().to(w1.dtype), gb1.to(b1.dtype), gw2.view(1, -1).to(w2.dtype), gb2.to(b2.dtype), None


class _PMLP2Evaluate(torch.autograd.Function):
    """_PMLPEvaluate for two hidden layers: bbx_pmlp2_logprob forward, bbx_pmlp2_grad backward (both hidden tiles are recomputed
    there), gradients for the six parameter tensors in torch.nn.Linear's own layouts.  No gradient for states, actions or rows.
    index: as in _PMLPEvaluate (bbx_pmlp2_logprob_at / bbx_pmlp2_grad_at)."""

    @staticmethod
    def forward(ctx, policy, states, rows, actions, w1, b1, w2, b2, w3, b3, index=None):
        R, cols = states.shape[-2:]
        S = rows.numel()
        N = S if index is None else index.numel()
        logp = torch.empty(N, dtype=torch.float32, device=states.device)
        ent = torch.empty(N, dtype=torch.float32, device=states.device)
        p = lambda x: C.c_void_p(x.data_ptr())
        with torch.cuda.device(states.device):
            w = policy._deep_weights()
            h1, h2 = w["hidden"]
            # (the prepared buffer is refilled in place when the weights change: backward reads THIS forward pass's weights
            # from a copy of its own, made on the stream behind the fill)
            prep = w["keep"][0].clone()
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if index is None:
                _ffi.check(_ffi.lib().bbx_pmlp2_logprob(p(states), p(rows), p(actions), N, R, cols, p(prep), h1, h2, p(logp), p(ent), s))
            else:
                _ffi.check(_ffi.lib().bbx_pmlp2_logprob_at(p(states), p(rows), p(actions), S, p(index), N, R, cols, p(prep), h1, h2, p(logp),
                                                           p(ent), s))
        ctx.policy, ctx.prep, ctx.hidden = policy, prep, (h1, h2)
        ctx.save_for_backward(states, rows, actions, w1, b1, w2, b2, w3, b3, index)
        return logp, ent

    @staticmethod
    def backward(ctx, glogp, gent):
        states, rows, actions, w1, b1, w2, b2, w3, b3, index = ctx.saved_tensors
        R, cols = states.shape[-2:]
        S = rows.numel()
        N = S if index is None else index.numel()
        h1, h2 = ctx.hidden
        dev = states.device
        glogp = glogp.contiguous().float(); gent = gent.contiguous().float()
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        gw1, gb1, gw2, gb2, gw3, gb3 = new(cols, h1), new(h1), new(h1, h2), new(h2), new(h2), new(1)
        p = lambda x: C.c_void_p(x.data_ptr())
        with torch.cuda.device(dev):
            ws = ctx.policy._grad2_workspace(N, R, cols, h1, h2, dev)
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if index is None:
                _ffi.check(_ffi.lib().bbx_pmlp2_grad(p(states), p(rows), p(actions), N, R, cols, p(ctx.prep), h1, h2, p(glogp), p(gent), p(ws),
                                                     p(gw1), p(gb1), p(gw2), p(gb2), p(gw3), p(gb3), s))
            else:
                _ffi.check(_ffi.lib().bbx_pmlp2_grad_at(p(states), p(rows), p(actions), S, p(index), N, R, cols, p(ctx.prep), h1, h2, p(glogp),
                                                        p(gent), p(ws), p(gw1), p(gb1), p(gw2), p(gb2), p(gw3), p(gb3), s))
        return (None, None, None, None, gw1.t().to(w1.dtype), gb1.to(b1.dtype), gw2.t().to(w2.dtype), gb2.to(b2.dtype),
                gw3.view(1, -1).to(w3.dtype), gb3.to(b3.dtype), None)


class PMLPPolicy(torch.nn.Module):
    """ParallelMultilayerPerceptron(hidden_layers) of the reference: every row of the -1-padded [batch, rows, cols] int
    block is embedded by the same MLP (relu), scored by one linear unit, padded rows get -1e9, log-softmax over rows."""

    def __init__(self, cols, hidden_layers=(128,), deep_kernels=False):
        super().__init__()
        self.deep_kernels = deep_kernels                              # two hidden layers: evaluate through bbx_pmlp2_logprob / bbx_pmlp2_grad
        dims = [cols] + list(hidden_layers)
        self.embedding = torch.nn.ModuleList([torch.nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:])])
        self.deciding = torch.nn.Linear(dims[-1], 1)
        self.cols = cols

    def forward(self, batch):
        """int [B, R, cols] with -1 padding -> log-probabilities float32 [B, R] (about -1e9 on padded rows)."""
        mask = batch[:, :, -1] != -1                                  # ParallelEmbeddingLayer.compute_mask
        x = batch.to(torch.float32)
        for layer in self.embedding:
            x = torch.relu(layer(x))
        x = self.deciding(x).squeeze(-1)
        x = x + (~mask).to(torch.float32) * -1e9
        return torch.log_softmax(x, dim=-1)

    @torch.no_grad()
    def act(self, obs, rows, u, actions=None, logprobs=None, stream=None, greedy=False):
        """Sample one action per environment by inverse CDF from the uniforms u [B] -> (actions int32 [B], logprobs
        float32 [B]) on the device.  One hidden layer: the fused HIP kernel (bbx_pmlp_act); two or three hidden layers of at
        most 128 units: bbx_pmlp2_act / bbx_pmlp3_act; otherwise torch ops.
        greedy=True (evaluation, run_episodes(greedy=True) of pg.py): the highest-probability row, the first one on ties,
        through the *_act_greedy kernels; u is not read and may be None.  Shapes the kernels refuse and CPU tensors: act_torch."""
        B, R, cols = obs.shape
        if not obs.is_cuda:
            return self.act_torch(obs, rows, u, actions, logprobs, greedy=greedy)
        lib = _ffi.lib()
        uarg = () if greedy else (C.c_void_p(u.data_ptr()),)
        if actions is None:
            actions = torch.empty(B, dtype=torch.int32, device=obs.device)
        if logprobs is None:
            logprobs = torch.empty(B, dtype=torch.float32, device=obs.device)
        if len(self.embedding) == 1 and self.fused_ok(cols, self.embedding[0].out_features) and R <= 2048:   # (the kernels score <= 2048 rows)
            w = self._fused_weights()
            s = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
            fn = lib.bbx_pmlp_act_greedy if greedy else lib.bbx_pmlp_act
            _ffi.check(fn(C.c_void_p(obs.data_ptr()), C.c_void_p(rows.data_ptr()), B, R, cols, w["prepared"], w["hidden"],
                          *uarg, C.c_void_p(actions.data_ptr()), C.c_void_p(logprobs.data_ptr()), C.c_void_p(s)))
            return actions, logprobs
        if self.deep_ok(cols) and R <= self.deep_max_rows():
            w = self._deep_weights()
            s = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
            if greedy:
                fn = lib.bbx_pmlp2_act_greedy if len(w["hidden"]) == 2 else lib.bbx_pmlp3_act_greedy
            else:
                fn = lib.bbx_pmlp2_act if len(w["hidden"]) == 2 else lib.bbx_pmlp3_act
            _ffi.check(fn(C.c_void_p(obs.data_ptr()), C.c_void_p(rows.data_ptr()), B, R, cols, w["prepared"], *w["hidden"],
                          *uarg, C.c_void_p(actions.data_ptr()), C.c_void_p(logprobs.data_ptr()), C.c_void_p(s)))
            return actions, logprobs
        return self.act_torch(obs, rows, u, actions, logprobs, greedy=greedy)

    def deep_ok(self, cols):
        """Two or three hidden layers of at most 128 units: the shapes bbx_pmlp2_act / bbx_pmlp3_act are built for."""
        return len(self.embedding) in (2, 3) and all(1 <= l.out_features <= 128 for l in self.embedding) and 1 <= cols <= 64

    def deep_max_rows(self):
        """Rows per environment the two- / three-layer kernels score: the logits of a wave's environment live in LDS beside the
        staged weights — 2048 rows, 1024 where three layers wider than 64 units (128 KB of weights) leave less room."""
        return 1024 if len(self.embedding) == 3 and max(l.out_features for l in self.embedding) > 64 else 2048

    def _deep_weights(self):
        """The two- / three-layer kernel's view of the weights (bbx_pmlp2_prepare / bbx_pmlp3_prepare), rebuilt only when a
        parameter changed, in the same buffer (a recorded graph keeps reading it)."""
        key = tuple(p._version for p in self.parameters()) + tuple(p.data_ptr() for p in self.parameters())
        c = self.__dict__.get("_deep_cache")
        if c is None or c["key"] != key:
            cols = self.embedding[0].in_features
            hidden = [l.out_features for l in self.embedding]
            t = []
            for l in self.embedding:
                t += [l.weight.detach().t().contiguous().float(), l.bias.detach().contiguous().float()]
            t += [self.deciding.weight.detach().reshape(-1).contiguous().float(), self.deciding.bias.detach().reshape(-1).contiguous().float()]
            lib = _ffi.lib()
            nfl = lib.bbx_pmlp2_prepared_floats(cols, *hidden) if len(hidden) == 2 else lib.bbx_pmlp3_prepared_floats(cols, *hidden)
            _ffi.check(min(nfl, 0))
            prep = c["keep"][0] if c is not None and c["keep"][0].numel() == nfl and c["keep"][0].device == t[0].device else \
                torch.empty(nfl, dtype=torch.float32, device=t[0].device)
            prepare = lib.bbx_pmlp2_prepare if len(hidden) == 2 else lib.bbx_pmlp3_prepare
            _ffi.check(prepare(*[C.c_void_p(x.data_ptr()) for x in t], cols, *hidden, C.c_void_p(prep.data_ptr()),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            c = {"key": key, "keep": (prep, t), "prepared": C.c_void_p(prep.data_ptr()), "hidden": hidden}
            self.__dict__["_deep_cache"] = c
        return c

    @staticmethod
    def fused_ok(cols, hidden):
        """Shapes the policy kernel is built for (bbx_pmlp_prepared_floats >= 0)."""
        return 1 <= hidden <= 256 and 1 <= cols <= 64

    def _fused_weights(self):
        """The kernels' view of the weights (bbx_pmlp_prepare: transposed, zero-padded to the tile sizes), rebuilt only when
        a parameter changed (an optimiser step bumps the tensors' version counters): no per-step transposes, no per-step
        host read of b2.  One hidden layer only: the layout has no room for a second."""
        if len(self.embedding) != 1:
            raise ValueError("_fused_weights: the one-layer kernels' weights of a policy with %d hidden layers (two: _deep_weights)" % len(self.embedding))
        lin = self.embedding[0]
        key = tuple(p._version for p in self.parameters()) + tuple(p.data_ptr() for p in self.parameters())
        c = self.__dict__.get("_fused_cache")
        if c is None or c["key"] != key:
            cols, hidden = lin.in_features, lin.out_features
            w1 = lin.weight.detach().t().contiguous().float()
            b1 = lin.bias.detach().contiguous().float()
            w2 = self.deciding.weight.detach().reshape(-1).contiguous().float()
            nfl = _ffi.lib().bbx_pmlp_prepared_floats(cols, hidden)
            _ffi.check(min(nfl, 0))
            prep = torch.empty(nfl, dtype=torch.float32, device=w1.device)
            # (b2 travels by value in the C call; reading it back would make every optimiser step wait for the device: the call gets
            # 0 and the bias is copied on the device into its place, the first of the layout's last four floats)
            _ffi.check(_ffi.lib().bbx_pmlp_prepare(C.c_void_p(w1.data_ptr()), C.c_void_p(b1.data_ptr()), C.c_void_p(w2.data_ptr()),
                                                   C.c_float(0.0), cols, hidden, C.c_void_p(prep.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            prep[nfl - 4:nfl - 3].copy_(self.deciding.bias.detach().reshape(1))
            c = {"key": key, "keep": prep, "prepared": C.c_void_p(prep.data_ptr()), "hidden": hidden}
            self.__dict__["_fused_cache"] = c
        return c

    def _grad_workspace(self, N, R, cols, hidden, device):
        """The workspace of bbx_pmlp_grad, kept between calls (it grows only; calls on one stream run in order)."""
        nfl = _ffi.lib().bbx_pmlp_grad_workspace_floats(N, R, cols, hidden)
        _ffi.check(min(nfl, 0))
        ws = self.__dict__.get("_grad_ws")
        if ws is None or ws.numel() < nfl or ws.device != device:
            ws = torch.empty(nfl, dtype=torch.float32, device=device)
            self.__dict__["_grad_ws"] = ws
        return ws

    def _grad2_workspace(self, N, R, cols, h1, h2, device):
        """The workspace of bbx_pmlp2_grad, kept between calls (it grows only; calls on one stream run in order)."""
        nfl = _ffi.lib().bbx_pmlp2_grad_workspace_floats(N, R, cols, h1, h2)
        _ffi.check(min(nfl, 0))
        ws = self.__dict__.get("_grad2_ws")
        if ws is None or ws.numel() < nfl or ws.device != device:
            ws = torch.empty(nfl, dtype=torch.float32, device=device)
            self.__dict__["_grad2_ws"] = ws
        return ws

    @staticmethod
    def _row_counts(states, rows):
        return (states[:, :, -1] != -1).sum(1).to(torch.int32) if rows is None else rows

    def evaluate(self, states, actions, rows=None):
        """The training-time view of recorded experience (pg.py _fit_policy_model): states int [N, R, cols], actions [N] ->
        (logprobs float32 [N] of the recorded actions, entropy float32 [N] of the distribution over each state's rows),
        differentiable with respect to the module's parameters.  rows [N]: the live rows per state (None: those whose last
        column is not -1, as forward masks).  No live rows: 0.0 and 0.0; an action outside the live rows: NaN.
        One hidden layer on the GPU: the HIP kernels bbx_pmlp_logprob / bbx_pmlp_grad; two hidden layers of at most 128 units
        on the GPU with deep_kernels set: bbx_pmlp2_logprob / bbx_pmlp2_grad; otherwise evaluate_torch."""
        N, R, cols = states.shape
        lin = self.embedding[0]
        if (states.is_cuda and len(self.embedding) == 1 and lin.weight.is_cuda and lin.weight.dtype == torch.float32
                and self.fused_ok(cols, lin.out_features) and 1 <= R <= 2048):
            rows = self._row_counts(states, rows).to(torch.int32).contiguous()
            st = states if states.dtype == torch.int32 else states.to(torch.int32)
            return _PMLPEvaluate.apply(self, st.contiguous(), rows, actions.to(torch.int32).contiguous(), lin.weight, lin.bias,
                                       self.deciding.weight, self.deciding.bias)
        if (self.deep_kernels and states.is_cuda and len(self.embedding) == 2 and self.deep_ok(cols) and 1 <= R <= 2048
                and all(q.is_cuda and q.dtype == torch.float32 for q in self.parameters())):
            rows = self._row_counts(states, rows).to(torch.int32).contiguous()
            st = states if states.dtype == torch.int32 else states.to(torch.int32)
            l2 = self.embedding[1]
            return _PMLP2Evaluate.apply(self, st.contiguous(), rows, actions.to(torch.int32).contiguous(), lin.weight, lin.bias, l2.weight, l2.bias,
                                        self.deciding.weight, self.deciding.bias)
        return self.evaluate_torch(states, actions, rows)

    def evaluate_at(self, states, actions, rows, index):
        """evaluate() of the recorded states index[k] WITHOUT gathering them: states int [S, R, cols] or [T, B, R, cols] with
        actions and rows [S] or [T, B] are whole buffers (DeviceTrajectoryBuffer.states / .actions / .rows as the rollout kernels
        left them), index int [n] holds flat step numbers into them (DeviceTrajectoryBuffer.get_index) -> (logprobs float32 [n],
        entropy float32 [n]), differentiable with respect to the module's parameters; for an index in range, the numbers of
        evaluate(states[index], actions[index], rows[index]) bit for bit.  An index outside the buffer on the kernel path: NaN
        and NaN, nothing for the gradients.
        The kernels (bbx_pmlp_logprob_at / bbx_pmlp_grad_at, bbx_pmlp2_..._at) read the buffers in place: under evaluate()'s
        conditions, and only where states, rows and actions ARE contiguous int32 CUDA tensors already — a buffer is never
        converted or copied as a whole.  Anything else gathers the n states and takes evaluate()."""
        lin = self.embedding[0]
        depth = self._in_place_depth(states, actions, rows)
        if depth:
            idx = index.to(device=states.device, dtype=torch.int32).contiguous()
            if depth == 1:
                return _PMLPEvaluate.apply(self, states, rows, actions, lin.weight, lin.bias, self.deciding.weight, self.deciding.bias, idx)
            l2 = self.embedding[1]
            return _PMLP2Evaluate.apply(self, states, rows, actions, lin.weight, lin.bias, l2.weight, l2.bias, self.deciding.weight, self.deciding.bias, idx)
        j = index.to(device=states.device, dtype=torch.int64)
        if states.dim() == 4:                                         # (no reshape: a non-contiguous buffer would be copied whole)
            t, b = j // states.shape[1], j % states.shape[1]
            return self.evaluate(states[t, b], actions[t, b], rows[t, b])
        return self.evaluate(states[j], actions[j], rows[j])

    def _in_place_depth(self, states, actions, rows):
        """1 or 2 where the training kernels of that many hidden layers can read states [..., R, cols], actions and rows where they
        lie (evaluate()'s conditions, and contiguous int32 CUDA tensors of matching sizes); 0: they cannot."""
        R, cols = states.shape[-2:]
        lin = self.embedding[0]
        S = rows.numel()
        in_place = (states.is_cuda and 1 <= R <= 2048 and states.numel() == S * R * cols and actions.numel() == S
                    and all(x.is_cuda and x.dtype == torch.int32 and x.is_contiguous() for x in (states, rows, actions)))
        if not in_place:
            return 0
        if len(self.embedding) == 1 and lin.weight.is_cuda and lin.weight.dtype == torch.float32 and self.fused_ok(cols, lin.out_features):
            return 1
        if (self.deep_kernels and len(self.embedding) == 2 and self.deep_ok(cols)
                and all(q.is_cuda and q.dtype == torch.float32 for q in self.parameters())):
            return 2
        return 0

    LOSS_MODES = {"pg": 0, "clip": 1, "penalty": 2}

    def ppo_step_at(self, states, actions, rows, index, old_logprobs, advantages, clip=0.2, ent_coef=0.0, mode="clip", c_kl=0.0):
        """One minibatch of the policy update (pg.py _fit_policy_model) in one library call: from the recorded states index[k] of
        the buffers states / actions / rows (as evaluate_at takes them), the rollout's log-probabilities old_logprobs [n] and the
        advantages [n] to the gradients of
            L = -mean_k u_k - ent_coef mean_k H_k
            u_k = logprob_k A_k                                         mode "pg"
                  min(r_k A_k, clamp(r_k, 1 - clip, 1 + clip) A_k)      mode "clip"       (r_k = exp(logprob_k - old_k))
                  r_k A_k - c_kl (old_k - logprob_k)                    mode "penalty"
        ADDED to the parameters' .grad as loss.backward() would (None becomes the tensor), in torch.nn.Linear's layouts.  The means
        are over the n positions (scale 1 / n); a position whose log-probability is NaN (index out of range, action outside the live
        rows) contributes nothing.  Returns (stats float64 [6] on the device: counted positions, sum u, sum H, sum (old - new),
        positions clipped, positions not counted; logprobs float32 [n]; entropy float32 [n]) — nothing is read back, nothing waits.
        Under evaluate_at's conditions for the kernels: bbx_pmlp_ppo_grad_at / bbx_pmlp2_ppo_grad_at (no autograd, no torch op over
        the n positions); anywhere else the same formulae with torch ops through evaluate_at and backward()."""
        depth = self._in_place_depth(states, actions, rows)
        if depth:
            idx = index.to(device=states.device, dtype=torch.int32).contiguous()
            return self._ppo_kernels(depth, states, rows, actions, idx, old_logprobs, advantages, clip, ent_coef, mode, c_kl)
        return self._ppo_torch(self.evaluate_at(states, actions, rows, index), old_logprobs, advantages, clip, ent_coef, mode, c_kl)

    def ppo_step(self, states, actions, rows=None, old_logprobs=None, advantages=None, clip=0.2, ent_coef=0.0, mode="clip", c_kl=0.0):
        """ppo_step_at for gathered tensors, as evaluate takes them: states int [N, R, cols], actions [N], rows [N] (None: the rows
        whose last column is not -1) — bbx_pmlp_ppo_grad / bbx_pmlp2_ppo_grad under evaluate()'s conditions for the kernels."""
        N, R, cols = states.shape
        lin = self.embedding[0]
        depth = 0
        if states.is_cuda and 1 <= R <= 2048:
            if len(self.embedding) == 1 and lin.weight.is_cuda and lin.weight.dtype == torch.float32 and self.fused_ok(cols, lin.out_features):
                depth = 1
            elif (self.deep_kernels and len(self.embedding) == 2 and self.deep_ok(cols)
                  and all(q.is_cuda and q.dtype == torch.float32 for q in self.parameters())):
                depth = 2
        if depth:
            rows = self._row_counts(states, rows).to(torch.int32).contiguous()
            st = states if states.dtype == torch.int32 else states.to(torch.int32)
            return self._ppo_kernels(depth, st.contiguous(), rows, actions.to(torch.int32).contiguous(), None, old_logprobs, advantages, clip,
                                     ent_coef, mode, c_kl)
        return self._ppo_torch(self.evaluate(states, actions, rows), old_logprobs, advantages, clip, ent_coef, mode, c_kl)

    def _ppo_workspace(self, depth, N, R, cols, hidden, device):
        """The workspace of bbx_pmlp_ppo_grad / bbx_pmlp2_ppo_grad, kept between calls (it grows only; calls on one stream run in
        order)."""
        lib = _ffi.lib()
        nfl = lib.bbx_pmlp_ppo_workspace_floats(N, R, cols, *hidden) if depth == 1 else lib.bbx_pmlp2_ppo_workspace_floats(N, R, cols, *hidden)
        _ffi.check(min(nfl, 0))
        ws = self.__dict__.get("_ppo_ws")
        if ws is None or ws.numel() < nfl or ws.device != device:
            ws = torch.empty(nfl, dtype=torch.float32, device=device)
            self.__dict__["_ppo_ws"] = ws
        return ws

    def _ppo_kernels(self, depth, states, rows, actions, index, old_logprobs, advantages, clip, ent_coef, mode, c_kl):
        R, cols = states.shape[-2:]
        S = rows.numel()
        N = S if index is None else index.numel()
        dev = states.device
        old = old_logprobs.to(device=dev, dtype=torch.float32).contiguous()
        adv = advantages.to(device=dev, dtype=torch.float32).contiguous()
        if old.numel() != N or adv.numel() != N:
            raise ValueError("ppo_step: %d positions, %d old log-probabilities, %d advantages" % (N, old.numel(), adv.numel()))
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        logp, ent, coef = new(N), new(N), new(2 * N)
        stats = torch.empty(6, dtype=torch.float64, device=dev)
        p = lambda x: C.c_void_p(x.data_ptr())
        loss = (self.LOSS_MODES[mode], C.c_float(1.0 / N if N else 0.0), C.c_float(clip), C.c_float(ent_coef), C.c_float(c_kl))
        lib = _ffi.lib()
        with torch.cuda.device(dev):
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            src = (p(states), p(rows), p(actions)) + ((N,) if index is None else (S, p(index), N)) + (R, cols)
            if depth == 1:
                w = self._fused_weights()
                hidden = (w["hidden"],)
                grads = [new(cols, hidden[0]), new(hidden[0]), new(hidden[0]), new(1)]
                fn = lib.bbx_pmlp_ppo_grad if index is None else lib.bbx_pmlp_ppo_grad_at
            else:
                w = self._deep_weights()
                hidden = tuple(w["hidden"])
                grads = [new(cols, hidden[0]), new(hidden[0]), new(hidden[0], hidden[1]), new(hidden[1]), new(hidden[1]), new(1)]
                fn = lib.bbx_pmlp2_ppo_grad if index is None else lib.bbx_pmlp2_ppo_grad_at
            ws = self._ppo_workspace(depth, N, R, cols, hidden, dev)
            _ffi.check(fn(*src, w["prepared"], *hidden, p(old), p(adv), *loss, p(logp), p(ent), p(coef), p(stats), p(ws), *[p(g) for g in grads], s))
        # torch.nn.Linear's layouts, added as backward() would
        lin = self.embedding[0]
        if depth == 1:
            params = (lin.weight, lin.bias, self.deciding.weight, self.deciding.bias)
            shaped = (grads[0].t(), grads[1], grads[2].view(1, -1), grads[3])
        else:
            l2 = self.embedding[1]
            params = (lin.weight, lin.bias, l2.weight, l2.bias, self.deciding.weight, self.deciding.bias)
            shaped = (grads[0].t(), grads[1], grads[2].t(), grads[3], grads[4].view(1, -1), grads[5])
        for q, g in zip(params, shaped):
            if q.grad is None:
                q.grad = g.contiguous()
            else:
                q.grad.add_(g)
        return stats, logp, ent

    def _ppo_torch(self, evaluated, old_logprobs, advantages, clip, ent_coef, mode, c_kl):
        """The loss epilogue of the kernels with torch ops, float32 in the same order, and backward() through `evaluated`."""
        logp, ent = evaluated
        kind = self.LOSS_MODES[mode]
        n = logp.numel()
        old = old_logprobs.to(device=logp.device, dtype=torch.float32)
        A = advantages.to(device=logp.device, dtype=torch.float32)
        counted = ~torch.isnan(logp)
        new = torch.where(counted, logp, old.detach())               # (a NaN must not reach exp: 0 * NaN in its backward)
        r = torch.exp(new - old)
        clipped = torch.zeros_like(counted)
        if kind == 0:
            u = new * A
        elif kind == 1:
            a, b = r * A, torch.clamp(r, 1.0 - clip, 1.0 + clip) * A
            u = torch.min(a, b)
            clipped = (a > b) & counted
        else:
            u = r * A - c_kl * (old - new)
        zero = torch.zeros_like(u)
        u = torch.where(counted, u, zero); H = torch.where(counted, ent, zero)
        if n:
            loss = -u.mean() - ent_coef * H.mean()
            if loss.requires_grad:
                loss.backward()
        d = lambda x: x.detach().to(torch.float64).sum()
        stats = torch.stack([d(counted), d(u), d(H), d(torch.where(counted, old - new, zero)), d(clipped), d(~counted)])
        return stats, logp.detach(), ent.detach()

    def evaluate_torch(self, states, actions, rows=None):
        """evaluate with torch ops and autograd (any depth, any device; the baseline of the kernels): forward, gather, and
        -(exp(lp) lp) summed over the live rows."""
        N, R, _ = states.shape
        if rows is None:
            lp = self.forward(states)
            live = states[:, :, -1] != -1
        else:                                                         # (the count masks, whatever the rows beyond it hold)
            live = torch.arange(R, device=states.device)[None, :] < torch.clamp(rows.to(torch.int64), 0, R)[:, None]
            lg = self._logits(states)
            lp = torch.log_softmax(torch.where(live, lg, torch.full_like(lg, -1e9)), dim=-1)
        n = live.sum(1)
        a = actions.to(torch.int64)
        ok = (a >= 0) & (a < n)
        picked = lp.gather(1, torch.where(ok, a, torch.zeros_like(a))[:, None]).squeeze(1)
        zero = torch.zeros_like(picked)
        logp = torch.where(n > 0, torch.where(ok, picked, torch.full_like(picked, float("nan"))), zero)
        lpl = torch.where(live, lp, torch.zeros_like(lp))
        ent = torch.where(n > 0, -(torch.exp(lpl) * lpl * live.to(lp.dtype)).sum(dim=1), zero)
        return logp, ent

    def _logits(self, batch):
        x = batch.to(self.deciding.weight.dtype)
        for layer in self.embedding:
            x = torch.relu(layer(x))
        return self.deciding(x).squeeze(-1)

    def act_torch(self, obs, rows, u, actions=None, logprobs=None, greedy=False):
        """The same draw with torch ops (the reference of the fused kernel; any depth).  greedy=True: the argmax over the live
        rows, the first index on ties (u unused, may be None)."""
        lp = self.forward(obs)
        n = torch.clamp(rows, max=obs.shape[1]).to(torch.int64)
        valid = torch.arange(obs.shape[1], device=obs.device)[None, :] < n[:, None]
        if greedy:
            best = torch.where(valid, lp, torch.full_like(lp, float("-inf")))
            top = best.max(dim=1, keepdim=True).values
            a = ((best == top) & valid).to(torch.int64).argmax(dim=1)   # (0 / 1 flags: argmax returns the first 1; no live row: 0)
        else:
            p = torch.where(valid, torch.exp(lp - lp.max(dim=1, keepdim=True).values), torch.zeros_like(lp))
            cdf = torch.cumsum(p, dim=1)
            target = u * cdf[:, -1]
            a = torch.minimum((cdf <= target[:, None]).sum(dim=1), n - 1).clamp(min=0)
        out_a = a.to(torch.int32)
        out_l = lp.gather(1, a[:, None]).squeeze(1)
        if actions is not None:
            actions.copy_(out_a); out_a = actions
        if logprobs is not None:
            logprobs.copy_(out_l); out_l = logprobs
        return out_a, out_l


class _PMLPValueEvaluate(torch.autograd.Function):
    """The values of a one-hidden-layer PMLPValue through bbx_pmlp_value, differentiable with respect to the four parameter tensors
    through bbx_pmlp_value_grad (the hidden activations are recomputed there).  No gradient for states or rows.
    index (int32 [n], optional): as in _PMLPEvaluate — states and rows are whole buffers read in place (bbx_pmlp_value_at /
    bbx_pmlp_value_grad_at), the output has length n."""

    @staticmethod
    def forward(ctx, critic, states, rows, w1, b1, w2, b2, index=None):
        R, cols = states.shape[-2:]
        S = rows.numel()
        N = S if index is None else index.numel()
        values = torch.empty(N, dtype=torch.float32, device=states.device)
        p = lambda x: C.c_void_p(x.data_ptr())
        with torch.cuda.device(states.device):
            w = critic._fused_weights()
            # (the prepared buffer is refilled in place when the weights change: backward reads THIS forward pass's weights from a
            # copy of its own, made on the stream behind the fill)
            prep = w["keep"].clone()
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            src = (p(states), p(rows)) + ((N,) if index is None else (S, p(index), N)) + (R, cols)
            fn = _ffi.lib().bbx_pmlp_value if index is None else _ffi.lib().bbx_pmlp_value_at
            _ffi.check(fn(*src, p(prep), w["hidden"], critic.pool_id, p(values), None, s))
        ctx.critic, ctx.prep, ctx.hidden, ctx.pool = critic, prep, w["hidden"], critic.pool_id
        ctx.save_for_backward(states, rows, w1, b1, w2, b2, index)
        return values

    @staticmethod
    def backward(ctx, gvalue):
        states, rows, w1, b1, w2, b2, index = ctx.saved_tensors
        R, cols = states.shape[-2:]
        S = rows.numel()
        N = S if index is None else index.numel()
        hidden = ctx.hidden
        dev = states.device
        gvalue = gvalue.contiguous().float()
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        gw1, gb1, gw2, gb2 = new(cols, hidden), new(hidden), new(hidden), new(1)
        p = lambda x: C.c_void_p(x.data_ptr())
        with torch.cuda.device(dev):
            ws = ctx.critic._workspace("grad", N, R, cols, hidden, dev)
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            src = (p(states), p(rows)) + ((N,) if index is None else (S, p(index), N)) + (R, cols)
            fn = _ffi.lib().bbx_pmlp_value_grad if index is None else _ffi.lib().bbx_pmlp_value_grad_at
            _ffi.check(fn(*src, p(ctx.prep), hidden, ctx.pool, p(gvalue), p(ws), p(gw1), p(gb1), p(gw2), p(gb2), s))
        return None, None, None, gw1.t().to(w1.dtype), gb1.to(b1.dtype), gw2.view(1, -1).to(w2.dtype), gb2.to(b2.dtype), None


class PMLPValue(torch.nn.Module):
    """A learned value baseline (critic) over the observation block: the row embedding of PMLPPolicy (`embedding`, relu), one
    linear unit per row (`head`), and a pool over a state's live rows in place of the softmax:
        pool="sum"   V = sum_r z_r        pool="mean"   V = that sum / n        pool="lse"   V = log sum_r exp z_r
    A state without live rows is worth 0.  One hidden layer of at most 256 units over at most 64 columns, float32 on the GPU: the
    HIP kernels (bbx_pmlp_value / bbx_pmlp_value_grad / bbx_pmlp_value_fit and their _at forms, which read a trajectory buffer in
    place); CPU tensors, more hidden layers or wider ones: the torch path (forward, values_torch, evaluate_torch).  `last_path`
    names the path the last call took ("kernels" or "torch")."""

    POOLS = {"sum": 0, "mean": 1, "lse": 2}                           # BBX_POOL_* of include/bbx.h

    def __init__(self, cols, hidden_layers=(128,), pool="sum"):
        super().__init__()
        if pool not in self.POOLS:
            raise ValueError("PMLPValue: pool is one of %s (got %r)" % (sorted(self.POOLS), pool))
        dims = [cols] + list(hidden_layers)
        self.embedding = torch.nn.ModuleList([torch.nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:])])
        self.head = torch.nn.Linear(dims[-1], 1)
        self.cols, self.pool, self.pool_id = cols, pool, self.POOLS[pool]
        self.last_path = None

    # ---- the torch path
    def _scores(self, batch):
        x = batch.to(self.head.weight.dtype)
        for layer in self.embedding:
            x = torch.relu(layer(x))
        return self.head(x).squeeze(-1)

    def evaluate_torch(self, states, rows=None):
        """Values float [N] of states int [N, R, cols] with torch ops and autograd (any depth, any device; the baseline of the
        kernels).  rows [N]: the live rows per state (None: those whose last column is not -1)."""
        self.last_path = "torch"
        N, R, _ = states.shape
        if rows is None:
            live = states[:, :, -1] != -1
        else:                                                         # (the count masks, whatever the rows beyond it hold)
            live = torch.arange(R, device=states.device)[None, :] < torch.clamp(rows.to(torch.int64), 0, R)[:, None]
        z = self._scores(states)
        n = live.sum(1)
        zero = torch.zeros_like(z)
        if self.pool == "lse":
            v = torch.logsumexp(torch.where(live, z, torch.full_like(z, -1e9)), dim=1)
        else:
            v = torch.where(live, z, zero).sum(dim=1)
            if self.pool == "mean":
                v = v / torch.clamp(n, min=1).to(v.dtype)
        return torch.where(n > 0, v, torch.zeros_like(v))

    def forward(self, batch):
        """int [B, R, cols] with -1 padding -> values [B]."""
        return self.evaluate_torch(batch)

    @torch.no_grad()
    def values_torch(self, states, rows=None, out=None, out64=None):
        R, cols = states.shape[-2:]
        v = self.evaluate_torch(states.reshape(-1, R, cols), None if rows is None else rows.reshape(-1))
        return self._deliver(v, out, out64)

    @staticmethod
    def _deliver(v, out, out64):
        if out64 is not None:
            out64.view(-1).copy_(v.to(torch.float64))
        if out is not None:
            out.view(-1).copy_(v)
        return out if out is not None else (out64 if out64 is not None else v)

    # ---- the kernels
    def kernels_ok(self, states):
        """Whether the HIP kernels take states [..., R, cols] with this module's weights (otherwise: the torch path)."""
        R, cols = states.shape[-2:]
        lin = self.embedding[0]
        return (states.is_cuda and len(self.embedding) == 1 and lin.weight.is_cuda and lin.weight.dtype == torch.float32
                and PMLPPolicy.fused_ok(cols, lin.out_features) and 1 <= R <= 2048)

    def _in_place(self, states, rows):
        """Whether the _at kernels can read states [..., R, cols] and rows where they lie (contiguous int32 CUDA tensors of
        matching sizes): a buffer is never converted or copied as a whole."""
        R, cols = states.shape[-2:]
        return (self.kernels_ok(states) and states.numel() == rows.numel() * R * cols
                and all(x.is_cuda and x.dtype == torch.int32 and x.is_contiguous() for x in (states, rows)))

    def _fused_weights(self):
        """The kernels' view of the weights (bbx_pmlp_prepare, the one-layer policy's layout), rebuilt only when a parameter
        changed (an optimiser step bumps the tensors' version counters), in the same buffer."""
        if len(self.embedding) != 1:
            raise ValueError("_fused_weights: the kernels take one hidden layer (this critic has %d)" % len(self.embedding))
        lin = self.embedding[0]
        key = tuple(p._version for p in self.parameters()) + tuple(p.data_ptr() for p in self.parameters())
        c = self.__dict__.get("_fused_cache")
        if c is None or c["key"] != key:
            cols, hidden = lin.in_features, lin.out_features
            w1 = lin.weight.detach().t().contiguous().float()
            b1 = lin.bias.detach().contiguous().float()
            w2 = self.head.weight.detach().reshape(-1).contiguous().float()
            nfl = _ffi.lib().bbx_pmlp_prepared_floats(cols, hidden)
            _ffi.check(min(nfl, 0))
            prep = c["keep"] if c is not None and c["keep"].numel() == nfl and c["keep"].device == w1.device else \
                torch.empty(nfl, dtype=torch.float32, device=w1.device)
            # (b2 travels by value in the C call; reading it back would make every optimiser step wait for the device: the call gets
            # 0 and the bias is copied on the device into its place, the first of the layout's last four floats)
            _ffi.check(_ffi.lib().bbx_pmlp_prepare(C.c_void_p(w1.data_ptr()), C.c_void_p(b1.data_ptr()), C.c_void_p(w2.data_ptr()),
                                                   C.c_float(0.0), cols, hidden, C.c_void_p(prep.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            prep[nfl - 4:nfl - 3].copy_(self.head.bias.detach().reshape(1))
            c = {"key": key, "keep": prep, "prepared": C.c_void_p(prep.data_ptr()), "hidden": hidden}
            self.__dict__["_fused_cache"] = c
        return c

    def _workspace(self, kind, N, R, cols, hidden, device):
        """The workspace of bbx_pmlp_value_grad ("grad") / bbx_pmlp_value_fit ("fit"), kept between calls (it grows only; calls on
        one stream run in order)."""
        lib = _ffi.lib()
        nfl = (lib.bbx_pmlp_value_fit_workspace_floats if kind == "fit" else lib.bbx_pmlp_value_grad_workspace_floats)(N, R, cols, hidden)
        _ffi.check(min(nfl, 0))
        ws = self.__dict__.get("_ws")
        if ws is None or ws.numel() < nfl or ws.device != device:
            ws = torch.empty(nfl, dtype=torch.float32, device=device)
            self.__dict__["_ws"] = ws
        return ws

    @staticmethod
    def _row_counts(states, rows):
        return (states[:, :, -1] != -1).sum(1).to(torch.int32) if rows is None else rows

    def _value_call(self, states, rows, index, out, out64):
        R, cols = states.shape[-2:]
        S = rows.numel()
        N = S if index is None else index.numel()
        dev = states.device
        if out is None and out64 is None:
            out = torch.empty(N, dtype=torch.float32, device=dev)
        for o, dt in ((out, torch.float32), (out64, torch.float64)):
            if o is not None and not (o.is_cuda and o.dtype == dt and o.is_contiguous() and o.numel() == N):
                raise ValueError("PMLPValue.values: out / out64 are contiguous float32 / float64 CUDA tensors of %d elements" % N)
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        with torch.cuda.device(dev):
            w = self._fused_weights()
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            src = (p(states), p(rows)) + ((N,) if index is None else (S, p(index), N)) + (R, cols)
            fn = _ffi.lib().bbx_pmlp_value if index is None else _ffi.lib().bbx_pmlp_value_at
            _ffi.check(fn(*src, w["prepared"], w["hidden"], self.pool_id, p(out), p(out64), s))
        self.last_path = "kernels"
        return out if out is not None else out64

    @torch.no_grad()
    def values(self, states, rows, out=None, out64=None):
        """Values of states int [..., R, cols] with rows [...] live rows each, no autograd: float32 into `out` and / or the same
        numbers widened into `out64` (float64: what DeviceTrajectoryBuffer.values holds), each of rows.numel() elements; neither:
        a new float32 tensor.  Returns out (out64 where only that was given).  On the GPU under kernels_ok: one bbx_pmlp_value
        call, over the tensors in place where they are contiguous int32; otherwise values_torch."""
        if not self.kernels_ok(states):
            return self.values_torch(states, rows, out, out64)
        R, cols = states.shape[-2:]
        st = (states if states.dtype == torch.int32 else states.to(torch.int32)).contiguous()
        rw = self._row_counts(st.view(-1, R, cols), None if rows is None else rows.reshape(-1)).to(torch.int32).contiguous()
        return self._value_call(st, rw, None, out, out64)

    @torch.no_grad()
    def values_at(self, states, rows, index, out=None, out64=None):
        """values() of the recorded states index[k] of the buffers states [S, R, cols] or [T, B, R, cols] and rows, read in place
        (bbx_pmlp_value_at; an index outside the buffer: NaN); where the kernels cannot read them in place the n states are
        gathered."""
        if self._in_place(states, rows):
            return self._value_call(states, rows, index.to(device=states.device, dtype=torch.int32).contiguous(), out, out64)
        st, rw = self._gather(states, rows, index)
        return self.values(st, rw, out, out64)

    @staticmethod
    def _gather(states, rows, index):
        R, cols = states.shape[-2:]
        j = index.to(device=states.device, dtype=torch.int64)
        if states.dim() == 4:                                         # (no reshape: a non-contiguous buffer would be copied whole)
            t, b = j // states.shape[1], j % states.shape[1]
            return states[t, b], rows[t, b]
        return states[j], rows[j]

    def evaluate(self, states, rows=None):
        """Values float32 [N] of states int [N, R, cols], differentiable with respect to the module's parameters: under kernels_ok
        bbx_pmlp_value forward and bbx_pmlp_value_grad backward; otherwise evaluate_torch."""
        if not self.kernels_ok(states):
            return self.evaluate_torch(states, rows)
        rows = self._row_counts(states, rows).to(torch.int32).contiguous()
        st = states if states.dtype == torch.int32 else states.to(torch.int32)
        self.last_path = "kernels"
        lin = self.embedding[0]
        return _PMLPValueEvaluate.apply(self, st.contiguous(), rows, lin.weight, lin.bias, self.head.weight, self.head.bias)

    def evaluate_at(self, states, rows, index):
        """evaluate() of the recorded states index[k] without gathering them (bbx_pmlp_value_at / bbx_pmlp_value_grad_at), as
        PMLPPolicy.evaluate_at; where the kernels cannot read the buffers in place the n states are gathered."""
        if self._in_place(states, rows):
            self.last_path = "kernels"
            lin = self.embedding[0]
            idx = index.to(device=states.device, dtype=torch.int32).contiguous()
            return _PMLPValueEvaluate.apply(self, states, rows, lin.weight, lin.bias, self.head.weight, self.head.bias, idx)
        return self.evaluate(*self._gather(states, rows, index))

    def fit_step_at(self, states, rows, index, targets):
        """One minibatch of the squared-error fit in one library call (bbx_pmlp_value_fit_at): from the recorded states index[k] of
        the buffers states / rows and the targets [n] to the gradients of
            L = 1/2 mean_k (V_k - target_k)^2
        ADDED to the parameters' .grad as loss.backward() would.  Returns (stats float64 [6] on the device: counted positions,
        sum d^2, sum V, sum target, sum target^2, positions not counted; values float32 [n]) — nothing is read back, nothing waits.
        Where the kernels cannot read the buffers in place: fit_step on the gathered states."""
        if self._in_place(states, rows):
            return self._fit_kernels(states, rows, index.to(device=states.device, dtype=torch.int32).contiguous(), targets)
        st, rw = self._gather(states, rows, index)
        return self.fit_step(st, rw, targets)

    def fit_step(self, states, rows, targets):
        """fit_step_at for gathered tensors: states int [N, R, cols], rows [N] (None: the rows whose last column is not -1) —
        bbx_pmlp_value_fit under kernels_ok; otherwise the same formulae with torch ops and backward()."""
        if self.kernels_ok(states):
            rows = self._row_counts(states, rows).to(torch.int32).contiguous()
            st = states if states.dtype == torch.int32 else states.to(torch.int32)
            return self._fit_kernels(st.contiguous(), rows, None, targets)
        v = self.evaluate_torch(states, rows)
        n = v.numel()
        t = targets.to(device=v.device, dtype=v.dtype)
        d = v - t
        if n:
            loss = 0.5 * (d * d).sum() / n
            if loss.requires_grad:
                loss.backward()
        s = lambda x: x.detach().to(torch.float64).sum()
        zero = torch.zeros((), dtype=torch.float64, device=v.device)
        stats = torch.stack([zero + n, s(d * d), s(v), s(t), s(t * t), zero])
        return stats, v.detach()

    def _fit_kernels(self, states, rows, index, targets):
        R, cols = states.shape[-2:]
        S = rows.numel()
        N = S if index is None else index.numel()
        dev = states.device
        tg = targets.to(device=dev, dtype=torch.float32).contiguous()
        if tg.numel() != N:
            raise ValueError("fit_step: %d positions, %d targets" % (N, tg.numel()))
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        values, coef = new(N), new(N)
        stats = torch.empty(6, dtype=torch.float64, device=dev)
        p = lambda x: C.c_void_p(x.data_ptr())
        lib = _ffi.lib()
        with torch.cuda.device(dev):
            w = self._fused_weights()
            hidden = w["hidden"]
            grads = [new(cols, hidden), new(hidden), new(hidden), new(1)]
            ws = self._workspace("fit", N, R, cols, hidden, dev)
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            src = (p(states), p(rows)) + ((N,) if index is None else (S, p(index), N)) + (R, cols)
            fn = lib.bbx_pmlp_value_fit if index is None else lib.bbx_pmlp_value_fit_at
            _ffi.check(fn(*src, w["prepared"], hidden, self.pool_id, p(tg), C.c_float(1.0 / N if N else 0.0), p(values), p(coef), p(stats), p(ws),
                          *[p(g) for g in grads], s))
        self.last_path = "kernels"
        lin = self.embedding[0]
        for q, g in zip((lin.weight, lin.bias, self.head.weight, self.head.bias), (grads[0].t(), grads[1], grads[2].view(1, -1), grads[3])):
            if q.grad is None:
                q.grad = g.contiguous()
            else:
                q.grad.add_(g)
        return stats, values


class DeviceTrajectoryBuffer:
    """TrajectoryBuffer (pg.py:79-240) for a batch of environments stepping in lockstep, kept on the device: per step the
    -1-padded state block [B, R, cols] (optional), action, reward, log-probability, value and done flag of every
    environment.  finish() turns rewards into discounted rewards-to-go and values into GAE advantages per EPISODE
    (episodes end where done is set; an episode still running at the end of the buffer is incomplete and left out, like
    the reference's `[:self.start]`); get() returns the training tensors with the reference's filtering (states with a
    single row are dropped) and advantage normalisation."""

    def __init__(self, nsteps, batch, gam=0.99, lam=0.97, obs_shape=None, device="cuda"):
        self.T, self.B, self.gam, self.lam = nsteps, batch, gam, lam
        self.actions = torch.zeros((nsteps, batch), dtype=torch.int32, device=device)
        self.rewards = torch.zeros((nsteps, batch), dtype=torch.float64, device=device)
        self.logprobs = torch.zeros((nsteps, batch), dtype=torch.float32, device=device)
        self.values = torch.zeros((nsteps, batch), dtype=torch.float64, device=device)
        self.dones = torch.zeros((nsteps, batch), dtype=torch.bool, device=device)
        self.rows = torch.zeros((nsteps, batch), dtype=torch.int32, device=device)
        self.states = torch.empty((nsteps, batch) + tuple(obs_shape), dtype=torch.int32, device=device) if obs_shape else None
        self.t = 0
        self.returns = self.advantages = self.complete = None

    def store(self, state, rows, action, reward, logprob, value, done):
        t = self.t
        if self.states is not None:
            self.states[t].copy_(state)
        self.rows[t].copy_(rows); self.actions[t].copy_(action); self.rewards[t].copy_(reward)
        self.logprobs[t].copy_(logprob); self.dones[t].copy_(done.to(torch.bool))
        if value is not None:
            self.values[t].copy_(value)
        self.t += 1

    def fill_values(self, critic, t0=0, t1=None):
        """self.values[t0:t1] (t1 None: the steps stored so far) <- the critic's values of the stored states, float64: a learned
        baseline for GAE after a rollout that recorded none (run_rollout_fused).  On the device one bbx_pmlp_value call over the
        block in place (PMLPValue.values with out64); CPU buffers take the critic's torch path.  returns / advantages / complete
        are cleared, so that the next get_index() finishes again.  A buffer that keeps no states: ValueError."""
        if self.states is None:
            raise ValueError("fill_values: the buffer keeps no states (DeviceTrajectoryBuffer(..., obs_shape=(rows, cols)))")
        t1 = self.t if t1 is None else t1
        if not 0 <= t0 <= t1 <= self.T:
            raise IndexError("fill_values: steps [%d, %d) of a buffer of %d" % (t0, t1, self.T))
        if t1 > t0:
            critic.values(self.states[t0:t1], self.rows[t0:t1], out64=self.values[t0:t1])
        self.returns = self.advantages = self.complete = None

    def finish(self):
        """Reverse scan over time with episode boundaries: ret_t = r_t + gam ret_{t+1}; delta_t = r_t - v_t + gam v_{t+1};
        adv_t = delta_t + gam lam adv_{t+1}; nothing crosses a done flag (pg.py:20-76 per trajectory).  Tensors on the GPU:
        one kernel (bbx_gae_device, one thread per environment); on the CPU: the torch loop (_finish_torch), whose results
        the kernel reproduces bit for bit."""
        T = self.t
        r, v, d = self.rewards[:T], self.values[:T], self.dones[:T]
        if not r.is_cuda:
            return self._finish_torch()
        ret = torch.empty_like(r); adv = torch.empty_like(r); comp = torch.empty_like(d)
        p = lambda x: C.c_void_p(x.data_ptr())
        with torch.cuda.device(r.device):
            _ffi.check(_ffi.lib().bbx_gae_device(p(r), p(v), p(d), T, self.B, float(self.gam), float(self.lam), p(ret), p(adv), p(comp),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.returns, self.advantages, self.complete = ret, adv, comp
        return ret, adv, comp

    def _finish_torch(self):
        """finish() with torch ops, about ten launches per step: CPU tensors, and the reference of the kernel."""
        T = self.t
        r, v, d = self.rewards[:T], self.values[:T], self.dones[:T]
        ret = torch.zeros_like(r); adv = torch.zeros_like(r); comp = torch.zeros_like(d)
        nret = torch.zeros(self.B, dtype=torch.float64, device=r.device); nadv = torch.zeros_like(nret)
        nval = torch.zeros_like(nret); ncomp = torch.zeros(self.B, dtype=torch.bool, device=r.device)
        for t in range(T - 1, -1, -1):
            last = d[t]                                              # step t ends its episode: nothing follows it
            nret = torch.where(last, torch.zeros_like(nret), nret); nadv = torch.where(last, torch.zeros_like(nadv), nadv)
            nval = torch.where(last, torch.zeros_like(nval), nval); ncomp = ncomp | last
            ret[t] = r[t] + self.gam * nret
            adv[t] = (r[t] - v[t] + self.gam * nval) + self.gam * self.lam * nadv
            comp[t] = ncomp
            nret, nadv, nval = ret[t], adv[t], v[t]
        self.returns, self.advantages, self.complete = ret, adv, comp
        return ret, adv, comp

    def get_index(self, batch_size=None, normalize_advantages=True, sort=False, drop_remainder=False, with_rows=False):
        """get() without the state blocks: the same selection, order, advantage normalisation and batching, but the first element
        of every tuple is an int32 tensor of flat step numbers t * B + b — positions in self.states.view(-1, R, cols),
        self.rows.view(-1) and self.actions.view(-1) — for PMLPPolicy.evaluate_at, which reads the states where the rollout
        left them.  With batch_size the tuples hold slices of ONE index tensor (a shuffle of the epoch is a permutation of it);
        nothing of the size of a state block is allocated, nothing waits for the device per batch, and a buffer without states
        gives the same indices."""
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
        out = [idx, at(self.actions), at(self.logprobs), adv, at(self.returns).to(torch.float32)]
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

    def get(self, batch_size=None, normalize_advantages=True, sort=False, drop_remainder=False, with_rows=False):
        """Training data of all complete-episode steps whose state had more than one row (pg.py:162-240): (states or None,
        actions, logprobs, advantages, values-to-fit), advantages normalised by their mean and population std over the
        complete steps (pg.py:176-178: before the single-row filter, like the reference), steps ordered trajectory after
        trajectory (environment-major).  batch_size=None: one tuple of whole tensors.  Otherwise the reference's
        padded_batch: a list of such tuples of at most batch_size steps each, the state block of a batch cut to the most
        rows any of its states has (-1 padding beyond a state's own rows, as stored); sort=True orders the steps by their
        number of rows first (less padding); drop_remainder=True leaves a short last batch out.  with_rows=True: every tuple
        carries the states' row counts (int32) as a sixth element (what PMLPPolicy.evaluate takes as `rows`).
        The selection is get_index's; the states are gathered here, once."""
        whole = self.get_index(None, normalize_advantages, sort, False, True)
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


def ppo_update(policy, buffer, optimizer, epochs, batch_size, clip=0.2, ent_coef=0.0, kld_limit=None, mode="clip", shuffle=True, generator=None,
               c_kl=0.0):
    """The policy update of the reference (pg.py _fit_policy_model) over a finished DeviceTrajectoryBuffer with states: `epochs`
    passes over buffer.get_index()'s steps in minibatches of batch_size — per epoch ONE permutation of the index list (shuffle; from
    `generator`, which lives on the buffer's device), per minibatch one policy.ppo_step_at on the buffers as the rollout left them,
    then optimizer.step() and optimizer.zero_grad(); the optimiser is the caller's.  One host read per epoch: the minibatches'
    stacked statistics.  With kld_limit the update stops after an epoch whose mean old - new log-probability exceeds it.
    Returns one dict per epoch run: "stats" (float64 [minibatches, 6], ppo_step_at's), and over the epoch's counted positions
    "loss", "entropy", "kl" (mean old - new) and "clip_frac"."""
    if buffer.states is None:
        raise ValueError("ppo_update: the buffer keeps no states (DeviceTrajectoryBuffer(..., obs_shape=(rows, cols)))")
    idx, _, old, adv, _ = buffer.get_index(None)
    n = int(idx.numel())
    out = []
    optimizer.zero_grad()
    for _ in range(epochs):
        if shuffle:
            perm = torch.randperm(n, device=idx.device, generator=generator)
            e_idx, e_old, e_adv = idx[perm], old[perm], adv[perm]
        else:
            e_idx, e_old, e_adv = idx, old, adv
        stats = []
        for i in range(0, n, batch_size):
            k = min(i + batch_size, n)
            st, _, _ = policy.ppo_step_at(buffer.states, buffer.actions, buffer.rows, e_idx[i:k], e_old[i:k], e_adv[i:k], clip=clip, ent_coef=ent_coef,
                                          mode=mode, c_kl=c_kl)
            optimizer.step()
            optimizer.zero_grad()
            stats.append(st)
        st = torch.stack(stats).cpu().numpy() if stats else np.zeros((0, 6))     # the epoch's one host read
        tot = st.sum(axis=0) if len(st) else np.zeros(6)
        cnt = max(tot[0], 1.0)
        out.append({"stats": st, "loss": -(tot[1] + ent_coef * tot[2]) / cnt, "entropy": tot[2] / cnt, "kl": tot[3] / cnt, "clip_frac": tot[4] / cnt})
        if kld_limit is not None and out[-1]["kl"] > kld_limit:
            break
    return out


def value_update(critic, buffer, optimizer, epochs, batch_size, shuffle=True, generator=None):
    """The counterpart of ppo_update for a PMLPValue critic (pg.py _fit_value_model): `epochs` passes over buffer.get_index()'s steps
    in minibatches of batch_size, the targets its fifth element (the discounted returns) — per epoch ONE permutation of the index
    list (shuffle; from `generator`, which lives on the buffer's device), per minibatch one critic.fit_step_at on the buffers as the
    rollout left them, then optimizer.step() and optimizer.zero_grad(); the optimiser is the caller's.  One host read per epoch: the
    minibatches' stacked statistics.  Returns one dict per epoch: "stats" (float64 [minibatches, 6], fit_step_at's), and over the
    epoch's counted positions "loss" (1/2 mean (V - target)^2, each minibatch under the weights it saw) and "explained_variance"
    (1 - mean (V - target)^2 / var(target); NaN where the targets do not vary)."""
    if buffer.states is None:
        raise ValueError("value_update: the buffer keeps no states (DeviceTrajectoryBuffer(..., obs_shape=(rows, cols)))")
    idx, _, _, _, ret = buffer.get_index(None)
    n = int(idx.numel())
    out = []
    optimizer.zero_grad()
    for _ in range(epochs):
        if shuffle:
            perm = torch.randperm(n, device=idx.device, generator=generator)
            e_idx, e_ret = idx[perm], ret[perm]
        else:
            e_idx, e_ret = idx, ret
        stats = []
        for i in range(0, n, batch_size):
            k = min(i + batch_size, n)
            st, _ = critic.fit_step_at(buffer.states, buffer.rows, e_idx[i:k], e_ret[i:k])
            optimizer.step()
            optimizer.zero_grad()
            stats.append(st)
        st = torch.stack(stats).cpu().numpy() if stats else np.zeros((0, 6))     # the epoch's one host read
        tot = st.sum(axis=0) if len(st) else np.zeros(6)
        cnt = max(tot[0], 1.0)
        var = tot[4] / cnt - (tot[3] / cnt) ** 2
        out.append({"stats": st, "loss": 0.5 * tot[1] / cnt, "explained_variance": 1.0 - (tot[1] / cnt) / var if var > 0 else float("nan")})
    return out


@_with_gc_paused
@torch.no_grad()
def run_rollout_fused(env, policy, nsteps, buffer=None, obs_rows=256, generator=None, chunk=256, greedy=False, critic=None):
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
    state-keeping buffer: ValueError before anything is queued."""
    if critic is not None and (buffer is None or buffer.states is None):
        raise ValueError("run_rollout_fused: a critic reads the recorded states (buffer=DeviceTrajectoryBuffer(..., obs_shape=(rows, cols)))")
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
    d = env.stats() - st0
    total = torch.tensor(-d[:, 1].astype(np.float64), device=dev)
    episodes = torch.tensor(d[:, 2], device=dev)
    return total, episodes


@_with_gc_paused
@torch.no_grad()
def run_rollout(env, policy, nsteps, buffer=None, obs_rows=256, generator=None, sync_every=64, graph=False,
                value_strategy=None, value_gamma=None, greedy=False):
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
    call, restored afterwards); no uniforms are drawn."""
    if value_strategy is not None and graph:
        raise ValueError("run_rollout: value_strategy cannot be recorded into a graph (bbx_values_device keeps host bookkeeping)")
    if value_strategy is not None and buffer is None:
        raise ValueError("run_rollout: value_strategy needs a buffer to write the values to")
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
            env.sync()
            nsync += 1
    finally:
        if one_call:
            env.policy_greedy(was_greedy)
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
    key = (id(policy), obs_rows, sync_every, bool(greedy))     # (a recording keeps the mode it was captured with)
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


def evaluate_policy(env, policy, episodes, greedy=True, obs_rows=256, chunk=64, max_steps=None, generator=None):
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
    Returns Evaluation(returns, lengths, complete, steps)."""
    if episodes < 1 or chunk < 1:
        raise ValueError("evaluate_policy: episodes and chunk must be positive")
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
