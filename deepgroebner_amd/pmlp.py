"""The PMLP policy and critic: the torch modules of the reference's networks, and the one layer through which both
call the hand-written HIP kernels of bbx_api_policy.cpp.

    PMLPPolicy                 ParallelMultilayerPerceptron           networks.py:522-571 (:49-95, :414-460)
    PMLPPolicy.act             log-softmax + inverse-CDF draw (or argmax, greedy=True) in one kernel (bbx_pmlp_act, bbx_pmlp2_act, bbx_pmlp3_act)
    PMLPPolicy.evaluate, evaluate_at   log pi(a | s) and entropy of recorded experience, differentiable: bbx_pmlp_logprob / bbx_pmlp_grad,
                               bbx_pmlp2_logprob / bbx_pmlp2_grad; the _at forms read a trajectory buffer where the rollout left it
    PMLPPolicy.ppo_step, ppo_step_at   one minibatch of the update — forward, PPO loss, statistics, weight gradients — in one library
                               call (bbx_pmlp_ppo_grad[_at] / bbx_pmlp2_ppo_grad[_at])           pg.py _fit_policy_model
    PMLPPolicy.xent_step, xent_step_at, xent, xent_at   cross-entropy against a target distribution over each state's rows (action
                               values, visit counts, an expert's pick): one library call per minibatch (bbx_pmlp_xent_grad[_at] /
                               bbx_pmlp2_xent_grad[_at]), the loss alone for held-out data (bbx_pmlp[2]_xent[_at])      az.py's policy fit
    PMLPValue                  a learned baseline (--value_model mlp, pg.py _fit_value_model): a critic over the recorded state
                               blocks — one launch for a whole buffer's values (bbx_pmlp_value), one library call per minibatch of the
                               squared-error fit (bbx_pmlp_value_fit[_at]); with two hidden layers and deep_kernels set the same through
                               bbx_pmlp2_value / bbx_pmlp2_value_grad / bbx_pmlp2_value_fit[_at]

The kernel-call layer (_PMLPKernels and the helpers in front of it) holds what every such call needs, once: the prepared weights
and their cache, the workspaces, the head of an argument list, the decision whether the kernels can take a call, the conversion
of its inputs, and the shaping of the kernels' gradient arrays into torch.nn.Linear's layouts.  The torch paths (forward,
evaluate_torch, act_torch, _ppo_torch, the torch branch of fit_step) stay apart: they are the baselines the kernels are tested
against.  deepgroebner_amd.rollout has the trajectory buffer and the rollout and update loops that drive these classes.

The default one-hidden-layer network runs on the matrix cores, either as a kernel of its own fed by the padded observation block
(bbx_pmlp_act), in front of the step in the same launch (bbx_policy_step_device), or inside the step loop
(bbx_policy_rollout_device).  Two hidden layers of at most 128 units run inside the step loop too (bbx_policy2_rollout_device) or
as a kernel of their own (bbx_pmlp2_act), three as a kernel of their own (bbx_pmlp3_act); deeper or wider networks take the torch
path.  Actions never visit the host.
"""
import collections
import ctypes as C

import torch

from . import _ffi


def _ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call_head(stem, states, rows, actions, index):
    """The entry point and the leading arguments of a call about states [..., R, cols] with rows (and actions, where the call takes
    them): `stem` over all S = rows.numel() of them, `stem`_at over the N positions index[k] of them (int32 [N]; the tensors are
    then whole buffers read in place).  Returns (function, leading arguments, S, N, R, cols)."""
    R, cols = states.shape[-2:]
    S = rows.numel()
    N = S if index is None else index.numel()
    src = (_ptr(states), _ptr(rows)) + (() if actions is None else (_ptr(actions),))
    count = (N,) if index is None else (S, _ptr(index), N)
    return getattr(_ffi.lib(), stem if index is None else stem + "_at"), src + count + (R, cols), S, N, R, cols


def _kernel_inputs(states, rows, actions=None):
    """states, rows and actions as the kernels read them: contiguous int32.  rows None: the rows whose last column is not -1."""
    R, cols = states.shape[-2:]
    st = (states if states.dtype == torch.int32 else states.to(torch.int32)).contiguous()
    if rows is None:
        rows = (st.view(-1, R, cols)[:, :, -1] != -1).sum(1)
    return st, rows.to(torch.int32).contiguous(), None if actions is None else actions.to(torch.int32).contiguous()


def _index32(index, states):
    return index.to(device=states.device, dtype=torch.int32).contiguous()


def _gather(index, *buffers):
    """x[index] of every buffer, [S, ...] or [T, B, ...] with flat step numbers in index."""
    j = index.to(device=buffers[0].device, dtype=torch.int64)
    if buffers[0].dim() == 4:                                         # (no reshape: a non-contiguous buffer would be copied whole)
        t, b = j // buffers[0].shape[1], j % buffers[0].shape[1]
        return tuple(x[t, b] for x in buffers)
    return tuple(x[j] for x in buffers)


def _grad_arrays(cols, hidden, device):
    """The kernels' gradient arrays: W [inputs][units] and b [units] per hidden layer, then the last layer's w [units] and b [1]."""
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
    dims = [cols] + list(hidden)
    out = []
    for a, b in zip(dims[:-1], dims[1:]):
        out += [new(a, b), new(b)]
    return out + [new(dims[-1]), new(1)]


def _linear_layouts(grads):
    """_grad_arrays in torch.nn.Linear's layouts (views): weight [units][inputs], the last layer's [1][units]."""
    return [g.t() if g.dim() == 2 else g for g in grads[:-2]] + [grads[-2].view(1, -1), grads[-1]]


def _add_to_grad(params, grads):
    """Adds into .grad as loss.backward() would: None becomes the tensor."""
    for q, g in zip(params, grads):
        if q.grad is None:
            q.grad = g.contiguous()
        else:
            q.grad.add_(g)


class _PMLPKernels(torch.nn.Module):
    """What PMLPPolicy and PMLPValue share in front of the kernels: `embedding` (the hidden layers) and `_last` (the linear unit
    behind them) are the subclass's."""

    deep_kernels = False

    @staticmethod
    def fused_ok(cols, hidden):
        """Shapes the one-layer kernels are built for (bbx_pmlp_prepared_floats >= 0)."""
        return 1 <= hidden <= 256 and 1 <= cols <= 64

    def deep_ok(self, cols):
        """Two or three hidden layers of at most 128 units: the shapes bbx_pmlp2_act / bbx_pmlp3_act are built for (two: the training
        kernels' and the critic's too)."""
        return len(self.embedding) in (2, 3) and all(1 <= l.out_features <= 128 for l in self.embedding) and 1 <= cols <= 64

    def _kernel_params(self):
        """The parameters in the kernels' order, which is the order of _grad_arrays (and of parameters())."""
        return [q for l in (*self.embedding, self._last) for q in (l.weight, l.bias)]

    def _kernel_depth(self, states, rows=None, actions=None, in_place=False, acting=False):
        """How many hidden layers the kernels that take states [..., R, cols] with this module's weights have; 0: none do (the torch
        path).  The training kernels (evaluate, ppo_step, values, fit_step): one hidden layer, or two with deep_kernels set, float32
        parameters on the GPU, 1 to 2048 rows.  in_place (the _at forms): states, rows and actions must also BE contiguous int32
        CUDA tensors of matching sizes already — a buffer is never converted or copied as a whole.  acting (act): the draw's
        kernels, which convert the weights themselves, take three layers too and score no rows as well."""
        if not states.is_cuda:
            return 0
        R, cols = states.shape[-2:]
        layers = self.embedding
        depth = len(layers)
        if depth == 1:
            ok = self.fused_ok(cols, layers[0].out_features) and R <= 2048
            weights = (layers[0].weight,)
        else:
            ok = (acting or (depth == 2 and self.deep_kernels)) and self.deep_ok(cols) and R <= (self.deep_max_rows() if acting else 2048)
            weights = self.parameters()
        if ok and not acting:
            ok = R >= 1 and all(q.is_cuda and q.dtype == torch.float32 for q in weights)
        if ok and in_place:
            S = rows.numel()
            ok = (states.numel() == S * R * cols and (actions is None or actions.numel() == S)
                  and all(x.is_cuda and x.dtype == torch.int32 and x.is_contiguous() for x in (states, rows, actions) if x is not None))
        return depth if ok else 0

    def _prepared_weights(self, slot, layers, last, refill):
        """The kernels' view of the weights (bbx_pmlp_prepare / bbx_pmlp2_prepare / bbx_pmlp3_prepare: transposed, zero-padded to the
        tile sizes), kept in self.<slot> and rebuilt only when a parameter changed (an optimiser step bumps the tensors' version
        counters): no per-step transposes, no per-step host read.  Returns {"key", "keep", "prepared" (c_void_p), "hidden",
        "refilled"}; one layer: "keep" is the buffer and "hidden" an int; more: "keep" is (buffer, the tensors it was filled from)
        and "hidden" a list.
        refill says what a change of the weights does to the buffer.  False (the one-layer policy): a fresh buffer per version; an
        earlier one stays as it was for whoever holds it.  True (the deeper policy, the critic): the same buffer is filled again
        — a recorded graph and the rollout kernels keep reading that address.
        Either way an autograd backward differentiates the weights of ITS OWN forward pass, not whatever the module holds by then:
        forward takes its buffer from _forward_weights, which clones a refilled one (on the stream, behind the fill)."""
        params = [q for l in (*layers, last) for q in (l.weight, l.bias)]    # (one pass: parameters() walks the module tree, 13 us against 6)
        key = tuple(p._version for p in params) + tuple(p.data_ptr() for p in params)
        c = self.__dict__.get(slot)
        if c is not None and c["key"] == key:
            return c
        one = len(layers) == 1
        cols = layers[0].in_features
        hidden = [l.out_features for l in layers]
        t = []
        for l in layers:
            t += [l.weight.detach().t().contiguous().float(), l.bias.detach().contiguous().float()]
        t.append(last.weight.detach().reshape(-1).contiguous().float())
        if not one:
            t.append(last.bias.detach().reshape(-1).contiguous().float())
        lib = _ffi.lib()
        if one:
            floats, prepare = lib.bbx_pmlp_prepared_floats, lib.bbx_pmlp_prepare
        elif len(layers) == 2:
            floats, prepare = lib.bbx_pmlp2_prepared_floats, lib.bbx_pmlp2_prepare
        else:
            floats, prepare = lib.bbx_pmlp3_prepared_floats, lib.bbx_pmlp3_prepare
        size = floats(cols, *hidden)
        _ffi.check(min(size, 0))
        prep = None
        if refill and c is not None:
            prep = c["keep"] if one else c["keep"][0]
        if prep is None or prep.numel() != size or prep.device != t[0].device:
            prep = torch.empty(size, dtype=torch.float32, device=t[0].device)
        # (one layer: b2 travels by value in the C call; reading it back would make every optimiser step wait for the device: the call
        # gets 0 and the bias is copied on the device into its place, the first of the layout's last four floats)
        b2 = (C.c_float(0.0),) if one else ()
        _ffi.check(prepare(*[_ptr(x) for x in t], *b2, cols, *hidden, _ptr(prep), _stream()))
        if one:
            prep[size - 4:size - 3].copy_(last.bias.detach().reshape(1))
        c = {"key": key, "keep": prep if one else (prep, t), "prepared": _ptr(prep), "hidden": hidden[0] if one else hidden, "refilled": refill}
        self.__dict__[slot] = c
        return c

    def _forward_weights(self, depth):
        """(hidden sizes as a tuple, the prepared weights an autograd forward computes with and hands to its backward): see
        _prepared_weights."""
        w = self._fused_weights() if depth == 1 else self._deep_weights()
        hidden, prep = ((w["hidden"],), w["keep"]) if depth == 1 else (tuple(w["hidden"]), w["keep"][0])
        return hidden, prep.clone() if w["refilled"] else prep

    def _workspace(self, slot, nfl, device):
        """A kernel's workspace of nfl floats, kept in self.<slot> between calls (it grows only; calls on one stream run in order)."""
        _ffi.check(min(nfl, 0))
        ws = self.__dict__.get(slot)
        if ws is None or ws.numel() < nfl or ws.device != device:
            ws = torch.empty(nfl, dtype=torch.float32, device=device)
            self.__dict__[slot] = ws
        return ws


# What tells the four autograd functions apart: the stems of the forward and the backward entry point (the backward's workspace is
# <backward>_workspace_floats), the module's workspace slot, the hidden layers, whether the critic's pool id travels along (recorded
# actions do where the function has them), and the number of outputs (the forward entry points have two output arguments: a
# critic's second stays empty).
_Kernels = collections.namedtuple("_Kernels", ["forward", "backward", "slot", "depth", "pool", "outputs"])
_POLICY = _Kernels("bbx_pmlp_logprob", "bbx_pmlp_grad", "_grad_ws", 1, False, 2)
_POLICY2 = _Kernels("bbx_pmlp2_logprob", "bbx_pmlp2_grad", "_grad2_ws", 2, False, 2)
_VALUE = _Kernels("bbx_pmlp_value", "bbx_pmlp_value_grad", "_ws", 1, True, 1)
_VALUE2 = _Kernels("bbx_pmlp2_value", "bbx_pmlp2_value_grad", "_ws", 2, True, 1)


def _forward(ctx, kind, module, states, rows, actions, index, params):
    """The forward pass of the four functions: `kind.outputs` float32 tensors, one element per state (per index)."""
    fn, head, _, N, _, _ = _call_head(kind.forward, states, rows, actions, index)
    out = [torch.empty(N, dtype=torch.float32, device=states.device) for _ in range(kind.outputs)]
    pool = (module.pool_id,) if kind.pool else ()
    with torch.cuda.device(states.device):
        hidden, prep = module._forward_weights(kind.depth)
        _ffi.check(fn(*head, _ptr(prep), *hidden, *pool, *[_ptr(x) for x in out], *[None] * (2 - kind.outputs), _stream()))
    ctx.module, ctx.prep, ctx.hidden, ctx.pool = module, prep, hidden, pool   # (the prepared weights of THIS forward pass)
    ctx.save_for_backward(states, rows, actions, index, *params)
    return tuple(out)


def _backward(ctx, kind, *cotangents):
    """The backward pass of the four functions: the parameters' gradients in torch.nn.Linear's layouts and the parameters' dtypes.
    The hidden activations are recomputed: nothing of size [N, R, hidden] is kept between forward and backward."""
    states, rows, actions, index, *params = ctx.saved_tensors
    fn, head, _, N, R, cols = _call_head(kind.backward, states, rows, actions, index)
    dev = states.device
    cotangents = [g.contiguous().float() for g in cotangents]
    grads = _grad_arrays(cols, ctx.hidden, dev)
    with torch.cuda.device(dev):
        ws = ctx.module._workspace(kind.slot, getattr(_ffi.lib(), kind.backward + "_workspace_floats")(N, R, cols, *ctx.hidden), dev)
        _ffi.check(fn(*head, _ptr(ctx.prep), *ctx.hidden, *ctx.pool, *[_ptr(g) for g in cotangents], _ptr(ws), *[_ptr(g) for g in grads], _stream()))
    return tuple(g.to(q.dtype) for g, q in zip(_linear_layouts(grads), params))


class _PMLPEvaluate(torch.autograd.Function):
    """log pi(a | s) and the entropy of pi(. | s) of a one-hidden-layer PMLPPolicy through bbx_pmlp_logprob, differentiable
    with respect to the four parameter tensors through bbx_pmlp_grad.  No gradient for states, actions or rows.
    index (int32 [n], optional): the call is about the recorded states index[k] of states [..., R, cols], rows and actions, which
    are then whole buffers read in place (bbx_pmlp_logprob_at / bbx_pmlp_grad_at); the outputs have length n."""

    @staticmethod
    def forward(ctx, policy, states, rows, actions, w1, b1, w2, b2, index=None):
        return _forward(ctx, _POLICY, policy, states, rows, actions, index, (w1, b1, w2, b2))

    @staticmethod
    def backward(ctx, glogp, gent):
        return (None,) * 4 + _backward(ctx, _POLICY, glogp, gent) + (None,)


class _PMLP2Evaluate(torch.autograd.Function):
    """_PMLPEvaluate for two hidden layers: bbx_pmlp2_logprob forward, bbx_pmlp2_grad backward, gradients for the six parameter
    tensors.  index: as in _PMLPEvaluate (bbx_pmlp2_logprob_at / bbx_pmlp2_grad_at)."""

    @staticmethod
    def forward(ctx, policy, states, rows, actions, w1, b1, w2, b2, w3, b3, index=None):
        return _forward(ctx, _POLICY2, policy, states, rows, actions, index, (w1, b1, w2, b2, w3, b3))

    @staticmethod
    def backward(ctx, glogp, gent):
        return (None,) * 4 + _backward(ctx, _POLICY2, glogp, gent) + (None,)


class _PMLPValueEvaluate(torch.autograd.Function):
    """The values of a one-hidden-layer PMLPValue through bbx_pmlp_value, differentiable with respect to the four parameter tensors
    through bbx_pmlp_value_grad.  No gradient for states or rows.  index: as in _PMLPEvaluate (bbx_pmlp_value_at /
    bbx_pmlp_value_grad_at)."""

    @staticmethod
    def forward(ctx, critic, states, rows, w1, b1, w2, b2, index=None):
        return _forward(ctx, _VALUE, critic, states, rows, None, index, (w1, b1, w2, b2))[0]

    @staticmethod
    def backward(ctx, gvalue):
        return (None,) * 3 + _backward(ctx, _VALUE, gvalue) + (None,)


class _PMLP2ValueEvaluate(torch.autograd.Function):
    """_PMLPValueEvaluate for two hidden layers: bbx_pmlp2_value forward, bbx_pmlp2_value_grad backward, gradients for the six
    parameter tensors.  index: as in _PMLPEvaluate (bbx_pmlp2_value_at / bbx_pmlp2_value_grad_at)."""

    @staticmethod
    def forward(ctx, critic, states, rows, w1, b1, w2, b2, w3, b3, index=None):
        return _forward(ctx, _VALUE2, critic, states, rows, None, index, (w1, b1, w2, b2, w3, b3))[0]

    @staticmethod
    def backward(ctx, gvalue):
        return (None,) * 3 + _backward(ctx, _VALUE2, gvalue) + (None,)


class PMLPPolicy(_PMLPKernels):
    """ParallelMultilayerPerceptron(hidden_layers) of the reference: every row of the -1-padded [batch, rows, cols] int
    block is embedded by the same MLP (relu), scored by one linear unit, padded rows get -1e9, log-softmax over rows."""

    def __init__(self, cols, hidden_layers=(128,), deep_kernels=False):
        super().__init__()
        self.deep_kernels = deep_kernels                              # two hidden layers: evaluate through bbx_pmlp2_logprob / bbx_pmlp2_grad
        dims = [cols] + list(hidden_layers)
        self.embedding = torch.nn.ModuleList([torch.nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:])])
        self.deciding = torch.nn.Linear(dims[-1], 1)
        self.cols = cols

    @property
    def _last(self):
        return self.deciding

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
        depth = self._kernel_depth(obs, acting=True)
        if not depth:
            return self.act_torch(obs, rows, u, actions, logprobs, greedy=greedy)
        if actions is None:
            actions = torch.empty(B, dtype=torch.int32, device=obs.device)
        if logprobs is None:
            logprobs = torch.empty(B, dtype=torch.float32, device=obs.device)
        w = self._fused_weights() if depth == 1 else self._deep_weights()
        hidden = (w["hidden"],) if depth == 1 else w["hidden"]
        s = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
        fn = getattr(_ffi.lib(), "bbx_pmlp%s_act%s" % ("" if depth == 1 else depth, "_greedy" if greedy else ""))
        _ffi.check(fn(_ptr(obs), _ptr(rows), B, R, cols, w["prepared"], *hidden, *(() if greedy else (_ptr(u),)), _ptr(actions), _ptr(logprobs),
                      C.c_void_p(s)))
        return actions, logprobs

    def deep_max_rows(self):
        """Rows per environment the two- / three-layer kernels score: the logits of a wave's environment live in LDS beside the
        staged weights — 2048 rows, 1024 where three layers wider than 64 units (128 KB of weights) leave less room."""
        return 1024 if len(self.embedding) == 3 and max(l.out_features for l in self.embedding) > 64 else 2048

    def _deep_weights(self):
        """The two- / three-layer kernels' view of the weights, refilled in place (_prepared_weights)."""
        return self._prepared_weights("_deep_cache", self.embedding, self.deciding, True)

    def _fused_weights(self):
        """The one-layer kernels' view of the weights, a fresh buffer per version (_prepared_weights).  One hidden layer only: the
        layout has no room for a second."""
        if len(self.embedding) != 1:
            raise ValueError("_fused_weights: the one-layer kernels' weights of a policy with %d hidden layers (two: _deep_weights)" % len(self.embedding))
        return self._prepared_weights("_fused_cache", self.embedding, self.deciding, False)

    def evaluate(self, states, actions, rows=None):
        """The training-time view of recorded experience (pg.py _fit_policy_model): states int [N, R, cols], actions [N] ->
        (logprobs float32 [N] of the recorded actions, entropy float32 [N] of the distribution over each state's rows),
        differentiable with respect to the module's parameters.  rows [N]: the live rows per state (None: those whose last
        column is not -1, as forward masks).  No live rows: 0.0 and 0.0; an action outside the live rows: NaN.
        One hidden layer on the GPU: the HIP kernels bbx_pmlp_logprob / bbx_pmlp_grad; two hidden layers of at most 128 units
        on the GPU with deep_kernels set: bbx_pmlp2_logprob / bbx_pmlp2_grad; otherwise evaluate_torch."""
        N, R, cols = states.shape                                     # (gathered states: a buffer [T, B, R, cols] goes through the _at form)
        depth = self._kernel_depth(states)
        if depth:
            return self._evaluate_kernels(depth, *_kernel_inputs(states, rows, actions))
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
        depth = self._kernel_depth(states, rows, actions, in_place=True)
        if depth:
            return self._evaluate_kernels(depth, states, rows, actions, _index32(index, states))
        return self.evaluate(*_gather(index, states, actions, rows))

    def _evaluate_kernels(self, depth, states, rows, actions, index=None):
        return (_PMLPEvaluate if depth == 1 else _PMLP2Evaluate).apply(self, states, rows, actions, *self._kernel_params(), index)

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
        depth = self._kernel_depth(states, rows, actions, in_place=True)
        if depth:
            return self._ppo_kernels(depth, states, rows, actions, _index32(index, states), old_logprobs, advantages, clip, ent_coef, mode, c_kl)
        return self._ppo_torch(self.evaluate_at(states, actions, rows, index), old_logprobs, advantages, clip, ent_coef, mode, c_kl)

    def ppo_step(self, states, actions, rows=None, old_logprobs=None, advantages=None, clip=0.2, ent_coef=0.0, mode="clip", c_kl=0.0):
        """ppo_step_at for gathered tensors, as evaluate takes them: states int [N, R, cols], actions [N], rows [N] (None: the rows
        whose last column is not -1) — bbx_pmlp_ppo_grad / bbx_pmlp2_ppo_grad under evaluate()'s conditions for the kernels."""
        N, R, cols = states.shape                                     # (gathered states: a buffer [T, B, R, cols] goes through the _at form)
        depth = self._kernel_depth(states)
        if depth:
            return self._ppo_kernels(depth, *_kernel_inputs(states, rows, actions), None, old_logprobs, advantages, clip, ent_coef, mode, c_kl)
        return self._ppo_torch(self.evaluate(states, actions, rows), old_logprobs, advantages, clip, ent_coef, mode, c_kl)

    def _ppo_kernels(self, depth, states, rows, actions, index, old_logprobs, advantages, clip, ent_coef, mode, c_kl):
        stem = "bbx_pmlp_ppo" if depth == 1 else "bbx_pmlp2_ppo"
        fn, head, _, N, R, cols = _call_head(stem + "_grad", states, rows, actions, index)
        dev = states.device
        old = old_logprobs.to(device=dev, dtype=torch.float32).contiguous()
        adv = advantages.to(device=dev, dtype=torch.float32).contiguous()
        if old.numel() != N or adv.numel() != N:
            raise ValueError("ppo_step: %d positions, %d old log-probabilities, %d advantages" % (N, old.numel(), adv.numel()))
        new = lambda n: torch.empty(n, dtype=torch.float32, device=dev)
        logp, ent, coef = new(N), new(N), new(2 * N)
        stats = torch.empty(6, dtype=torch.float64, device=dev)
        loss = (self.LOSS_MODES[mode], C.c_float(1.0 / N if N else 0.0), C.c_float(clip), C.c_float(ent_coef), C.c_float(c_kl))
        with torch.cuda.device(dev):
            w = self._fused_weights() if depth == 1 else self._deep_weights()
            hidden = (w["hidden"],) if depth == 1 else tuple(w["hidden"])
            grads = _grad_arrays(cols, hidden, dev)
            ws = self._workspace("_ppo_ws", getattr(_ffi.lib(), stem + "_workspace_floats")(N, R, cols, *hidden), dev)
            _ffi.check(fn(*head, w["prepared"], *hidden, _ptr(old), _ptr(adv), *loss, _ptr(logp), _ptr(ent), _ptr(coef), _ptr(stats), _ptr(ws),
                          *[_ptr(g) for g in grads], _stream()))
        _add_to_grad(self._kernel_params(), _linear_layouts(grads))
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

    # ---- cross-entropy against a target distribution over each state's rows
    def xent_step_at(self, states, rows, index, targets, weights=None, scale=None):
        """One minibatch of imitation in one library call: from the recorded states index[k] of the buffers states / rows (as
        evaluate_at takes them) and the target rows targets [S, R] or [T, B, R] (float32, addressed like the states: a softmax of
        action values, a search's visit counts, an expert's pick as a one-hot row; what lies beyond a state's live rows is ignored,
        NaN included) to the gradients of
            L = scale sum_k w_k l_k          l_k = -sum_r t_r log p_r          (weights [n] or None: 1; scale None: 1 / n)
        ADDED to the parameters' .grad as loss.backward() would (None becomes the tensor).  A position is not counted — l = NaN,
        nothing in any sum or gradient — where a live target is negative or not finite, its weight is not finite, or (kernels) its
        index lies outside the buffer.  Returns (stats float64 [6] on the device: counted positions, sum w l, sum w T (T = sum_r t_r),
        sum H, sum w, positions not counted; losses float32 [n]; entropy float32 [n]) — nothing is read back, nothing waits.
        Under ppo_step_at's conditions for the kernels, and targets a contiguous float32 CUDA tensor: bbx_pmlp_xent_grad_at /
        bbx_pmlp2_xent_grad_at; anywhere else (three hidden layers, more than 2048 rows, CPU tensors) the same formulae with torch
        ops and backward() on the gathered states (_xent_torch)."""
        depth = self._kernel_depth(states, rows, in_place=True)
        if depth and self._targets_in_place(targets, states):
            return self._xent_kernels(depth, states, rows, targets, _index32(index, states), weights, scale, True)
        return self.xent_step(*_gather(index, states, rows, targets), weights=weights, scale=scale)

    def xent_step(self, states, rows, targets, weights=None, scale=None):
        """xent_step_at for gathered tensors: states int [N, R, cols], rows [N] (None: the rows whose last column is not -1), targets
        [N, R] — bbx_pmlp_xent_grad / bbx_pmlp2_xent_grad under evaluate()'s conditions for the kernels."""
        N, R, cols = states.shape
        depth = self._kernel_depth(states)
        if depth:
            st, rw, _ = _kernel_inputs(states, rows)
            return self._xent_kernels(depth, st, rw, targets.to(device=st.device, dtype=torch.float32).contiguous(), None, weights, scale, True)
        return self._xent_torch(states, rows, targets, weights, scale, True)

    @torch.no_grad()
    def xent_at(self, states, rows, index, targets, weights=None):
        """The losses of xent_step_at without gradients or statistics (held-out data): (losses float32 [n], entropy float32 [n]);
        weights only decide which positions count.  bbx_pmlp_xent_at / bbx_pmlp2_xent_at, or the torch path."""
        depth = self._kernel_depth(states, rows, in_place=True)
        if depth and self._targets_in_place(targets, states):
            return self._xent_kernels(depth, states, rows, targets, _index32(index, states), weights, None, False)
        return self.xent(*_gather(index, states, rows, targets), weights=weights)

    @torch.no_grad()
    def xent(self, states, rows, targets, weights=None):
        """xent_at for gathered tensors (bbx_pmlp_xent / bbx_pmlp2_xent, or the torch path)."""
        N, R, cols = states.shape
        depth = self._kernel_depth(states)
        if depth:
            st, rw, _ = _kernel_inputs(states, rows)
            return self._xent_kernels(depth, st, rw, targets.to(device=st.device, dtype=torch.float32).contiguous(), None, weights, None, False)
        return self._xent_torch(states, rows, targets, weights, None, False)[1:]

    @staticmethod
    def _targets_in_place(targets, states):
        R, cols = states.shape[-2:]
        return (targets.is_cuda and targets.dtype == torch.float32 and targets.is_contiguous() and targets.shape[-1] == R
                and targets.numel() * cols == states.numel())

    def _xent_kernels(self, depth, states, rows, targets, index, weights, scale, grad):
        stem = "bbx_pmlp_xent" if depth == 1 else "bbx_pmlp2_xent"
        fn, head, S, N, R, cols = _call_head(stem + ("_grad" if grad else ""), states, rows, targets, index)
        dev = states.device
        if targets.numel() != S * R:
            raise ValueError("xent: %d states of %d rows, %d targets" % (S, R, targets.numel()))
        w = None if weights is None else weights.to(device=dev, dtype=torch.float32).contiguous()
        if w is not None and w.numel() != N:
            raise ValueError("xent: %d positions, %d weights" % (N, w.numel()))
        sc = C.c_float((1.0 / N if N else 0.0) if scale is None else float(scale))
        new = lambda n: torch.empty(n, dtype=torch.float32, device=dev)
        losses, ent = new(N), new(N)
        with torch.cuda.device(dev):
            pw = self._fused_weights() if depth == 1 else self._deep_weights()
            hidden = (pw["hidden"],) if depth == 1 else tuple(pw["hidden"])
            if not grad:
                _ffi.check(fn(*head, pw["prepared"], *hidden, _ptr(w), sc, _ptr(losses), _ptr(ent), _stream()))
                return losses, ent
            coef = new(2 * N)
            stats = torch.empty(6, dtype=torch.float64, device=dev)
            grads = _grad_arrays(cols, hidden, dev)
            ws = self._workspace("_ppo_ws", getattr(_ffi.lib(), stem + "_workspace_floats")(N, R, cols, *hidden), dev)
            _ffi.check(fn(*head, pw["prepared"], *hidden, _ptr(w), sc, _ptr(losses), _ptr(ent), _ptr(coef), _ptr(stats), _ptr(ws),
                          *[_ptr(g) for g in grads], _stream()))
        _add_to_grad(self._kernel_params(), _linear_layouts(grads))
        return stats, losses, ent

    def _xent_torch(self, states, rows, targets, weights, scale, backward):
        """The cross-entropy of the kernels with torch ops (any depth, any device) and, with `backward`, backward() through it:
        (stats, losses, entropy) as xent_step returns them."""
        N, R, _ = states.shape
        if rows is None:
            n = (states[:, :, -1] != -1).sum(1)
        else:
            n = torch.clamp(rows.to(device=states.device, dtype=torch.int64), 0, R)
        live = torch.arange(R, device=states.device)[None, :] < n[:, None]
        with torch.set_grad_enabled(backward):
            z = self._logits(states)
            lp = torch.log_softmax(torch.where(live, z, torch.full_like(z, -1e9)), dim=-1)
            lpl = torch.where(live, lp, torch.zeros_like(lp))
            t = torch.where(live, targets.to(device=z.device, dtype=z.dtype), torch.zeros_like(z))
            w = torch.ones(N, dtype=z.dtype, device=z.device) if weights is None else weights.to(device=z.device, dtype=z.dtype)
            counted = ~(((t < 0) | ~torch.isfinite(t)).any(dim=1)) & torch.isfinite(w)
            t = torch.where(counted[:, None], t, torch.zeros_like(t))
            w = torch.where(counted, w, torch.zeros_like(w))
            l = -(t * lpl).sum(dim=1)
            H = -(torch.exp(lpl) * lpl * live.to(lp.dtype)).sum(dim=1)
            sc = (1.0 / N if N else 0.0) if scale is None else float(scale)
            if backward and N:
                loss = sc * (w * l).sum()
                if loss.requires_grad:
                    loss.backward()
        d = lambda x: x.detach().to(torch.float64).sum()
        stats = torch.stack([d(counted), d(w * l), d(w * t.sum(dim=1)), d(torch.where(counted, H, torch.zeros_like(H))), d(w), d(~counted)])
        nan = torch.full_like(l, float("nan"))
        return stats, torch.where(counted, l, nan).detach(), H.detach()

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


class PMLPValue(_PMLPKernels):
    """A learned value baseline (critic) over the observation block: the row embedding of PMLPPolicy (`embedding`, relu), one
    linear unit per row (`head`), and a pool over a state's live rows in place of the softmax:
        pool="sum"   V = sum_r z_r        pool="mean"   V = that sum / n        pool="lse"   V = log sum_r exp z_r
    A state without live rows is worth 0.  One hidden layer of at most 256 units over at most 64 columns, float32 on the GPU: the
    HIP kernels (bbx_pmlp_value / bbx_pmlp_value_grad / bbx_pmlp_value_fit and their _at forms, which read a trajectory buffer in
    place); two hidden layers of at most 128 units with deep_kernels set: their two-layer counterparts (bbx_pmlp2_value / ..._grad /
    ..._fit and the _at forms); CPU tensors, two layers without the flag, more hidden layers or wider ones: the torch path (forward,
    values_torch, evaluate_torch).  `last_path` names the path the last call took ("kernels" or "torch")."""

    POOLS = {"sum": 0, "mean": 1, "lse": 2}                           # BBX_POOL_* of include/bbx.h

    def __init__(self, cols, hidden_layers=(128,), pool="sum", deep_kernels=False):
        super().__init__()
        self.deep_kernels = deep_kernels                              # two hidden layers: the bbx_pmlp2_value* kernels in place of the torch path
        if pool not in self.POOLS:
            raise ValueError("PMLPValue: pool is one of %s (got %r)" % (sorted(self.POOLS), pool))
        dims = [cols] + list(hidden_layers)
        self.embedding = torch.nn.ModuleList([torch.nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:])])
        self.head = torch.nn.Linear(dims[-1], 1)
        self.cols, self.pool, self.pool_id = cols, pool, self.POOLS[pool]
        self.last_path = None

    @property
    def _last(self):
        return self.head

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
        return self._kernel_depth(states) in (1, 2)

    def _in_place(self, states, rows):
        """Whether the _at kernels can read states [..., R, cols] and rows where they lie."""
        return self._kernel_depth(states, rows, in_place=True) in (1, 2)

    def _deep_weights(self):
        """The two-layer kernels' view of the weights (the two-layer policy's layout), refilled in place (_prepared_weights)."""
        return self._prepared_weights("_deep_cache", self.embedding, self.head, True)

    def _kernels(self):
        """(the entry points' stem, the prepared weights, the hidden sizes as a tuple) of this module's depth."""
        if len(self.embedding) == 1:
            w = self._fused_weights()
            return "bbx_pmlp_value", w, (w["hidden"],)
        w = self._deep_weights()
        return "bbx_pmlp2_value", w, tuple(w["hidden"])

    def _evaluate_kernels(self, states, rows, index=None):
        self.last_path = "kernels"
        fn = _PMLPValueEvaluate if len(self.embedding) == 1 else _PMLP2ValueEvaluate
        return fn.apply(self, states, rows, *self._kernel_params(), index)

    def _fused_weights(self):
        """The kernels' view of the weights (the one-layer policy's layout), refilled in place (_prepared_weights)."""
        if len(self.embedding) != 1:
            raise ValueError("_fused_weights: the kernels take one hidden layer (this critic has %d)" % len(self.embedding))
        return self._prepared_weights("_fused_cache", self.embedding, self.head, True)

    def _value_call(self, states, rows, index, out, out64):
        dev = states.device
        with torch.cuda.device(dev):
            stem, w, hidden = self._kernels()
        fn, head, _, N, _, _ = _call_head(stem, states, rows, None, index)
        if out is None and out64 is None:
            out = torch.empty(N, dtype=torch.float32, device=dev)
        for o, dt in ((out, torch.float32), (out64, torch.float64)):
            if o is not None and not (o.is_cuda and o.dtype == dt and o.is_contiguous() and o.numel() == N):
                raise ValueError("PMLPValue.values: out / out64 are contiguous float32 / float64 CUDA tensors of %d elements" % N)
        with torch.cuda.device(dev):
            _ffi.check(fn(*head, w["prepared"], *hidden, self.pool_id, _ptr(out), _ptr(out64), _stream()))
        self.last_path = "kernels"
        return out if out is not None else out64

    @torch.no_grad()
    def values(self, states, rows, out=None, out64=None):
        """Values of states int [..., R, cols] with rows [...] live rows each, no autograd: float32 into `out` and / or the same
        numbers widened into `out64` (float64: what DeviceTrajectoryBuffer.values holds), each of rows.numel() elements; neither:
        a new float32 tensor.  Returns out (out64 where only that was given).  On the GPU under kernels_ok: one bbx_pmlp_value
        (two hidden layers: bbx_pmlp2_value) call, over the tensors in place where they are contiguous int32; otherwise values_torch."""
        if not self.kernels_ok(states):
            return self.values_torch(states, rows, out, out64)
        st, rw, _ = _kernel_inputs(states, rows)
        return self._value_call(st, rw, None, out, out64)

    @torch.no_grad()
    def values_at(self, states, rows, index, out=None, out64=None):
        """values() of the recorded states index[k] of the buffers states [S, R, cols] or [T, B, R, cols] and rows, read in place
        (bbx_pmlp_value_at; an index outside the buffer: NaN); where the kernels cannot read them in place the n states are
        gathered."""
        if self._in_place(states, rows):
            return self._value_call(states, rows, _index32(index, states), out, out64)
        return self.values(*_gather(index, states, rows), out, out64)

    def evaluate(self, states, rows=None):
        """Values float32 [N] of states int [N, R, cols], differentiable with respect to the module's parameters: under kernels_ok
        bbx_pmlp_value forward and bbx_pmlp_value_grad backward; otherwise evaluate_torch."""
        if not self.kernels_ok(states):
            return self.evaluate_torch(states, rows)
        st, rw, _ = _kernel_inputs(states, rows)
        return self._evaluate_kernels(st, rw)

    def evaluate_at(self, states, rows, index):
        """evaluate() of the recorded states index[k] without gathering them (bbx_pmlp_value_at / bbx_pmlp_value_grad_at), as
        PMLPPolicy.evaluate_at; where the kernels cannot read the buffers in place the n states are gathered."""
        if self._in_place(states, rows):
            return self._evaluate_kernels(states, rows, _index32(index, states))
        return self.evaluate(*_gather(index, states, rows))

    def fit_step_at(self, states, rows, index, targets):
        """One minibatch of the squared-error fit in one library call (bbx_pmlp_value_fit_at): from the recorded states index[k] of
        the buffers states / rows and the targets [n] to the gradients of
            L = 1/2 mean_k (V_k - target_k)^2
        ADDED to the parameters' .grad as loss.backward() would.  Returns (stats float64 [6] on the device: counted positions,
        sum d^2, sum V, sum target, sum target^2, positions not counted; values float32 [n]) — nothing is read back, nothing waits.
        Where the kernels cannot read the buffers in place: fit_step on the gathered states."""
        if self._in_place(states, rows):
            return self._fit_kernels(states, rows, _index32(index, states), targets)
        return self.fit_step(*_gather(index, states, rows), targets)

    def fit_step(self, states, rows, targets):
        """fit_step_at for gathered tensors: states int [N, R, cols], rows [N] (None: the rows whose last column is not -1) —
        bbx_pmlp_value_fit under kernels_ok; otherwise the same formulae with torch ops and backward()."""
        if self.kernels_ok(states):
            st, rw, _ = _kernel_inputs(states, rows)
            return self._fit_kernels(st, rw, None, targets)
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
        dev = states.device
        with torch.cuda.device(dev):
            stem, w, hidden = self._kernels()
        fn, head, _, N, R, cols = _call_head(stem + "_fit", states, rows, None, index)
        tg = targets.to(device=dev, dtype=torch.float32).contiguous()
        if tg.numel() != N:
            raise ValueError("fit_step: %d positions, %d targets" % (N, tg.numel()))
        values, coef = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(2))
        stats = torch.empty(6, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            grads = _grad_arrays(cols, hidden, dev)
            ws = self._workspace("_ws", getattr(_ffi.lib(), stem + "_fit_workspace_floats")(N, R, cols, *hidden), dev)
            _ffi.check(fn(*head, w["prepared"], *hidden, self.pool_id, _ptr(tg), C.c_float(1.0 / N if N else 0.0), _ptr(values), _ptr(coef),
                          _ptr(stats), _ptr(ws), *[_ptr(g) for g in grads], _stream()))
        self.last_path = "kernels"
        _add_to_grad(self._kernel_params(), _linear_layouts(grads))
        return stats, values
