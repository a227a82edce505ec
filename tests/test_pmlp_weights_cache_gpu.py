"""The prepared-weights contract of deepgroebner_amd.pmlp, for every kind of module that has kernels: a backward pass differentiates
the weights of ITS OWN forward pass, whatever happened to the parameters in between — although the one-layer policy allocates a
fresh prepared buffer per weight version and the two-layer policy and the critic refill one buffer in place.

How the parameters change in between matters to torch before it matters here.  The autograd functions save the parameters for
backward, so a change IN PLACE (p.add_(0.25) under no_grad, an optimiser step) bumps their version counters and torch itself refuses
the backward pass ("modified by an inplace operation") before any kernel runs: measured on an MI355X with the functions as they
were before the kernel-call layer was shared, and unchanged since.  What reaches the kernels' backward with other weights in the
module is a change that gives the parameters new storage (p.data = ...; Module.to, .float()): the versions stay, the addresses in
the cache key move, the cache rebuilds.  The test pins both."""
import types

import pytest

from tests import policy_cases as pc
from tests import value_cases as vc

pytestmark = pytest.mark.gpu

COLS, R, LIVE = 6, 4, (0, 1, 2, 4)                                    # four states in blocks of 4 rows
ACTIONS = (0, 0, 1, 3)
COTANGENTS = ((0.5, -1.0, 2.0, 0.25), (1.0, 0.5, -0.75, 0.125))
KINDS = {"policy": ((32,), None), "policy2": ((32, 32), None), "critic-sum": ((32,), "sum"), "critic-mean": ((32,), "mean"),
         "critic-lse": ((32,), "lse")}                                # (hidden layers, pool)


def _forward_backward(kind, change):
    """A fresh module of `kind`: evaluate; every parameter moved by 0.25 — change "in place": p.add_, "storage": p.data = a new
    tensor, None: not at all —; backward."""
    import torch
    hidden, pool = KINDS[kind]
    w, obs, rows = vc.value_case(COLS, hidden, LIVE, R, 9100 + len(hidden))
    obs, rows = torch.from_numpy(obs).cuda(), torch.from_numpy(rows).cuda()
    if pool is None:
        m = pc.to_policy(w, "cuda")
        m.deep_kernels = len(hidden) == 2
        actions = torch.tensor(ACTIONS, dtype=torch.int32, device="cuda")
        run = lambda: m.evaluate(obs, actions, rows)
        record = m._fused_weights if len(hidden) == 1 else m._deep_weights
    else:
        m = vc.to_critic(w, pool, "cuda")
        run = lambda: (m.evaluate(obs, rows),)
        record = m._fused_weights
    out = run()
    assert type(out[0].grad_fn).__name__.startswith("_PMLP"), "the kernel path"
    rec = record()
    buffer = rec["keep"] if len(hidden) == 1 else rec["keep"][0]
    held = buffer.cpu().numpy().tobytes()
    if change:
        with torch.no_grad():
            for p in m.parameters():
                if change == "in place":
                    p.add_(0.25)
                else:
                    p.data = p.data + 0.25
        record()                                                      # (a buffer that is refilled in place holds the new weights from here)
    torch.autograd.backward(out, [torch.tensor(c, device="cuda") for c in COTANGENTS[:len(out)]])
    return types.SimpleNamespace(run=run, record=record, rec=rec, buffer=buffer, held=held, out=[o.detach().cpu().numpy() for o in out],
                                 grads=[p.grad.cpu().numpy() for p in m.parameters()])


@pytest.mark.parametrize("kind", list(KINDS))
def test_backward_reads_the_weights_of_its_own_forward_pass(kind):
    hidden, _ = KINDS[kind]
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        _forward_backward(kind, change="in place")
    plain = _forward_backward(kind, change=None)
    moved = _forward_backward(kind, change="storage")
    assert [o.tobytes() for o in moved.out] == [o.tobytes() for o in plain.out]
    assert len(moved.grads) == len(plain.grads) == 2 * len(hidden) + 2
    for g, want in zip(moved.grads, plain.grads):
        assert g.dtype == want.dtype and g.shape == want.shape and g.tobytes() == want.tobytes(), kind
    # the cache did notice the change
    again = [o.detach().cpu().numpy() for o in moved.run()]
    assert any(a.tobytes() != o.tobytes() for a, o in zip(again, moved.out)), kind
    if kind == "policy":                                              # a fresh buffer per version: the earlier one keeps its bytes
        assert moved.buffer.cpu().numpy().tobytes() == moved.held
    else:                                                             # refilled in place
        assert moved.record()["prepared"].value == moved.rec["prepared"].value
