"""Every output array of the PMLP training and policy kernels on fixed-seed cases, for a byte-for-byte comparison of two builds
(a refactor of bbx_pmlp.h / bbx_pmlp_grad.h / bbx_pmlp_value.h / bbx_pmlp2_grad.h must not move a bit).

    python scripts/dump_pmlp_outputs.py OUT.npz            the tree this file lies in: build it first; needs a GPU; seconds
    python scripts/dump_pmlp_outputs.py --compare A.npz B.npz     exit status 1 and the names of the arrays that differ; arrays of
                                                                  groups that only the second file has (written by a later tree
                                                                  with more entry points) are counted, not compared

Cases, from the generators of tests/ (value_cases.grad_case over policy_cases): per shape nine states with 0, 1, 2, 31, 32, 33, 64,
65 and 129 live rows in blocks of 130 rows (three waves per unit group, each striding over three states; one recorded action
outside its state's rows), and an index list with a repeated index, -1 and n_src.  The shapes between them reach every unit-block
count NB in {1, 2, 4, 8} and every k-step count KS in {3, 6, 10, 16, 32} of the one-layer kernels, two column blocks (64 columns) and
more than one unit group (256 units).  Calls: bbx_pmlp_grad[_at] with and without d_gent, bbx_pmlp_value_grad[_at] for the three pools,
bbx_pmlp_ppo_grad_at and bbx_pmlp_value_fit_at with statistics and workspace tail, bbx_pmlp_act, bbx_pmlp_act_greedy; once:
bbx_pmlp2_grad, and one bbx_policy_step_device step (the fused step kernel) on 64 environments with 6 and with 12 columns.
A second group, module/..., goes through the Python classes instead (a refactor of deepgroebner_amd/pmlp.py must not move a bit
either): see module_arrays.  A third, value2/... and module2/..., holds the two-layer critic: bbx_pmlp2_value[_at],
bbx_pmlp2_value_grad[_at] and bbx_pmlp2_value_fit_at for the three pools on the two-layer case's states and weights, and the public
methods of a PMLPValue with deep_kernels (value2_arrays)."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SHAPES = [(6, 32), (11, 64), (12, 128), (6, 256), (20, 100), (32, 256), (64, 48), (64, 256)]    # (cols, hidden)
LIVE = (0, 1, 2, 31, 32, 33, 64, 65, 129)
R = 130
INDEX = (8, 3, 3, -1, 9, 0, 5, 7, 1, 2, 6, 4)                    # into the nine states: 3 twice, -1 and n_src out of range


def compare(a, b):
    A, B = np.load(a), np.load(b)
    group = lambda k: k.split("/")[0]
    new = sorted(k for k in B.files if group(k) not in {group(x) for x in A.files})
    bad = sorted((set(A.files) ^ set(B.files)) - set(new))
    bad += [k for k in A.files if k in B.files and (A[k].dtype != B[k].dtype or A[k].shape != B[k].shape or A[k].tobytes() != B[k].tobytes())]
    print("%d arrays, %d bytes; differing: %s%s" % (len(A.files), sum(A[k].nbytes for k in A.files), bad or "none",
                                                    "; %d arrays of groups only the second file has (%s)" % (len(new), ", ".join(sorted({group(k) for k in new}))) if new else ""))
    return 1 if bad else 0


def module_arrays(keep, device="cuda"):
    """The second group, module/...: the same kind of cases through the public methods of PMLPPolicy and PMLPValue and through
    ppo_update / value_update, on the first and third shape of SHAPES and the two-layer case."""
    import torch
    from deepgroebner_amd import DeviceTrajectoryBuffer, ppo_update, value_update
    from tests import policy_cases as pc
    from tests import value_cases as vc
    dev = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a if dt is None else np.asarray(a, dtype=dt))).to(device)
    grads = lambda m: [q.grad for q in m.parameters()]
    for cols, hidden in ((6, (32,)), (12, (128,)), (12, (64, 128))):
        tag = "module/" + pc.label(cols, hidden)
        w, obs, rows = vc.value_case(cols, hidden, LIVE, R, 5100 + cols + sum(hidden))
        rng = np.random.default_rng(88 + cols + len(hidden))
        N = len(rows)
        actions = (rng.integers(0, 1 << 30, size=N) % np.maximum(rows, 1)).astype(np.int32)
        actions[4] = rows[4]                                      # one action outside the live rows
        dobs, drows, dact, dindex = dev(obs), dev(rows), dev(actions), dev(INDEX, np.int32)
        n = len(INDEX)
        per = {m: [dev(rng.normal(size=m), np.float32) for _ in range(3)] for m in (N, n)}

        def policy():
            pol = pc.to_policy(w, device)
            pol.deep_kernels = len(hidden) == 2
            return pol

        for at in (False, True):
            a, b, c = per[n if at else N]
            sfx = "_at" if at else ""
            pol = policy()
            lp, ent = pol.evaluate_at(dobs, dact, drows, dindex) if at else pol.evaluate(dobs, dact, drows)
            torch.autograd.backward((lp, ent), (a, b))
            keep("%s/evaluate%s" % (tag, sfx), lp.detach(), ent.detach(), *grads(pol))
            for mode in ("pg", "clip", "penalty"):
                pol = policy()
                kw = dict(clip=0.2, ent_coef=0.01, mode=mode, c_kl=0.5)
                res = pol.ppo_step_at(dobs, dact, drows, dindex, a, b, **kw) if at else pol.ppo_step(dobs, dact, drows, a, b, **kw)
                keep("%s/ppo_step%s/%s" % (tag, sfx, mode), *res, *grads(pol))
            if len(hidden) != 1:
                continue
            for pool in vc.POOLS:
                what = "%s/%%s%s/%s" % (tag, sfx, pool)
                cr = vc.to_critic(w, pool, device)
                keep(what % "values", cr.values_at(dobs, drows, dindex) if at else cr.values(dobs, drows))
                v = cr.evaluate_at(dobs, drows, dindex) if at else cr.evaluate(dobs, drows)
                v.backward(c)
                keep(what % "evaluate", v.detach(), *grads(cr))
                cr = vc.to_critic(w, pool, device)
                res = cr.fit_step_at(dobs, drows, dindex, c) if at else cr.fit_step(dobs, drows, c)
                keep(what % "fit_step", *res, *grads(cr))

        # one epoch of each update loop, in order, with SGD, on a buffer of 6 steps of 4 environments written by hand
        T, B, RB = 6, 4, 8
        buf = DeviceTrajectoryBuffer(T, B, obs_shape=(RB, cols), device=device)
        brows = rng.integers(1, RB + 1, size=(T, B)).astype(np.int32)
        bobs = pc.fill_padding(pc.random_blocks(T * B, RB, cols, 97 + cols, emax=3), brows.reshape(-1), False).reshape(T, B, RB, cols)
        dones = rng.random(size=(T, B)) < 0.3
        dones[T - 1, :3] = True                                   # (the fourth environment's last episode stays incomplete)
        buf.states.copy_(dev(bobs)); buf.rows.copy_(dev(brows)); buf.dones.copy_(dev(dones))
        buf.actions.copy_(dev((rng.integers(0, 1 << 30, size=(T, B)) % brows).astype(np.int32)))
        buf.rewards.copy_(dev(-rng.integers(1, 20, size=(T, B)).astype(np.float64)))
        buf.logprobs.copy_(dev(-rng.random(size=(T, B)) * 2.0, np.float32))
        buf.t = T
        pol = policy()
        ep = ppo_update(pol, buf, torch.optim.SGD(pol.parameters(), lr=0.01), 1, 5, ent_coef=0.01, shuffle=False)
        keep("%s/ppo_update" % tag, *[torch.as_tensor(np.asarray(ep[0][k], dtype=np.float64)) for k in ("stats", "loss", "entropy", "kl", "clip_frac")],
             *[q.detach() for q in pol.parameters()])
        if len(hidden) == 1:
            for pool in vc.POOLS:
                cr = vc.to_critic(w, pool, device)
                ep = value_update(cr, buf, torch.optim.SGD(cr.parameters(), lr=0.01), 1, 5, shuffle=False)
                keep("%s/value_update/%s" % (tag, pool), *[torch.as_tensor(np.asarray(ep[0][k], dtype=np.float64)) for k in ("stats", "loss", "explained_variance")],
                     *[q.detach() for q in cr.parameters()])


def value2_arrays(keep, lib, p, dev, nan, stream):
    """The third group: the two-layer critic through the C ABI (value2/...) and through PMLPValue(deep_kernels=True) (module2/...)."""
    import torch
    from deepgroebner_amd import _ffi
    from tests import policy_cases as pc
    from tests import value_cases as vc
    cols, hidden = 12, (64, 128)
    w, obs, rows, g = vc.grad_case(cols, hidden, LIVE, R, 6100)
    N, index = len(rows), np.array(INDEX, dtype=np.int32)
    n = len(index)
    rng = np.random.default_rng(6101)
    dobs, drows, dindex = dev(obs), dev(rows), dev(index)
    per = {m: [dev(rng.normal(size=m), np.float32) for _ in range(2)] for m in (N, n)}
    pol = pc.to_policy(w, "cuda")
    dw = pol._deep_weights()
    h1, h2 = dw["hidden"]
    grads = lambda: [nan(cols * h1), nan(h1), nan(h1 * h2), nan(h2), nan(h2), nan(1)]
    for pool in range(3):
        for at in (False, True):
            m, sfx = (n, "_at") if at else (N, "")
            cnt = (N, p(dindex), n) if at else (N,)
            c, d = per[m]
            v32, v64 = nan(m), nan(m, torch.float64)
            _ffi.check(getattr(lib, "bbx_pmlp2_value" + sfx)(p(dobs), p(drows), *cnt, R, cols, dw["prepared"], h1, h2, pool, p(v32), p(v64), stream()))
            keep("value2/value%s/pool%d" % (sfx, pool), v32, v64)
            G, ws = grads(), nan(lib.bbx_pmlp2_value_grad_workspace_floats(m, R, cols, h1, h2))
            _ffi.check(getattr(lib, "bbx_pmlp2_value_grad" + sfx)(p(dobs), p(drows), *cnt, R, cols, dw["prepared"], h1, h2, pool, p(c), p(ws), *map(p, G), stream()))
            keep("value2/value_grad%s/pool%d" % (sfx, pool), *G)
        gfl = lib.bbx_pmlp2_grad_workspace_floats(n, R, cols, h1, h2)
        G, ws = grads(), nan(lib.bbx_pmlp2_value_fit_workspace_floats(n, R, cols, h1, h2))
        val, coef, stats = nan(n), nan(n), nan(6, torch.float64)
        _ffi.check(lib.bbx_pmlp2_value_fit_at(p(dobs), p(drows), N, p(dindex), n, R, cols, dw["prepared"], h1, h2, pool, p(per[n][1]), C.c_float(1.0 / n), p(val),
                                              p(coef), p(stats), p(ws), *map(p, G), stream()))
        keep("value2/value_fit_at/pool%d" % pool, val, coef, stats, ws[gfl:], *G)
    pgrads = lambda m: [q.grad for q in m.parameters()]
    for pool in vc.POOLS:
        for at in (False, True):
            c = per[n if at else N][0]
            what = "module2/%s/%%s%s/%s" % (pc.label(cols, hidden), "_at" if at else "", pool)
            new = lambda: vc.to_critic(w, pool, "cuda")
            cr = new(); cr.deep_kernels = True
            keep(what % "values", cr.values_at(dobs, drows, dindex) if at else cr.values(dobs, drows))
            v = cr.evaluate_at(dobs, drows, dindex) if at else cr.evaluate(dobs, drows)
            v.backward(c)
            keep(what % "evaluate", v.detach(), *pgrads(cr))
            cr = new(); cr.deep_kernels = True
            res = cr.fit_step_at(dobs, drows, dindex, c) if at else cr.fit_step(dobs, drows, c)
            keep(what % "fit_step", *res, *pgrads(cr))


def main(path):
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv, _ffi
    from tests import policy_cases as pc
    from tests import value_cases as vc
    lib = _ffi.lib()
    out = {}
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    dev = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a if dt is None else np.asarray(a, dtype=dt))).cuda()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan = lambda n, dt=torch.float32: torch.full((n,), float("nan"), dtype=dt, device="cuda")

    def keep(name, *tensors):
        torch.cuda.synchronize()
        for i, t in enumerate(tensors):
            out["%s/%d" % (name, i)] = t.cpu().numpy()

    for cols, hidden in SHAPES:
        tag = "%dx%d" % (cols, hidden)
        w, obs, rows, g = vc.grad_case(cols, (hidden,), LIVE, R, 4100 + cols + hidden)
        rng = np.random.default_rng(77 + cols)
        N = len(rows)
        actions = (rng.integers(0, 1 << 30, size=N) % np.maximum(rows, 1)).astype(np.int32)
        actions[4] = rows[4]                                      # one action outside the live rows
        index = np.array(INDEX, dtype=np.int32)
        n = len(index)
        pol = pc.to_policy(w, "cuda")
        fw = pol._fused_weights()
        prep, H = fw["prepared"], fw["hidden"]
        dobs, drows, dact, dindex = dev(obs), dev(rows), dev(actions), dev(index)
        per = {N: [dev(rng.normal(size=N), np.float32) for _ in range(4)], n: [dev(rng.normal(size=n), np.float32) for _ in range(4)]}
        grads = lambda: [nan(cols * hidden), nan(hidden), nan(hidden), nan(1)]
        for at in (False, True):
            m = n if at else N
            src = (p(dobs), p(drows))
            cnt = (N, p(dindex), n) if at else (N,)
            a, b, c, d = per[m]
            sfx = "_at" if at else ""
            for gent in (b, None):
                G, ws = grads(), nan(lib.bbx_pmlp_grad_workspace_floats(m, R, cols, hidden))
                _ffi.check(getattr(lib, "bbx_pmlp_grad" + sfx)(*src, p(dact), *cnt, R, cols, prep, H, p(a), p(gent), p(ws), *map(p, G), stream()))
                keep("%s/grad%s/%s" % (tag, sfx, "gent" if gent is not None else "nogent"), *G)
            for pool in range(3):
                G, ws = grads(), nan(lib.bbx_pmlp_value_grad_workspace_floats(m, R, cols, hidden))
                _ffi.check(getattr(lib, "bbx_pmlp_value_grad" + sfx)(*src, *cnt, R, cols, prep, H, pool, p(c), p(ws), *map(p, G), stream()))
                keep("%s/value_grad%s/pool%d" % (tag, sfx, pool), *G)
        a, b, c, d = per[n]
        gfl = lib.bbx_pmlp_grad_workspace_floats(n, R, cols, hidden)
        for mode in (0, 1, 2):
            G, ws = grads(), nan(lib.bbx_pmlp_ppo_workspace_floats(n, R, cols, hidden))
            lp, ent, coef, stats = nan(n), nan(n), nan(2 * n), nan(6, torch.float64)
            _ffi.check(lib.bbx_pmlp_ppo_grad_at(p(dobs), p(drows), p(dact), N, p(dindex), n, R, cols, prep, H, p(a), p(b), mode, C.c_float(1.0 / n),
                                                C.c_float(0.2), C.c_float(0.01), C.c_float(0.5), p(lp), p(ent), p(coef), p(stats), p(ws), *map(p, G), stream()))
            keep("%s/ppo_grad_at/mode%d" % (tag, mode), lp, ent, coef, stats, ws[gfl:], *G)
        for pool in range(3):
            G, ws = grads(), nan(lib.bbx_pmlp_value_fit_workspace_floats(n, R, cols, hidden))
            val, coef, stats = nan(n), nan(n), nan(6, torch.float64)
            _ffi.check(lib.bbx_pmlp_value_fit_at(p(dobs), p(drows), N, p(dindex), n, R, cols, prep, H, pool, p(d), C.c_float(1.0 / n), p(val), p(coef),
                                                 p(stats), p(ws), *map(p, G), stream()))
            keep("%s/value_fit_at/pool%d" % (tag, pool), val, coef, stats, ws[gfl:], *G)
        u = dev(rng.random(size=N), np.float32)
        for greedy in (False, True):
            A, L = torch.full((N,), -7, dtype=torch.int32, device="cuda"), nan(N)
            if greedy:
                _ffi.check(lib.bbx_pmlp_act_greedy(p(dobs), p(drows), N, R, cols, prep, H, p(A), p(L), stream()))
            else:
                _ffi.check(lib.bbx_pmlp_act(p(dobs), p(drows), N, R, cols, prep, H, p(u), p(A), p(L), stream()))
            keep("%s/act%s" % (tag, "_greedy" if greedy else ""), A, L)
        if (cols, hidden) == (12, 128):                           # two hidden layers, once, on the same states
            w2 = pc.make_weights(cols, (64, 128), 4300)
            pol2 = pc.to_policy(w2, "cuda")
            dw = pol2._deep_weights()
            h1, h2 = dw["hidden"]
            G = [nan(cols * h1), nan(h1), nan(h1 * h2), nan(h2), nan(h2), nan(1)]
            ws = nan(lib.bbx_pmlp2_grad_workspace_floats(N, R, cols, h1, h2))
            a, b = per[N][:2]
            _ffi.check(lib.bbx_pmlp2_grad(p(dobs), p(drows), p(dact), N, R, cols, dw["prepared"], h1, h2, p(a), p(b), p(ws), *map(p, G), stream()))
            keep("%s/pmlp2_grad" % tag, *G)

    for k in (1, 2):                                              # the fused policy + step kernel: 6 and 12 columns, 128 units
        B, RO = 64, 64
        env = VecLeadMonomialsEnv("3-20-10-weighted", batch=B, k=k)
        env.seed(np.arange(B) + 500); env.reset(); env.accounting(False)
        pol = pc.to_policy(pc.make_weights(env.cols, (128,), 4400 + k), "cuda")
        fw = pol._fused_weights()
        s = torch.cuda.current_stream().cuda_stream
        rew, done = torch.zeros(B, dtype=torch.float64, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda")
        obs, rows = torch.full((B, RO, env.cols), -1, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
        env.rollout_device("first", 0, False, s, rew, done, rows, obs, RO, True, False); env.sync()
        u = dev(np.random.default_rng(4500 + k).random(size=B), np.float32)
        A, L = torch.full((B,), -7, dtype=torch.int32, device="cuda"), nan(B)
        env.policy_step_device(fw["prepared"], fw["hidden"], u, A, L, rew, done, rows, obs, RO, 1, s); env.sync()
        keep("policy_step/k%d" % k, A, L, rew, done, rows, obs)

    module_arrays(keep)
    value2_arrays(keep, lib, p, dev, nan, stream)
    np.savez(path, **out)
    print("%d arrays, %d bytes -> %s" % (len(out), sum(v.nbytes for v in out.values()), path))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2 or sys.argv[1].startswith("-"):
        sys.exit(__doc__)
    main(sys.argv[1])
