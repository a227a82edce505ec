"""Expert iteration on 3-20-10-weighted: the PMLP policy is trained towards a one-step lookahead of a strategy's action values.

Per iteration: a batch of environments steps under the CURRENT policy (sampled); at every step the target row of every environment
— action_value_targets(env.action_values(strategy), ...), a softmax of Q(s, a) = r + gamma * value(strategy) over the state's pairs at
--temperature — is recorded beside the state in a DeviceTrajectoryBuffer(targets=True); then imitation_update runs --epochs passes of
cross-entropy minibatches over every recorded state (PMLPPolicy.xent_step_at: bbx_pmlp_xent_grad_at), and evaluate_policy(greedy=True)
measures the greedy policy on fresh episodes.  Prints one line per iteration: loss of the last epoch and mean greedy return.

    python scripts/train_lookahead.py [--envs 64] [--iterations 10] [--steps 16] [--rows 128] [--hidden 128] [--temperature 1.0]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from deepgroebner_amd import VecLeadMonomialsEnv
from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, action_value_targets, evaluate_policy, imitation_update

ap = argparse.ArgumentParser()
ap.add_argument("--dist", default="3-20-10-weighted")
ap.add_argument("--envs", type=int, default=64)
ap.add_argument("--iterations", type=int, default=10)
ap.add_argument("--steps", type=int, default=16, help="vector steps recorded per iteration")
ap.add_argument("--rows", type=int, default=128, help="rows of the observation block (a pair set with more rows is an error, never cut)")
ap.add_argument("--hidden", type=lambda t: [int(h) for h in t.split(",")], default=[128])
ap.add_argument("--strategy", default="degree")
ap.add_argument("--gamma", type=float, default=0.99)
ap.add_argument("--temperature", type=float, default=1.0)
ap.add_argument("--epochs", type=int, default=4)
ap.add_argument("--batch-size", type=int, default=256)
ap.add_argument("--lr", type=float, default=1e-3)
ap.add_argument("--eval-episodes", type=int, default=2)
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("train_lookahead: no GPU")

torch.manual_seed(a.seed)
B, T, R = a.envs, a.steps, a.rows
env = VecLeadMonomialsEnv(a.dist, batch=B, k=2)
env.seed(np.arange(B) + 1000 * a.seed + 1); env.reset()
test = VecLeadMonomialsEnv(a.dist, batch=B, k=2)
policy = PMLPPolicy(env.cols, a.hidden, deep_kernels=len(a.hidden) == 2).cuda()
opt = torch.optim.Adam(policy.parameters(), lr=a.lr)
gen = torch.Generator(device="cuda"); gen.manual_seed(a.seed)
stream = torch.cuda.current_stream().cuda_stream
obs = torch.empty((B, R, env.cols), dtype=torch.int32, device="cuda")
rew = torch.zeros(B, dtype=torch.float64, device="cuda"); done = torch.zeros(B, dtype=torch.uint8, device="cuda")
rows = torch.zeros(B, dtype=torch.int32, device="cuda")
env.rollout_device("first", 0, False, stream, rew, done, rows, obs, R, True, False)      # (a zero-step launch: the block and the row counts)
env.sync()


def greedy_return():
    test.seed(np.arange(B) + 777)                                                        # the same ideals every time
    ev = evaluate_policy(test, policy, a.eval_episodes, greedy=True, obs_rows=max(R, 256), max_steps=4096)
    return float(torch.nanmean(ev.returns))


print("iteration  states  loss      entropy   greedy_mean_return")
print("%9d  %6d  %8s  %8s  %.2f" % (0, 0, "-", "-", greedy_return()))
for it in range(1, a.iterations + 1):
    buf = DeviceTrajectoryBuffer(T, B, obs_shape=(R, env.cols), targets=True)
    for t in range(T):
        q = torch.from_numpy(env.action_values(a.strategy, a.gamma)).cuda()
        target = action_value_targets(q, rows, R, a.temperature)
        state, count = obs.clone(), rows.clone()
        actions, logp = policy.act(obs, rows, torch.rand(B, device="cuda", generator=gen))
        env.step_device(actions, rew, done, rows, obs, R, True, stream, auto_reset=True)
        env.sync()
        buf.store(state, count, actions, rew, logp, None, done, target=target)
    out = imitation_update(policy, buf, opt, a.epochs, a.batch_size, generator=gen)
    print("%9d  %6d  %8.5f  %8.5f  %.2f" % (it, T * B, out[-1]["loss"], out[-1]["entropy"], greedy_return()))
