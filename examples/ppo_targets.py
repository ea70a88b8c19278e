#!/usr/bin/env python3
"""examples/ppo_targets.py -- from "rollout done" to "first minibatch" of a recurrent PPO trainer without leaving the device: two traced rollouts, the
critic's values of their frames (a stand-in here), rollout_targets for advantages, returns and their moments (include/memgym.h: mg_rollout_targets /
mg_sum_columns), and minibatches of episode sequences with the normalised advantages and the returns gathered next to the actions
(split_episodes / EpisodeSequences.gather).

    python examples/ppo_targets.py [--env MortarMayhem-Grid-v0] [--envs 4096] [--steps 128] [--length 16] [--batch 256] [--gamma 0.99] [--lam 0.95]

Same-step auto-reset: an episode that ends bootstraps from 0 and `done` is all the call needs.  (Under autoreset_mode="next_step" pass the restart flags
as skip= and truncated= without final_value: examples/next_step_rollout.py collects them.)  Prints, per rollout, the advantages' mean and deviation
and what the first minibatch holds."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endless-memory-gym_amd"))
import torch  # noqa: E402

import memory_gym_amd  # noqa: E402
from memory_gym_amd.episodes import rollout_targets  # noqa: E402


def critic(env, ro):
    """a stand-in for the value network: [K + 1, N] float32 from the trace's frame records (the share of set bytes in a record) -- a trainer draws the
    frames (draw_sequences) and runs its network"""
    return ro.frames.ne(0).float().mean(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MortarMayhem-Grid-v0")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--length", type=int, default=16)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    args = ap.parse_args()
    n, K, L, M = args.envs, args.steps, args.length, args.batch
    env = memory_gym_amd.make(args.env, num_envs=n, device=0)
    env.reset(seed=torch.arange(n, dtype=torch.int64, device="cuda"))
    ro = env.new_rollout(K)
    targets = None
    for rollout in range(2):
        env.advance_traced(ro, eps=0.1, seed=0, step=rollout * K, render=False)
        value = critic(env, ro)
        # one launch for adv / ret / valid and the per-instance moments, one small launch for their sums; the second rollout writes into the first's tensors
        targets = rollout_targets(env, ro.reward, ro.done, value, gamma=args.gamma, lam=args.lam, out=targets, moments=True)
        normalized = targets.normalized()  # torch expressions over the moments: nothing comes to the host
        seqs = env.split_episodes(ro.done, L, capacity=n * ((K + L - 1) // L) + K * n // 8)
        sel = torch.randperm(seqs.capacity, device="cuda")[:M].to(torch.int32)  # (entries beyond the count give padding rows and error bit 512: see below)
        sel = torch.where(sel < seqs.count, sel, torch.full_like(sel, -1))
        adv = seqs.gather(normalized, sel=sel)       # [M, L], zero at the pads
        ret = seqs.gather(targets.ret, sel=sel)      # [M, L]
        actions = seqs.gather(ro.actions, sel=sel)   # [M, L] or [M, L, 2]
        # ... ratio = exp(logp(policy(obs), actions) - old_logp); loss = -(min(ratio * adv, clip(ratio) * adv)) + c * (v - ret) ** 2, under the mask ...
        print("rollout %d: %d samples, advantages mean %+.4f, deviation %.4f; a minibatch of %d sequences x %d steps: adv %s, ret %s, actions %s"
              % (rollout, int(targets.moments[0]), float(targets.mean()), float(targets.std()), M, L, tuple(adv.shape), tuple(ret.shape), tuple(actions.shape)))
        assert adv.shape == ret.shape == (M, L) and bool(torch.isfinite(adv).all())
    env.check_errors()
    env.close()


if __name__ == "__main__":
    main()
