#!/usr/bin/env python3
"""examples/collect_expert_pairs.py -- demonstrations for behaviour cloning from the library's own scripted teacher: (observation,
expert action) pairs collected on the GPU, nothing leaves it.  The teacher's LABEL for a state is expert_actions(eps=0); the actions
that are PLAYED carry a share `--eps` of random ones, so that the data set also holds the states a learner reaches by its mistakes
(off the path, late for a tile, beside the coin) with the teacher's answer to them -- DAgger's idea with a random perturbation in
place of the learner.  Both come from one launch each per step (include/memgym.h: mg_expert_actions).

    python examples/collect_expert_pairs.py [--env MysteryPath-Grid-v0] [--envs 4096] [--steps 128] [--eps 0.1] [--out pairs.pt]

Prints pairs per second, the teacher's return per finished episode and how often label and played action differ."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endless-memory-gym_amd"))
import torch  # noqa: E402

import memory_gym_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MysteryPath-Grid-v0")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--out", default=None, help="torch.save the pairs here (uint8 observations in image order, int32 labels)")
    args = ap.parse_args()
    n = args.envs
    env = memory_gym_amd.make(args.env, num_envs=n, device=0, obs_format="u8_chw")  # a uint8 rollout buffer in the network's order
    obs, _ = env.reset(seed=torch.arange(n, dtype=torch.int64, device="cuda"))
    vis = (lambda o: o["visual_observation"] if isinstance(o, dict) else o)
    width = (n,) if env.action_dim == 1 else (n, 2)
    frames = torch.empty((args.steps,) + tuple(vis(obs).shape), dtype=torch.uint8, device="cuda")
    labels = torch.empty((args.steps,) + width, dtype=torch.int32, device="cuda")
    played = torch.empty(width, dtype=torch.int32, device="cuda")
    returns, episodes, differ = torch.zeros((), dtype=torch.float64, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda"), 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.steps):
        frames[t].copy_(vis(obs))                               # the observation the label belongs to (env.obs is overwritten by step)
        env.expert_actions(0.0, 0, t, out=labels[t])            # the teacher's answer in this state
        env.expert_actions(args.eps, 0, t, out=played)          # what is played: the same, or a random action (hash of seed, step, instance)
        obs, _, done, _, info = env.step(played)
        returns += (info["reward"] * done).sum()
        episodes += done.sum()
        differ = differ + (labels[t] != played).reshape(n, -1).any(1).sum()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    env.check_errors()
    print("%s x%d: %d pairs in %.2f s (%.2f M pairs/s); %d episodes finished, return per episode %.3f; played != label in %.1f %% of the pairs"
          % (args.env, n, n * args.steps, dt, n * args.steps / dt / 1e6, int(episodes), float(returns) / max(int(episodes), 1),
             100.0 * float(differ) / (n * args.steps)))
    if args.out:
        torch.save({"env": args.env, "obs": frames.cpu(), "action": labels.cpu()}, args.out)
    env.close()


if __name__ == "__main__":
    main()
