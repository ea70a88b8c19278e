#!/usr/bin/env python3
"""examples/branch_from_state.py -- K continuations of the SAME states, without a frame: save a batch on the device, play K action sequences
from it headless, reload between them (VecMemoryGym.save_instances / load_instances, include/memgym.h: mg_save_instances), and report how far
the returns of the continuations spread per state -- the counterfactual probe a memory benchmark exists for ("same state, other behaviour").

    python examples/branch_from_state.py [--env Endless-MysteryPath-v0] [--envs 256] [--warmup 40] [--branches 8] [--horizon 60] [--eps 0.3]

Branch b plays the scripted teacher with its own hash seed at exploration rate --eps, so the branches differ only where the random actions
do.  Everything stays on the device: per branch one load (a few small launches) and `horizon` headless steps."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endless-memory-gym_amd"))
import torch  # noqa: E402

import memory_gym_amd  # noqa: E402


def branch_returns(env, snap, branches, horizon, eps):
    """-> float64 [branches, N]: the sum of step rewards of every branch from the saved states (auto-reset on: a branch goes on into new episodes)"""
    out = torch.zeros((branches, env.num_envs), dtype=torch.float64, device=env.device)
    for b in range(branches):
        env.load_instances(snap, render=False)
        for t in range(horizon):
            env.step(env.expert_actions(eps, seed=1000 + b, step=t), render=False)
            out[b] += env.reward64
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="Endless-MysteryPath-v0")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--branches", type=int, default=8)
    ap.add_argument("--horizon", type=int, default=60)
    ap.add_argument("--eps", type=float, default=0.3)
    args = ap.parse_args()
    env = memory_gym_amd.make(args.env, num_envs=args.envs, device=0)
    env.reset(seed=0)
    env.advance(args.warmup, eps=0.1, seed=1, render=False, stats=False)  # into the episodes
    snap = env.save_instances()
    r = branch_returns(env, snap, args.branches, args.horizon, args.eps)
    again = branch_returns(env, snap, 1, args.horizon, args.eps)  # branch 0 a second time: a reloaded state replays bit for bit
    assert torch.equal(again[0], r[0]), "a reloaded state did not replay"
    spread = r.max(0).values - r.min(0).values
    print("%s: %d states x %d branches x %d steps, %d bytes per record" % (args.env, args.envs, args.branches, args.horizon, env.instance_bytes))
    print("return per branch (mean over states): " + " ".join("%.3f" % x for x in r.mean(1).tolist()))
    print("spread of the branches' returns per state: mean %.3f, max %.3f, states whose branches all agree: %d"
          % (float(spread.mean()), float(spread.max()), int((spread == 0).sum())))
    env.check_errors()
    env.close()


if __name__ == "__main__":
    main()
