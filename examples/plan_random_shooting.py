#!/usr/bin/env python3
"""examples/plan_random_shooting.py -- planning by random shooting, on the device: at every decision step save the batch, play B random K-step
action tapes from it without a frame (VecMemoryGym.play, include/memgym.h: mg_play; until_done=True, so a branch stops where its episode ends and is
not reset), reload, and take the first action of the best branch per instance.  The mean return of that planner is printed against a uniformly random
policy's on the same seeds.

    python examples/plan_random_shooting.py [--env MortarMayhem-Grid-v0] [--envs 256] [--decisions 120] [--branches 16] [--horizon 12]

Per decision step: B loads (a few small launches each) and B play() calls -- one launch each on the Mortar Mayhem ids -- instead of B x K steps from
Python.  (Mortar Mayhem rewards a command only when it is verified, several steps after the move, so a short horizon mostly learns to stay alive;
the point here is the save -> branch -> play -> compare workflow.)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endless-memory-gym_amd"))
import torch  # noqa: E402

import memory_gym_amd  # noqa: E402


def random_tape(env, steps, generator):
    """int32 [steps, N] (Discrete(4)) or [steps, N, 2] (MultiDiscrete([3, 3])): uniformly random actions"""
    shape, high = ((steps, env.num_envs), 4) if env.action_dim == 1 else ((steps, env.num_envs, 2), 3)
    return torch.randint(0, high, shape, generator=generator, device=env.device, dtype=torch.int32)


def plan(env, branches, horizon, generator):
    """-> the first action of the best of `branches` random tapes per instance; the handle is left in the state it was called in"""
    snap = env.save_instances()
    best = torch.full((env.num_envs,), -float("inf"), dtype=torch.float64, device=env.device)
    action = None
    for b in range(branches):
        if b:
            env.load_instances(snap, render=False)
        tape = random_tape(env, horizon, generator)
        _, st = env.play(tape, until_done=True, render=False)
        # the branch's return, and among equal returns the branch that survived longer
        score = st["reward"] + 1e-6 * st["steps"].double()
        better = score > best
        best = torch.where(better, score, best)
        pick = better if env.action_dim == 1 else better[:, None]
        action = tape[0].clone() if action is None else torch.where(pick, tape[0], action)
    env.load_instances(snap, render=False)
    return action


def episode_returns(env, decisions, policy):
    """-> (sum of step rewards per instance over `decisions` steps with auto-reset, episodes ended)"""
    total = torch.zeros(env.num_envs, dtype=torch.float64, device=env.device)
    episodes = 0
    for _ in range(decisions):
        _, _, done, _, _ = env.step(policy(env), render=False)
        total += env.reward64
        episodes += int(done.sum())
    return total, episodes


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--env", default="MortarMayhem-Grid-v0")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--decisions", type=int, default=120)  # (the first 40 steps of a default episode only show the commands: the agent is frozen)
    ap.add_argument("--branches", type=int, default=16)
    ap.add_argument("--horizon", type=int, default=12)
    args = ap.parse_args()
    env = memory_gym_amd.make(args.env, num_envs=args.envs, device=0)
    g = torch.Generator(device=env.device).manual_seed(0)
    env.reset(seed=0)
    planned, ep_p = episode_returns(env, args.decisions, lambda e: plan(e, args.branches, args.horizon, g))
    env.reset(seed=0)
    rand, ep_r = episode_returns(env, args.decisions, lambda e: random_tape(e, 1, g)[0])
    print("%s: %d instances x %d decisions, %d branches x %d steps per decision" % (args.env, args.envs, args.decisions, args.branches, args.horizon))
    print("mean return: random shooting %.4f (%d episodes ended), random policy %.4f (%d episodes ended)"
          % (float(planned.mean()), ep_p, float(rand.mean()), ep_r))
    env.check_errors()
    env.close()


if __name__ == "__main__":
    main()
