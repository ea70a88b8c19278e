#!/usr/bin/env python3
"""examples/teacher_sweep.py -- what the scripted teacher reaches under a list of option dictionaries: success rate, return and length per
finished episode, with NO frame drawn (VecMemoryGym.advance, include/memgym.h: mg_advance).  An upper bound on return per curriculum
setting, and a check that a setting is solvable at all, at the price of the game logic alone -- the raster is 85-95 % of a drawn step.

    python examples/teacher_sweep.py [--env MortarMayhem-Grid-v0] [--envs 4096] [--steps 2000] [--eps 0.0]
                                     [--options '{"command_count": [5]}' '{"command_count": [10], "explosion_delay": [3]}' ...]

Per option dictionary one line: episodes finished, success rate (ids that report "success"), return and length per episode, steps per
second.  Episodes still under way when the steps run out are not counted; terminal observations do not exist here."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endless-memory-gym_amd"))
import torch  # noqa: E402

import memory_gym_amd  # noqa: E402

DEFAULT_SWEEP = ['{"command_count": [3]}', '{"command_count": [5]}', '{"command_count": [10]}', '{"command_count": [10], "explosion_delay": [3]}']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MortarMayhem-Grid-v0")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--eps", type=float, default=0.0, help="share of uniformly random actions (0 = the teacher, 1 = the random policy)")
    ap.add_argument("--options", nargs="*", default=None, help="one JSON dictionary of reset options per setting")
    args = ap.parse_args()
    settings = [json.loads(s) for s in (args.options if args.options is not None else (DEFAULT_SWEEP if args.env == "MortarMayhem-Grid-v0" else ["{}"]))]
    n = args.envs
    env = memory_gym_amd.make(args.env, num_envs=n, device=0)
    seeds = torch.arange(n, dtype=torch.int64, device="cuda")
    for options in settings:
        env.reset(seed=seeds, options=options)  # (the one frame this setting draws: the reset's)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, st = env.advance(args.steps, eps=args.eps, seed=0, step=0, render=False)
        episodes = int(st["episodes"].sum())  # (synchronises)
        dt = time.perf_counter() - t0
        env.check_errors()
        per = lambda key: float(st[key].sum()) / max(episodes, 1)
        success = ("%.3f" % per("success")) if "success" in st else "n/a"
        print("%s %s: %d episodes, success rate %s, return %.3f and length %.1f per episode, reward per instance %.3f; %.1f M env-steps/s"
              % (args.env, json.dumps(options), episodes, success, per("episode_reward"), per("episode_length"), float(st["reward"].mean()),
                 n * args.steps / dt / 1e6))
    env.close()


if __name__ == "__main__":
    main()
