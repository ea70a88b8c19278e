#!/usr/bin/env python3
"""tools/expert_bench.py [--envs N] [--steps K] [--warmup W] [--settle S] [--eps E] [--ids ID ...]  -- every env id under the device-side scripted
teacher (include/memgym.h mg_expert_actions, eps 0.1 by default) against uniform random actions, at the instance counts of bench.py's DEFAULT_ENVS
(the BASELINE sizes), and the expert launch's own time from HIP events.

Per id, one line of JSON: env-steps/s with random actions (drawn on the device, one torch.randint per step: what bench.py's workload does),
env-steps/s with the expert's actions (one mg_expert_actions launch per step in place of the randint), the mean duration of the expert launch
alone (events around `reps` back-to-back launches, the states as the timed run left them) and finished episodes per step under either policy.
A policy changes what a step costs -- an expert's episodes last longer or shorter, its agents reach the parts of a path nobody has drawn yet --
so the two rates are not the launch's price; that is the third figure.  MEMGYM_HIP_LIB selects the library.  A tool, not a test."""
import argparse
import ast
import json
import os
import re
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endless-memory-gym_amd"))
import memory_gym_amd  # noqa: E402


def default_envs():
    """bench.py's DEFAULT_ENVS, read from its source (importing the benchmark would run its set-up)"""
    src = open(os.path.join(ROOT, "bench.py")).read()
    return ast.literal_eval(re.search(r"^DEFAULT_ENVS = (\{.*?\})$", src, re.S | re.M).group(1))


def timed(env, policy, steps):
    """-> (seconds, finished episodes) of `steps` steps under policy(t) -> actions"""
    ndone = torch.zeros((), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(steps):
        _, _, done, _, _ = env.step(policy(t))
        ndone += done.sum()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, int(ndone.item())


def measure(env_id, n, args):
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    seeds = torch.arange(n, dtype=torch.int64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    shape, high = ((n,), 4) if env.action_dim == 1 else ((n, 2), 3)
    buf = torch.empty(shape, dtype=torch.int32, device="cuda")
    policies = {"random": lambda t: torch.randint(0, high, shape, device="cuda", generator=g, dtype=torch.int32),
                "expert": lambda t: env.expert_actions(args.eps, 1, t, out=buf)}
    out = {"env": env_id, "envs": n, "eps": args.eps, "steps": args.steps}
    for name, policy in policies.items():
        env.reset(seed=seeds)
        for t in range(args.settle + args.warmup):  # the episodes de-synchronise under the policy that is measured
            env.step(policy(t))
        dt, ndone = timed(env, lambda t: policy(args.settle + args.warmup + t), args.steps)
        out[name + "_Msteps_s"] = round(n * args.steps / dt / 1e6, 2)
        out[name + "_us_per_step"] = round(dt / args.steps * 1e6, 2)
        out[name + "_resets_per_step"] = round(ndone / args.steps, 2)
        env.check_errors()
    # the expert launch alone, in the states the expert's run has reached
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for t in range(10):
        env.expert_actions(args.eps, 1, t, out=buf)
    a.record()
    for t in range(args.reps):
        env.expert_actions(args.eps, 1, t, out=buf)
    b.record()
    b.synchronize()
    out["expert_launch_us"] = round(a.elapsed_time(b) * 1e3 / args.reps, 2)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=0, help="instances per id (default: bench.py's DEFAULT_ENVS)")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--settle", type=int, default=200)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=200, help="back-to-back expert launches between the two events")
    ap.add_argument("--ids", nargs="*", default=None)
    ap.add_argument("--spinup", type=float, default=2.0, help="seconds of untimed steps before the first id")
    args = ap.parse_args()
    sizes = default_envs()
    if args.spinup > 0:  # the process's first launches meet a GPU that has been idle: not part of any id's figures
        env = memory_gym_amd.make("MortarMayhem-Grid-v0", num_envs=16384, device=0)
        env.reset(seed=0)
        a = torch.zeros(16384, dtype=torch.int32, device="cuda")
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.spinup:
            for _ in range(100):
                env.step(a)
            torch.cuda.synchronize()
        env.close()
    for env_id in args.ids or sorted(sizes):
        print(json.dumps(measure(env_id, args.envs or sizes[env_id], args)), flush=True)


if __name__ == "__main__":
    main()
