#!/usr/bin/env python3
"""tools/masked_step_bench.py [ENV N ...] [--steps K] [--rounds R] [--out FILE.md]  -- what a masked step costs (include/memgym.h: mg_step_masked).
Without ENV N: one id per family at the instance counts of bench.py's DEFAULT_ENVS (the BASELINE sizes).

Per id, on ONE handle and in ONE process, legs alternated A/B/A/B for `--rounds` rounds (every leg continues from the states the leg before it
left); each figure is microseconds per call of a window of `--steps` calls that ends in a device synchronisation, reported as the median of the
rounds with their smallest and largest value.  Actions are uniform random (one torch.randint per call, in every leg); the masks are made before the
clock starts and reused: Bernoulli masks (16 different ones per share, taken in turn) and contiguous blocks (the first share x N instances).
  step             mg_step, the handle's own (fused) arrangement -- the control
  ones             mg_step_masked with an all-ones mask: the plain arrangement with the MASKED step kernel and the masked raster
  1/2, 1/8, 1/64   mg_step_masked with that share of the instances active, Bernoulli / in one block
  headless 1/2     the masked headless step (obs_dev == NULL), Bernoulli 1/2
One JSON line per id on stdout; --out appends the table as markdown.  MEMGYM_HIP_LIB selects the library.  A tool, not a test."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endless-memory-gym_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import memory_gym_amd  # noqa: E402
from headless_bench import alternate, cell, default_envs  # noqa: E402

ONE_PER_FAMILY = ("MortarMayhem-Grid-v0", "SearingSpotlights-v0", "MysteryPath-Grid-v0", "Endless-MysteryPath-v0")
SHARES = (2, 8, 64)


def measure(env_id, n, args):
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    env.reset(seed=torch.arange(n, dtype=torch.int64, device="cuda"))
    g = torch.Generator(device="cuda").manual_seed(1)
    shape, high = ((n,), 4) if env.action_dim == 1 else ((n, 2), 3)

    def random_actions():
        return torch.randint(0, high, shape, device="cuda", generator=g, dtype=torch.int32)

    def masked(masks, render=True):
        def fn(k):
            env.step(random_actions(), render=render, mask=masks[k % len(masks)])
            return 1
        return fn

    def plain(_):
        env.step(random_actions())
        return 1

    env.advance(200, eps=0.1, seed=1, render=False, stats=False)  # the episodes out of phase
    legs = {"step": plain, "ones": masked([torch.ones(n, dtype=torch.uint8, device="cuda")])}
    for s in SHARES:
        legs["bernoulli 1/%d" % s] = masked([(torch.rand(n, device="cuda", generator=g) < 1.0 / s).to(torch.uint8) for _ in range(16)])
        block = torch.zeros(n, dtype=torch.uint8, device="cuda")
        block[:n // s] = 1
        legs["block 1/%d" % s] = masked([block])
    legs["headless 1/2"] = masked([(torch.rand(n, device="cuda", generator=g) < 0.5).to(torch.uint8) for _ in range(16)], render=False)
    out = {"env": env_id, "envs": n, "steps": args.steps, "rounds": args.rounds, "us_per_call": alternate(legs, args.steps, args.rounds)}
    env.redraw()
    env.check_errors()
    env.close()
    return out


def table(rows):
    names = list(rows[0]["us_per_call"])
    md = ["### microseconds per call: median (min-max) of the rounds", "", "| id | instances | " + " | ".join(names) + " |", "|---|---|" + "---|" * len(names)]
    for r in rows:
        md.append("| %s | %d | %s |" % (r["env"], r["envs"], " | ".join(cell(r["us_per_call"][k]) for k in names)))
    return "\n".join(md) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pairs", nargs="*", help="ENV N ENV N ...")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("masked_step_bench.py needs the MI355X: nothing here is measured on a CPU")
    sizes = default_envs()
    todo = list(zip(args.pairs[0::2], (int(x) for x in args.pairs[1::2]))) if args.pairs else [(e, sizes[e]) for e in ONE_PER_FAMILY]
    rows = []
    for env_id, n in todo:
        rows.append(measure(env_id, n, args))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(table(rows))


if __name__ == "__main__":
    main()
