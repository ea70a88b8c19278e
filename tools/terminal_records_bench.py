#!/usr/bin/env python3
"""tools/terminal_records_bench.py [ENV N] [--calls K] [--rounds R] [--out FILE.md]  -- what keeping the terminal frames as records costs and saves
(include/memgym.h: mg_info_buffers.final_frames_dev).  Without ENV N: one id per family plus Endless-MysteryPath-v0 at the instance counts of bench.py's
DEFAULT_ENVS (the BASELINE sizes).

Per id, FOUR handles in ONE process -- the same seeds, the same teacher (eps 0.1), the same 200 steps behind the reset, so that they are in the same states
and finish the same episodes -- legs alternated A/B/C/D/A/B/C/D for `--rounds` rounds; each figure is microseconds per step of a window of `--calls`
steps (the teacher's launch included in every leg) that ends in a device synchronisation, reported as the median of the rounds with their smallest and
largest value:
  (a) the headless step                                  step(render=False)
  (b) the headless step with final_frames                step(render=False) on a final_frames=True handle
  (c) the drawn step with final_observation=True         the gymnasium vector convention with frames (the fused launches keep the terminal frames)
  (d) the drawn step with final_frames                   the headless arrangement with records, then the dense raster launch
(b) - (a) is what the records cost; (c) - (b) what a headless trainer in the vector convention gains.  One JSON line per id on stdout; --out appends the
table as markdown.  MEMGYM_HIP_LIB selects the library.  A tool, not a test."""
import argparse
import ast
import json
import os
import re
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endless-memory-gym_amd"))
import memory_gym_amd  # noqa: E402

IDS = ("MortarMayhem-Grid-v0", "MysteryPath-Grid-v0", "Endless-MysteryPath-v0", "SearingSpotlights-v0")
LEGS = {"a_headless": (dict(), False), "b_headless_records": (dict(final_frames=True), False),
        "c_drawn_final_observation": (dict(final_observation=True), True), "d_drawn_records": (dict(final_frames=True), True)}


def default_envs():
    """bench.py's DEFAULT_ENVS, read from its source (importing the benchmark would run its set-up)"""
    src = open(os.path.join(ROOT, "bench.py")).read()
    return ast.literal_eval(re.search(r"^DEFAULT_ENVS = (\{.*?\})$", src, re.S | re.M).group(1))


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def measure(env_id, n, args):
    out = {"env": env_id, "envs": n, "calls": args.calls, "rounds": args.rounds}
    seeds = torch.arange(n, dtype=torch.int64, device="cuda")
    legs, finished = {}, {}
    for name, (kw, render) in LEGS.items():
        env = memory_gym_amd.make(env_id, num_envs=n, device=0, **kw)
        env.reset(seed=seeds)
        env.advance(200, eps=0.1, seed=1, render=False, stats=False)  # the episodes out of phase
        buf = torch.empty((n,) if env.action_dim == 1 else (n, 2), dtype=torch.int32, device="cuda")
        state = {"t": 0, "done": torch.zeros((), dtype=torch.int64, device="cuda")}

        def step(env=env, buf=buf, state=state, render=render):
            state["t"] += 1
            _, _, done, _, _ = env.step(env.expert_actions(0.1, 1, state["t"], out=buf), render=render)
            state["done"] += done.sum()

        legs[name] = (env, step, state)
    out["record_bytes"] = legs["b_headless_records"][0].frame_record_bytes
    for _, step, _ in legs.values():  # warm-up: every leg, untimed (all four advance by the same steps)
        window(step, 8)
    got = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, (_, step, _) in legs.items():
            got[k].append(window(step, args.calls))
    out["us_per_step"] = {k: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)] for k, v in got.items()}
    for k, (env, _, state) in legs.items():
        finished[k] = int(state["done"])
        env.check_errors()
        env.close()
    assert len(set(finished.values())) == 1, "the four handles did not finish the same episodes: %s" % finished
    out["finished_per_step"] = round(finished["a_headless"] / ((8 + args.calls * args.rounds)), 1)
    return out


def cell(v):
    return "%.1f (%.1f-%.1f)" % tuple(v)


def table(rows):
    md = ["### us per step: median (min-max) of the rounds", "",
          "| id | instances | episodes ending per step | (a) headless | (b) headless + records | (c) drawn + final_observation | (d) drawn + records | (b) - (a) | (c) / (b) |",
          "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        u = r["us_per_step"]
        a, b, c, d = (u[k] for k in LEGS)
        md.append("| %s | %d | %.1f | %s | %s | %s | %s | %+.1f | x%.2f |" % (r["env"], r["envs"], r["finished_per_step"], cell(a), cell(b), cell(c), cell(d),
                                                                           b[0] - a[0], c[0] / b[0]))
    return "\n".join(md) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("env", nargs="?")
    ap.add_argument("n", nargs="?", type=int)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("terminal_records_bench.py needs the MI355X: nothing here is measured on a CPU")
    sizes = default_envs()
    todo = [(args.env, args.n or sizes[args.env])] if args.env else [(e, sizes[e]) for e in IDS]
    rows = []
    for env_id, n in todo:
        rows.append(measure(env_id, n, args))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(table(rows))


if __name__ == "__main__":
    main()
