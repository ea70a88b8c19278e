#!/usr/bin/env python3
"""tools/next_step_bench.py [ENV N] [--formats u8_xyc,bf16_chw] [--calls K] [--rounds R] [--out FILE.md]  -- what a step in next-step auto-reset mode
(include/memgym.h: mg_step_next; make(..., autoreset_mode="next_step")) costs beside the two same-step conventions.  Without ENV N: all ten ids at the
instance counts of bench.py's DEFAULT_ENVS (the BASELINE sizes).

Per id and format, FOUR handles in ONE process -- the same seeds, the same teacher (eps 0.1), the same 200 steps behind the reset -- legs alternated
A/B/C/D/A/B/C/D for `--rounds` rounds after an untimed pass; each figure is microseconds per step of a window of `--calls` steps (the teacher's launch
included in every leg) that ends in a device synchronisation, reported as the median of the rounds with their smallest and largest value:
  (A) step() with final_observation=True      the gymnasium 0.29 vector convention with frames: the control
  (B) step()                                  the plain same-step auto-reset step
  (C) step() with autoreset_mode="next_step"  the family's NEXT kernels (mortar, spotlight ids) or the composed pair (Mystery Path ids)
  (D) (C) with MEMGYM_NEXT_FUSE=0             the composed pair on every id -- the lab build only (MEMGYM_HIP_LIB=.../lib/lab/libmemgym_hip_lab.so); the
                                              switch is read at every call, so it is flipped around this leg's windows.  "d_generic" in the JSON says whether
                                              the leg really left the NEXT kernels (false with the product library: (D) is then (C) again).
One JSON line per id and format on stdout; --out appends the table as markdown.  A tool, not a test."""
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

LEGS = {"A_final_observation": dict(final_observation=True), "B_same_step": dict(), "C_next_step": dict(autoreset_mode="next_step"),
        "D_next_step_composed": dict(autoreset_mode="next_step")}
SWITCH = "MEMGYM_NEXT_FUSE"


def default_envs():
    """bench.py's DEFAULT_ENVS, read from its source (importing the benchmark would run its set-up)"""
    src = open(os.path.join(ROOT, "bench.py")).read()
    return ast.literal_eval(re.search(r"^DEFAULT_ENVS = (\{.*?\})$", src, re.S | re.M).group(1))


def window(fn, calls, composed):
    if composed:
        os.environ[SWITCH] = "0"
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e6
    finally:
        os.environ.pop(SWITCH, None)


def measure(env_id, n, fmt, args):
    out = {"env": env_id, "envs": n, "obs_format": fmt, "calls": args.calls, "rounds": args.rounds}
    seeds = torch.arange(n, dtype=torch.int64, device="cuda")
    legs = {}
    for name, kw in LEGS.items():
        env = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format=fmt, **kw)
        env.reset(seed=seeds)
        env.advance(200, eps=0.1, seed=1, render=False, stats=False)  # the episodes out of phase
        buf = torch.empty((n,) if env.action_dim == 1 else (n, 2), dtype=torch.int32, device="cuda")
        state = {"t": 0, "done": torch.zeros((), dtype=torch.int64, device="cuda")}

        def step(env=env, buf=buf, state=state):
            state["t"] += 1
            _, _, done, _, _ = env.step(env.expert_actions(0.1, 1, state["t"], out=buf))
            state["done"] += done.sum()

        legs[name] = (env, step, state)
    composed = {k: k.startswith("D_") for k in legs}
    for k, (_, step, _) in legs.items():  # the untimed pass: every leg (the next-step handles allocate their scratch here)
        window(step, 8, composed[k])
    fused0 = legs["D_next_step_composed"][0].debug_counter("next_fused_steps")
    got = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, (_, step, _) in legs.items():
            got[k].append(window(step, args.calls, composed[k]))
    out["us_per_step"] = {k: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)] for k, v in got.items()}
    out["d_generic"] = legs["D_next_step_composed"][0].debug_counter("next_fused_steps") == fused0
    out["c_fused"] = legs["C_next_step"][0].debug_counter("next_fused_steps") > 0
    finished = {}
    for k, (env, _, state) in legs.items():
        finished[k] = int(state["done"])
        env.check_errors()
        env.close()
    assert finished["A_final_observation"] == finished["B_same_step"] and finished["C_next_step"] == finished["D_next_step_composed"], finished
    steps = 8 + args.calls * args.rounds
    out["finished_per_step"] = {"same_step": round(finished["B_same_step"] / steps, 1), "next_step": round(finished["C_next_step"] / steps, 1)}
    return out


def cell(v):
    return "%.1f (%.1f-%.1f)" % tuple(v)


def table(rows):
    md = ["### us per step: median (min-max) of the rounds", "",
          "| id | format | instances | (A) final_observation | (B) same-step | (C) next-step | (D) next-step, composed | C - A | C - B | C - D |",
          "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        a, b, c, d = (r["us_per_step"][k] for k in LEGS)
        md.append("| %s | %s | %d | %s | %s | %s%s | %s | %+.1f | %+.1f | %s |" % (
            r["env"], r["obs_format"], r["envs"], cell(a), cell(b), cell(c), "" if r["c_fused"] else " (composed)", cell(d) if r["d_generic"] else "= (C)",
            c[0] - a[0], c[0] - b[0], "%+.1f" % (c[0] - d[0]) if r["d_generic"] and r["c_fused"] else "--"))
    return "\n".join(md) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("env", nargs="?")
    ap.add_argument("n", nargs="?", type=int)
    ap.add_argument("--formats", default="u8_xyc,bf16_chw")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("next_step_bench.py needs the MI355X: nothing here is measured on a CPU")
    sizes = default_envs()
    todo = [(args.env, args.n or sizes[args.env])] if args.env else list(sizes.items())
    rows = []
    for fmt in args.formats.split(","):
        for env_id, n in todo:
            rows.append(measure(env_id, n, fmt, args))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(table(rows))


if __name__ == "__main__":
    main()
