#!/usr/bin/env python3
"""tools/headless_bench.py [ENV N] [--steps K] [--rounds R] [--out FILE.md]  -- what stepping without drawing saves (include/memgym.h: mg_step with
obs_dev == NULL, mg_advance).  Without ENV N: all ten ids at the instance counts of bench.py's DEFAULT_ENVS (the BASELINE sizes).

Per id, on ONE handle and in ONE process, legs alternated A/B/A/B for `--rounds` rounds (every leg continues from the states the leg before it
left: drawn and headless steps leave the same states); each figure is microseconds per step of a window of `--steps` steps that ends in a device
synchronisation, reported as the median of the rounds with their smallest and largest value:
  (a) drawn step (the control: the code path every earlier build has) against headless step, under uniform random actions (one torch.randint
      per step) and under the scripted teacher at eps 0.1 (one mg_expert_actions launch per step);
  (b) mg_advance(64) against the explicit loop of expert_actions + step(render=False) from Python, and against that loop of 64 pairs captured
      into a graph and replayed (windows of --steps rounded to whole multiples of 64);
  (c) the five mortar ids: mg_advance's in-launch form (mortar_advance_kernel) against its loop form in the same build -- the lab build's
      MEMGYM_MORTAR_ADVANCE_FUSE switch, flipped between the legs; skipped (null) when the library loaded is not the lab build.
One JSON line per id on stdout; --out appends the three tables as markdown.  MEMGYM_HIP_LIB selects the library.  A tool, not a test."""
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

MORTAR = ("MortarMayhem-Grid-v0", "MortarMayhem-v0", "Endless-MortarMayhem-v0", "MortarMayhemB-Grid-v0", "MortarMayhemB-v0")
SWITCH = "MEMGYM_MORTAR_ADVANCE_FUSE"


def default_envs():
    """bench.py's DEFAULT_ENVS, read from its source (importing the benchmark would run its set-up)"""
    src = open(os.path.join(ROOT, "bench.py")).read()
    return ast.literal_eval(re.search(r"^DEFAULT_ENVS = (\{.*?\})$", src, re.S | re.M).group(1))


def window(fn, steps):
    """microseconds per step of fn() -> steps taken, repeated until `steps` steps are done, ending in a synchronisation"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done = 0
    while done < steps:
        done += fn(done)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / done * 1e6


def alternate(legs, steps, rounds):
    """legs: {name: fn}; A/B/A/B -> {name: [median, min, max]} in microseconds per step"""
    for fn in legs.values():  # warm-up: every leg once, untimed
        window(fn, min(steps, 64))
    got = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            got[k].append(window(fn, steps))
    return {k: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)] for k, v in got.items()}


def measure(env_id, n, args):
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    env.reset(seed=torch.arange(n, dtype=torch.int64, device="cuda"))
    g = torch.Generator(device="cuda").manual_seed(1)
    shape, high = ((n,), 4) if env.action_dim == 1 else ((n, 2), 3)
    buf = torch.empty(shape, dtype=torch.int32, device="cuda")
    clock = [0]  # the teacher's step number: every call a new one

    def random_actions():
        return torch.randint(0, high, shape, device="cuda", generator=g, dtype=torch.int32)

    def teacher():
        clock[0] += 1
        return env.expert_actions(0.1, 1, clock[0], out=buf)

    def stepper(policy, render):
        def fn(_):
            env.step(policy(), render=render)
            return 1
        return fn

    env.advance(200, eps=0.1, seed=1, render=False, stats=False)  # the episodes out of phase (and mg_advance's scratch allocated)
    out = {"env": env_id, "envs": n, "steps": args.steps, "rounds": args.rounds}
    a = alternate({"random_drawn": stepper(random_actions, True), "random_headless": stepper(random_actions, False),
                   "teacher_drawn": stepper(teacher, True), "teacher_headless": stepper(teacher, False)}, args.steps, args.rounds)
    out["a_us_per_step"] = a

    # (b) mg_advance(64) / the loop from Python / the loop captured
    def adv(_):
        clock[0] += 64
        env.advance(64, eps=0.1, seed=1, step=clock[0], render=False)
        return 64

    def loop(_):
        for _ in range(64):
            env.step(teacher(), render=False)
        return 64

    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loop(0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        loop(0)

    def replay(_):
        graph.replay()
        return 64

    steps64 = max(64, args.steps // 64 * 64)
    out["b_us_per_step"] = alternate({"advance64": adv, "python_loop": loop, "graph_loop": replay}, steps64, args.rounds)

    # (c) mortar: the in-launch form against the loop form of the same (lab) build
    out["c_us_per_step"] = None
    if env_id in MORTAR and "lab" in os.path.basename(os.environ.get("MEMGYM_HIP_LIB", "")):
        def form(fused):
            def fn(_):
                os.environ[SWITCH] = "1" if fused else "0"
                clock[0] += 64
                env.advance(64, eps=0.1, seed=1, step=clock[0], render=False)
                return 64
            return fn
        f0, h0 = env.debug_counter("advance_fused_steps"), env.debug_counter("headless_steps")
        out["c_us_per_step"] = alternate({"in_launch": form(True), "loop_form": form(False)}, steps64, args.rounds)
        os.environ.pop(SWITCH, None)
        f1, h1 = env.debug_counter("advance_fused_steps"), env.debug_counter("headless_steps")
        assert f1 > f0 and h1 > h0, "the switch did not select both forms: is this the lab build?"
    env.check_errors()
    env.close()
    return out


def cell(v):
    return "%.1f (%.1f-%.1f)" % tuple(v)


def tables(rows):
    md = ["### (a) drawn against headless step, us per step: median (min-max) of the rounds", "",
          "| id | instances | random, drawn | random, headless | teacher 0.1, drawn | teacher 0.1, headless |", "|---|---|---|---|---|---|"]
    for r in rows:
        a = r["a_us_per_step"]
        md.append("| %s | %d | %s | %s | %s | %s |" % (r["env"], r["envs"], cell(a["random_drawn"]), cell(a["random_headless"]), cell(a["teacher_drawn"]), cell(a["teacher_headless"])))
    md += ["", "### (b) mg_advance(64) against the loop, us per step", "", "| id | instances | mg_advance(64) | loop from Python | loop replayed from a graph |", "|---|---|---|---|---|"]
    for r in rows:
        b = r["b_us_per_step"]
        md.append("| %s | %d | %s | %s | %s |" % (r["env"], r["envs"], cell(b["advance64"]), cell(b["python_loop"]), cell(b["graph_loop"])))
    md += ["", "### (c) mortar ids: in-launch form against the loop form of the same build, us per step", "", "| id | instances | in-launch | loop form |", "|---|---|---|---|"]
    for r in rows:
        if r["c_us_per_step"]:
            c = r["c_us_per_step"]
            md.append("| %s | %d | %s | %s |" % (r["env"], r["envs"], cell(c["in_launch"]), cell(c["loop_form"])))
    return "\n".join(md) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("env", nargs="?")
    ap.add_argument("n", nargs="?", type=int)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("headless_bench.py needs the MI355X: nothing here is measured on a CPU")
    sizes = default_envs()
    todo = [(args.env, args.n or sizes[args.env])] if args.env else list(sizes.items())
    rows = []
    for env_id, n in todo:
        rows.append(measure(env_id, n, args))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(tables(rows))


if __name__ == "__main__":
    main()
