#!/usr/bin/env python3
"""tools/play_bench.py [ENV N] [--steps K] [--rounds R] [--out FILE.md]  -- what playing a caller-supplied tape inside the library saves
(include/memgym.h: mg_play).  Without ENV N: all ten ids at the instance counts of bench.py's DEFAULT_ENVS (the BASELINE sizes).

Per id, on ONE handle and in ONE process, legs alternated A/B/A/B for `--rounds` rounds; each figure is microseconds per step of a window of
`--steps` steps (whole multiples of 64) that ends in a device synchronisation, reported as the median of the rounds with their smallest and largest
value.  The tape is the scripted teacher's at eps 0.3, recorded once for 64 steps from the states the legs start in; every leg plays it with
auto-reset and continues from the states the leg before it left:
  (a) play(tape) -- mg_play, MG_PLAY_THROUGH;
  (b) the Python loop `for t: step(tape[t], render=False)` of the same build -- what a user writes without mg_play;
  (c) that loop of 64 steps captured into a graph and replayed;
  (d) the five mortar ids: play(tape) in its loop form (the lab build's MEMGYM_MORTAR_PLAY_FUSE=0, flipped between the legs); skipped (null)
      when the library loaded is not the lab build.
MortarMayhem-Grid-v0 also gets (e): K = 200, play(until_done=True) from a reloaded snapshot against play() through the same tape from the same
snapshot -- lanes leave the loop at their own episode's end there, so the pair shows what wave divergence costs (and what the early end saves).
One JSON line per id on stdout; --out appends the tables as markdown.  MEMGYM_HIP_LIB selects the library.  A tool, not a test."""
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
SWITCH = "MEMGYM_MORTAR_PLAY_FUSE"
K = 64


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
        done += fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / done * 1e6


def alternate(legs, steps, rounds):
    """legs: {name: fn}; A/B/A/B -> {name: [median, min, max]} in microseconds per step"""
    for fn in legs.values():  # warm-up: every leg once, untimed
        window(fn, 1)
    got = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            got[k].append(window(fn, steps))
    return {k: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)] for k, v in got.items()}


def teacher_tape(env, steps, snap):
    """the teacher's eps-0.3 tape of `steps` steps from the handle's states, which are restored afterwards"""
    rows = []
    for t in range(steps):
        rows.append(env.expert_actions(0.3, 7, t).clone())
        env.step(rows[-1], render=False)
    env.load_instances(snap, render=False)
    return torch.stack(rows).contiguous()


def measure(env_id, n, args):
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    env.reset(seed=torch.arange(n, dtype=torch.int64, device="cuda"))
    env.advance(200, eps=0.1, seed=1, render=False, stats=False)  # the episodes out of phase
    snap = env.save_instances()
    tape = teacher_tape(env, K, snap)
    env.play(tape, render=False)  # (mg_play's scratch allocated)
    env.load_instances(snap, render=False)

    def play():
        env.play(tape, render=False)
        return K

    def loop():
        for t in range(K):
            env.step(tape[t], render=False)
        return K

    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loop()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        loop()

    def replay():
        graph.replay()
        return K

    steps = max(K, args.steps // K * K)
    out = {"env": env_id, "envs": n, "steps": steps, "rounds": args.rounds}
    legs = {"play": play, "python_loop": loop, "graph_loop": replay}
    lab = env_id in MORTAR and "lab" in os.path.basename(os.environ.get("MEMGYM_HIP_LIB", ""))
    if lab:
        def form(fused):
            def fn():
                os.environ[SWITCH] = "1" if fused else "0"
                env.play(tape, render=False)
                os.environ.pop(SWITCH, None)
                return K
            return fn
        legs["play_loop_form"] = form(False)
    f0, h0 = env.debug_counter("play_fused_steps"), env.debug_counter("headless_steps")
    out["us_per_step"] = alternate(legs, steps, args.rounds)
    f1, h1 = env.debug_counter("play_fused_steps"), env.debug_counter("headless_steps")
    if lab:
        assert f1 > f0 and h1 > h0, "the switch did not select both forms: is this the lab build?"
    out["episode_mode"] = None
    if env_id == "MortarMayhem-Grid-v0":  # (e) K = 200: until done against through, both from the same snapshot
        env.load_instances(snap, render=False)
        long_tape = teacher_tape(env, 200, snap)

        def leg(until_done):
            def fn():
                env.load_instances(snap, render=False)
                env.play(long_tape, until_done=until_done, render=False)
                return 200
            return fn

        def load_only():
            env.load_instances(snap, render=False)
            return 200
        out["episode_mode"] = alternate({"through200": leg(False), "until_done200": leg(True), "load_alone": load_only}, 200 * max(1, steps // 200), args.rounds)
        _, st = env.play(long_tape, until_done=True, render=False)
        out["episode_mode"]["mean_steps_played"] = round(float(st["steps"].double().mean()), 1)
    env.check_errors()
    env.close()
    return out


def cell(v):
    return "%.1f (%.1f-%.1f)" % tuple(v[:3])


def ratio(a, b):
    """a's median over b's, with the range the two spreads allow"""
    return "x%.2f (x%.2f-x%.2f)" % (a[0] / b[0], a[1] / b[2], a[2] / b[1])


def tables(rows):
    md = ["### play(64 steps) against the loops, us per step: median (min-max) of the rounds; ratios: the other leg over play", "",
          "| id | instances | (a) play | (b) loop from Python | (c) loop replayed from a graph | (d) play, loop form | (b)/(a) | (d)/(a) |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        u = r["us_per_step"]
        d = u.get("play_loop_form")
        md.append("| %s | %d | %s | %s | %s | %s | %s | %s |" % (r["env"], r["envs"], cell(u["play"]), cell(u["python_loop"]), cell(u["graph_loop"]),
                                                          cell(d) if d else "-", ratio(u["python_loop"], u["play"]), ratio(d, u["play"]) if d else "-"))
    for r in rows:
        e = r["episode_mode"]
        if e:
            md += ["", "### %s, %d instances, K = 200 from one snapshot: us per tape step (the load included in both; the load alone: %s)" % (r["env"], r["envs"], cell(e["load_alone"])), "",
                   "| through | until done | mean steps played until done |", "|---|---|---|",
                   "| %s | %s | %.1f of 200 |" % (cell(e["through200"]), cell(e["until_done200"]), e["mean_steps_played"])]
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
        sys.exit("play_bench.py needs the MI355X: nothing here is measured on a CPU")
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
