#!/usr/bin/env python3
"""tools/debug_records_bench.py [ENV N] [--rounds R] [--steps T] [--out FILE.md]  -- what keeping the debug view of a few instances costs and saves
(include/memgym.h: mg_save_debug_frames / mg_draw_debug_frames).  Without ENV N: one id per family at the instance counts of bench.py's DEFAULT_ENVS (the
BASELINE sizes).

Per id, in ONE process, legs alternated A/B/A/B for `--rounds` rounds; each figure is the median of the rounds with their smallest and largest value:
  (a) save_debug_frames of 4 instances per step against the headless step it follows: headless steps alone, headless step + save, the save alone
      (us per step, windows of 64 steps that end in a device synchronisation).
  (b) a video of 4 instances over T = 200 steps: ONE draw_debug_frames of the T x 4 records at 336 (plus the T saves it needs, reported apart), against
      the route without records, render_debug()[S] once per step over the same T steps (ms per video).  N is the largest of the BASELINE size and its
      halves at which render_debug()'s output and scratch fit the free memory, and is reported.
  (c) the draw's bandwidth: 16,384 rows at 336 (5.5 GB) from the records of 16,384 instances, against a linear fill of the same bytes in the same process
      (torch.Tensor.fill_: the ceiling the draw is to be read against), GB/s.
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

PER_FAMILY = ("MortarMayhem-Grid-v0", "Endless-MysteryPath-v0", "SearingSpotlights-v0")
VIEW_BYTES = 336 * 336 * 3
BW_ROWS = 16384


def default_envs():
    """bench.py's DEFAULT_ENVS, read from its source (importing the benchmark would run its set-up)"""
    src = open(os.path.join(ROOT, "bench.py")).read()
    return ast.literal_eval(re.search(r"^DEFAULT_ENVS = (\{.*?\})$", src, re.S | re.M).group(1))


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(calls):
        fn(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def alternate(legs, calls, rounds, warm=True):
    """legs: {name: fn}; A/B/A/B -> {name: [median, min, max]} in microseconds per call"""
    if warm:
        for fn in legs.values():
            window(fn, min(calls, 4))
    got = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            got[k].append(window(fn, calls))
    return {k: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)] for k, v in got.items()}


def measure(env_id, n, args):
    T = args.steps
    free, _ = torch.cuda.mem_get_info()
    while n > 64 and n * (VIEW_BYTES + 84 * 84 * 3) + BW_ROWS * VIEW_BYTES + (8 << 30) > free:  # the parent's route must fit: its output and its scratch
        n //= 2
    out = {"env": env_id, "envs": n, "rounds": args.rounds, "steps": T}
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    env.reset(seed=torch.arange(n, dtype=torch.int64, device="cuda"))
    env.advance(200, eps=0.1, seed=1, render=False, stats=False)  # the episodes out of phase
    S = [0, n // 3, n // 2, n - 1]
    idx = torch.tensor(S, dtype=torch.int32, device="cuda")
    sl = idx.long()
    store = torch.zeros((T, 4, env.frame_record_bytes), dtype=torch.uint8, device="cuda")
    buf = torch.empty((n,) if env.action_dim == 1 else (n, 2), dtype=torch.int32, device="cuda")
    clock = [0]

    def headless(_):
        clock[0] += 1
        env.step(env.expert_actions(0.1, 1, clock[0], out=buf), render=False)

    def headless_save(k):
        headless(k)
        env.save_debug_frames(idx=idx, out=store[k % T])

    def save_alone(k):
        env.save_debug_frames(idx=idx, out=store[k % T])

    out["a_us_per_step"] = alternate({"headless": headless, "headless_save": headless_save, "save_alone": save_alone}, 64, args.rounds)

    # (b) the video of 4 instances over T steps, both routes over the same kind of steps
    video = torch.empty((T * 4, 336, 336, 3), dtype=torch.uint8, device="cuda")
    records = memory_gym_amd.DebugFrameRecords(store, env.frame_layout())

    def by_records(_):
        for t in range(T):
            headless_save(t)
        env.draw_debug_frames(records, out=video)

    def by_render_debug(_):
        for t in range(T):
            headless(t)
            video[4 * t:4 * t + 4] = env.render_debug()[sl]

    def steps_alone(_):
        for t in range(T):
            headless(t)

    def draw_alone(_):
        env.draw_debug_frames(records, out=video)

    b = alternate({"steps_alone": steps_alone, "by_records": by_records, "by_render_debug": by_render_debug, "draw_alone": draw_alone}, 1, args.rounds, warm=False)
    out["b_ms_per_video"] = {k: [round(x / 1e3, 3) for x in v] for k, v in b.items()}
    del video
    torch.cuda.empty_cache()

    # (c) bandwidth of the draw at 16,384 rows against a linear fill of the same bytes
    rows = BW_ROWS
    rec = env.save_debug_frames(idx=torch.arange(min(rows, n), dtype=torch.int32, device="cuda"))
    pick = torch.arange(rows, dtype=torch.int32, device="cuda") % rec.count  # (fewer instances than rows: the records repeat)
    big = torch.empty((rows, 336, 336, 3), dtype=torch.uint8, device="cuda")
    c = alternate({"fill": lambda _: big.fill_(7), "draw_336": lambda _: env.draw_debug_frames(rec, pick=pick, out=big)}, 8, args.rounds)
    out["c_gb_per_s"] = {k: [round(rows * VIEW_BYTES / (x * 1e-6) / 1e9, 1) for x in (v[0], v[2], v[1])] for k, v in c.items()}  # (median, min, max of the RATE)
    small = torch.empty((rows, 84, 84, 3), dtype=torch.uint8, device="cuda")
    c84 = alternate({"draw_84": lambda _: env.draw_debug_frames(rec, pick=pick, out=small, size=84)}, 8, args.rounds)
    out["c_us_per_call"] = {"fill": c["fill"], "draw_336": c["draw_336"], "draw_84": c84["draw_84"]}
    env.check_errors()
    env.close()
    return out


def cell(v, fmt="%.1f"):
    return (fmt + " (" + fmt + "-" + fmt + ")") % tuple(v)


def tables(rows):
    md = ["### (a) save_debug_frames of 4 instances against the headless step it follows, us per step: median (min-max) of the rounds", "",
          "| id | instances | headless step | headless step + save | save alone |", "|---|---|---|---|---|"]
    for r in rows:
        a = r["a_us_per_step"]
        md.append("| %s | %d | %s | %s | %s |" % (r["env"], r["envs"], cell(a["headless"]), cell(a["headless_save"]), cell(a["save_alone"])))
    md += ["", "### (b) a video of 4 instances over %d steps, ms per video" % rows[0]["steps"], "",
           "| id | instances (N) | the steps alone | steps + saves + ONE draw | steps + render_debug()[S] per step | the draw alone |", "|---|---|---|---|---|---|"]
    for r in rows:
        b = r["b_ms_per_video"]
        md.append("| %s | %d | %s | %s | %s | %s |" % (r["env"], r["envs"], cell(b["steps_alone"], "%.2f"), cell(b["by_records"], "%.2f"),
                                                      cell(b["by_render_debug"], "%.2f"), cell(b["draw_alone"], "%.3f")))
    md += ["", "### (c) the draw at 16,384 rows (5.5 GB at 336) against a linear fill of the same bytes, GB/s", "",
           "| id | fill_ | draw at 336 | draw / fill | draw at 84, us per call |", "|---|---|---|---|---|"]
    for r in rows:
        c = r["c_gb_per_s"]
        md.append("| %s | %s | %s | %.2f | %s |" % (r["env"], cell(c["fill"]), cell(c["draw_336"]), c["draw_336"][0] / c["fill"][0], cell(r["c_us_per_call"]["draw_84"])))
    return "\n".join(md) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("env", nargs="?")
    ap.add_argument("n", nargs="?", type=int)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("debug_records_bench.py needs the MI355X: nothing here is measured on a CPU")
    sizes = default_envs()
    todo = [(args.env, args.n or sizes[args.env])] if args.env else [(e, sizes[e]) for e in PER_FAMILY]
    rows = []
    for env_id, n in todo:
        rows.append(measure(env_id, n, args))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(tables(rows))


if __name__ == "__main__":
    main()
