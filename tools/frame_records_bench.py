#!/usr/bin/env python3
"""tools/frame_records_bench.py [ENV N] [--calls K] [--rounds R] [--out FILE.md]  -- what keeping frames as descriptors costs and saves (include/memgym.h:
mg_save_frames / mg_draw_frames).  Without ENV N: one id per family at the instance counts of bench.py's DEFAULT_ENVS (the BASELINE sizes).

Per id, on ONE handle per format and in ONE process, legs alternated A/B/A/B for `--rounds` rounds; each figure is microseconds per call of a window of
`--calls` calls that ends in a device synchronisation, reported as the median of the rounds with their smallest and largest value:
  (a) an identity draw_frames of num_envs records into the handle's own `obs` against redraw() of the same handle into the same buffer, u8_xyc and
      bf16_chw.  The two write the same frames (checked), so redraw() is the control.
  (b) a uniformly random pick of num_envs rows out of a 32-step store drawn in bf16_chw, against the torch route from a kept u8_chw rollout of the same 32
      steps, `rollout[idx].to(bfloat16) / 255`, and against index_select on a kept bf16_chw rollout where that fits the free memory.
  (c) save_frames per step against the headless step it follows: headless steps alone against headless step + save_frames(out=store[t]).
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
STORE_STEPS = 32


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


def alternate(legs, calls, rounds):
    """legs: {name: fn}; A/B/A/B -> {name: [median, min, max]} in microseconds per call"""
    for fn in legs.values():  # warm-up: every leg once, untimed
        window(fn, min(calls, 8))
    got = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            got[k].append(window(fn, calls))
    return {k: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)] for k, v in got.items()}


def measure(env_id, n, args):
    out = {"env": env_id, "envs": n, "calls": args.calls, "rounds": args.rounds}
    seeds = torch.arange(n, dtype=torch.int64, device="cuda")
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    env.reset(seed=seeds)
    env.advance(200, eps=0.1, seed=1, render=False, stats=False)  # the episodes out of phase
    env.redraw()
    out["record_bytes"] = env.frame_record_bytes

    # (c) first: it fills the 32-step store the other legs draw from
    store = torch.zeros((STORE_STEPS, n, env.frame_record_bytes), dtype=torch.uint8, device="cuda")
    buf = torch.empty((n,) if env.action_dim == 1 else (n, 2), dtype=torch.int32, device="cuda")
    clock = [0]

    def headless(_):
        clock[0] += 1
        env.step(env.expert_actions(0.1, 1, clock[0], out=buf), render=False)

    def headless_save(k):
        headless(k)
        env.save_frames(out=store[k % STORE_STEPS])

    def save_alone(k):
        env.save_frames(out=store[k % STORE_STEPS])

    out["c_us_per_step"] = alternate({"headless": headless, "headless_save": headless_save, "save_alone": save_alone}, max(args.calls, STORE_STEPS), args.rounds)
    for t in range(STORE_STEPS):  # every row of the store from consecutive steps
        headless_save(t)
    records = memory_gym_amd.FrameRecords(store, env.frame_layout())

    # (a) identity draw against redraw(), per format
    out["a_us_per_call"] = {}
    for fmt in ("u8_xyc", "bf16_chw"):
        h = env if fmt == "u8_xyc" else memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format=fmt)
        if h is not env:  # (the same seeds and the same teacher: out of phase like the first handle)
            h.reset(seed=seeds)
            h.advance(200, eps=0.1, seed=1, render=False, stats=False)
        want = h.redraw().clone()
        rec = h.save_frames()
        assert torch.equal(h.draw_frames(rec, out=h.obs), want), "the identity draw and redraw() write different frames"
        out["a_us_per_call"][fmt] = alternate({"redraw": lambda _: h.redraw(), "draw_frames": lambda _: h.draw_frames(rec, out=h.obs)}, args.calls, args.rounds)
        del want, rec
        if h is not env:
            h.close()
            del h
        torch.cuda.empty_cache()

    # (b) a random minibatch of n rows out of the 32-step store, bf16_chw
    g = torch.Generator(device="cuda").manual_seed(3)
    picks = [torch.randint(0, STORE_STEPS * n, (n,), device="cuda", generator=g, dtype=torch.int32) for _ in range(8)]
    picks64 = [p.long() for p in picks]
    batch = torch.empty((n, 3, 84, 84), dtype=torch.bfloat16, device="cuda")
    rollout_u8 = env.draw_frames(records, obs_format="u8_chw")  # the kept uint8 rollout, [32 n, 3, 84, 84]
    legs = {"draw_frames": lambda k: env.draw_frames(records, pick=picks[k % 8], out=batch, obs_format="bf16_chw"),
            "torch_from_u8": lambda k: torch.div(rollout_u8[picks64[k % 8]].to(torch.bfloat16), 255, out=batch)}
    check = env.draw_frames(records, pick=picks[0], obs_format="bf16_chw")
    assert torch.equal(check, (rollout_u8[picks64[0]].to(torch.float32) / 255).to(torch.bfloat16)), "the two routes give different minibatches"
    del check
    free, _ = torch.cuda.mem_get_info()
    rollout_bf16 = None
    if free > STORE_STEPS * n * 84 * 84 * 3 * 2 + (8 << 30):
        rollout_bf16 = env.draw_frames(records, obs_format="bf16_chw")
        legs["index_select_bf16"] = lambda k: torch.index_select(rollout_bf16, 0, picks64[k % 8], out=batch)
    out["b_us_per_call"] = alternate(legs, args.calls, args.rounds)
    out["b_kept_bytes"] = {"records": store.numel(), "u8_rollout": rollout_u8.numel(), "bf16_rollout": rollout_u8.numel() * 2}
    env.check_errors()
    env.close()
    return out


def cell(v):
    return "%.1f (%.1f-%.1f)" % tuple(v)


def tables(rows):
    md = ["### (a) identity draw_frames against redraw(), us per call: median (min-max) of the rounds", "",
          "| id | instances | u8_xyc redraw() | u8_xyc draw_frames | bf16_chw redraw() | bf16_chw draw_frames |", "|---|---|---|---|---|---|"]
    for r in rows:
        a = r["a_us_per_call"]
        md.append("| %s | %d | %s | %s | %s | %s |" % (r["env"], r["envs"], cell(a["u8_xyc"]["redraw"]), cell(a["u8_xyc"]["draw_frames"]),
                                                       cell(a["bf16_chw"]["redraw"]), cell(a["bf16_chw"]["draw_frames"])))
    md += ["", "### (b) a random minibatch of num_envs rows out of a 32-step store, bf16_chw, us per call", "",
           "| id | instances | draw_frames from records | torch from a kept u8_chw rollout | index_select on a kept bf16_chw rollout | bytes kept: records / u8 / bf16 |",
           "|---|---|---|---|---|---|"]
    for r in rows:
        b, k = r["b_us_per_call"], r["b_kept_bytes"]
        md.append("| %s | %d | %s | %s | %s | %.3f / %.1f / %.1f GB |" % (r["env"], r["envs"], cell(b["draw_frames"]), cell(b["torch_from_u8"]),
                                                                         cell(b["index_select_bf16"]) if "index_select_bf16" in b else "does not fit",
                                                                         k["records"] / 1e9, k["u8_rollout"] / 1e9, k["bf16_rollout"] / 1e9))
    md += ["", "### (c) save_frames per step against the headless step it follows, us per step", "",
           "| id | instances | headless step | headless step + save_frames | save_frames alone |", "|---|---|---|---|---|"]
    for r in rows:
        c = r["c_us_per_step"]
        md.append("| %s | %d | %s | %s | %s |" % (r["env"], r["envs"], cell(c["headless"]), cell(c["headless_save"]), cell(c["save_alone"])))
    return "\n".join(md) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("env", nargs="?")
    ap.add_argument("n", nargs="?", type=int)
    ap.add_argument("--calls", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frame_records_bench.py needs the MI355X: nothing here is measured on a CPU")
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
