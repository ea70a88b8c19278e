#!/usr/bin/env python3
"""tools/instances_bench.py [ENV N ...] [--calls K] [--rounds R] [--out FILE.md]  -- what saving and loading instances costs (include/memgym.h:
mg_save_instances / mg_load_instances).  Without ENV N: 65,536 MortarMayhem-Grid-v0, 32,768 Endless-MysteryPath-v0, 16,384 Endless-SearingSpotlights-v0.

Per id, on ONE handle and in ONE process, legs alternated A/B/A/B for `--rounds` rounds; each figure is microseconds per call of a window of `--calls`
calls that ends in a device synchronisation, reported as the median of the rounds with their smallest and largest value.
  save all / load all / load all + frames                     every instance, idx = NULL
  save 1/64 / load 1/64 / load 1/64 + frames                  a scattered 1/64 of the instances through an index tensor
                                                              (the first "+ frames" call of a window follows frameless loads and draws everybody, the others the loaded rows)
  copy_ (all) / copy_ (1/64)                                  CONTROL: a device-to-device Tensor.copy_ of as many bytes as the records of that leg -- the ceiling
                                                              of the row copy (which reads and writes those bytes as well); "ratio" = control / save
  state_dict + load_state_dict                                what a user had before: the whole handle through host memory, synchronous
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
from headless_bench import alternate, cell  # noqa: E402

DEFAULT = (("MortarMayhem-Grid-v0", 65536), ("Endless-MysteryPath-v0", 32768), ("Endless-SearingSpotlights-v0", 16384))


def measure(env_id, n, args):
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    env.reset(seed=torch.arange(n, dtype=torch.int64, device="cuda"))
    env.advance(200, eps=0.1, seed=1, render=True, stats=False)  # the episodes out of phase
    g = torch.Generator(device="cuda").manual_seed(1)
    few = torch.randperm(n, device="cuda", generator=g)[:max(n // 64, 1)].sort().values.to(torch.int32)
    all_snap, few_snap = env.save_instances(), env.save_instances(idx=few)
    env.load_instances(all_snap)  # (the handle's first load allocates its scratch)
    nbytes = env.instance_bytes
    ctl = {k: (torch.empty_like(s.records), torch.empty_like(s.records)) for k, s in (("all", all_snap), ("few", few_snap))}

    def call(fn):
        def leg(_):
            fn()
            return 1
        return leg

    legs = {"save all": call(lambda: env.save_instances(out=all_snap)), "load all": call(lambda: env.load_instances(all_snap, render=False)),
            "load all + frames": call(lambda: env.load_instances(all_snap)),
            "save 1/64": call(lambda: env.save_instances(idx=few, out=few_snap)), "load 1/64": call(lambda: env.load_instances(few_snap, idx=few, render=False)),
            "load 1/64 + frames": call(lambda: env.load_instances(few_snap, idx=few)),
            "copy_ (all)": call(lambda: ctl["all"][0].copy_(ctl["all"][1])), "copy_ (1/64)": call(lambda: ctl["few"][0].copy_(ctl["few"][1]))}
    us = alternate(legs, args.calls, args.rounds)

    def whole_handle(_):
        env.load_state_dict(env.state_dict())
        return 1
    us.update(alternate({"state_dict + load_state_dict": whole_handle}, max(args.calls // 16, 4), args.rounds))
    env.redraw()
    env.check_errors()
    env.close()
    return {"env": env_id, "envs": n, "record_bytes": nbytes, "calls": args.calls, "rounds": args.rounds, "us_per_call": us,
            "ratio_copy_over_save_all": round(us["copy_ (all)"][0] / us["save all"][0], 3),
            "ratio_copy_over_load_all": round(us["copy_ (all)"][0] / us["load all"][0], 3)}


def table(rows):
    names = list(rows[0]["us_per_call"])
    md = ["us per call: median (min-max) of the rounds", "", "| leg | " + " | ".join("%s x %d (%d B / record)" % (r["env"], r["envs"], r["record_bytes"]) for r in rows) + " |",
          "|---|" + "---|" * len(rows)]
    for k in names:
        md.append("| %s | " % k + " | ".join(cell(r["us_per_call"][k]) for r in rows) + " |")
    md.append("| copy_ / save all | " + " | ".join("%.2f" % r["ratio_copy_over_save_all"] for r in rows) + " |")
    md.append("| copy_ / load all | " + " | ".join("%.2f" % r["ratio_copy_over_load_all"] for r in rows) + " |")
    return "\n".join(md) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pairs", nargs="*")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out")
    args = ap.parse_args()
    pairs = [(args.pairs[k], int(args.pairs[k + 1])) for k in range(0, len(args.pairs), 2)] or DEFAULT
    rows = []
    for env_id, n in pairs:
        rows.append(measure(env_id, n, args))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(table(rows))


if __name__ == "__main__":
    main()
