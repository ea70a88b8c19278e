#!/usr/bin/env python3
"""tools/rollout_trace_bench.py [ENV N] [--steps S] [--rounds R] [--out FILE.md]  -- what keeping a rollout inside the library costs and saves
(include/memgym.h: mg_advance_traced / mg_play_traced).  Without ENV N: all ten ids at the instance counts of bench.py's DEFAULT_ENVS (the BASELINE sizes).

Per id, on ONE handle and in ONE process, legs alternated A/B/A/B for `--rounds` rounds; each figure is microseconds per step of a window of `--steps`
steps (whole multiples of K = 64) that ends in a device synchronisation, reported as the median of the rounds with their smallest and largest value.
Every leg plays the teacher at eps 0.3 (or its recorded tape) with auto-reset and continues from the states the leg before it left:
  (a) advance_traced(ro), K = 64             frame records, actions, reward, done
  (b) advance_traced(ro with labels)         ... and the teacher's eps-0 answers
  (c) advance(64)                            untraced: what tracing itself costs is (a) - (c) and (b) - (c)
  (d) the records loop from Python           `for t: expert_actions(out=A[t]); step(A[t], render=False); save_frames(out=store[t + 1])` -- the parent's way to
                                             the data of (a), examples/rollout_from_records.py
  (e) the drawn loop from Python             examples/collect_expert_pairs.py: copy the frame, two expert launches, a DRAWN step; the frames go to a ring of
                                             four rows here (64 rows of 65,536 frames are 89 GB), the work per step is the example's
  (f) play(tape, trace=ro)                   frame records, reward, done of a recorded tape
  (g) play(tape, trace=True)                 mg_play with its reward / done traces, no frame records
  (h) / (i) the five mortar ids: (a) and (f) in their LOOP FORM (the lab build's MEMGYM_MORTAR_ADVANCE_FUSE=0 / MEMGYM_MORTAR_PLAY_FUSE=0, flipped between the
                                             legs); skipped (null) when the library loaded is not the lab build.
One JSON line per id on stdout; --out appends the tables as markdown.  MEMGYM_HIP_LIB selects the library.  A tool, not a test."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from play_bench import MORTAR, alternate, cell, default_envs, ratio, teacher_tape  # noqa: E402  (puts the package on the path)

import memory_gym_amd  # noqa: E402

K = 64
EPS, SEED = 0.3, 7


def measure(env_id, n, args):
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    env.reset(seed=torch.arange(n, dtype=torch.int64, device="cuda"))
    env.advance(200, eps=0.1, seed=1, render=False, stats=False)  # the episodes out of phase
    snap = env.save_instances()
    tape = teacher_tape(env, K, snap)
    ro, ro_labels = env.new_rollout(K), env.new_rollout(K, labels=True)
    vis = (lambda o: o["visual_observation"] if isinstance(o, dict) else o)
    ring = torch.empty((4,) + tuple(vis(env.redraw()).shape), dtype=torch.uint8, device="cuda")
    played = torch.empty_like(ro.actions[0])
    env.play(tape, trace=ro, render=False)  # (the scratch of both calls allocated)
    env.advance_traced(ro, eps=EPS, seed=SEED, step=0, render=False)
    env.load_instances(snap, render=False)

    def traced(trace, switch=None):
        def fn():
            if switch:
                os.environ[switch] = "0"
            if trace is None:
                env.advance(K, eps=EPS, seed=SEED, step=0, render=False)
            else:
                env.advance_traced(trace, eps=EPS, seed=SEED, step=0, render=False)
            if switch:
                os.environ.pop(switch, None)
            return K
        return fn

    def played_tape(trace, switch=None):
        def fn():
            if switch:
                os.environ[switch] = "0"
            env.play(tape, trace=trace, render=False)
            if switch:
                os.environ.pop(switch, None)
            return K
        return fn

    def records_loop():
        env.save_frames(out=ro.frames[0])
        for t in range(K):
            env.expert_actions(EPS, SEED, t, out=ro.actions[t])
            env.step(ro.actions[t], render=False)
            env.save_frames(out=ro.frames[t + 1])
        return K

    def drawn_loop():
        obs = env.redraw()
        for t in range(K):
            ring[t % 4].copy_(vis(obs))
            env.expert_actions(0.0, SEED, t, out=ro_labels.labels[t])
            env.expert_actions(EPS, SEED, t, out=played)
            obs, _, _, _, _ = env.step(played)
        return K

    steps = max(K, args.steps // K * K)
    out = {"env": env_id, "envs": n, "steps": steps, "rounds": args.rounds}
    legs = {"advance_traced": traced(ro), "advance_traced_labels": traced(ro_labels), "advance": traced(None), "records_loop": records_loop,
            "drawn_loop": drawn_loop, "play_traced": played_tape(ro), "play_reward_done": played_tape(True)}
    lab = env_id in MORTAR and "lab" in os.path.basename(os.environ.get("MEMGYM_HIP_LIB", ""))
    if lab:
        legs["advance_traced_loop_form"] = traced(ro, "MEMGYM_MORTAR_ADVANCE_FUSE")
        legs["play_traced_loop_form"] = played_tape(ro, "MEMGYM_MORTAR_PLAY_FUSE")
    c0 = [env.debug_counter(k) for k in ("traced_steps", "traced_fused_steps")]
    out["us_per_step"] = alternate(legs, steps, args.rounds)
    c1 = [env.debug_counter(k) for k in ("traced_steps", "traced_fused_steps")]
    out["traced_steps"], out["traced_fused_steps"] = c1[0] - c0[0], c1[1] - c0[1]
    if lab:
        assert 0 < out["traced_fused_steps"] < out["traced_steps"], "the switches did not select both forms: is this the lab build?"
    env.check_errors()
    env.close()
    return out


def tables(rows):
    md = ["### K = 64 steps under the teacher (eps 0.3), us per step: median (min-max) of the rounds", "",
          "| id | instances | (a) advance, traced | (b) ... with labels | (c) advance, untraced | (d) records loop from Python | (e) drawn loop from Python | (d)/(a) | (e)/(a) |",
          "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        u = r["us_per_step"]
        md.append("| %s | %d | %s | %s | %s | %s | %s | %s | %s |" % (r["env"], r["envs"], cell(u["advance_traced"]), cell(u["advance_traced_labels"]), cell(u["advance"]),
                                                                    cell(u["records_loop"]), cell(u["drawn_loop"]), ratio(u["records_loop"], u["advance_traced"]),
                                                                    ratio(u["drawn_loop"], u["advance_traced"])))
    md += ["", "### a recorded tape of 64 steps, and the in-launch forms against their own loop forms (lab build), us per step", "",
           "| id | instances | (f) play, traced | (g) play, reward / done only | (h) advance traced, loop form | (i) play traced, loop form | (h)/(a) | (i)/(f) |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        u = r["us_per_step"]
        h, i = u.get("advance_traced_loop_form"), u.get("play_traced_loop_form")
        md.append("| %s | %d | %s | %s | %s | %s | %s | %s |" % (r["env"], r["envs"], cell(u["play_traced"]), cell(u["play_reward_done"]), cell(h) if h else "-", cell(i) if i else "-",
                                                          ratio(h, u["advance_traced"]) if h else "-", ratio(i, u["play_traced"]) if i else "-"))
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
        sys.exit("rollout_trace_bench.py needs the MI355X: nothing here is measured on a CPU")
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
