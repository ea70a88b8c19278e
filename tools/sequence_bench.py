#!/usr/bin/env python3
"""tools/sequence_bench.py [ENV N] [--steps K] [--length L] [--batch M] [--rounds R] [--arrange A] [--out FILE.md]  -- what cutting a rollout into episode sequences
and drawing padded minibatches of them costs (include/memgym.h: mg_split_episodes / mg_sequence_picks / mg_draw_frames_padded).  Without ENV N:
MortarMayhem-Grid-v0, Endless-MysteryPath-v0 and SearingSpotlights-v0 at the instance counts of bench.py's DEFAULT_ENVS (the BASELINE sizes).

Per id, on ONE handle and in ONE process: a K-step trace under the teacher (eps 0.3, episodes out of phase), then the legs below alternated A/B/A/B
for `--rounds` rounds.  Each figure is microseconds per call of a window of `--calls` calls that ends in a device synchronisation, reported as the
median of the rounds with their smallest and largest value.
  split + picks of ALL sequences
    (s) split_episodes(done, L, capacity) + picks(m=capacity)     four launches, nothing leaves the device
    (h) the host loop a trainer runs today                        done to the host, a Python loop over the instances (numpy per instance), the picks
                                                                  built with numpy, picks and mask back to the device; ONE call per round
  the padded draw of a shuffled minibatch of M sequences = M * L rows, in u8_xyc and bf16_chw
    (p) draw_frames_padded(frames, pick)                          the PAD form of the gather raster
    (a) draw_frames(frames, pick with the pads replaced by 0)     the existing gather, unchanged: it composes and stores a frame where (p) stores zeros
    (b) what a caller composes today                              draw_frames of the valid rows into a temporary, zero the output, index_copy_ (the
                                                                  valid-row index is computed outside the window, which flatters this leg)
One JSON line per id on stdout; --out appends the tables as markdown.  MEMGYM_HIP_LIB selects the library.  A tool, not a test."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from play_bench import alternate, cell, default_envs, ratio  # noqa: E402  (puts the package on the path)

import memory_gym_amd  # noqa: E402

IDS = ("MortarMayhem-Grid-v0", "Endless-MysteryPath-v0", "SearingSpotlights-v0")
EPS, SEED = 0.3, 7


def host_split(done, length):
    """The per-worker loop of a recurrent trainer: -> int32 [S, 3] (instance, t0, len), ordered by (instance, t0)"""
    K, N = done.shape
    rows = []
    for i in range(N):
        ends = np.flatnonzero(done[:, i]) + 1
        if not len(ends) or ends[-1] != K:
            ends = np.append(ends, K)
        start = 0
        for e in ends:
            t0 = np.arange(start, e, length)
            ln = np.minimum(length, e - t0)
            rows.append(np.stack([np.full(len(t0), i), t0, ln], 1))
            start = e
    return np.concatenate(rows).astype(np.int32)


def host_picks(table, length, n):
    l = np.arange(length, dtype=np.int32)[None, :]
    pick = (table[:, 1:2] + l) * n + table[:, 0:1]
    mask = l < table[:, 2:3]
    return np.where(mask, pick, -1).astype(np.int32), mask


def measure(env_id, n, args):
    K, L, M = args.steps, args.length, args.batch
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    env.reset(seed=torch.arange(n, dtype=torch.int64, device="cuda"))
    env.advance(200, eps=0.1, seed=1, render=False, stats=False)  # the episodes out of phase
    ro = env.new_rollout(K)
    env.advance_traced(ro, eps=EPS, seed=SEED, step=0, render=False, stats=False)
    frames = memory_gym_amd.FrameRecords(ro.frames, ro.frame_layout)
    seqs = env.split_episodes(ro.done, L)  # (the handle's scratch; the capacity that always suffices)
    S, cap = len(seqs), seqs.capacity
    table = seqs.table[:S].cpu().numpy()
    want = host_split(ro.done.cpu().numpy(), L)
    assert np.array_equal(table[:, :3], want), "the host loop and the device disagree"
    hp, hm = host_picks(want, L, n)
    pick_all, mask_all = seqs.picks()
    assert np.array_equal(pick_all.cpu().numpy(), hp) and np.array_equal(mask_all.cpu().numpy(), hm)
    del pick_all, mask_all

    def device_leg():
        env.split_episodes(ro.done, L, capacity=cap).picks(m=cap)
        return 1

    def host_leg():
        t = host_split(ro.done.cpu().numpy(), L)
        p, m = host_picks(t, L, n)
        torch.as_tensor(p).cuda(), torch.as_tensor(m).cuda()
        return 1

    out = {"env": env_id, "envs": n, "steps": K, "length": L, "sequences": S, "capacity": cap, "full_sequences": int((table[:, 2] == L).sum()),
           "batch": M, "rounds": args.rounds, "calls": args.calls, "arrange": args.arrange}
    out["split_us"] = alternate({"device": device_leg}, args.calls, args.rounds)
    out["split_us"].update(alternate({"host_loop": host_leg}, 1, args.rounds))

    g = torch.Generator().manual_seed(0)
    sel = torch.randperm(S, generator=g)[:M].to(torch.int32).cuda()
    pick = seqs.picks(sel=sel)[0].view(-1)
    rows = pick.numel()
    if args.arrange != "sequences":  # the same rows, the padding rows elsewhere: how the zero rows are dealt to the workgroups (a row's workgroup is j % grid)
        kept, pads = pick[pick >= 0], int((pick < 0).sum())
        at = torch.arange(pads, device="cuda") * rows // pads if args.arrange == "even" else torch.arange(pads, device="cuda")
        is_pad = torch.zeros(rows, dtype=torch.bool, device="cuda")
        is_pad[at] = True
        pick = torch.full_like(pick, -1)
        pick[~is_pad] = kept
    valid = torch.nonzero(pick >= 0).flatten()
    pick_valid = pick[valid].contiguous()
    pick0 = pick.clamp(min=0)
    out["rows"], out["pad_share"] = rows, round(1.0 - valid.numel() / rows, 4)
    out["draw_us"] = {}
    for fmt in ("u8_xyc", "bf16_chw"):
        _, dt, shape = env.OBS_FORMATS[fmt]
        obs = torch.empty((rows,) + shape, dtype=dt, device="cuda")
        tmp = torch.empty((valid.numel(),) + shape, dtype=dt, device="cuda")

        def padded():
            env.draw_frames_padded(frames, pick, out=obs, obs_format=fmt)
            return 1

        def gather():
            env.draw_frames(frames, pick=pick0, out=obs, obs_format=fmt)
            return 1

        def composed():
            env.draw_frames(frames, pick=pick_valid, out=tmp, obs_format=fmt)
            obs.zero_()
            obs.index_copy_(0, valid, tmp)
            return 1

        padded()
        ref = obs.clone()
        composed()
        assert torch.equal(ref.view(torch.uint8), obs.view(torch.uint8)), "the padded draw and the composition disagree"
        del ref
        out["draw_us"][fmt] = alternate({"padded": padded, "gather": gather, "composed": composed}, args.calls, args.rounds)
        del obs, tmp
    env.check_errors()
    env.close()
    return out


def tables(rows):
    md = ["### split + picks of all sequences, us per call: median (min-max) of the rounds", "",
          "| id | instances | K | L | sequences (full) | (s) device | (h) host loop | (h)/(s) |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        u = r["split_us"]
        md.append("| %s | %d | %d | %d | %d (%d) | %s | %s | %s |" % (r["env"], r["envs"], r["steps"], r["length"], r["sequences"], r["full_sequences"], cell(u["device"]),
                                                                 cell(u["host_loop"]), ratio(u["host_loop"], u["device"])))
    md += ["", "### the padded draw of a shuffled minibatch, us per call", "",
           "| id | format | rows | pad rows | (p) padded | (a) gather, pads as record 0 | (b) composed today | (p)/(a) | (b)/(p) |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        for fmt, u in r["draw_us"].items():
            md.append("| %s | %s | %d | %.1f %% | %s | %s | %s | %s | %s |" % (r["env"], fmt, r["rows"], 100 * r["pad_share"], cell(u["padded"]), cell(u["gather"]),
                                                                         cell(u["composed"]), ratio(u["padded"], u["gather"]), ratio(u["composed"], u["padded"])))
    return "\n".join(md) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("env", nargs="?")
    ap.add_argument("n", nargs="?", type=int)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--length", type=int, default=16)
    ap.add_argument("--batch", type=int, default=4096, help="sequences per minibatch: the draw is of batch * length rows")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--arrange", choices=("sequences", "even", "front"), default="sequences",
                    help="where the minibatch's padding rows lie: behind their sequences (what a trainer draws), evenly spaced, or all in front")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sequence_bench.py needs the MI355X: nothing here is measured on a CPU")
    sizes = default_envs()
    todo = [(args.env, args.n or sizes[args.env])] if args.env else [(k, sizes[k]) for k in IDS]
    rows = []
    for env_id, n in todo:
        rows.append(measure(env_id, n, args))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(tables(rows))


if __name__ == "__main__":
    main()
