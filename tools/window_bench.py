#!/usr/bin/env python3
"""tools/window_bench.py [ENV N] [--steps K] [--rounds R] [--calls C] [--skip-gather] [--out FILE.md]  -- what the memory windows of a transformer agent cost
(include/memgym.h: mg_episode_positions / mg_window_picks / mg_gather_rows_padded).  Without ENV N: MortarMayhem-Grid-v0, Endless-MysteryPath-v0 and
SearingSpotlights-v0 at the instance counts of bench.py's DEFAULT_ENVS (the BASELINE sizes).

Everything in ONE process, the legs of a comparison alternated A/B/A/B for `--rounds` rounds.  Each figure is microseconds per call of a window of
`--calls` calls that ends in a device synchronisation, reported as the median of the rounds with their smallest and largest value.
  positions + picks (per id: a K-step trace under the teacher, lag 1, back 0; M = 4,096 shuffled samples and M = K * N; W in 16, 64, 256 where M * W fits an int32)
    (k) episode_windows(done, W).picks(sel)          two launches, nothing leaves the device
    (t) the torch expression on the device           episode starts by a cumulative maximum, the windows by broadcasting; int32 throughout
    (h) the host loop (M = 4,096 only)               done to the host, numpy per instance for the positions, the windows with numpy, pick and mask back to
                                                     the device; ONE call per round
  draw_windows of 4,096 windows of W = 16 (65,536 rows) in u8_xyc and bf16_chw, next to draw_sequences of 4,096 sequences of L = 16: the same raster
  gather (once, on the first handle): M * W = 65,536 and 1,048,576 rows of 4 / 768 / 1,024 / 2,048 bytes, 10 % pads, picked at random from a store of
  1,048,576 rows
    (g) gather_rows(x, pick, out)                    mg_gather_rows_padded
    (e) what EpisodeSequences.gather does today      x[pick.clamp(min=0).long()], then torch.where(mask, rows, 0)
    (c) a device-to-device copy of the output's bytes: the ceiling; (c)/(g) is the share of it the kernel reaches
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
EPS, SEED, LAG = 0.3, 7, 1
INT32_MAX = 2**31 - 1


def torch_positions(done):
    """done bool [K, N] -> int32 [K + 1, N]: the row an episode began at by a cumulative maximum over `row behind a done`"""
    K, N = done.shape
    rows = torch.arange(K + 1, dtype=torch.int32, device=done.device)[:, None]
    start = torch.zeros((K + 1, N), dtype=torch.int32, device=done.device)
    start[1:] = torch.where(done, rows[1:], 0)
    return rows - torch.cummax(start, 0).values


def torch_picks(pos, sel, window, lag, back):
    K1, N = pos.shape
    t, i = torch.div(sel, N, rounding_mode="floor"), sel % N
    hi = t - lag
    lo = torch.maximum(torch.maximum(t - pos.view(-1)[sel.long()], hi - window + 1), torch.full_like(t, -back))
    length = (hi - lo + 1).clamp(min=0)
    l = torch.arange(window, dtype=torch.int32, device=pos.device)[None, :]
    mask = l < length[:, None]
    return torch.where(mask, (back + lo[:, None] + l) * N + i[:, None], -1), mask, length


def host_windows(done, sel, window, lag, back):
    """the per-instance loop of a trainer's host code: positions column by column, then the windows of the selection"""
    K, N = done.shape
    pos = np.zeros((K + 1, N), dtype=np.int32)
    rows = np.arange(1, K + 1, dtype=np.int32)
    for i in range(N):
        pos[1:, i] = rows - np.maximum.accumulate(np.where(done[:, i], rows, 0))
    t, i = sel // N, sel % N
    hi = t - lag
    lo = np.maximum(np.maximum(t - pos.reshape(-1)[sel], hi - window + 1), -back)
    length = np.maximum(hi - lo + 1, 0)
    l = np.arange(window, dtype=np.int32)[None, :]
    mask = l < length[:, None]
    return np.where(mask, (back + lo[:, None] + l) * N + i[:, None], -1).astype(np.int32), mask


def measure_gather(env, args):
    out = []
    R = 1 << 20
    g = torch.Generator(device="cuda").manual_seed(0)
    for row_bytes in (4, 768, 1024, 2048):
        x = torch.randn((R, row_bytes // 4), dtype=torch.float32, device="cuda", generator=g)
        for rows in (1 << 16, 1 << 20):
            pick = torch.randint(0, R, (rows,), dtype=torch.int32, device="cuda", generator=g)
            pick[torch.rand(rows, device="cuda", generator=g) < 0.1] = -1
            mask = pick >= 0
            dst = torch.empty((rows, row_bytes // 4), dtype=torch.float32, device="cuda")
            other = torch.randn((rows, row_bytes // 4), dtype=torch.float32, device="cuda", generator=g)

            def kernel():
                env.gather_rows(x, pick, out=dst)
                return 1

            def expression():
                got = x[pick.clamp(min=0).long()]
                torch.where(mask[:, None], got, torch.zeros_like(got))
                return 1

            def copy():
                dst.copy_(other)
                return 1

            got = x[pick.clamp(min=0).long()]
            kernel()
            assert torch.equal(dst, torch.where(mask[:, None], got, torch.zeros_like(got))), "the kernel and the expression disagree"
            del got
            us = alternate({"kernel": kernel, "expression": expression, "copy": copy}, args.calls, args.rounds)
            out.append({"row_bytes": row_bytes, "rows": rows, "pad_share": round(1.0 - float(mask.float().mean()), 4), "us": us,
                        "kernel_gbps": round(2 * rows * row_bytes * 0.9 / us["kernel"][0] / 1e3, 1)})
            del dst, other
        del x
    return out


def measure(env_id, n, args, gather):
    K = args.steps
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    env.reset(seed=torch.arange(n, dtype=torch.int64, device="cuda"))
    env.advance(200, eps=0.1, seed=1, render=False, stats=False)  # the episodes out of phase
    ro = env.new_rollout(K)
    env.advance_traced(ro, eps=EPS, seed=SEED, step=0, render=False, stats=False)
    done = ro.done
    out = {"env": env_id, "envs": n, "steps": K, "done_share": round(float(done.float().mean()), 5), "rounds": args.rounds, "calls": args.calls, "picks_us": []}
    gen = torch.Generator().manual_seed(0)
    samples = (K + 1) * n
    for M in (4096, K * n):
        sel = (torch.randperm(samples, generator=gen)[:M] if M == 4096 else torch.arange(M)).to(torch.int32).cuda()
        for W in (16, 64, 256):
            if M * W > INT32_MAX:
                continue

            def kernel():
                env.episode_windows(done, W, lag=LAG).picks(sel=sel)
                return 1

            def expression():
                torch_picks(torch_positions(done), sel, W, LAG, 0)
                return 1

            pick, mask, length = env.episode_windows(done, W, lag=LAG).picks(sel=sel)
            tp, tm, tl = torch_picks(torch_positions(done), sel, W, LAG, 0)
            assert torch.equal(pick, tp) and torch.equal(mask, tm) and torch.equal(length, tl), "the kernels and the torch expression disagree"
            del pick, mask, length, tp, tm, tl
            us = alternate({"kernels": kernel, "expression": expression}, args.calls, args.rounds)
            if M == 4096:
                sel_host = sel.cpu().numpy().astype(np.int64)

                def host():
                    p, m = host_windows(done.cpu().numpy(), sel_host, W, LAG, 0)
                    torch.as_tensor(p).cuda(), torch.as_tensor(m).cuda()
                    return 1

                us.update(alternate({"host_loop": host}, 1, args.rounds))
            out["picks_us"].append({"m": M, "window": W, "us": us})
            torch.cuda.empty_cache()

    # draw_windows next to draw_sequences: 4,096 rows of 16 frames each
    M, W = 4096, 16
    sel = torch.randperm(samples, generator=gen)[:M].to(torch.int32).cuda()
    win = env.episode_windows(done, W)
    seqs = env.split_episodes(done, W)
    seq_sel = torch.randperm(len(seqs), generator=gen)[:M].to(torch.int32).cuda()
    out["draw_us"] = {}
    for fmt in ("u8_xyc", "bf16_chw"):
        _, dt, shape = env.OBS_FORMATS[fmt]
        obs = torch.empty((M, W) + shape, dtype=dt, device="cuda")

        def windows():
            env.draw_windows(ro, win, sel=sel, out=obs, obs_format=fmt)
            return 1

        def sequences():
            env.draw_sequences(ro, seqs, sel=seq_sel, out=obs, obs_format=fmt)
            return 1

        us = alternate({"draw_windows": windows, "draw_sequences": sequences}, args.calls, args.rounds)
        us["pad_share"] = {"draw_windows": round(1.0 - float(win.picks(sel=sel)[1].float().mean()), 4),
                           "draw_sequences": round(1.0 - float(seqs.picks(sel=seq_sel)[1].float().mean()), 4)}
        out["draw_us"][fmt] = us
        del obs
    if gather:
        out["gather"] = measure_gather(env, args)
    env.check_errors()
    env.close()
    return out


def tables(rows):
    md = ["### positions + picks, us per call: median (min-max) of the rounds", "",
          "| id | instances | K | M | W | (k) kernels | (t) torch expression | (h) host loop | (t)/(k) | (h)/(k) |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        for p in r["picks_us"]:
            u = p["us"]
            h = u.get("host_loop")
            md.append("| %s | %d | %d | %d | %d | %s | %s | %s | %s | %s |" % (r["env"], r["envs"], r["steps"], p["m"], p["window"], cell(u["kernels"]), cell(u["expression"]),
                                                                             cell(h) if h else "-", ratio(u["expression"], u["kernels"]), ratio(h, u["kernels"]) if h else "-"))
    md += ["", "### draw_windows next to draw_sequences, 4,096 x 16 rows, us per call", "",
           "| id | format | draw_windows (pad rows) | draw_sequences (pad rows) | windows / sequences |", "|---|---|---|---|---|"]
    for r in rows:
        for fmt, u in r["draw_us"].items():
            md.append("| %s | %s | %s (%.1f %%) | %s (%.1f %%) | %s |" % (r["env"], fmt, cell(u["draw_windows"]), 100 * u["pad_share"]["draw_windows"], cell(u["draw_sequences"]),
                                                                        100 * u["pad_share"]["draw_sequences"], ratio(u["draw_windows"], u["draw_sequences"])))
    for r in rows:
        if "gather" not in r:
            continue
        md += ["", "### gather of rows with 10 % pads from a store of 1,048,576 rows, us per call (GB/s: bytes read and written by the kernel)", "",
               "| row bytes | rows | (g) kernel | GB/s | (e) torch expression | (c) copy of the output | (e)/(g) | (c)/(g) |", "|---|---|---|---|---|---|---|---|"]
        for q in r["gather"]:
            u = q["us"]
            md.append("| %d | %d | %s | %.0f | %s | %s | %s | %s |" % (q["row_bytes"], q["rows"], cell(u["kernel"]), q["kernel_gbps"], cell(u["expression"]), cell(u["copy"]),
                                                                     ratio(u["expression"], u["kernel"]), ratio(u["copy"], u["kernel"])))
    return "\n".join(md) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("env", nargs="?")
    ap.add_argument("n", nargs="?", type=int)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-gather", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("window_bench.py needs the MI355X: nothing here is measured on a CPU")
    sizes = default_envs()
    todo = [(args.env, args.n or sizes[args.env])] if args.env else [(k, sizes[k]) for k in IDS]
    rows = []
    for k, (env_id, n) in enumerate(todo):
        rows.append(measure(env_id, n, args, k == 0 and not args.skip_gather))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(tables(rows))


if __name__ == "__main__":
    main()
