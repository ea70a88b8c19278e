#!/usr/bin/env python3
"""examples/collect_expert_records.py -- the task of collect_expert_pairs.py, (observation, expert action) pairs for behaviour cloning, collected as
ROLLOUT TRACES: one advance_traced(ro, eps) per chunk keeps every step's frame record (16 / 64 / 128 bytes instead of a 21 KB frame), the action
played and the teacher's label (include/memgym.h: mg_advance_traced); training then draws only the minibatch it asks for, in the network's format,
straight into its input tensor (RolloutTrace.draw).  Nothing leaves the GPU.

    python examples/collect_expert_records.py [--env MysteryPath-Grid-v0] [--envs 4096] [--steps 128] [--chunk 64] [--eps 0.1] [--batch 4096] [--batches 32]

Prints pairs per second for both phases -- collecting the records, drawing minibatches from them -- and how often label and played action differ."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endless-memory-gym_amd"))
import torch  # noqa: E402

import memory_gym_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MysteryPath-Grid-v0")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--chunk", type=int, default=64, help="steps per advance() call: one RolloutTrace per chunk")
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--batches", type=int, default=32)
    args = ap.parse_args()
    n, K = args.envs, args.chunk
    env = memory_gym_amd.make(args.env, num_envs=n, device=0)
    env.reset(seed=torch.arange(n, dtype=torch.int64, device="cuda"))
    chunks = [env.new_rollout(K, labels=True) for _ in range(max(1, args.steps // K))]
    env.advance_traced(chunks[0], eps=args.eps, seed=0, step=0, render=False)  # (untimed: the call's scratch is allocated and its kernels are loaded once per handle)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    episodes = 0
    for c, ro in enumerate(chunks):
        _, st = env.advance_traced(ro, eps=args.eps, seed=0, step=(1 + c) * K, render=False)  # ro.frames[t]: the state actions[t] / labels[t] belong to
        episodes = episodes + st["episodes"].sum()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    pairs = n * K * len(chunks)
    differ = sum(int((ro.labels != ro.actions).reshape(K * n, -1).any(1).sum()) for ro in chunks)
    print("%s x%d: %d pairs kept as records in %.3f s (%.2f M pairs/s), %.1f MB of records; %d episodes finished; played != label in %.1f %% of the pairs"
          % (args.env, n, pairs, dt, pairs / dt / 1e6, sum(ro.frames.numel() for ro in chunks) / 1e6, int(episodes), 100.0 * differ / pairs))

    # training time: minibatches of (frame, label) drawn from the records in the network's format; frames[K] has no label (it is the next chunk's row 0)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.empty((args.batch, 3, 84, 84), dtype=torch.bfloat16, device="cuda")
    width = (args.batch,) if env.action_dim == 1 else (args.batch, 2)
    y = torch.empty(width, dtype=torch.int32, device="cuda")
    chunks[0].draw(env, [0], [0], out=x[:1], obs_format="bf16_chw")  # (untimed: the draw's kernel is loaded once per process)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(args.batches):
        ro = chunks[b % len(chunks)]
        t = torch.randint(0, K, (args.batch,), generator=g, device="cuda")
        i = torch.randint(0, n, (args.batch,), generator=g, device="cuda")
        ro.draw(env, t, i, out=x, obs_format="bf16_chw")
        y.copy_(ro.labels[t, i])
        # ... loss(policy(x), y).backward() ...
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("%d minibatches of %d pairs drawn in bf16_chw in %.3f s (%.2f M pairs/s)" % (args.batches, args.batch, dt, args.batches * args.batch / dt / 1e6))
    env.check_errors()
    env.close()


if __name__ == "__main__":
    main()
