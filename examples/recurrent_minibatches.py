#!/usr/bin/env python3
"""examples/recurrent_minibatches.py -- the data path of a RECURRENT trainer, on the device from end to end: one advance_traced(ro) keeps a rollout as
frame records, split_episodes cuts it into episodes at done and chops them into sequences of at most L steps (include/memgym.h: mg_split_episodes),
and every minibatch of M shuffled sequences is drawn as a zero-padded [M, L, 3, 84, 84] bfloat16 tensor with its loss mask, actions and rewards
(draw_sequences / EpisodeSequences.gather).  No host loop over the instances, and nothing leaves the GPU.

    python examples/recurrent_minibatches.py [--env MortarMayhem-Grid-v0] [--envs 4096] [--steps 128] [--length 16] [--batch 256] [--eps 0.1]

Prints how many sequences the rollout gave, the share of padding, and sequences per second for the split and for the minibatches."""
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
    ap.add_argument("--env", default="MortarMayhem-Grid-v0")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--length", type=int, default=16, help="steps per sequence: the recurrent network is unrolled over this many")
    ap.add_argument("--batch", type=int, default=256, help="sequences per minibatch")
    ap.add_argument("--eps", type=float, default=0.1)
    args = ap.parse_args()
    n, K, L, M = args.envs, args.steps, args.length, args.batch
    env = memory_gym_amd.make(args.env, num_envs=n, device=0)
    env.reset(seed=torch.arange(n, dtype=torch.int64, device="cuda"))
    ro = env.new_rollout(K)
    env.advance_traced(ro, eps=args.eps, seed=0, step=0, render=False)  # ro.frames[t]: the observation ro.actions[t] was played in

    # the cut.  capacity=None sizes the table from done.sum() (one look at the host); a trainer that wants the whole path enqueue-only passes a capacity
    seqs = env.split_episodes(ro.done, L)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seqs = env.split_episodes(ro.done, L, capacity=seqs.capacity)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    S = len(seqs)
    lens = seqs.table[:S, 2]
    print("%s x%d, %d steps: %d sequences of at most %d steps (%d full, %.1f %% of their rows padding), cut in %.0f us"
          % (args.env, n, K, S, L, int((lens == L).sum()), 100.0 * (1.0 - float(lens.sum()) / (S * L)), dt * 1e6))

    # one epoch of shuffled minibatches; the last one is padded to M sequences with -1 (rows of zeros, mask 0) so that every batch has one shape
    order = torch.randperm(S, device="cuda").to(torch.int32)
    batches = (S + M - 1) // M
    order = torch.cat([order, torch.full((batches * M - S,), -1, dtype=torch.int32, device="cuda")]).view(batches, M)
    obs = torch.empty((M, L, 3, 84, 84), dtype=torch.bfloat16, device="cuda")
    env.draw_sequences(ro, seqs, sel=order[0], out=obs, obs_format="bf16_chw")  # (untimed: the draw's kernel is loaded once per process)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(batches):
        sel = order[b]
        _, mask = env.draw_sequences(ro, seqs, sel=sel, out=obs, obs_format="bf16_chw")  # obs [M, L, 3, 84, 84], mask bool [M, L]
        actions = seqs.gather(ro.actions, sel=sel)  # [M, L] or [M, L, 2], zero at the pads
        rewards = seqs.gather(ro.reward, sel=sel)   # [M, L]
        # ... h = 0 at the start of every sequence; loss = (criterion(policy(obs, h), actions, rewards) * mask).sum() / mask.sum(); loss.backward() ...
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("%d minibatches of %d sequences x %d steps drawn in bf16_chw with mask, actions and rewards in %.3f s (%.0f sequences/s, %.2f M frames/s)"
          % (batches, M, L, dt, batches * M / dt, batches * M * L / dt / 1e6))
    assert actions.shape[:2] == rewards.shape == mask.shape == (M, L)
    env.check_errors()
    env.close()


if __name__ == "__main__":
    main()
