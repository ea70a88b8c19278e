#!/usr/bin/env python3
"""examples/rollout_from_records.py -- a rollout kept as frame RECORDS, not as frames (include/memgym.h: mg_save_frames / mg_draw_frames).

A teacher-driven rollout of T steps: the policy's input is drawn into the ONE [N] observation buffer per step as always, and what is kept of every step
is the descriptor row behind each frame -- 16 / 64 / 128 bytes instead of 21,168 (uint8) or 42,336 (bfloat16).  At training time shuffled minibatches are
drawn from the [T, N, bytes] store straight into the network's input tensor, in bf16_chw, whatever format the rollout ran in.

    python examples/rollout_from_records.py [--env MortarMayhem-Grid-v0] [--envs 4096] [--steps 128] [--batch 4096] [--headless]

--headless: the rollout is not drawn at all (step(render=False)); the records still hold every frame.
Prints the bytes kept against the bytes the frames would take, and checks one minibatch against frames cloned during the rollout."""
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
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--headless", action="store_true")
    args = ap.parse_args()
    N, T = args.envs, args.steps
    env = memory_gym_amd.make(args.env, num_envs=N, device=0)
    env.reset(seed=torch.arange(N, dtype=torch.int64, device="cuda"))
    store = torch.empty((T, N, env.frame_record_bytes), dtype=torch.uint8, device="cuda")
    rewards = torch.empty((T, N), dtype=torch.float32, device="cuda")
    probe_t, probe = T // 2, None  # one step's frames are cloned, to check a minibatch against
    for t in range(T):
        env.save_frames(out=store[t])  # the observation the action of step t answers
        if t == probe_t:
            if args.headless:
                env.redraw()
            probe = env.obs.clone()
        a = env.expert_actions(eps=0.2, seed=1, step=t)  # (a policy would read env.obs here)
        _, r, _, _, _ = env.step(a, render=not args.headless)
        rewards[t] = r
    records = memory_gym_amd.FrameRecords(store, env.frame_layout())
    kept, frames_u8 = store.numel(), T * N * 84 * 84 * 3
    print("%s: %d instances x %d steps = %d frames kept as %d-byte records: %.1f MB instead of %.2f GB of uint8 frames (x%d) or %.2f GB in bf16_chw" % (
        args.env, N, T, T * N, env.frame_record_bytes, kept / 1e6, frames_u8 / 1e9, frames_u8 // kept, 2 * frames_u8 / 1e9))

    # training time: shuffled minibatches, drawn in the network's format into its input tensor
    batch = torch.empty((args.batch, 3, 84, 84), dtype=torch.bfloat16, device="cuda")
    order = torch.randperm(T * N, device="cuda").to(torch.int32)
    n_batches = min(16, T * N // args.batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(n_batches):
        pick = order[b * args.batch:(b + 1) * args.batch]
        env.draw_frames(records, pick=pick, out=batch, obs_format="bf16_chw")
        # ... forward / backward on `batch`, rewards.view(-1)[pick.long()], ...
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("%d shuffled minibatches of %d frames drawn in bf16_chw: %.1f us each" % (n_batches, args.batch, dt / max(n_batches, 1) * 1e6))
    pick = (probe_t * N + torch.randperm(N, device="cuda")[:min(N, args.batch)]).to(torch.int32)
    got = env.draw_frames(records, pick=pick, obs_format="bf16_chw")
    want = (probe[(pick - probe_t * N).long()].permute(0, 3, 2, 1).to(torch.float32) / 255).to(torch.bfloat16)
    assert torch.equal(got, want), "a minibatch drawn from the records differs from the frames of the rollout"
    print("a minibatch of step %d equals the frames the rollout showed, bit for bit" % probe_t)
    env.check_errors()
    env.close()


if __name__ == "__main__":
    main()
