#!/usr/bin/env python3
"""examples/transformer_windows.py -- the data path of a TransformerXL-style trainer with a sliding episodic memory, on the device from end to end: two
consecutive traced rollouts, and for every training sample (t, i) of the second one the window of instance i's previous W steps inside the same
episode -- reaching back into the FIRST rollout where the episode began there (include/memgym.h: mg_episode_positions / mg_window_picks).  The positions
and the last `back` rows are carried from one rollout to the next; minibatches of [M, W] observation windows are drawn in bfloat16 (draw_windows), and
the memory of past hidden states is gathered from the trainer's own per-step store with lag = 1 (EpisodeWindows.gather: mg_gather_rows_padded).

    python examples/transformer_windows.py [--env MortarMayhem-Grid-v0] [--envs 4096] [--steps 128] [--window 16] [--back 16] [--batch 256] [--hidden 384]

Prints the share of padding, how many windows reach into the previous rollout, and windows per second."""
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
    ap.add_argument("--window", type=int, default=16, help="rows of a memory window")
    ap.add_argument("--back", type=int, default=16, help="rows of the previous rollout a window may reach into (at most --steps)")
    ap.add_argument("--batch", type=int, default=256, help="samples per minibatch")
    ap.add_argument("--hidden", type=int, default=384, help="floats of a hidden state: the rows of the trainer's own store")
    ap.add_argument("--eps", type=float, default=0.1)
    args = ap.parse_args()
    n, K, W, back, M, H = args.envs, args.steps, args.window, args.back, args.batch, args.hidden
    env = memory_gym_amd.make(args.env, num_envs=n, device=0)
    env.reset(seed=torch.arange(n, dtype=torch.int64, device="cuda"))

    carry = None                      # positions behind the previous rollout's last step: the next call's pos0
    tail_frames = tail_hidden = None  # the last `back` rows in front of the previous rollout's row K
    for r in range(2):
        ro = env.new_rollout(K)
        env.advance_traced(ro, eps=args.eps, seed=0, step=r * K, render=False, stats=False)  # ro.frames[0] is the previous rollout's frames[K]
        hidden = torch.randn((K + 1, n, H), device="cuda")  # the hidden state the policy computed at every frame (a dummy here)
        b = 0 if r == 0 else back
        frames_win = env.episode_windows(ro.done, W, lag=0, back=b, pos0=carry)  # windows of frames end with the sample's own frame
        memory_win = env.episode_windows(ro.done, W, lag=1, back=b, pos0=carry)  # memories end one step earlier
        if r == 1:
            store = memory_gym_amd.FrameRecords(torch.cat((tail_frames, ro.frames)), env.frame_layout())  # [back + K + 1, N, bytes]
            mem_store = memory_win.store(hidden, tail_hidden)  # cat(prefix, hidden) over [back + K + 1, N], flattened, made once per rollout
            samples = torch.randperm(K * n, device="cuda").to(torch.int32)  # rows 0 .. K - 1: row K is the bootstrap observation
            batches = min(32, (K * n) // M)
            obs = torch.empty((M, W, 3, 84, 84), dtype=torch.bfloat16, device="cuda")
            env.draw_windows(store, frames_win, sel=samples[:M], out=obs, obs_format="bf16_chw")  # (untimed: the kernels are loaded once per process)
            env.gather_rows(mem_store, memory_win.picks(sel=samples[:M])[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pads = reach = 0
            for k in range(batches):
                sel = samples[k * M:(k + 1) * M]
                _, mask, length = env.draw_windows(store, frames_win, sel=sel, out=obs, obs_format="bf16_chw")  # obs [M, W, 3, 84, 84], mask [M, W], len [M]
                pick, mem_mask, _ = memory_win.picks(sel=sel)
                memory = env.gather_rows(mem_store, pick)  # [M, W, H], zero rows at the pads (memory_win.gather(hidden, sel, tail_hidden) in one call)
                pads += (~mask).sum()
                reach += (pick[:, 0] >= 0).logical_and(pick[:, 0] < back * n).sum()
                # (the valid rows come first, oldest first: the sample's own frame is obs[j, length[j] - 1])
                # ... logits = policy(obs, mask, memory, mem_mask); loss.backward() ...
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print("%s x%d, rollout 2 of %d steps: %d minibatches of %d windows x %d rows (%.1f %% padding, %d windows begin in rollout 1) with %d-float "
                  "memories in %.3f s: %.0f windows/s" % (args.env, n, K, batches, M, W, 100.0 * float(pads) / (batches * M * W), int(reach), H, dt, batches * M / dt))
            assert memory.shape == (M, W, H) and mask.shape == mem_mask.shape == (M, W)
        carry = frames_win.carry
        tail_frames, tail_hidden = ro.frames[K - back:K].clone(), hidden[K - back:K].clone()
    env.check_errors()
    env.close()


if __name__ == "__main__":
    main()
