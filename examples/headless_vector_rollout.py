#!/usr/bin/env python3
"""examples/headless_vector_rollout.py -- a PPO-style collector in the gymnasium vector convention that never draws a frame it does not train on
(include/memgym.h: mg_info_buffers.final_frames_dev; GymnasiumVectorEnv(final_frames=True)).

The collector steps HEADLESS.  What it keeps of every step is the frame record behind the observation the action answers (16 / 64 / 128 bytes), and where
an episode ends inside a step -- the vector convention resets it in the same call -- the record of the frame it ENDED on, infos["final_frames"] under the
mask infos["_final_frames"]: that frame is what a value network has to see to bootstrap an episode that was cut off (a time limit, a capacity of this
build), and it is the one frame the reset frame replaces.  Afterwards the returns are computed with the bootstrap values of exactly those frames, and
shuffled minibatches are drawn from the records in the network's format.

    python examples/headless_vector_rollout.py [--env Endless-MortarMayhem-v0] [--envs 4096] [--steps 128] [--batch 4096] [--gamma 0.99]

The "value network" is a stand-in (the mean of the frame): the point is which frames reach it, not what it says.  Checks the terminal frames of one step
against a twin that draws them (final_observation=True) and prints what was drawn against what a drawn collector would have written."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endless-memory-gym_amd"))
import torch  # noqa: E402

from memory_gym_amd.vector import GymnasiumVectorEnv  # noqa: E402


def value(frames):
    """stand-in for the critic: bf16_chw frames [k, 3, 84, 84] -> float32 [k]"""
    return frames.to(torch.float32).mean(dim=(1, 2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="Endless-MortarMayhem-v0")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--gamma", type=float, default=0.99)
    args = ap.parse_args()
    N, T = args.envs, args.steps
    envs = GymnasiumVectorEnv(args.env, N, device=0, final_frames=True)
    twin = GymnasiumVectorEnv(args.env, N, device=0)  # the convention WITH frames, for the check only
    envs.reset(seed=0)
    twin.reset(seed=0)
    vec = envs.env
    B = vec.frame_record_bytes
    obs_rec = torch.empty((T + 1, N, B), dtype=torch.uint8, device="cuda")   # the observation each action answers (row T: the one behind the last step)
    final_rec = torch.zeros((T, N, B), dtype=torch.uint8, device="cuda")    # the frame an episode ended on, where ended[t, i]
    rewards = torch.empty((T, N), dtype=torch.float32, device="cuda")
    ended = torch.empty((T, N), dtype=torch.bool, device="cuda")
    truncated = torch.empty((T, N), dtype=torch.bool, device="cuda")
    probe_t, checked = None, 0
    for t in range(T):
        vec.save_frames(out=obs_rec[t])
        a = envs.expert_actions(eps=0.2, seed=1, step=t)  # (a policy would draw obs_rec[t] in its format here, or keep one drawn buffer: envs.redraw())
        obs, r, term, trunc, infos = envs.step(a)
        assert obs is None  # headless: nothing was drawn
        rewards[t], ended[t], truncated[t] = r, infos["_final_frames"], trunc
        final_rec[t] = infos["final_frames"].records  # (N x 16 .. 128 bytes; rows are valid where ended[t])
        _, _, term2, _, infos2 = twin.step(a)
        if probe_t is None and int(term2.sum()) > 0:  # the first step in which somebody finishes: the records draw what the twin drew
            idx, frames = envs.final_observations(infos)
            assert torch.equal(frames, infos2["final_observation"][term2]), "the terminal records do not draw the twin's terminal observations"
            probe_t, checked = t, len(idx)
    vec.save_frames(out=obs_rec[T])
    layout = vec.frame_layout()

    # returns with the bootstrap values of the frames the episodes ENDED on (every end is bootstrapped here, as a time limit would be; a trainer masks with
    # `truncated` to bootstrap only those) and of the frames behind the last step
    flat_final = final_rec.view(T * N, B)
    where = torch.nonzero(ended.view(-1)).flatten()
    boot = torch.zeros(T * N, dtype=torch.float32, device="cuda")
    for lo in range(0, where.numel(), args.batch):
        pick = where[lo:lo + args.batch].to(torch.int32)
        boot[pick.long()] = value(vec.draw_frames(flat_final, pick=pick, obs_format="bf16_chw"))
    last = torch.empty(N, dtype=torch.float32, device="cuda")
    for lo in range(0, N, args.batch):
        pick = torch.arange(lo, min(lo + args.batch, N), dtype=torch.int32, device="cuda")
        last[pick.long()] = value(vec.draw_frames(obs_rec[T], pick=pick, obs_format="bf16_chw"))
    boot = boot.view(T, N)
    returns = torch.empty((T, N), dtype=torch.float32, device="cuda")
    nxt = last
    for t in range(T - 1, -1, -1):
        nxt = rewards[t] + args.gamma * torch.where(ended[t], boot[t], nxt)
        returns[t] = nxt

    # training time: shuffled minibatches of the observations, drawn in the network's format
    batch = torch.empty((args.batch, 3, 84, 84), dtype=torch.bfloat16, device="cuda")
    order = torch.randperm(T * N, device="cuda").to(torch.int32)
    records = obs_rec[:T].view(T * N, B)
    n_batches = min(8, T * N // args.batch)
    for b in range(n_batches):
        pick = order[b * args.batch:(b + 1) * args.batch]
        vec.draw_frames(records, pick=pick, out=batch, obs_format="bf16_chw")
        # ... forward / backward on `batch` against returns.view(-1)[pick.long()] ...
    torch.cuda.synchronize()
    assert layout == vec.frame_layout()
    n_ended = int(ended.sum())
    drawn = n_ended + N + n_batches * args.batch
    print("%s: %d instances x %d headless steps, %d episodes ended (%d truncated); kept %.1f MB of records" % (
        args.env, N, T, n_ended, int(truncated.sum()), (obs_rec.numel() + final_rec.numel()) / 1e6))
    print("frames drawn: %d (terminal %d + last %d + minibatches %d) where a drawn collector in the vector convention writes %d observations and keeps a second "
          "[N] buffer of terminal ones" % (drawn, n_ended, N, n_batches * args.batch, T * N))
    if probe_t is not None:
        print("step %d: the %d terminal records draw the terminal observations of a twin that keeps them as frames, bit for bit" % (probe_t, checked))
    print("mean return %.4f" % float(returns.mean()))
    vec.check_errors()
    envs.close()
    twin.close()


if __name__ == "__main__":
    main()
