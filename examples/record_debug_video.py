#!/usr/bin/env python3
"""examples/record_debug_video.py -- a short ground-truth video of a FEW instances while many train (include/memgym.h: mg_save_debug_frames /
mg_draw_debug_frames).

render_debug() draws the view of every instance, synchronously: 22 GB at 65,536 instances to look at four of them.  Here four of N instances are watched
under the teacher for T steps: one save_debug_frames per step keeps their debug-view descriptors (16 / 64 / 128 bytes each) in a [T, 4, bytes] store, and
ONE draw_debug_frames at the end gives the [T, 4, 336, 336, 3] video -- what the reference's *_gt.gif recordings show.

    python examples/record_debug_video.py [--env Endless-MysteryPath-v0] [--envs 4096] [--steps 200] [--watch 0 1 2 3] [--out debug_video]

Writes OUT.npy (uint8 [T, 4, 336, 336, 3]) and, only if an image library (imageio or PIL) is importable, OUT_<instance>.gif per watched instance."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endless-memory-gym_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import memory_gym_amd  # noqa: E402


def write_gifs(video, watch, out):
    """video: uint8 [T, k, 336, 336, 3] -> the files written (none without an image library)"""
    try:
        import imageio
        for k, i in enumerate(watch):
            imageio.mimsave("%s_%d.gif" % (out, i), list(video[:, k]), duration=0.066)
    except ImportError:
        try:
            from PIL import Image
        except ImportError:
            return []
        for k, i in enumerate(watch):
            frames = [Image.fromarray(f) for f in video[:, k]]
            frames[0].save("%s_%d.gif" % (out, i), save_all=True, append_images=frames[1:], duration=66, loop=0)
    return ["%s_%d.gif" % (out, i) for i in watch]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="Endless-MysteryPath-v0")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--watch", type=int, nargs=4, default=[0, 1, 2, 3])
    ap.add_argument("--out", default="debug_video")
    args = ap.parse_args()
    N, T = args.envs, args.steps
    env = memory_gym_amd.make(args.env, num_envs=N, device=0)
    env.reset(seed=torch.arange(N, dtype=torch.int64, device="cuda"))
    watch = torch.tensor(args.watch, dtype=torch.int32, device="cuda")  # (distinct instances: a repeated index is not detected on the device)
    assert len(set(args.watch)) == len(args.watch) and all(0 <= i < N for i in args.watch), "--watch: four distinct instances of the handle"
    store = torch.zeros((T, len(args.watch), env.frame_record_bytes), dtype=torch.uint8, device="cuda")
    for t in range(T):
        env.step(env.expert_actions(eps=0.1, seed=1, step=t), render=False)  # (training would read env.obs of a drawn step here)
        env.save_debug_frames(idx=watch, out=store[t])  # one small launch; nothing synchronises
    video = env.draw_debug_frames(memory_gym_amd.DebugFrameRecords(store, env.frame_layout()))  # ONE launch: T x 4 views
    video = video.view(T, len(args.watch), 336, 336, 3).cpu().numpy()
    np.save(args.out + ".npy", video)
    gifs = write_gifs(video, args.watch, args.out)
    print("%s: %d of %d instances watched for %d steps: %d bytes of records kept, %.1f MB of video drawn once (render_debug() per step: %.1f GB each)" % (
        args.env, len(args.watch), N, T, store.numel(), video.nbytes / 1e6, N * 336 * 336 * 3 / 1e9))
    print("wrote %s.npy%s" % (args.out, "".join(", " + g for g in gifs) if gifs else " (no image library: no GIF)"))
    env.check_errors()
    env.close()


if __name__ == "__main__":
    main()
