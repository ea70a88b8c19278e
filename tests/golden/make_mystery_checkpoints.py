#!/usr/bin/env python3
"""Checkpoints of the three Mystery Path ids as ONE commit's build wrote them, and what that build computed from them afterwards.

Run once on an MI355X against a build of the commit whose checkpoints later builds have to keep loading:

    python tests/golden/make_mystery_checkpoints.py --commit <that commit's id> [--out FILE]   ->  tests/golden/mystery_checkpoints.npz

Per case (CASES): reset with fixed seeds, WARM steps under expert_actions(eps=0.3) -- episodes end, paths are regenerated, the endless id
appends segments and owes some -- then state_dict() is stored (the blob, the options as JSON, the capacity, `seeded`), then REPLAY more
steps whose actions, rewards, dones, ground truth and info records (where an episode ended) are stored, with the frames after the
first and the last of them and the rng_words of every instance at the end.  tests/test_gpu_mystery_checkpoints.py loads each state into
a fresh handle, replays the actions and requires all of it bit for bit: a build that reorders, resizes or drops a blob of the state does
not get there.

A case's replay is lengthened (by REPLAY steps at a time) until an episode has ended inside it; the script fails if none ever does.
The fixture is DATA: the state blobs and the recorded results.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "endless-memory-gym_amd"))

N, WARM, REPLAY, REPLAY_MAX, EPS = 3, 30, 40, 400, 0.3
# name -> (env id, reset options, capacity, seed of the reset, seed of the policy's draws)
CASES = {
    "mp": ("MysteryPath-v0", dict(max_steps=24), None, 31, 101),
    "mpg": ("MysteryPath-Grid-v0", dict(max_steps=24), None, 32, 102),
    "emp": ("Endless-MysteryPath-v0", None, None, 33, 103),
    "emp_cap7": ("Endless-MysteryPath-v0", None, {"path_segments": 7}, 34, 104),
}


def record(env, actions):
    """One step; -> the step's results as numpy arrays (info records: where an episode ended, 0 elsewhere)."""
    obs, rew, done, _, info = env.step(actions)
    d = done.cpu().numpy()
    out = {"reward": rew.cpu().numpy().copy(), "done": d.copy()}
    if env.gt_dim:
        out["ground_truth"] = info["ground_truth"].cpu().numpy().copy()
    for nm in ["reward", "length"] + list(env.info_names):
        v = info[nm].cpu().numpy()
        out["info_" + nm] = np.where(d, v, np.zeros_like(v))
    return obs, out


def main():
    import memory_gym_amd

    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="id of the commit the loaded library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "mystery_checkpoints.npz"))
    args = ap.parse_args()
    out = {"commit": np.array(args.commit), "cases": np.array(sorted(CASES))}
    for name, (env_id, options, capacity, seed, pseed) in sorted(CASES.items()):
        env = memory_gym_amd.make(env_id, num_envs=N, device=0, capacity=capacity)
        env.reset(seed=seed + 1000 * np.arange(N, dtype=np.int64), options=options)
        warm_done = 0
        for t in range(WARM):
            _, _, done, _, _ = env.step(env.expert_actions(eps=EPS, seed=pseed, step=t))
            warm_done += int(done.sum())
        sd = env.state_dict()
        assert sd["env_id"] == env_id and sd["num_envs"] == N and "option_sets" not in sd
        out[name + "/blob"] = sd["blob"].copy()
        out[name + "/options"] = np.array(json.dumps(sd["options"], sort_keys=True))
        out[name + "/capacity"] = np.array(json.dumps(sd["capacity"], sort_keys=True))
        out[name + "/seeded"] = np.array(bool(sd["seeded"]))
        actions, steps, frames, n_done = [], [], [], 0
        while n_done == 0 and len(steps) < REPLAY_MAX:
            for _ in range(REPLAY):
                a = env.expert_actions(eps=EPS, seed=pseed, step=WARM + len(steps))
                obs, rec = record(env, a)
                if not steps:
                    frames.append(obs.cpu().numpy().copy())
                actions.append(a.cpu().numpy().copy())
                steps.append(rec)
                n_done += int(rec["done"].sum())
        assert n_done > 0, "%s: no episode ended within %d replayed steps" % (name, len(steps))
        frames.append(obs.cpu().numpy().copy())
        out[name + "/actions"] = np.stack(actions)
        for key in steps[0]:
            out[name + "/" + key] = np.stack([s[key] for s in steps])
        out[name + "/frames"] = np.stack(frames)  # after the first and after the last replayed step
        out[name + "/rng_words"] = np.stack([env.rng_words(i) for i in range(N)])
        env.check_errors()
        print("%-9s %-24s blob %7d B, %d episodes ended in the %d warm steps, %d in the %d replayed ones"
              % (name, env_id, sd["blob"].size, warm_done, WARM, n_done, len(steps)))
        env.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out) // 1024, "KiB")


if __name__ == "__main__":
    main()
