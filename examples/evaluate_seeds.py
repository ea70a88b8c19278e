#!/usr/bin/env python3
"""examples/evaluate_seeds.py -- exactly ONE episode per seed, the evaluation protocol of the Memory Gym paper, in one handle: every instance
plays its seed's episode under the scripted teacher and is then left alone (VecMemoryGym.step(mask=...), include/memgym.h: mg_step_masked),
so no instance is stepped past its end and nothing has to be filtered afterwards.

    python examples/evaluate_seeds.py [--env MortarMayhem-Grid-v0] [--seeds 64] [--first-seed 0] [--eps 0.1] [--options '{"command_count": [5]}'] [--check]

Per seed one line: return, length and the named aux infos of its episode.  --check (on a GPU machine) plays the same seeds a second time the
way it had to be done before -- every instance stepped every time with auto-reset on, the first episode's record picked out afterwards --
and compares per seed; it reads nothing outside the repository."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endless-memory-gym_amd"))
import torch  # noqa: E402

import memory_gym_amd  # noqa: E402


def evaluate(env, seeds, eps=0.0, hash_seed=0, options=None, max_steps=None, masked=True):
    """One episode per seed on the handle `env` (len(seeds) == env.num_envs) under expert_actions(eps, hash_seed, t) at step t.
    -> dict of [N] tensors: "return" (float64), "length" (int32), one float32 tensor per entry of env.info_names, "episodes" (int32: episodes
    recorded per instance, 1 everywhere when the loop ended by itself) and "steps" (the loop's length, an int).  The loop ends when every
    instance has finished, or after max_steps (default: the handle's max_episode_steps, which bounds an episode where the id has one).
    masked=False is the workaround this replaces: everybody steps with auto-reset on and only the first episode's record is kept."""
    n = env.num_envs
    env.reset(seed=seeds, options=options)
    limit = max_steps if max_steps is not None else env.max_episode_steps
    if limit is None or limit < 0:
        raise ValueError("this id's episodes have no bound under these options: pass max_steps")
    dev = env.device
    finished = torch.zeros(n, dtype=torch.bool, device=dev)
    out = {"return": torch.zeros(n, dtype=torch.float64, device=dev), "length": torch.zeros(n, dtype=torch.int32, device=dev),
           "episodes": torch.zeros(n, dtype=torch.int32, device=dev)}
    for nm in env.info_names:
        out[nm] = torch.zeros(n, dtype=torch.float32, device=dev)
    t = 0
    while t < limit and not bool(finished.all()):
        a = env.expert_actions(eps, hash_seed, t)
        if masked:  # the finished instances are left alone: `done` is False for them
            _, _, done, _, info = env.step(a, render=False, mask=~finished)
            first = done
        else:
            _, _, done, _, info = env.step(a, render=False)
            first = done & ~finished
        out["return"] = torch.where(first, info["reward"], out["return"])
        out["length"] = torch.where(first, info["length"], out["length"])
        for nm in env.info_names:
            out[nm] = torch.where(first, info[nm], out[nm])
        out["episodes"] += first.to(torch.int32)
        finished |= done
        t += 1
    env.check_errors()
    out["steps"] = t
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MortarMayhem-Grid-v0")
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--first-seed", type=int, default=0)
    ap.add_argument("--eps", type=float, default=0.1, help="share of uniformly random actions (0 = the teacher, 1 = the random policy)")
    ap.add_argument("--hash-seed", type=int, default=0)
    ap.add_argument("--options", default=None, help="a JSON dictionary of reset options")
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--check", action="store_true", help="compare with the unmasked workaround on the same seeds")
    args = ap.parse_args()
    n = args.seeds
    options = json.loads(args.options) if args.options else None
    seeds = torch.arange(n, dtype=torch.int64, device="cuda") + args.first_seed
    env = memory_gym_amd.make(args.env, num_envs=n, device=0)
    res = evaluate(env, seeds, args.eps, args.hash_seed, options, args.max_steps)
    cpu = {k: (v.cpu().tolist() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}
    for i in range(n):
        aux = ", ".join("%s %g" % (nm, cpu[nm][i]) for nm in env.info_names)
        print("seed %d: return %.4f, length %d%s%s" % (args.first_seed + i, cpu["return"][i], cpu["length"][i], ", " if aux else "", aux)
              if cpu["episodes"][i] else "seed %d: unfinished after %d steps" % (args.first_seed + i, cpu["steps"]))
    print("%s: %d seeds, %d finished in %d steps, mean return %.4f, mean length %.1f; %d masked steps"
          % (args.env, n, sum(cpu["episodes"]), cpu["steps"], sum(cpu["return"]) / n, sum(cpu["length"]) / n, env.debug_counter("masked_steps")))
    if args.check:
        twin = memory_gym_amd.make(args.env, num_envs=n, device=0)
        want = evaluate(twin, seeds, args.eps, args.hash_seed, options, args.max_steps, masked=False)
        for k in res:
            same = torch.equal(res[k], want[k]) if isinstance(res[k], torch.Tensor) else res[k] == want[k]
            if not same:
                sys.exit("check FAILED: %r differs from the unmasked run" % k)
        twin.close()
        print("check ok: every seed's record equals the first episode of an unmasked auto-reset run")
    env.close()


if __name__ == "__main__":
    main()
