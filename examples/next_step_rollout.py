#!/usr/bin/env python3
"""examples/next_step_rollout.py -- a PPO-shaped collection loop on a handle in next-step auto-reset mode (make(..., autoreset_mode="next_step"),
include/memgym.h: mg_step_next; gymnasium >= 1.0's default convention): the step that ends an episode returns the TERMINAL observation as its
ordinary observation, so the value to bootstrap from where an episode was cut off is v(obs) where done -- no second buffer, no "final_observation".
The step after it ignores the instance's action and returns the first observation of the new episode with reward 0: that transition is no
sample, its slot is masked out of the loss.

    python examples/next_step_rollout.py [--env MortarMayhem-Grid-v0] [--envs 1024] [--steps 128] [--gamma 0.99] [--lam 0.95]

The policy is the scripted teacher with a share of random actions, the value function a stand-in (the mean brightness of the frame): the loop,
the masks and the advantage recursion are what a trainer would keep.  Prints the number of valid samples, of episodes and their mean return."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endless-memory-gym_amd"))
import torch  # noqa: E402

import memory_gym_amd  # noqa: E402


def value(obs):
    """a stand-in for the critic: [N] float32 from the frames"""
    frames = obs["visual_observation"] if isinstance(obs, dict) else obs
    return frames.reshape(frames.shape[0], -1).float().mean(1) / 255.0


def collect(env, steps, gamma, lam, eps=0.1):
    """`steps` calls of step() -> dict of [steps, N] tensors: "valid" (False where the call restarted the instance: no transition), "reward", "done",
    "value", "advantage" (GAE; an episode's end is treated as a time limit, so its last step bootstraps from the terminal observation the same
    call returned), and the finished episodes' returns."""
    n, dev = env.num_envs, env.device
    valid = torch.zeros((steps, n), dtype=torch.bool, device=dev)
    reward = torch.zeros((steps, n), dtype=torch.float32, device=dev)
    done = torch.zeros((steps, n), dtype=torch.bool, device=dev)
    values = torch.zeros((steps, n), dtype=torch.float32, device=dev)
    after = torch.zeros((steps, n), dtype=torch.float32, device=dev)  # v(observation the call returned): the terminal observation's where done
    returns = []
    obs = env.obs if env.vector_obs is None else {"visual_observation": env.obs, "vector_observation": env.vector_obs}
    prev_done = env.done_u8.view(torch.bool).clone()  # the pending flags: these instances are restarted by the next call
    for t in range(steps):
        values[t] = value(obs)
        valid[t] = ~prev_done
        obs, r, d, _, info = env.step(env.expert_actions(eps, 0, t))
        reward[t], done[t], after[t] = r, d, value(obs)
        if bool(d.any()):
            returns.append(info["reward"][d].clone())
        prev_done = d.clone()
    adv = torch.zeros((steps, n), dtype=torch.float32, device=dev)
    carry = torch.zeros(n, dtype=torch.float32, device=dev)
    for t in reversed(range(steps)):
        # after[t] is v(s_{t+1}) inside an episode and v(terminal observation) at its end; nothing flows back across an end or a restart
        delta = reward[t] + gamma * after[t] - values[t]
        carry = torch.where(valid[t], delta + gamma * lam * torch.where(done[t], torch.zeros_like(carry), carry), torch.zeros_like(carry))
        adv[t] = carry
    env.check_errors()
    return {"valid": valid, "reward": reward, "done": done, "value": values, "advantage": adv,
            "episode_returns": torch.cat(returns) if returns else torch.zeros(0, dtype=torch.float64, device=dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="MortarMayhem-Grid-v0")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    args = ap.parse_args()
    env = memory_gym_amd.make(args.env, num_envs=args.envs, device=0, autoreset_mode="next_step")
    env.reset(seed=0)
    ro = collect(env, args.steps, args.gamma, args.lam)
    ep = ro["episode_returns"]
    print("%s: %d of %d slots are samples, %d episodes ended, mean return %.4f; %d next-step calls, %d in the family's own kernel"
          % (args.env, int(ro["valid"].sum()), ro["valid"].numel(), ep.numel(), float(ep.mean()) if ep.numel() else float("nan"),
             env.debug_counter("next_steps"), env.debug_counter("next_fused_steps")))
    env.close()


if __name__ == "__main__":
    main()
