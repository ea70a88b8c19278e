"""`MemoryGymEnv`: the num_envs == 1 adapter with the reference's exact single-instance signature (numpy obs, Python float reward, bool done, False,
dict info) over a VecMemoryGym of one instance."""
import ctypes as C

import numpy as np
import torch

from . import _native
from .vec_env import VecMemoryGym

try:  # a real gymnasium.Env when the host has gymnasium (the reference's CustomEnv(gym.Env), environment.py:3-7)
    import gymnasium as _gym
    _EnvBase = _gym.Env
except Exception:  # gymnasium is not a dependency of the hot path
    _gym = None
    _EnvBase = object


class MemoryGymEnv(_EnvBase):
    """Single-instance environment with the reference's exact signatures (reset -> (obs, info); step -> 5-tuple of numpy
    obs, Python float reward, bool, False, dict) -- what `gymnasium.make(id)` returns.  Subclasses gymnasium.Env when
    gymnasium is importable; without it the same protocol surface (`unwrapped`, `spec`, `np_random`, `metadata`,
    `render_mode`, spaces) is provided here, so code written against the reference runs either way.

    Round 5: the single-instance fast path of the C ABI (include/memgym.h: mg_single_open / mg_single_reset / mg_single_step).
    Observation, reward, done, ground truth and the end-of-episode record live in pinned host memory that is mapped into the
    device; the kernels read the action from it and store their results straight into it, so step() is ONE native call (store the
    action, enqueue the step's launches, wait for the stream) and a copy of the 21-KB frame -- no torch operation.  (Rounds 1-4: an
    H2D action copy, two indexing kernels, three D2H copies and a stream synchronisation per step: 14 k steps/s.)"""

    metadata = {"render_modes": ["rgb_array", "debug_rgb_array"], "render_fps": 25}
    spec = None
    env_id = None  # set by the per-id subclasses in memory_gym_amd.envs

    def __init__(self, env_id=None, device=None, render_mode=None, capacity=None):
        env_id = env_id or self.env_id
        self.vec = VecMemoryGym(env_id, 1, device, render_mode, capacity=capacity)
        self.vec.autoreset = False
        self.action_space = self.vec.action_space
        self.observation_space = self.vec.observation_space
        self.has_ground_truth_info = self.vec.has_ground_truth_info
        if self.has_ground_truth_info:
            self.ground_truth_space = self.vec.ground_truth_space
        self.render_mode = render_mode
        self._np_random = None
        io = _native.new_struct(_native.SingleIO)
        with torch.cuda.device(self.vec.device):
            _native.check(_native.LIB.mg_single_open(self.vec._h, C.byref(io)), "mg_single_open")
        self._io = io

        def view(ptr, ctype, shape):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=shape)
        self._obs_host = view(io.obs, C.c_uint8, (84, 84, 3))
        self._vec_host = view(io.vec, C.c_float, (self.vec.vec_dim,)) if self.vec.vec_dim else None
        self._reward_host = view(io.reward, C.c_double, (1,))
        self._done_host = view(io.done, C.c_uint8, (1,))
        self._gt_host = view(io.gt, C.c_double, (max(self.vec.gt_dim, 1),))
        self._ep_reward_host = view(io.ep_reward, C.c_double, (1,))
        self._ep_length_host = view(io.ep_length, C.c_int32, (1,))
        self._aux_host = [view(io.aux[k], C.c_float, (1,)) for k in range(len(self.vec.info_names))]
        self._two_actions = self.vec.action_dim == 2
        # (the launch stream is torch's CURRENT stream at every call, like the batched path: a handle cached at construction or at the last
        # reset may be another stream than the caller's by now, or a released one -- ADVICE r5)
        self._raw_stream = self.vec._raw_stream
        self._step_fn, self._h, self._errword = _native.LIB.mg_single_step, self.vec._h, self.vec._err
        if self.vec.vector_obs is not None:
            # mg_single_open re-bound the handle's vector observation to the mapped block: `vec.vector_obs` (the batched tensor) is no
            # longer written; this adapter's observations carry the vector from the mapped block
            self.vec.vector_obs_stale = True
        self._peek = _native.LIB.mg_peek_errors

    # ---- gymnasium.Env protocol surface that exists with or without gymnasium
    @property
    def unwrapped(self):
        return self

    @property
    def np_random(self):
        """A numpy Generator like gymnasium.Env.np_random (the environment's own draws happen on the device, from the
        PCG64 stream that reset(seed) seeds exactly like gymnasium does; this host-side generator is seeded alike)."""
        if self._np_random is None:
            self._np_random = np.random.Generator(np.random.PCG64(np.random.SeedSequence()))
        return self._np_random

    @np_random.setter
    def np_random(self, value):
        self._np_random = value

    def _observation(self):
        o = self._obs_host.copy()
        if self._vec_host is not None:
            o = {"visual_observation": o, "vector_observation": self._vec_host.copy()}
        return o

    @property
    def max_episode_steps(self):
        return self.vec.max_episode_steps

    def reset(self, seed=None, return_info=True, options=None):
        if seed is not None:  # gymnasium.Env.reset(seed): the host-side generator follows the same seed
            self._np_random = np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(seed))))
        v = self.vec
        with torch.cuda.device(v.device):
            v._apply_options(options)
            if seed is None and not v._seeded:  # first reset without a seed: OS entropy, like gymnasium's np_random(None)
                seed = int(np.random.SeedSequence().generate_state(1, np.uint64)[0] >> np.uint64(1))
            _native.check(_native.LIB.mg_single_reset(self._h, 0 if seed is None else int(seed), 0 if seed is None else 1, C.c_void_p(self._raw_stream())), "mg_single_reset")
            v._seeded = True
        out = {}
        if v.gt_dim:
            out["ground_truth"] = self._gt_host[:v.gt_dim].copy()
        return self._observation(), out

    def step(self, action):
        if self._two_actions:
            a0, a1 = int(action[0]), int(action[1])
        else:
            a0 = a1 = int(action)
        rc = self._step_fn(self._h, a0, a1, self._raw_stream())
        if rc != 0:  # negative: the call failed; positive: device error bits as they stand (include/memgym.h)
            if rc < 0:
                _native.check(rc, "mg_single_step")
            if rc & ~self.vec._tolerated:
                self.vec.check_errors()
        r, d = float(self._reward_host[0]), bool(self._done_host[0])  # r: the reference's Python float, bit for bit
        out = {}
        if d:  # end of episode (rare): the reference's terminal info dict
            out["reward"] = float(self._ep_reward_host[0])
            out["length"] = int(self._ep_length_host[0])
            for nm, a in zip(self.vec.info_names, self._aux_host):
                out[nm] = float(a[0])
        if self.vec.gt_dim:
            out["ground_truth"] = self._gt_host[:self.vec.gt_dim].copy()
        return self._observation(), r, d, False, out

    def expert_action(self, eps=0.0, seed=0, step=None):
        """The scripted teacher's action in the current state (VecMemoryGym.expert_actions with one instance): an int for Discrete ids, a
        numpy int array of two for MultiDiscrete ids -- what step() takes.  Not a hot path (a launch and a copy to the host)."""
        a = self.vec.expert_actions(eps, seed, step).cpu().numpy()
        return a[0].copy() if self._two_actions else int(a[0])

    def render(self):
        if self.render_mode == "debug_rgb_array":
            return self.vec.render_debug()[0].cpu().numpy()
        return self._obs_host.transpose(1, 0, 2).copy()  # mortar_mayhem_grid.py:401-402

    def state_dict(self):
        return self.vec.state_dict()

    def load_state_dict(self, sd):
        self.vec.load_state_dict(sd)

    def snapshot(self):
        """The instance as it stands, in device memory (VecMemoryGym.save_instances) -- for restore()."""
        return self.vec.save_instances()

    def restore(self, snap):
        """Put the instance back where snapshot() found it (VecMemoryGym.load_instances): the following steps give what the steps after the
        snapshot gave.  -> the observation of that moment, as reset() returns it.  Not a hot path (a launch, a frame and a copy to the host)."""
        v = self.vec
        v.load_instances(snap, render=True)
        torch.cuda.current_stream(v.device).synchronize()
        self._obs_host[...] = v.obs[0].cpu().numpy()
        if v.gt_dim:
            self._gt_host[:v.gt_dim] = (v.gt64 if v.gt64 is not None else v.gt)[0].double().cpu().numpy()
        return self._observation()

    def close(self):
        self.vec.close()
