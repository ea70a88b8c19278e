"""Batched, device-resident Memory Gym environments behind the reference's env ids and reset-options dict.

`VecMemoryGym(env_id, num_envs, device)` holds `num_envs` independent instances of one of the reference's
environments (memory_gym/__init__.py:13-61) on one MI355X.  reset()/step() enqueue HIP kernels on torch's current
stream and return torch tensors that alias the kernels' output buffers (no copies, no host synchronisation):

    obs      uint8  [N, 84, 84, 3]  indexed [env][x][y][c], exactly the reference's array3d layout
    reward   float32 [N]
    done     bool   [N]             (`truncation` is always False in the reference)
    info     dict of tensors: "done_mask", end-of-episode records ("reward", "length", "success", ...) that are valid
             where done_mask is set, and "ground_truth" [N, G] for the endless envs.

`MemoryGymEnv` is the num_envs == 1 adapter with the reference's exact single-instance signature
(numpy obs, Python float reward, bool done, False, dict info).

This module holds the handle.  What it returns and takes lives below it and is re-exported here under the names it always had: the observation
memory (obs_memory.py), the value types with their handle-free checks (records.py, episodes.py, over _args.py), the handle's calls over kept
rollouts (record_calls.py, its base class); the adapter (single.py) sits on top of it.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _native
from ._args import MAX_PICK, aligned_on, index_tensor, ptr  # noqa: F401
from .episodes import (EpisodeSequences, EpisodeWindows, RolloutTargets, check_episode_windows, check_gather_rows, check_rollout_targets,  # noqa: F401
                       check_split_episodes, check_window_frames, rollout_targets)
from .obs_memory import alloc_obs_buffer, is_balanced_buffer  # noqa: F401
from .record_calls import RecordCalls
from .records import (MAX_DRAW_RECORDS, OBS_FORMATS, DebugFrameRecords, FrameRecords, InstanceSnapshot, RolloutTrace, _distinct_host_index,  # noqa: F401
                      check_frame_draw, check_frame_save, check_instance_load, check_instance_save, check_rollout_trace)
from .reset_params import DEFAULTS, calc_max_episode_steps, process_reset_params

ENV_IDS = list(DEFAULTS.keys())


class _Space:
    def __init__(self, kind, **kw):
        self.kind = kind
        self.__dict__.update(kw)

    def __repr__(self):
        return "%s(%s)" % (self.kind, ", ".join("%s=%r" % kv for kv in self.__dict__.items() if kv[0] != "kind"))


def _spaces(action_dim, gt_dim, vec_dim=0):
    try:  # use real gymnasium spaces when the host has them
        from gymnasium import spaces
        act = spaces.Discrete(4) if action_dim == 1 else spaces.MultiDiscrete([3, 3])
        obs = spaces.Box(low=0, high=255, shape=[84, 84, 3], dtype=np.uint8)
        if vec_dim:  # MortarMayhemB*: mortar_mayhem_b_grid.py:83-96
            obs = spaces.Dict({"visual_observation": obs,
                               "vector_observation": spaces.Box(low=np.zeros(vec_dim, np.float32), high=np.ones(vec_dim, np.float32),
                                                                shape=(vec_dim,), dtype=np.float32)})
        gt = None if gt_dim == 0 else spaces.Box(low=np.zeros(gt_dim, np.float32), high=np.ones(gt_dim, np.float32),
                                                  shape=(gt_dim,), dtype=np.float32)
    except Exception:
        act = _Space("Discrete", n=4) if action_dim == 1 else _Space("MultiDiscrete", nvec=[3, 3])
        obs = _Space("Box", low=0, high=255, shape=[84, 84, 3], dtype=np.uint8)
        if vec_dim:
            obs = _Space("Dict", spaces={"visual_observation": obs, "vector_observation": _Space(
                "Box", low=0.0, high=1.0, shape=(vec_dim,), dtype=np.float32)})
        gt = None if gt_dim == 0 else _Space("Box", low=0.0, high=1.0, shape=(gt_dim,), dtype=np.float32)
    return act, obs, gt


class VecMemoryGym(RecordCalls):
    metadata ={"render_modes": ["rgb_array", "debug_rgb_array"], "render_fps": 25}

    OBS_FORMATS = OBS_FORMATS
    # "same_step": an instance that finishes is reset inside the call (gymnasium 0.29's vector convention); "disabled": autoreset = False, the caller
    # resets with a masked reset(); "next_step": gymnasium >= 1.0's AutoresetMode.NEXT_STEP (include/memgym.h: mg_step_next), see step()
    AUTORESET_MODES = ("same_step", "next_step", "disabled")

    def __init__(self, env_id, num_envs=1, device=None, render_mode=None, obs_format="u8_xyc", final_observation=False,
                 obs_buffer=None, obs_placement=None, ground_truth64=False, on_capacity="raise", capacity=None,
                 autoreset_mode="same_step", final_frames=False):
        if env_id not in DEFAULTS:
            raise ValueError("unknown env id %r" % (env_id,))
        if autoreset_mode not in self.AUTORESET_MODES:
            raise ValueError("autoreset_mode must be one of %s" % (self.AUTORESET_MODES,))
        if autoreset_mode == "next_step" and (final_observation or final_frames):
            raise ValueError("autoreset_mode='next_step' together with final_observation=True / final_frames=True: there are no terminal rows in "
                             "this mode, the observation of the step that ends an episode IS the terminal observation")
        if obs_format not in self.OBS_FORMATS:
            raise ValueError("obs_format must be one of %s" % sorted(self.OBS_FORMATS))
        if final_observation and final_frames:
            raise ValueError("final_observation=True together with final_frames=True: terminal frames are kept as frames or as records, pick one")
        if not torch.cuda.is_available():
            raise RuntimeError("memory_gym_amd needs a ROCm GPU (MI355X); no CPU fallback exists")
        self.env_id = env_id
        self.num_envs = int(num_envs)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   (device if isinstance(device, int) else torch.device(device).index or 0))
        self.render_mode = render_mode
        h = C.c_void_p()
        _native.check(_native.LIB.mg_create(env_id.encode(), self.num_envs, self.device.index, C.byref(h)), "mg_create")
        self._h = h
        # capacity={"path_segments": 1024} / {"commands": 2048}: room for the lists the reference grows without limit (include/memgym.h:
        # mg_set_capacity; the defaults -- 128 segments = 1,024 tiles, 512 commands -- are what every measured number of this repo uses)
        self.capacity = {}
        for what, value in (capacity or {}).items():
            with torch.cuda.device(self.device):
                rc = _native.LIB.mg_set_capacity(h, what.encode(), int(value))
            if rc != 0:
                raise ValueError("capacity[%r] = %r: %s" % (what, value, _native.last_error()))
            self.capacity[what] = int(value)
        self.action_dim = _native.LIB.mg_action_dim(h)
        self.gt_dim = _native.LIB.mg_gt_dim(h)
        self.vec_dim = _native.LIB.mg_vec_dim(h)
        self.has_ground_truth_info = self.gt_dim > 0
        self.action_space, self.observation_space, self.ground_truth_space = _spaces(self.action_dim, self.gt_dim, self.vec_dim)
        N, dev = self.num_envs, self.device
        # "u8_xyc" is the reference's observation; "f32_chw"/"f16_chw" are obs/255 in [c][y][x] order, converted inside
        # the raster kernel's stream-out (what a trainer would otherwise compute from the uint8 frame every step); "u8_chw" is the
        # reference's bytes in [c][y][x] order: obs[i, c, y, x] == u8_xyc obs[i, x, y, c] -- a uint8 rollout buffer in image order
        self.obs_format = obs_format
        code, dt, shape = self.OBS_FORMATS[obs_format]
        _native.check(_native.LIB.mg_set_obs_format(h, code), "mg_set_obs_format")
        assert _native.LIB.mg_obs_bytes(h) == 84 * 84 * 3 * torch.empty((), dtype=dt).element_size()
        self.obs_placement_info = None
        if obs_placement is None:
            obs_placement = os.environ.get("MEMGYM_OBS_PLACEMENT", "balanced")
        if obs_placement not in ("balanced", "plain"):
            raise ValueError("obs_placement must be 'balanced' or 'plain'")
        if obs_buffer is None:
            # "balanced": physical pages from two HBM zones (include/memgym.h: mg_obs_alloc; 12-15 % on the raster kernel);
            # buffers of 304 MiB or less and "plain" are ordinary allocations
            nbytes = N * 84 * 84 * 3 * torch.empty((), dtype=dt).element_size()
            self.obs = None
            if obs_placement == "balanced" and nbytes > (304 << 20):
                try:
                    self.obs, self.obs_placement_info = alloc_obs_buffer((N,) + shape, dt, dev)
                except RuntimeError as e:  # e.g. out of memory during the search: an ordinary allocation works as well
                    import warnings
                    warnings.warn("memory_gym_amd: balanced observation buffer not available (%s); using a plain allocation" % (e,))
            if self.obs is None:
                self.obs = torch.empty((N,) + shape, dtype=dt, device=dev)
        else:
            # caller-owned observation memory: the raster kernel writes the frames there (any device-accessible address,
            # e.g. this rank's rows of a peer-mapped buffer on another GPU: memory_gym_amd.dist.PeerObsBuffer)
            if tuple(obs_buffer.shape) != (N,) + shape or obs_buffer.dtype != dt or not obs_buffer.is_cuda or not obs_buffer.is_contiguous():
                raise ValueError("obs_buffer must be a contiguous CUDA tensor of shape %s and dtype %s" % ((N,) + shape, dt))
            self.obs = obs_buffer
        # gymnasium-0.29 vector convention: keep the terminal frame of instances that finish (and auto-reset) in a step
        self.final_obs = torch.zeros((N,) + shape, dtype=dt, device=dev) if final_observation else None
        # MortarMayhemB*: obs is the reference's Dict; `vector_obs` is written by the library whenever an instance resets
        self.vector_obs = None
        if self.vec_dim:
            self.vector_obs = torch.zeros((N, self.vec_dim), dtype=torch.float32, device=dev)
            _native.check(_native.LIB.mg_bind_vector_obs(h, self.vector_obs.data_ptr()), "mg_bind_vector_obs")
        self.reward = torch.zeros(N, dtype=torch.float32, device=dev)
        self.reward64 = torch.zeros(N, dtype=torch.float64, device=dev)  # the reference's Python float, unrounded
        self.done_u8 = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.gt = torch.zeros((N, max(self.gt_dim, 1)), dtype=torch.float32, device=dev)
        # ground_truth64=True: info["ground_truth"] is the reference's float64 array (endless_mortar_mayhem.py:259,358: 0.6, not
        # float32's 0.60000002), computed by one more small launch per call (include/memgym.h: gt64_dev); default: float32
        self.gt64 = torch.zeros((N, max(self.gt_dim, 1)), dtype=torch.float64, device=dev) if (ground_truth64 and self.gt_dim) else None
        self.ep_reward = torch.zeros(N, dtype=torch.float64, device=dev)
        self.ep_length = torch.zeros(N, dtype=torch.int32, device=dev)
        self.info_names = []
        for k in range(_native.MG_INFO_SLOTS):
            nm = _native.LIB.mg_info_name(h, k)
            if nm is None:
                break
            self.info_names.append(nm.decode())
        self.aux = [torch.zeros(N, dtype=torch.float32, device=dev) for _ in self.info_names]
        self._info = _native.new_struct(_native.InfoBuffers)
        self._err = C.c_int(0)
        self._info.ep_reward_dev = self.ep_reward.data_ptr()
        self._info.ep_length_dev = self.ep_length.data_ptr()
        for k, t in enumerate(self.aux):
            self._info.aux_dev[k] = t.data_ptr()
        self._info.final_obs_dev = ptr(self.final_obs)
        self._info.reward64_dev = self.reward64.data_ptr()
        self._info.gt64_dev = ptr(self.gt64)
        # What happens when ONE instance reaches a capacity of this build (128 path segments, 128 fall-off cells, 512 commands, 16 live
        # spotlights; the reference's lists are unbounded).  The kernels end that instance's episode and raise a sticky error bit either
        # way.  "raise" (default): step() turns the bit into a RuntimeError -- nothing that differs from the reference goes unnoticed.
        # "truncate": step() reports the instance as truncated (`truncated[i]`, info["capacity_exceeded"][i]) and the batch goes on: one
        # instance of 262,144 that outlives a list does not abort a rollout (missing #1).
        if on_capacity not in ("raise", "truncate"):
            raise ValueError("on_capacity must be 'raise' or 'truncate'")
        self.on_capacity = on_capacity
        self.capacity_u8 = torch.zeros(N, dtype=torch.uint8, device=dev) if on_capacity == "truncate" else None
        self._info.capacity_dev = ptr(self.capacity_u8)
        # final_frames=True: the same convention WITHOUT frames (include/memgym.h: mg_info_buffers.final_frames_dev) -- the frame an episode ended on is
        # kept as its frame record, 16 / 64 / 128 bytes, so step(render=False) stays legal; draw_frames(info["final_frames"], pick=...) draws the rows
        self.final_frames = None
        if final_frames:
            self.final_frames = FrameRecords(torch.zeros((N, self.frame_record_bytes), dtype=torch.uint8, device=dev), self.frame_layout())
            self._info.final_frames_dev = self.final_frames.records.data_ptr()
        self._tolerated = self.CAPACITY_BITS if on_capacity == "truncate" else 0
        self.reset_params = process_reset_params(env_id, None)
        self._applied = dict(DEFAULTS[env_id])
        self._set_params = [self._applied]  # what each option set of the handle holds (set 0 = the handle-wide one)
        self._set_of = None                 # int32 [N]: the set instance i runs under, once a masked reset has used other options
        self.max_episode_steps = None
        self.autoreset = autoreset_mode != "disabled"
        # next-step auto-reset: fixed for the handle's life.  The PENDING flags are `done_u8` itself -- the done of the last step() -- which step() hands
        # to mg_step_next as restart_dev and done_dev at once; _clear_pending() zeroes them in every call whose results are defined on the states as they stand
        self._next_step = autoreset_mode == "next_step"
        self._seeded = False  # no instance has an RNG stream before the first reset (or load_state_dict)
        self._swapped = False  # use_obs_buffer() since the last call that wrote every row
        self._stale = False    # step(render=False) / advance(render=False) since the last call that wrote every row: `obs` holds old bytes
        self._copy_snap = None  # copy_instances(): the scratch snapshot, kept from call to call
        self._adv = None       # advance(): the sums' tensors and the mg_advance_out over them, made at the first call
        self._play = None      # play(): the sums' tensors, the mg_advance_out over them and the traces per K, made at the first call
        # `truncation` is always False in the reference; on_capacity="truncate": True where the episode ended on a capacity of this build
        self._truncated = self.capacity_u8.view(torch.bool) if self.capacity_u8 is not None else torch.zeros(N, dtype=torch.bool, device=dev)
        self._n_actions = self.num_envs * self.action_dim
        self._expert_calls = 0  # expert_actions(step=None): the per-handle call counter
        self._p_err = C.byref(self._err)
        self._bind_step()

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        return C.c_void_p(self._raw_stream())

    def _raw_stream(self):
        """torch's CURRENT stream of the handle's device as a raw hipStream_t (it is looked up at every call: the caller may be inside
        `with torch.cuda.stream(...)`)."""
        try:
            return torch._C._cuda_getCurrentRawStream(self.device.index)  # (~0.2 us; the public accessor builds a Stream object: ~2 us)
        except AttributeError:
            return torch.cuda.current_stream(self.device).cuda_stream

    def _bind_step(self):
        """The arguments of mg_step that do not change from call to call, resolved once (pointers of the output tensors, the info
        dictionary): at a few thousand instances a step lasts 20-30 us on the GPU and the host side of step() was as long
        (round 5).  use_obs_buffer / use_step_buffers call it again."""
        self._p_reward = self.reward.data_ptr()
        self._p_done = self.done_u8.data_ptr()
        self._p_gt = self.gt.data_ptr() if self.gt_dim else None
        self._p_info = C.byref(self._info)
        self._done_bool = self.done_u8.view(torch.bool)
        info = {"done_mask": self._done_bool, "reward": self.ep_reward, "length": self.ep_length}
        for nm, t in zip(self.info_names, self.aux):
            info[nm] = t
        if self.gt_dim:
            info["ground_truth"] = self.gt if self.gt64 is None else self.gt64
        if self.capacity_u8 is not None:
            info["capacity_exceeded"] = self._truncated
        self._info_dict = info

    def _write_set(self, set_id, params):
        """Bring option set `set_id` of the handle to `params` (only the keys that differ from what it holds are sent)."""
        have = self._set_params[set_id]
        for k, v in params.items():
            if k in have and have[k] == v:
                continue
            vals = [float(x) for x in v] if isinstance(v, (list, tuple, np.ndarray)) else [float(v)]
            arr = (C.c_double * len(vals))(*vals)
            if set_id == 0:
                rc = _native.LIB.mg_set_option(self._h, k.encode(), arr, len(vals))
            else:
                rc = _native.LIB.mg_set_option_set(self._h, set_id, k.encode(), arr, len(vals))
            if rc == -2:
                raise AssertionError("Provided reset parameter (" + str(k) + ") is not valid. Check spelling.")
            if rc == -4:
                raise AssertionError(_native.last_error())
            if rc != 0:
                raise NotImplementedError("reset parameter %s=%r%s: %s" % (k, v, "" if set_id == 0 else " for a subset of the instances", _native.last_error()))
            have[k] = v

    def _apply_options_masked(self, options, mask):
        """reset(options=..., mask=...): like the reference's reset(seed, options) of ONE instance (mortar_mayhem_grid.py:213-236),
        the options belong to the instances that are being reset and to nobody else.  The handle keeps up to
        MG_MAX_OPTION_SETS parameter sets (include/memgym.h: mg_set_option_set); the masked instances are moved to the set that
        holds these options (a free one is filled if none does).  options=None keeps every masked instance under the options it
        has (a masked reset is this library's extension -- the re-start of finished instances; it is reset(mask=None, options=None)
        that means "the defaults for everybody", like the reference's)."""
        if options is None:
            return
        params = process_reset_params(self.env_id, options)
        k = next((j for j, p in enumerate(self._set_params) if p == params), None)
        if k == 0 and self._set_of is None:
            return  # everybody runs under these options already
        if k is None:
            used = set([0])
            if self._set_of is not None:
                used |= set(torch.unique(self._set_of).cpu().tolist())  # (synchronises: only when a new set is needed)
            free = [j for j in range(1, _native.MG_MAX_OPTION_SETS) if j not in used]
            if not free:
                raise NotImplementedError("more than %d different option sets alive in one handle" % _native.MG_MAX_OPTION_SETS)
            k = free[0]
            self._room_for_set(k)
            # EVERY key is sent (an empty `have`): the library then checks each geometry key against the handle's geometry and
            # refuses a set whose agent_scale / arena_size / ... differs from it -- also when the value asked for is the
            # reference's default and the handle's is not (diffing against the defaults sent nothing in that case and
            # the instances silently ran under the handle's geometry)
            self._set_params[k] = {}
            try:
                self._write_set(k, params)
            except Exception:
                self._set_params[k] = {}  # half-written: never matched by a later reset, rewritten in full when it is reused
                raise
        if self._set_of is None:
            self._bind_set_index(True)
        self._set_of[mask.to(device=self.device, dtype=torch.bool)] = k

    def _room_for_set(self, k):
        """`_set_params` reaches option set k: the slots it lacks are empty sets"""
        while len(self._set_params) <= k:
            self._set_params.append({})

    def _bind_set_index(self, on):
        """The per-instance option-set index `_set_of` (include/memgym.h: mg_bind_option_sets): on -- a new one, everybody under set 0, is bound;
        off -- it is unbound and forgotten, the handle is back in its one-set launch arrangement."""
        if on:
            self._set_of = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        _native.check(_native.LIB.mg_bind_option_sets(self._h, self._set_of.data_ptr() if on else None), "mg_bind_option_sets")
        if not on:
            self._set_of = None

    def _apply_options(self, options):
        params = process_reset_params(self.env_id, options)
        self._write_set(0, params)
        if self._set_of is not None:
            # a reset of every instance: all of them run under these options.  The per-instance index is unbound again, so the
            # handle is back in its one-set launch arrangement (one-launch mortar step, fused resets, lazy segments), and the other
            # sets are forgotten: their geometry entries may be stale now, a later masked reset writes the set it needs in full.
            self._bind_set_index(False)
        del self._set_params[1:]
        self.reset_params = params
        if self.env_id in ("MortarMayhemB-Grid-v0", "MortarMayhemB-v0"):  # mortar_mayhem_b_grid.py:149-153
            self.max_episode_steps = calc_max_episode_steps(
                max(params["command_count"]), 0, 0, max(params["explosion_delay"]), max(params["explosion_duration"]))
        elif self.env_id in ("MortarMayhem-Grid-v0", "MortarMayhem-v0"):
            self.max_episode_steps = calc_max_episode_steps(
                max(params["command_count"]), max(params["command_show_duration"]), max(params["command_show_delay"]),
                max(params["explosion_delay"]), max(params["explosion_duration"]))
        else:
            self.max_episode_steps = params.get("max_steps", None)

    def _seed_tensor(self, seed):
        if seed is None:
            if self._seeded:
                return None
            # first reset without a seed: like gymnasium's np_random(None), every instance starts from OS entropy
            seed = np.random.SeedSequence().generate_state(self.num_envs, np.uint64) >> np.uint64(1)
            seed = seed.astype(np.int64)
        if isinstance(seed, torch.Tensor):
            s = seed.to(device=self.device, dtype=torch.int64)
        elif np.isscalar(seed):
            # one integer seeds instance i with seed + i (instance 0 == the reference's reset(seed=seed))
            s = torch.arange(self.num_envs, device=self.device, dtype=torch.int64) + int(seed)
        else:
            s = torch.as_tensor(np.asarray(seed, dtype=np.int64), device=self.device)
        assert s.numel() == self.num_envs
        return s.contiguous()

    # ------------------------------------------------------------------ API
    def reset(self, seed=None, return_info=True, options=None, mask=None):
        """Env.reset(seed, options) for all instances, or for those selected by the bool/uint8 tensor `mask`: the options then belong
        to those instances only (per-instance option sets, include/memgym.h: mg_set_option_set); mask with options=None re-starts
        them under the options each of them has.  `reset_params` and `max_episode_steps` describe the options of the latest FULL
        reset (option set 0); a masked reset with options does not change them."""
        with torch.cuda.device(self.device):
            if mask is not None and seed is None and not self._seeded:  # (checked before any option state changes)
                raise RuntimeError("a masked reset(seed=None) needs an earlier full reset: the other instances have no RNG stream yet")
            if mask is None:
                self._apply_options(options)
            else:
                self._apply_options_masked(options, mask)
            s = self._seed_tensor(seed)
            m = None if mask is None else mask.to(device=self.device, dtype=torch.uint8).contiguous()
            if m is not None and (self._swapped or self._stale):
                # a masked reset writes the rows of the masked instances only; after use_obs_buffer() the other rows of the new
                # buffer hold whatever was there, and after headless steps (render=False) frames of long ago: draw every instance's
                # CURRENT frame into it first (one raster launch, these sequences only).  (Rows a masked reset had left untouched
                # right before the swap stay as they are: mg_render.)
                _native.check(_native.LIB.mg_render(self._h, self.obs.data_ptr(), self._stream()), "mg_render")
            self._swapped = self._stale = False
            self._clear_pending()
            _native.check(_native.LIB.mg_reset(self._h, ptr(s), ptr(m), self.obs.data_ptr(), self._p_gt, self._stream()), "mg_reset")
            self._refresh_gt64()
            self._seeded = True
        info = {"ground_truth": self.gt if self.gt64 is None else self.gt64} if self.gt_dim else {}
        return self._obs(), info

    def step(self, actions, render=True, mask=None):
        """Env.step for every instance.  render=False is the HEADLESS step (include/memgym.h: mg_step with obs_dev == NULL): everything but
        the frames -- state, random streams, rewards, dones, infos -- is what the drawn step gives, the first element of the returned tuple
        is None and `obs` keeps its old bytes until redraw(), the next drawn step or a reset.  Terminal observations are frames: a handle
        made with final_observation=True refuses render=False (ValueError) before anything is stepped.  A handle made with final_frames=True keeps
        the frame an episode ended on as a frame RECORD instead (include/memgym.h: mg_info_buffers.final_frames_dev) and steps headless like any other:
        with auto-reset on, info["final_frames"] is `final_frames` (a FrameRecords [N, frame_record_bytes]), its rows valid where info["done_mask"] is
        set -- draw_frames(info["final_frames"], pick=idx, obs_format=...) draws them, in any format, whenever training wants them.
        mask: step a SUBSET (include/memgym.h: mg_step_masked) -- a bool or uint8 tensor [N] on the device, or anything torch.as_tensor
        takes; instance i steps iff mask[i] != 0, and its results are those of a handle in which it alone had been stepped by step() with
        the same actions in the same order.  The other instances are left alone: state, random stream and their row of `obs`, of the
        ground truth and of final_observation stay; the action entries of inactive instances are not interpreted.  The return values keep
        their shapes: `reward` is 0 and info["done_mask"] False for inactive instances, the OTHER info rows of inactive instances (the
        episode record "reward" / "length", the named aux infos, "capacity_exceeded" aside, which is False) keep their previous contents.
        A mask of the wrong length raises ValueError before anything is stepped; mask=None is the ordinary step.  render=False with a
        mask is the masked headless step.  Evaluation of one episode per seed: `finished |= done` and step(a, mask=~finished) until all
        are finished (examples/evaluate_seeds.py).
        autoreset_mode="next_step" (include/memgym.h: mg_step_next; gymnasium >= 1.0's default): the step that ends an episode returns the TERMINAL
        observation as its ordinary observation -- bootstrap from `obs` where `done` -- and the following step() ignores that instance's action and
        returns the first observation of the new episode with reward 0 and done False.  The pending flags are the done of the handle's last step();
        reset(), advance(), advance_traced(), play(), load_instances(), copy_instances() and load_state_dict() clear them.  info["done_mask"] and the
        episode-record rows are valid where done; there is no "final_observation" / "final_frames" key.  mask=... and render=False are refused
        (ValueError) before anything is stepped."""
        if self._next_step and (mask is not None or not render):
            raise ValueError("step(%s) on a handle with autoreset_mode='next_step': the mode has neither a masked nor a headless form"
                             % ("mask=..." if mask is not None else "render=False"))
        if not render and self.final_obs is not None:
            raise ValueError("step(render=False) on a handle with final_observation=True: terminal observations are frames")
        m = None
        if mask is not None:
            m = self._mask_u8("step", mask)
        a = actions
        if not (isinstance(a, torch.Tensor) and a.dtype == torch.int32 and a.device == self.device and a.is_contiguous()):
            a = self._to_actions(a)
        assert a.numel() == self._n_actions, "actions must have shape [N] or [N, 2]"
        if torch.cuda.current_device() != self.device.index:
            with torch.cuda.device(self.device):
                self._launch_step(a, render, m)
        else:
            self._launch_step(a, render, m)
        if render:
            self._swapped = self._stale = False  # a drawn step writes every row (a masked one: has drawn every row first where one was old)
        else:
            self._stale = True
        _native.LIB.mg_peek_errors(self._h, self._p_err)  # host-mapped word: no synchronisation
        if self._err.value & ~self._tolerated:
            self.check_errors()
        info = dict(self._info_dict)
        if self.final_obs is not None and self.autoreset:  # rows valid where done_mask is set
            info["final_observation"] = self.final_obs
        if self.final_frames is not None:
            self.final_frames.layout = self.frame_layout()  # (the rows written by this call are records of the handle as it is now)
            if self.autoreset:  # rows valid where done_mask is set
                info["final_frames"] = self.final_frames
        return (self._obs() if render else None), self.reward, self._done_bool, self._truncated, info

    def _clear_pending(self):
        """autoreset_mode="next_step": no instance is restarted by the next step()."""
        if self._next_step:
            self.done_u8.zero_()

    def _mask_u8(self, what, mask):
        """The mask of step(mask=...) / play(mask=...) -> a contiguous uint8 tensor [N] on the handle's device; ValueError for another shape."""
        m = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(mask)
        if m.numel() != self.num_envs or m.dim() != 1:
            raise ValueError("%s(mask=...): the mask must have shape [%d], got %s" % (what, self.num_envs, tuple(m.shape)))
        if m.dtype == torch.bool and m.device == self.device and m.is_contiguous():
            return m.view(torch.uint8)  # (the same bytes: True is 1)
        if not (m.dtype == torch.uint8 and m.device == self.device and m.is_contiguous()):
            m = (m != 0).to(device=self.device, dtype=torch.uint8).contiguous()
        return m

    def _to_actions(self, a):
        """actions that are not yet a contiguous int32 tensor on the handle's device (step() and play() ask that themselves) -> one"""
        a = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
        return a.to(device=self.device, dtype=torch.int32).contiguous()

    def _refresh_gt64(self):
        """ground_truth64=True: the float64 ground truth follows the states as they stand (one small launch)"""
        if self.gt64 is not None:
            _native.check(_native.LIB.mg_ground_truth64(self._h, self.gt64.data_ptr(), self._stream()), "mg_ground_truth64")

    def _after_steps(self):
        """The end of advance() / play(): `obs` is stale, and a device error bit raised so far is reported (step() does the same look inline)."""
        self._stale = True
        _native.LIB.mg_peek_errors(self._h, self._p_err)  # host-mapped word: no synchronisation
        if self._err.value & ~self._tolerated:
            self.check_errors()

    def _teacher_args(self, eps, seed, step):
        """(eps, seed, step) as the library takes them: a double and two 64-bit words; step=None is the handle's call counter"""
        mask = (1 << 64) - 1
        return float(eps), int(seed) & mask, int(self._expert_calls if step is None else step) & mask

    @property
    def autoreset_mode(self):
        return "next_step" if self._next_step else ("same_step" if self.autoreset else "disabled")

    def _launch_step(self, a, render=True, m=None):
        if self._next_step:  # restart_dev IS done_dev: each instance's flag is read before its done is written
            rc = _native.LIB.mg_step_next(self._h, a.data_ptr(), self._p_done, self.obs.data_ptr(), self._p_reward, self._p_done, self._p_gt, self._p_info,
                                          self._raw_stream())
            if rc != 0:
                _native.check(rc, "mg_step_next")
            return
        if m is not None:
            if render and (self._swapped or self._stale):
                # a drawn masked step writes the rows of the active instances only: after use_obs_buffer() or headless steps the other rows
                # hold old bytes -- draw every instance's CURRENT frame first, as the masked reset() does (one raster launch, these sequences only)
                _native.check(_native.LIB.mg_render(self._h, self.obs.data_ptr(), self._raw_stream()), "mg_render")
            rc = _native.LIB.mg_step_masked(self._h, a.data_ptr(), m.data_ptr(), self.obs.data_ptr() if render else None, self._p_reward, self._p_done,
                                            self._p_gt, self._p_info, 1 if self.autoreset else 0, self._raw_stream())
            if rc != 0:
                _native.check(rc, "mg_step_masked")
            return
        rc = _native.LIB.mg_step(self._h, a.data_ptr(), self.obs.data_ptr() if render else None, self._p_reward, self._p_done, self._p_gt, self._p_info,
                                 1 if self.autoreset else 0, self._raw_stream())
        if rc != 0:
            _native.check(rc, "mg_step")

    def redraw(self):
        """Draw every instance's CURRENT frame into `obs` (include/memgym.h: mg_render) -- after headless steps exactly the frame the
        last step would have drawn, the first frame of the new episode where that step auto-reset the instance.  Returns what reset()
        returns as observation.  One raster launch on the current stream; no state changes."""
        with torch.cuda.device(self.device):
            _native.check(_native.LIB.mg_render(self._h, self.obs.data_ptr(), self._stream()), "mg_render")
        self._swapped = self._stale = False
        return self._obs()

    def new_rollout(self, steps, labels=False):
        """A RolloutTrace for `steps` steps of this handle (zeros; frames [steps + 1, N, frame_record_bytes]) to pass to advance_traced() /
        play(trace=...), as often as you like.  labels=True adds the tensor for the teacher's answers (advance only)."""
        K, N, dev = int(steps), self.num_envs, self.device
        if K < 1:
            raise ValueError("new_rollout: steps must be >= 1, got %d" % K)
        acts = (K, N) if self.action_dim == 1 else (K, N, 2)
        return RolloutTrace(torch.zeros((K + 1, N, self.frame_record_bytes), dtype=torch.uint8, device=dev), 0,
                            torch.zeros(acts, dtype=torch.int32, device=dev), torch.zeros(acts, dtype=torch.int32, device=dev) if labels else None,
                            torch.zeros((K, N), dtype=torch.float32, device=dev), torch.zeros((K, N), dtype=torch.bool, device=dev))

    def _trace_rows(self, ro, teacher):
        """frames[0] <- the current frames (save_frames); -> the mg_rollout_trace over frames[1:] and the other tensors of a checked RolloutTrace"""
        rows = _native.new_struct(_native.RolloutTraceRows)
        if ro.frames is not None:
            self.save_frames(out=ro.frames[0])
            ro.frame_layout = self.frame_layout()
            rows.frames_dev = ro.frames[1:].data_ptr()
        rows.reward_dev, rows.done_dev = ptr(ro.reward), ptr(ro.done)
        if teacher:
            rows.actions_dev, rows.labels_dev = ptr(ro.actions), ptr(ro.labels)
        return rows

    def advance(self, steps, eps=0.0, seed=0, step=None, render=True, stats=True):
        """`steps` steps under the scripted teacher without a frame (include/memgym.h: mg_advance): state, random streams and error
        bits afterwards are those after `for t: step(expert_actions(eps, seed, step + t), render=False)` with auto-reset, whatever
        `autoreset` says.  eps = 0 is the teacher, eps = 1 the uniformly random policy.  Uses: the warm-up behind reset(seed=...) that takes
        the episodes out of phase; the teacher's return and success rate per curriculum setting; a check that an option set is solvable.
        -> (obs or None, stats).  render=True draws the frames the last step left (redraw()); render=False leaves `obs` stale.
        stats (None with stats=False): a dict of [N] tensors over THIS call's steps, overwritten by the next call -- "reward" (float64,
        the step rewards added in step order), "episodes" (int32, episodes that ended), "episode_reward" (float64) / "episode_length" (int64):
        sums of info["reward"] / info["length"] over those episodes, and one float64 sum per entry of `info_names` (e.g. "success").
        step=None continues the call numbering of expert_actions() and advances it by `steps`.  Episodes that end inside the call are
        counted, not shown: there are no terminal observations here, on any handle.  Nothing synchronises; the handle's first call
        allocates scratch, every later one is capturable (the arguments are then the captured values).  The five Mortar Mayhem ids
        run the whole loop inside one launch per 1,024 steps; the other five take it launch by launch.
        advance_traced() is this call keeping every step in a RolloutTrace."""
        return self._advance(int(steps), eps, seed, step, render, stats, None)

    def advance_traced(self, trace, eps=0.0, seed=0, step=None, render=True, stats=True):
        """advance(trace.steps, ...) that KEEPS the rollout in `trace`, a RolloutTrace (new_rollout) (include/memgym.h: mg_advance_traced): trace.frames[0]
        the frames before the call, and per step t the action played (actions[t]), the teacher's answer at eps = 0 where the trace has labels (labels[t]),
        reward[t], done[t] and the frame record after the step (frames[t + 1]); trace.draw() draws any pick of them later.  State, streams, stats and
        the return value are those of advance() with the same arguments.  A trace of the wrong N / dtype / device / alignment raises ValueError
        before anything is launched.  (A method of its own: advance()'s parameter list is kept as it is.)"""
        self._require_started("advance_traced")
        if not isinstance(trace, RolloutTrace):
            raise ValueError("advance_traced: need the RolloutTrace new_rollout returned")
        try:
            steps = trace.steps
        except (AttributeError, IndexError, StopIteration):
            raise ValueError("advance_traced: the trace's tensors do not say how many steps it holds") from None
        check_rollout_trace(trace, steps, self.num_envs, self.action_dim, self.frame_record_bytes, True, self.device)
        return self._advance(steps, eps, seed, step, render, stats, trace)

    def _advance(self, steps, eps, seed, step, render, stats, trace):
        if self._adv is None and stats:
            self._adv = self._sum_tensors()
        args = self._teacher_args(eps, seed, step)
        out = C.byref(self._adv[1]) if stats else None
        with torch.cuda.device(self.device):
            self._clear_pending()
            if trace is not None:
                rows = self._trace_rows(trace, True)
                _native.check(_native.LIB.mg_advance_traced(self._h, steps, *args, self._p_gt, out, C.byref(rows), self._stream()), "mg_advance_traced")
            else:
                _native.check(_native.LIB.mg_advance(self._h, steps, *args, self._p_gt, out, self._stream()), "mg_advance")
            self._refresh_gt64()
        if step is None:
            self._expert_calls += steps
        self._after_steps()
        return (self.redraw() if render else None), (dict(self._adv[0]) if stats else None)

    def _sum_tensors(self):
        """the [N] tensors of advance()'s / play()'s stats and the mg_advance_out over them"""
        N, dev = self.num_envs, self.device
        t = {"reward": torch.zeros(N, dtype=torch.float64, device=dev), "episodes": torch.zeros(N, dtype=torch.int32, device=dev),
             "episode_reward": torch.zeros(N, dtype=torch.float64, device=dev), "episode_length": torch.zeros(N, dtype=torch.int64, device=dev)}
        out = _native.new_struct(_native.AdvanceOut)
        out.reward_sum_dev, out.episodes_dev = t["reward"].data_ptr(), t["episodes"].data_ptr()
        out.ep_reward_sum_dev, out.ep_length_sum_dev = t["episode_reward"].data_ptr(), t["episode_length"].data_ptr()
        for k, nm in enumerate(self.info_names):
            t[nm] = torch.zeros(N, dtype=torch.float64, device=dev)
            out.aux_sum_dev[k] = t[nm].data_ptr()
        return t, out

    def play(self, actions, until_done=False, mask=None, render=True, stats=True, trace=False):
        """K steps of YOUR OWN action sequences without a frame (include/memgym.h: mg_play) -- what advance() is for the scripted teacher: random
        shooting from a saved state (save_instances / load_instances), replaying demonstrations, counterfactual probes, stored tapes of one episode
        per seed.  actions: anything torch.as_tensor takes, of shape [K, N] (Discrete ids) or [K, N, 2] (MultiDiscrete ids); row t is what step()
        takes at step t.  A wrong shape raises ValueError before anything is stepped.
        until_done=False: state, random streams and error bits afterwards are those after `for t: step(actions[t], render=False)` with auto-reset,
        whatever `autoreset` says.  until_done=True: every instance plays until ITS episode ends, is then left alone and is NOT reset -- the loop
        `step(actions[t], render=False, mask=alive); alive &= ~done` of a handle with autoreset = False; a finished instance stays in its terminal
        state (redraw() shows its terminal frame) until you reset it (reset(mask=...)) or load a record into it.
        mask: as in step(mask=...), the instances that play at all; the others keep state, stream and frame.
        -> (obs or None, stats).  render=True draws the frame each instance's last step left (redraw()); render=False leaves `obs` stale.
        stats: the keys of advance() over THIS call's steps plus "steps" (int32 [N]: the steps each instance took); trace=True adds
        "reward_trace" (float32 [K, N]) and "done_trace" (bool [K, N]), zero where an instance did not step.  The tensors are kept per handle
        (the traces per K) and overwritten by the next call; stats=False, trace=False returns None in their place.  Nothing synchronises; the
        handle's first call allocates scratch and is refused inside a capture (call it once eagerly, with the K and the trace setting the capture
        will use, so that the stats tensors exist too); every later one is capturable (tape and mask are read at replay).  The five Mortar Mayhem ids run
        the whole loop inside one launch per 1,024 steps; the other five take it launch by launch.
        trace=<a RolloutTrace of K steps> (new_rollout) KEEPS the rollout instead (include/memgym.h: mg_play_traced): trace.frames[0] the frames before
        the call, and per step t trace.reward[t], trace.done[t] and the frame record after the step, trace.frames[t + 1] -- for an instance that did
        not step (paused by `mask`, or finished under until_done) the record of the frame it keeps, reward 0, done False.  trace.actions is not written:
        the tape is yours.  stats then holds the sums and "steps" alone.  A trace of the wrong K / N / dtype / device / alignment raises ValueError before
        anything is launched."""
        a = actions
        if not (isinstance(a, torch.Tensor) and a.dtype == torch.int32 and a.device == self.device and a.is_contiguous()):
            a = self._to_actions(a)
        want = (self.num_envs,) if self.action_dim == 1 else (self.num_envs, 2)
        if a.dim() != len(want) + 1 or tuple(a.shape[1:]) != want or a.shape[0] < 1:
            raise ValueError("play(actions): the tape must have shape [K, %s] with K >= 1, got %s" % (", ".join(str(x) for x in want), tuple(a.shape)))
        K = int(a.shape[0])
        m = None if mask is None else self._mask_u8("play", mask)
        ro = trace if not isinstance(trace, bool) and trace is not None else None
        if ro is not None:
            self._require_started("play(trace=...)")
            check_rollout_trace(ro, K, self.num_envs, self.action_dim, self.frame_record_bytes, False, self.device)
            trace = False
        if self._play is None:
            t, out = self._sum_tensors()
            t["steps"] = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
            self._play = (t, out, {})
        sums, out, traces = self._play
        if trace and K not in traces:
            traces[K] = (torch.zeros((K, self.num_envs), dtype=torch.float32, device=self.device),
                         torch.zeros((K, self.num_envs), dtype=torch.uint8, device=self.device))
        rt, dt = traces[K] if trace else (None, None)
        mode = _native.MG_PLAY_EPISODE if until_done else _native.MG_PLAY_THROUGH
        steps_dev, out = (sums["steps"].data_ptr(), C.byref(out)) if stats else (None, None)
        with torch.cuda.device(self.device):
            self._clear_pending()
            if ro is not None:
                rows = self._trace_rows(ro, False)
                _native.check(_native.LIB.mg_play_traced(self._h, a.data_ptr(), K, mode, ptr(m), steps_dev, self._p_gt, out, C.byref(rows), self._stream()),
                              "mg_play_traced")
            else:
                _native.check(_native.LIB.mg_play(self._h, a.data_ptr(), K, mode, ptr(m), ptr(rt), ptr(dt), steps_dev, self._p_gt, out, self._stream()), "mg_play")
            self._refresh_gt64()
        self._after_steps()
        st = dict(sums) if stats else ({} if trace else None)
        if trace:
            st["reward_trace"], st["done_trace"] = rt, dt.view(torch.bool)
        return (self.redraw() if render else None), st

    def expert_actions(self, eps=0.0, seed=0, step=None, out=None):
        """The scripted teacher (include/memgym.h: mg_expert_actions): for every instance the action the CPU oracle's expert hook gives
        in its CURRENT state -- after the last reset() / step(), the new episode's state where that step auto-reset the instance -- as an
        int32 tensor [N] (Discrete ids) or [N, 2] (MultiDiscrete ids) that step() takes as it is.  With probability `eps` an instance gets
        a uniformly random action instead: a counter-based hash of (seed, step, instance), the oracle's mgo_batch_expert, so equal
        arguments give equal actions.  step=None numbers the calls of this handle 0, 1, 2, ...  `out`: a contiguous int32 tensor of that
        shape on the handle's device to write into.  One small launch on the current stream: nothing synchronises, no state changes, no
        instance's random stream moves.  Uses: demonstrations for behaviour cloning, DAgger labels (query it in the states the LEARNER
        reaches), an upper bound on return per curriculum setting, a check that an option set is solvable."""
        shape = (self.num_envs,) if self.action_dim == 1 else (self.num_envs, 2)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=self.device)
        elif not (isinstance(out, torch.Tensor) and out.dtype == torch.int32 and out.device == self.device and out.is_contiguous() and tuple(out.shape) == shape):
            raise ValueError("expert_actions: out must be a contiguous int32 tensor of shape %s on %s" % (shape, self.device))
        with torch.cuda.device(self.device):
            _native.check(_native.LIB.mg_expert_actions(self._h, *self._teacher_args(eps, seed, step), out.data_ptr(), self._stream()), "mg_expert_actions")
        self._expert_calls += 1
        return out

    # ------------------------------------------------------------------ instance records
    @property
    def instance_bytes(self):
        return int(_native.LIB.mg_instance_bytes(self._h))

    @property
    def instance_layout(self):
        return int(_native.LIB.mg_instance_layout(self._h))

    def _require_started(self, what):
        if not self._seeded:
            raise ValueError("%s: before the first reset (or load_state_dict)" % what)

    def save_instances(self, idx=None, out=None):
        """Save single instances to device memory (include/memgym.h: mg_save_instances) -> InstanceSnapshot.  idx: the instances, an integer
        tensor / list (None: all, in order); entries < 0 are skipped (their records keep their bytes).  out: a snapshot of the same number of
        records to write into (its tensors are reused, nothing is allocated with one option set).  One small launch on the current stream;
        nothing synchronises and nothing observable changes on any instance."""
        self._require_started("save_instances")
        nbytes = self.instance_bytes
        idx, k = check_instance_save(nbytes, self.num_envs, idx, out, self.device)
        records = out.records if out is not None else torch.empty((k, nbytes), dtype=torch.uint8, device=self.device)
        aligned_on("save_instances", "out.records", self.device, records)
        with torch.cuda.device(self.device):
            _native.check(_native.LIB.mg_save_instances(self._h, ptr(idx), k, records.data_ptr(), self._stream()), "mg_save_instances")
            set_of = None
            if self._set_of is not None:  # the caller owns the set index (include/memgym.h): it travels beside the records
                set_of = self._set_of.clone() if idx is None else self._set_of[idx.clamp(0, self.num_envs - 1).long()]
        if out is not None:
            out.layout, out.set_of = self.instance_layout, set_of
            return out
        return InstanceSnapshot(records, self.instance_layout, set_of)

    def _scatter_rows(self, dst, tgt, rows):
        """dst[tgt[j]] = rows[j]; tgt[j] == len(dst) names nobody (a skipped entry).  No host look."""
        ext = torch.cat([dst, dst[:1]])
        ext.index_copy_(0, tgt, rows.to(dst.dtype))
        dst.copy_(ext[:dst.shape[0]])

    def load_instances(self, snap, idx=None, rec=None, render=True):
        """Load records of `snap` into instances (include/memgym.h: mg_load_instances): instance idx[j] <- record rec[j] (rec=None: record j;
        idx=None: instance j).  From then on instance idx[j] gives, for the same actions, bit for bit what the saved instance gave from the moment
        of the save; every other instance keeps everything.  Entries idx[j] < 0 are skipped; the instances named must be distinct; one record may go
        to many instances.  render=True returns `obs` like redraw(): the loaded instances' rows are drawn -- and, where `obs` was stale
        (render=False steps, use_obs_buffer()), everybody's, so `obs` never holds a mixture.  render=False draws nothing, marks `obs` stale and
        returns None (refused on a final_observation handle, like step(render=False)).  The option-set indices saved with the records are copied
        into the handle's binding, the loaded rows of the ground truth are refreshed, `final_observation` rows are left alone.  ValueError,
        before anything is enqueued: a snapshot of another handle or of an earlier geometry, records of the wrong width, index tensors of the
        wrong dtype or length.  Launches only; nothing synchronises."""
        self._require_started("load_instances")
        if not render and self.final_obs is not None:
            raise ValueError("load_instances(render=False) on a handle with final_observation=True: terminal observations are frames")
        N = self.num_envs
        idx, rec = check_instance_load(snap, self.instance_layout, self.instance_bytes, N, idx, rec, self.device)
        aligned_on("load_instances", "snapshot.records", self.device, snap.records)
        if snap.set_of is not None and self._set_of is None:
            raise ValueError("load_instances: the snapshot was taken under per-instance option sets, which a full reset has dropped since")
        k = snap.count
        m = N if idx is None else idx.numel()
        draw_all = render and (self._swapped or self._stale)
        obs_ptr = self.obs.data_ptr() if (render and not draw_all) else None
        with torch.cuda.device(self.device):
            # The C call takes ONE count for its entries and its records (rec_of_dev[j] in 0 .. count-1): the entries are dealt out in calls of
            # exactly k, padded with idx = -1, so that any record of the snapshot can be named and none beyond it
            if m == k:
                calls = [(idx, rec)]
            else:
                total = (m + k - 1) // k * k
                pi = torch.full((total,), -1, dtype=torch.int32, device=self.device)
                pi[:m] = torch.arange(m, dtype=torch.int32, device=self.device) if idx is None else idx
                pr = torch.zeros(total, dtype=torch.int32, device=self.device)
                pr[:m] = torch.arange(m, dtype=torch.int32, device=self.device) if rec is None else rec
                calls = [(pi[c:c + k], pr[c:c + k]) for c in range(0, total, k)]
            self._clear_pending()
            for ci, cr in calls:
                _native.check(_native.LIB.mg_load_instances(self._h, ptr(ci), ptr(cr), k, snap.records.data_ptr(), obs_ptr, self._stream()), "mg_load_instances")
            # what the handle keeps beside the state: the set index (the caller's, include/memgym.h) and the ground truth rows
            whole = idx is None and rec is None  # instance j <- record j for every j
            tgt = src = None
            if not whole and (self._set_of is not None or self.gt_dim):
                i64 = (torch.arange(m, device=self.device) if idx is None else idx.long())
                src = (torch.arange(m, device=self.device) if rec is None else rec.long())
                ok = (i64 >= 0) & (i64 < N) & (src >= 0) & (src < k)
                tgt = torch.where(ok, i64, torch.full_like(i64, N))
                src = src.clamp(0, k - 1)
            if self._set_of is not None:
                sets = snap.set_of if snap.set_of is not None else torch.zeros(k, dtype=torch.int32, device=self.device)
                if whole:
                    self._set_of.copy_(sets)
                else:
                    self._scatter_rows(self._set_of, tgt, sets[src])
            if self.gt_dim:
                g = torch.empty((N, self.gt_dim), dtype=torch.float64, device=self.device)
                _native.check(_native.LIB.mg_ground_truth64(self._h, g.data_ptr(), self._stream()), "mg_ground_truth64")
                for dst in (self.gt, self.gt64):
                    if dst is None:
                        continue
                    if whole:
                        dst.copy_(g.to(dst.dtype))
                    else:
                        self._scatter_rows(dst, tgt, g[tgt.clamp(0, N - 1)])
        if not render:  # (an index out of range raises bit 512, sticky: the next step() / check_errors() reports it)
            self._stale = True
            return None
        if draw_all:
            return self.redraw()
        return self._obs()

    def copy_instances(self, src, dst, render=True):
        """Instance dst[j] <- instance src[j] inside the handle: a save followed by a load through a scratch snapshot the handle keeps, so `src` and
        `dst` may overlap (a permutation in place).  Returns what load_instances returns."""
        self._require_started("copy_instances")
        src = index_tensor("copy_instances", "src", src, self.device)
        dst = index_tensor("copy_instances", "dst", dst, self.device)
        if src.numel() != dst.numel():
            raise ValueError("copy_instances: src and dst must have the same length, got %d and %d" % (src.numel(), dst.numel()))
        if src.numel() == 0:
            return self._obs() if render else None
        s = self._copy_snap
        if s is None or tuple(s.records.shape) != (src.numel(), self.instance_bytes):
            s = None
        self._copy_snap = self.save_instances(src, out=s)
        return self.load_instances(self._copy_snap, idx=dst, render=render)

    def new_obs_buffer(self):
        """A second observation buffer like `obs` (same shape, dtype, device and -- if `obs` came from mg_obs_alloc -- the same
        zone-balanced placement), for consumers that double-buffer (use_obs_buffer)."""
        if self.obs_placement_info is not None:
            try:
                t, _ = alloc_obs_buffer(tuple(self.obs.shape), self.obs.dtype, self.device)
                return t
            except RuntimeError:
                pass
        return torch.empty_like(self.obs)

    def use_obs_buffer(self, tensor):
        """Make `tensor` (same shape / dtype / device as `obs`) the buffer the NEXT reset / step writes its observations to
        (mg_step takes the buffer per call).  A consumer that still reads the previous buffer -- e.g. a gather to another
        rank running beside the next step (memory_gym_amd.dist.ObsGatherer) -- alternates between two buffers this way.
        A step() or a full reset() writes every row of the new buffer; a MASKED reset right after a swap first draws the
        current frame of every instance into it (the rows it does not reset would otherwise be stale)."""
        if tuple(tensor.shape) != tuple(self.obs.shape) or tensor.dtype != self.obs.dtype or tensor.device != self.obs.device or not tensor.is_contiguous():
            raise ValueError("use_obs_buffer: need a contiguous tensor like env.obs")
        self.obs = tensor
        self._swapped = True
        self._bind_step()

    def use_step_buffers(self, reward, done_u8):
        """Make `reward` (float32 [N]) and `done_u8` (uint8 [N]) the tensors the NEXT step stores its rewards / dones into (mg_step
        takes both per call) -- e.g. two views of one packed buffer that is shipped to another rank with the frames
        (memory_gym_amd.dist.ObsGatherer: BASELINE config 5's "obs (+reward, done)")."""
        for t, dt in ((reward, torch.float32), (done_u8, torch.uint8)):
            if tuple(t.shape) != (self.num_envs,) or t.dtype != dt or t.device != self.device or not t.is_contiguous():
                raise ValueError("use_step_buffers: need contiguous float32 [N] / uint8 [N] tensors on the handle's device")
        if reward.data_ptr() % 4:
            raise ValueError("use_step_buffers: the reward tensor must be 4-byte aligned")
        if self._next_step:  # (the done tensor holds the pending flags: they move with it)
            done_u8.copy_(self.done_u8)
        self.reward, self.done_u8 = reward, done_u8
        self._bind_step()

    def _obs(self):
        if self.vector_obs is None:
            return self.obs
        return {"visual_observation": self.obs, "vector_observation": self.vector_obs}

    def render(self):
        """rgb_array mode of the reference: fliplr(rot90(obs, 3)) == transpose to [y][x][c] (mortar_mayhem_grid.py:401-402);
        debug_rgb_array mode: the ground-truth view of every instance, uint8 [N, 336, 336, 3] (:403-405, include/memgym.h
        mg_render_debug)."""
        if self.render_mode == "debug_rgb_array":
            return self.render_debug()
        if self.obs_format == "u8_chw":
            return self.obs.permute(0, 2, 3, 1)
        if self.obs_format != "u8_xyc":
            return (self.obs.permute(0, 2, 3, 1).float() * 255.0).round().to(torch.uint8)
        return self.obs.permute(0, 2, 1, 3)

    def render_debug(self):
        out = torch.empty((self.num_envs, 336, 336, 3), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(_native.LIB.mg_render_debug(self._h, out.data_ptr(), self._stream()), "mg_render_debug")
        return out

    def state_dict(self):
        n = _native.LIB.mg_state_size(self._h)
        buf = np.empty(n, np.uint8)
        with torch.cuda.device(self.device):
            _native.check(_native.LIB.mg_get_state(self._h, buf.ctypes.data, n), "mg_get_state")
        # the reset options in force belong to the state: geometry, schedules and limits are derived from them
        sd = {"env_id": self.env_id, "num_envs": self.num_envs, "blob": buf, "options": dict(self._applied), "seeded": self._seeded,
              "capacity": dict(self.capacity)}
        if self._set_of is not None:  # per-instance option sets in use
            sd["option_sets"] = [dict(p) for p in self._set_params]
            sd["set_of"] = self._set_of.cpu().numpy()
        if self._next_step:  # the pending flags belong to a rollout in this mode: a checkpointed one resumes bit for bit
            sd["next_step_pending"] = self.done_u8.cpu().numpy().copy()
        return sd

    def load_state_dict(self, sd):
        """Restore a checkpoint, also into a handle that was never reset: the options in force when it was taken are
        applied first (a rebuild of the geometry happens at the restore, not at some later reset), then the state."""
        assert sd["env_id"] == self.env_id and sd["num_envs"] == self.num_envs
        if sd.get("capacity", {}) != self.capacity:
            raise ValueError("the checkpoint was taken with capacity=%r, this handle was made with %r" % (sd.get("capacity", {}), self.capacity))
        with torch.cuda.device(self.device):
            opts = sd.get("options")
            if opts is not None and any(self._applied.get(k) != v for k, v in opts.items()):
                # options only take effect at a reset: do one (its frames and RNG consumption are overwritten right below)
                self.reset(seed=0, options={k: v for k, v in opts.items() if k in DEFAULTS[self.env_id]})
                # whatever that throw-away reset flagged (e.g. use_exit=False on instances that have no exit YET: the restored
                # ones bring theirs) says nothing about the restored episodes
                _native.LIB.mg_poll_errors(self._h, C.byref(C.c_int()))
            if sd.get("option_sets") is not None:
                for k, p in enumerate(sd["option_sets"]):
                    self._room_for_set(k)
                    if k > 0 and p:  # (an empty entry: a slot that was never filled or half-written when the checkpoint was taken)
                        self._set_params[k] = {}
                        self._write_set(k, process_reset_params(self.env_id, {kk: vv for kk, vv in p.items() if kk in DEFAULTS[self.env_id]}))
                if self._set_of is None:
                    self._bind_set_index(True)
                self._set_of.copy_(torch.as_tensor(np.asarray(sd["set_of"], dtype=np.int32), device=self.device))
            elif self._set_of is not None:  # the checkpoint was taken with one option set: back to that arrangement
                self._bind_set_index(False)
                del self._set_params[1:]
            buf = np.ascontiguousarray(sd["blob"], dtype=np.uint8)
            _native.check(_native.LIB.mg_set_state(self._h, buf.ctypes.data, buf.size), "mg_set_state")
            self._seeded = bool(sd.get("seeded", True))  # (env.obs shows the restored episodes from the next step on)
            self._clear_pending()
            if self._next_step and sd.get("next_step_pending") is not None:
                self.done_u8.copy_(torch.as_tensor(np.asarray(sd["next_step_pending"], dtype=np.uint8), device=self.device))

    def set_profiling(self, every):
        """Bracket the kernels of every `every`-th step with HIP events (0/False = off, 1/True = every step)."""
        _native.check(_native.LIB.mg_set_profiling(self._h, int(every)), "mg_set_profiling")

    def get_profile(self, kind):
        """(total_ms, launches) of the logic (kind 0) or raster (kind 1) kernel since the last call."""
        ms, n = C.c_double(), C.c_int64()
        _native.check(_native.LIB.mg_get_profile(self._h, kind, C.byref(ms), C.byref(n)), "mg_get_profile")
        return ms.value, n.value

    CAPACITY_BITS = 1 | 4 | 8 | 32  # the bits that say "an instance reached a capacity of this build and its episode was ended"

    ERROR_BITS = {1: "more than 16 live spotlights in one instance (raise spawn_interval / spot speeds or lower initial_spawns)",
                  2: "path generation found no valid path (pygame_assets.py:723-724 raises here too)",
                  4: "endless path longer than 128 segments", 8: "more than 128 distinct fall-off cells",
                  16: "past-path window wider than 16 columns",
                  32: "Endless Mortar Mayhem command list reached its 512-entry capacity (the episode was ended)",
                  64: "a deferred-reset queue overflowed (a previous fused launch did not drain it)",
                  256: "use_exit=False for an instance that never had an exit (the reference raises AttributeError at this reset)",
                  512: "save_instances / load_instances / save_frames / draw_frames / draw_frames_padded / draw_sequences / save_debug_frames / "
                       "draw_debug_frames / EpisodeSequences.picks / EpisodeWindows.picks / draw_windows / gather_rows: an instance, record, sequence, "
                       "sample or row index out of range (the entry was skipped)"}

    def check_errors(self):
        """Raise if a kernel flagged a capacity/failure condition since the last call (synchronises the device).
        step() looks at the same bits after every call without synchronising and ends up here when one is set."""
        f = C.c_int()
        _native.check(_native.LIB.mg_poll_errors(self._h, C.byref(f)), "mg_poll_errors")
        self.capacity_events = getattr(self, "capacity_events", 0) | (f.value & self._tolerated)  # (kinds seen so far, on_capacity="truncate")
        f.value &= ~self._tolerated
        if f.value:
            what = "; ".join(m for b, m in self.ERROR_BITS.items() if f.value & b)
            hint = " (make(..., on_capacity='truncate') reports such instances as truncated instead of raising)" if f.value & self.CAPACITY_BITS else ""
            raise RuntimeError("memory_gym_amd: device error flags 0x%x: %s -- the frames of the affected instances are "
                               "no longer the reference's (include/memgym.h: mg_poll_errors)%s" % (f.value, what, hint))

    def rng_words(self, i):
        w = np.zeros(6, np.uint64)
        _native.check(_native.LIB.mg_debug_rng(self._h, int(i), w.ctypes.data), "mg_debug_rng")
        return w

    def set_rng_words(self, i, words):
        """Test hook (include/memgym.h: mg_debug_set_rng): instance i continues with the PCG64 stream given in rng_words()' six words."""
        w = np.ascontiguousarray([int(x) for x in words], dtype=np.uint64)
        assert w.shape == (6,)
        _native.check(_native.LIB.mg_debug_set_rng(self._h, int(i), w.ctypes.data), "mg_debug_set_rng")

    def debug_counter(self, name):
        """Named test / telemetry counter of the handle (include/memgym.h: mg_debug_counter), e.g. "one_launch_rescues"."""
        v = C.c_int64()
        _native.check(_native.LIB.mg_debug_counter(self._h, name.encode(), C.byref(v)), "mg_debug_counter")
        return v.value

    def close(self):
        if getattr(self, "_h", None):
            _native.LIB.mg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


from .single import MemoryGymEnv  # noqa: E402,F401  (the adapter is built on the class above; it keeps its name here too)
