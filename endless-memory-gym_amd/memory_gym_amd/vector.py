"""gymnasium.vector.VectorEnv-shaped front end: what a trainer written against gymnasium 0.29's
vector API (the version the reference pins, setup.py:35) expects from `gymnasium.vector.make(id, num_envs)`:

    obs, infos = envs.reset(seed=..., options=...)
    obs, rewards, terminations, truncations, infos = envs.step(actions)

* sub-environments that terminate are reset in the same call; `obs[i]` is then the first observation of the new
  episode, `infos["final_observation"][i]` the terminal observation and `infos["final_info"][i]` the reference's
  end-of-episode info dict (e.g. mortar_mayhem_grid.py:356-362); `infos["_final_observation"]` / `["_final_info"]`
  are the boolean masks.  `truncations` is all False (the reference never truncates).
* `reset(seed=s)` seeds sub-environment i with `s + i`, like gymnasium's vector envs.

By default everything stays on the GPU as torch tensors (`final_observation` is a full [N, ...] tensor whose rows are
valid where the mask is set; `final_info` a dict of [N] tensors).  With `as_numpy=True` the outputs are converted to
exactly gymnasium's host-side layout (numpy arrays, object arrays of per-env entries / None); that costs a device
synchronisation and a copy of the observations per step and is meant for small `num_envs` and plumbing tests.
"""
import numpy as np
import torch

from .vec_env import VecMemoryGym

try:  # inherit when the host has gymnasium, so isinstance checks of trainers pass
    from gymnasium.vector import VectorEnv as _Base
except Exception:  # gymnasium is not a dependency of the hot path
    _Base = object


class GymnasiumVectorEnv(_Base):
    def __init__(self, env_id, num_envs, device=None, obs_format="u8_xyc", as_numpy=False, on_capacity="raise", capacity=None,
                 autoreset_mode="same_step", final_frames=False):
        # autoreset_mode="next_step": gymnasium >= 1.0's default convention (AutoresetMode.NEXT_STEP; include/memgym.h: mg_step_next) -- the step that ends an
        # episode returns the terminal observation as `obs`, the following step ignores that sub-environment's action and returns the first observation of
        # the new episode with reward 0 and both flags False.  There is no "final_observation" / "final_info": the end-of-episode entries ("reward", "length",
        # the id's aux names) are [N] arrays directly in `infos`, with masks infos["_" + key], as gymnasium >= 1.0 aggregates sub-environment infos.
        if autoreset_mode not in ("same_step", "next_step"):
            raise ValueError("GymnasiumVectorEnv: autoreset_mode must be 'same_step' or 'next_step'")
        self.autoreset_mode = autoreset_mode
        if autoreset_mode == "next_step":
            if final_frames:
                raise ValueError("autoreset_mode='next_step' together with final_frames=True: there are no terminal rows in this mode")
            self.final_frames = False
            self.env = VecMemoryGym(env_id, num_envs=num_envs, device=device, obs_format=obs_format, ground_truth64=bool(as_numpy), on_capacity=on_capacity,
                                    capacity=capacity, autoreset_mode="next_step")
            self._finish_init(num_envs, as_numpy)
            return
        # as_numpy: gymnasium's host-side layout with the reference's dtypes -- rewards and info["ground_truth"] as float64
        # on_capacity="truncate": a sub-environment whose episode this build ended on one of its capacities (VecMemoryGym) comes back with
        # terminations[i] = False and truncations[i] = True, like a time limit; its final_observation / final_info are set as for any end
        # final_frames=True: the same convention WITHOUT FRAMES -- step() is the headless step (obs is None; redraw() draws the current frames), and the frame
        # an episode ended on comes back as its frame record: infos["final_frames"] (a FrameRecords [N, bytes]) with the mask infos["_final_frames"];
        # final_observations(infos) draws exactly the finished rows when the trainer wants them (the bootstrap value of a truncated episode)
        self.final_frames = bool(final_frames)
        self.env = VecMemoryGym(env_id, num_envs=num_envs, device=device, obs_format=obs_format, final_observation=not self.final_frames,
                                ground_truth64=bool(as_numpy), on_capacity=on_capacity, capacity=capacity, final_frames=self.final_frames)
        self._finish_init(num_envs, as_numpy)

    def _finish_init(self, num_envs, as_numpy):
        self.as_numpy = bool(as_numpy)
        done = False
        if _Base is not object:  # gymnasium 0.29: VectorEnv.__init__(num_envs, observation_space, action_space) batches the spaces
            try:
                _Base.__init__(self, int(num_envs), self.env.observation_space, self.env.action_space)
                done = True
            except TypeError:  # gymnasium 1.x: no constructor arguments, attributes are set by the subclass
                _Base.__init__(self)
        if not done:
            self.num_envs = int(num_envs)
            self.is_vector_env = True
            self.single_observation_space = self.env.observation_space
            self.single_action_space = self.env.action_space
            self.observation_space, self.action_space = self._batched_spaces()
            self.closed = False
        self.metadata = dict(self.env.metadata)  # (a copy: the mode is this object's, not the class's)
        try:  # gymnasium >= 1.0 names the modes; older ones (and hosts without gymnasium) get the string
            from gymnasium.vector import AutoresetMode
            self.metadata["autoreset_mode"] = AutoresetMode.NEXT_STEP if self.autoreset_mode == "next_step" else AutoresetMode.SAME_STEP
        except Exception:
            self.metadata["autoreset_mode"] = self.autoreset_mode
        self.spec = None

    def _batched_spaces(self):
        try:
            from gymnasium.vector.utils import batch_space
            return (batch_space(self.single_observation_space, self.num_envs),
                    batch_space(self.single_action_space, self.num_envs))
        except Exception:
            return self.single_observation_space, self.single_action_space

    # ------------------------------------------------------------------ conversions
    def _host(self, x):
        if x is None:
            return None
        if isinstance(x, dict):
            return {k: self._host(v) for k, v in x.items()}
        return x.cpu().numpy() if self.as_numpy else x

    def _final_info(self, ep, d):
        """gymnasium's host-side `final_info`: an object array [N] that holds the end-of-episode dict of sub-environment i where d[i], None elsewhere"""
        finfo = np.full(self.num_envs, None, dtype=object)
        host_ep = {k: v.cpu().numpy() for k, v in ep.items()}
        for i in np.nonzero(d)[0]:
            finfo[i] = {k: (int(v[i]) if k == "length" else float(v[i])) for k, v in host_ep.items()}
        return finfo

    def reset(self, seed=None, options=None):
        obs, info = self.env.reset(seed=seed, options=options)
        return self._host(obs), self._host(info)

    def _step_next(self, actions):
        obs, reward, done, trunc, info = self.env.step(actions)
        term = done if self.env.capacity_u8 is None else (done & ~trunc)  # gymnasium: an episode ends EITHER terminated or truncated
        infos = {}
        if "ground_truth" in info:
            infos["ground_truth"] = info["ground_truth"]
        if "capacity_exceeded" in info:
            infos["capacity_exceeded"] = info["capacity_exceeded"]
        for k in ["reward", "length"] + list(self.env.info_names):  # rows valid where the mask is set
            infos[k] = info[k]
            infos["_" + k] = done
        if not self.as_numpy:
            return obs, reward, term, trunc, infos
        return self._host(obs), self.env.reward64.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(), self._host(infos)

    def step(self, actions):
        if self.autoreset_mode == "next_step":
            return self._step_next(actions)
        obs, reward, done, trunc, info = self.env.step(actions, render=not self.final_frames)
        ep = {"reward": info["reward"], "length": info["length"]}
        for nm in self.env.info_names:
            ep[nm] = info[nm]
        infos = {}
        if "ground_truth" in info:
            infos["ground_truth"] = info["ground_truth"]
        term = done if self.env.capacity_u8 is None else (done & ~trunc)  # gymnasium: an episode ends EITHER terminated or truncated
        if "capacity_exceeded" in info:
            infos["capacity_exceeded"] = info["capacity_exceeded"]
        if self.final_frames:  # (records stay on the device whatever as_numpy says: they are drawn from there)
            infos.update(final_frames=info["final_frames"], _final_frames=done)
            if not self.as_numpy:
                infos.update(final_info=ep, _final_info=done)
                return obs, reward, term, trunc, infos
            d = done.cpu().numpy()
            out = self._host({k: v for k, v in infos.items() if k != "final_frames"})
            out["final_frames"] = infos["final_frames"]
            if d.any():
                out.update(final_info=self._final_info(ep, d), _final_info=d.copy())
            return None, self.env.reward64.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(), out
        if not self.as_numpy:
            infos.update(final_observation=info["final_observation"], _final_observation=done, final_info=ep, _final_info=done)
            return obs, reward, term, trunc, infos
        d = done.cpu().numpy()
        out = self._host(infos)
        if d.any():
            idx = np.nonzero(d)[0]
            fobs = np.full(self.num_envs, None, dtype=object)
            rows = info["final_observation"][torch.as_tensor(idx, device=done.device)].cpu().numpy()
            for j, i in enumerate(idx):
                fobs[i] = rows[j]
            out.update(final_observation=fobs, _final_observation=d.copy(), final_info=self._final_info(ep, d), _final_info=d.copy())
        return self._host(obs), self.env.reward64.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(), out  # (the reference's Python floats: doubles)

    def final_observations(self, info, out=None, obs_format=None):
        """The terminal observations of the sub-environments that finished in the step `info` came from, drawn from its frame records (final_frames=True):
        -> (idx, frames) with idx the finished sub-environments in ascending order (int64 tensor) and frames[j] the observation episode idx[j] ended on, in
        `obs_format` (default: the handle's) -- one gather-raster launch over exactly those rows (VecMemoryGym.draw_frames); numpy with as_numpy.  Looks at
        the mask on the host (one synchronisation); out: a tensor [len(idx), ...] to draw into.  No finished sub-environment: (empty idx, None)."""
        if "final_frames" not in info:
            raise ValueError("final_observations: the info dict carries no frame records (GymnasiumVectorEnv(final_frames=True))")
        mask = info["_final_frames"]
        idx = torch.nonzero(torch.as_tensor(mask, device=self.env.device)).flatten()
        if idx.numel() == 0:
            return self._host(idx), None
        frames = self.env.draw_frames(info["final_frames"], pick=idx.to(torch.int32), out=out, obs_format=obs_format)
        return self._host(idx), self._host(frames)

    def redraw(self):
        """VecMemoryGym.redraw: the current observations after headless steps (numpy with as_numpy)."""
        return self._host(self.env.redraw())

    def expert_actions(self, eps=0.0, seed=0, step=None, out=None):
        """The scripted teacher's actions in the current states (VecMemoryGym.expert_actions): what step() takes; numpy with as_numpy."""
        return self._host(self.env.expert_actions(eps=eps, seed=seed, step=step, out=out))

    def new_rollout(self, steps, labels=False):
        """VecMemoryGym.new_rollout -> RolloutTrace (device tensors, whatever as_numpy says: a trace is drawn from on the device)."""
        return self.env.new_rollout(steps, labels=labels)

    def split_episodes(self, done, length, steps=None, starts=None, capacity=None):
        """VecMemoryGym.split_episodes -> EpisodeSequences (device tensors, whatever as_numpy says: sequences are drawn from on the device)."""
        return self.env.split_episodes(done, length, steps=steps, starts=starts, capacity=capacity)

    def draw_frames_padded(self, records, pick, out=None, obs_format=None):
        """VecMemoryGym.draw_frames_padded: draw_frames whose picks below 0 give rows of zeros (a device tensor, whatever as_numpy says)."""
        return self.env.draw_frames_padded(records, pick, out=out, obs_format=obs_format)

    def draw_sequences(self, frames, seqs, sel=None, out=None, obs_format=None):
        """VecMemoryGym.draw_sequences -> (obs [M, L, ...], mask [M, L]) of a minibatch of sequences (device tensors, whatever as_numpy says)."""
        return self.env.draw_sequences(frames, seqs, sel=sel, out=out, obs_format=obs_format)

    def episode_positions(self, done, steps=None, pos0=None):
        """VecMemoryGym.episode_positions -> int32 [K + 1, N] (a device tensor, whatever as_numpy says: positions are picked from on the device)."""
        return self.env.episode_positions(done, steps=steps, pos0=pos0)

    def episode_windows(self, done, window, lag=0, back=0, steps=None, pos0=None):
        """VecMemoryGym.episode_windows -> EpisodeWindows (device tensors, whatever as_numpy says: windows are drawn and gathered on the device)."""
        return self.env.episode_windows(done, window, lag=lag, back=back, steps=steps, pos0=pos0)

    def gather_rows(self, x, pick, out=None):
        """VecMemoryGym.gather_rows: rows of a store by index, zero rows where the pick is below 0 (a device tensor, whatever as_numpy says)."""
        return self.env.gather_rows(x, pick, out=out)

    def draw_windows(self, frames, windows, sel=None, out=None, obs_format=None):
        """VecMemoryGym.draw_windows -> (obs [M, W, ...], mask [M, W], len [M]) of a minibatch of windows (device tensors, whatever as_numpy says)."""
        return self.env.draw_windows(frames, windows, sel=sel, out=out, obs_format=obs_format)

    def advance(self, steps, eps=0.0, seed=0, step=None, render=True, stats=True):
        """`steps` steps under the scripted teacher without a frame (VecMemoryGym.advance) -> (obs or None, stats); numpy with as_numpy.
        Episodes that end inside the call are NOT reported as `final_observation` / `final_info`: they are counted and summed in `stats`."""
        obs, st = self.env.advance(steps, eps=eps, seed=seed, step=step, render=render, stats=stats)
        return self._host(obs), self._host(st)

    def advance_traced(self, trace, eps=0.0, seed=0, step=None, render=True, stats=True):
        """VecMemoryGym.advance_traced: advance(trace.steps, ...) that keeps every step's frame record, action, label, reward and done in `trace`, a
        RolloutTrace (new_rollout) -> (obs or None, stats); numpy with as_numpy."""
        obs, st = self.env.advance_traced(trace, eps=eps, seed=seed, step=step, render=render, stats=stats)
        return self._host(obs), self._host(st)

    def play(self, actions, until_done=False, mask=None, render=True, stats=True, trace=False):
        """K steps of caller-supplied action sequences without a frame (VecMemoryGym.play) -> (obs or None, stats); numpy with as_numpy.
        Episodes that end inside the call are NOT reported as `final_observation` / `final_info`: they are counted and summed in `stats`.
        trace: False / True as in VecMemoryGym.play, or a RolloutTrace (new_rollout) that keeps every step's frame record, reward and done."""
        obs, st = self.env.play(actions, until_done=until_done, mask=mask, render=render, stats=stats, trace=trace)
        return self._host(obs), self._host(st)

    def save_instances(self, idx=None, out=None):
        """VecMemoryGym.save_instances: single instances to device memory -> InstanceSnapshot."""
        return self.env.save_instances(idx=idx, out=out)

    def load_instances(self, snap, idx=None, rec=None, render=True):
        """VecMemoryGym.load_instances -> obs (numpy with as_numpy); this handle keeps terminal observations, so render=False is refused."""
        return self._host(self.env.load_instances(snap, idx=idx, rec=rec, render=render))

    def copy_instances(self, src, dst, render=True):
        """VecMemoryGym.copy_instances -> obs (numpy with as_numpy)."""
        return self._host(self.env.copy_instances(src, dst, render=render))

    # gymnasium.vector.VectorEnv API surface used by trainers
    def step_async(self, actions):
        self._pending = actions

    def step_wait(self):
        return self.step(self._pending)

    def reset_async(self, seed=None, options=None):
        self._pending_reset = (seed, options)

    def reset_wait(self, seed=None, options=None):
        # what reset_async left is used ONCE; arguments given here go before it (a later reset_wait(seed=2) does not reset with an old seed)
        s, o = self.__dict__.pop("_pending_reset", (None, None))
        return self.reset(seed=s if seed is None else seed, options=o if options is None else options)

    def close(self, **kwargs):
        if not self.closed:
            self.env.close()
            self.closed = True

    def close_extras(self, **kwargs):
        self.env.close()

    @property
    def unwrapped(self):
        return self
