"""Characterisation of the host side's refusals that need a handle (GPU): one Discrete and one MultiDiscrete id, three instances, a rollout of two
steps.  Every bad call is compared with the exception type and the message it gave when the table below was recorded, for exact equality; layout
words and device indices differ from run to run and are replaced by a fixed token, nothing else is.  Every refusal is raised on the host before a
launch, each handle stays usable behind them (a step() and check_errors() close the run), and the value paths that share helpers -- the stats of
advance() and play(), draw_frames against draw_frames_padded -- are compared with the expression written out here.
`python tests/test_gpu_host_messages.py` prints the table as the code at hand gives it."""
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IDS = {"MortarMayhem-Grid-v0": {"A": "(3,)", "T": "[K, 3]"}, "MortarMayhem-v0": {"A": "(3, 2)", "T": "[K, 3, 2]"}}  # Discrete, MultiDiscrete


def outcome(call):
    try:
        got = call()
    except Exception as e:
        text = re.sub(r"cuda:\d+", "cuda:<i>", re.sub(r"0x[0-9a-f]+", "0x<layout>", str(e)))
        return (type(e).__name__, text)
    return ("accepted", "%s %s" % (got.dtype, tuple(got.shape)) if isinstance(got, torch.Tensor) else "")


def collect(env_id):
    """-> name -> outcome of every bad call, on fresh handles of `env_id`; the value paths are asserted on the way"""
    import memory_gym_amd
    from memory_gym_amd import vec_env as V

    got = {}
    env = memory_gym_amd.make(env_id, num_envs=3, device=0)
    dev = env.device
    acts = torch.zeros((3, 2) if env.action_dim == 2 else (3,), dtype=torch.int32, device=dev)
    tape = torch.zeros((2,) + tuple(acts.shape), dtype=torch.int32, device=dev)
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)
    ro = env.new_rollout(2)

    # ---- before the first reset: every public method that asks for a started handle
    before = {"advance_traced": lambda: env.advance_traced(ro), "play(trace=...)": lambda: env.play(tape, trace=ro),
              "save_instances": lambda: env.save_instances(), "load_instances": lambda: env.load_instances(None),
              "copy_instances": lambda: env.copy_instances([0], [1]), "save_frames": lambda: env.save_frames(),
              "draw_frames": lambda: env.draw_frames(None), "draw_frames_padded": lambda: env.draw_frames_padded(None, None),
              "split_episodes": lambda: env.split_episodes(None, 1), "draw_sequences": lambda: env.draw_sequences(None, None),
              "episode_positions": lambda: env.episode_positions(None), "episode_windows": lambda: env.episode_windows(None, 1),
              "draw_windows": lambda: env.draw_windows(None, None), "save_debug_frames": lambda: env.save_debug_frames(),
              "draw_debug_frames": lambda: env.draw_debug_frames(None)}
    for name, call in before.items():
        got["before reset: " + name] = outcome(call)
    env.reset(seed=0)
    ro = env.new_rollout(2)

    # ---- a misaligned out: a uint8 buffer viewed from byte offset 1
    def skewed(*shape):
        n = int(np.prod(shape))
        return u8(n + 16)[1:1 + n].view(shape)

    B, nb = env.frame_record_bytes, env.instance_bytes
    rec, dbg, snap = env.save_frames(), env.save_debug_frames(), env.save_instances()
    got["misaligned: save_instances"] = outcome(lambda: env.save_instances(out=V.InstanceSnapshot(skewed(3, nb), env.instance_layout)))
    got["misaligned: load_instances"] = outcome(lambda: env.load_instances(V.InstanceSnapshot(skewed(3, nb), snap.layout)))
    got["misaligned: save_frames"] = outcome(lambda: env.save_frames(out=skewed(3, B)))
    got["misaligned: save_debug_frames"] = outcome(lambda: env.save_debug_frames(out=skewed(3, B)))
    got["misaligned: draw_frames"] = outcome(lambda: env.draw_frames(rec, out=skewed(3, 84, 84, 3)))
    got["misaligned: draw_frames_padded"] = outcome(lambda: env.draw_frames_padded(rec, [0, -1, 2], out=skewed(3, 84, 84, 3)))
    got["misaligned: draw_debug_frames"] = outcome(lambda: env.draw_debug_frames(dbg, out=skewed(3, 336, 336, 3)))
    got["misaligned records: draw_frames"] = outcome(lambda: env.draw_frames(skewed(3, B)))

    # ---- step / play / expert_actions / the buffers / the checkpoint
    got["step: a mask of length 2"] = outcome(lambda: env.step(acts, mask=torch.ones(2, dtype=torch.bool, device=dev)))
    got["step: a mask [3, 1]"] = outcome(lambda: env.step(acts, mask=[[1], [1], [1]]))
    got["play: a mask of length 2"] = outcome(lambda: env.play(tape, mask=[1, 1]))
    got["play: a tape of the wrong rank"] = outcome(lambda: env.play(torch.zeros(3, dtype=torch.int32)))
    got["play x2: a tape of the wrong rank and a mask of length 2"] = outcome(lambda: env.play(np.zeros(3), mask=[1, 1]))
    got["play x2: a mask of length 2 and a trace of three steps"] = outcome(lambda: env.play(tape, mask=[1, 1], trace=env.new_rollout(3)))
    got["play: a trace of three steps"] = outcome(lambda: env.play(tape, trace=env.new_rollout(3)))
    got["advance_traced: no trace"] = outcome(lambda: env.advance_traced(rec))
    got["expert_actions: a float out"] = outcome(lambda: env.expert_actions(out=torch.zeros(tuple(acts.shape), device=dev)))
    got["use_obs_buffer: float32"] = outcome(lambda: env.use_obs_buffer(torch.zeros_like(env.obs, dtype=torch.float32)))
    got["use_step_buffers: a float64 reward"] = outcome(lambda: env.use_step_buffers(torch.zeros(3, dtype=torch.float64, device=dev), u8(3)))
    got["use_step_buffers: an int32 done"] = outcome(lambda: env.use_step_buffers(torch.zeros(3, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)))
    got["load_state_dict: another capacity"] = outcome(lambda: env.load_state_dict(dict(env.state_dict(), capacity={"commands": 1024})))
    got["copy_instances: two lengths"] = outcome(lambda: env.copy_instances([0, 1], [2]))
    got["copy_instances: a float src"] = outcome(lambda: env.copy_instances([0.5], [2]))

    # ---- records through the handle
    stale = lambda r, cls: cls(r.records, r.layout ^ 1)
    got["draw_frames: a stale layout"] = outcome(lambda: env.draw_frames(stale(rec, V.FrameRecords)))
    got["draw_frames: debug-view records"] = outcome(lambda: env.draw_frames(dbg))
    got["draw_frames_padded: an unknown format"] = outcome(lambda: env.draw_frames_padded(rec, [0], obs_format="rgb"))
    got["draw_debug_frames: frame records"] = outcome(lambda: env.draw_debug_frames(rec))
    got["draw_debug_frames: a stale layout"] = outcome(lambda: env.draw_debug_frames(stale(dbg, V.DebugFrameRecords)))
    got["draw_debug_frames: size 100"] = outcome(lambda: env.draw_debug_frames(dbg, size=100))
    got["draw_debug_frames: a float pick"] = outcome(lambda: env.draw_debug_frames(dbg, pick=[0.5]))
    got["draw_debug_frames: a pick in two dimensions"] = outcome(lambda: env.draw_debug_frames(dbg, pick=[[0, 1]]))
    got["draw_debug_frames: records of another width"] = outcome(lambda: env.draw_debug_frames(u8(3, B + 16)))
    got["draw_debug_frames: no records"] = outcome(lambda: env.draw_debug_frames(u8(0, B), pick=[0]))
    got["draw_debug_frames: out of the small size"] = outcome(lambda: env.draw_debug_frames(dbg, out=u8(3, 84, 84, 3)))
    got["draw_debug_frames x2: frame records and size 100"] = outcome(lambda: env.draw_debug_frames(rec, size=100))
    got["draw_debug_frames x2: a stale layout and a float pick"] = outcome(lambda: env.draw_debug_frames(stale(dbg, V.DebugFrameRecords), pick=[0.5]))
    got["draw_debug_frames x2: a float pick and out of the small size"] = outcome(lambda: env.draw_debug_frames(dbg, pick=[0.5], out=u8(1, 84, 84, 3)))
    got["save_debug_frames: an instance named twice"] = outcome(lambda: env.save_debug_frames(idx=[0, 0]))
    got["save_debug_frames: out holds frame records"] = outcome(lambda: env.save_debug_frames(out=rec))
    got["save_debug_frames: out of two records"] = outcome(lambda: env.save_debug_frames(out=u8(2, B)))
    got["save_debug_frames x2: named twice and out holds frame records"] = outcome(lambda: env.save_debug_frames(idx=[0, 0], out=rec))
    got["save_frames: out of two records"] = outcome(lambda: env.save_frames(out=u8(2, B)))

    # ---- sequences and windows of a traced rollout
    env.advance_traced(ro, render=False)
    ro3 = env.new_rollout(3)
    seqs = env.split_episodes(ro.done, 2, capacity=12)
    win = env.episode_windows(ro.done, 2)
    f32 = lambda *shape: torch.zeros(shape, device=dev)
    got["draw_sequences: no sequences"] = outcome(lambda: env.draw_sequences(ro, "seqs"))
    got["draw_sequences: a trace of three steps"] = outcome(lambda: env.draw_sequences(ro3, seqs))
    got["draw_sequences: a trace without frames"] = outcome(lambda: env.draw_sequences(V.RolloutTrace(None, 0, None, None, ro.reward, ro.done), seqs))
    got["draw_sequences: an unknown format"] = outcome(lambda: env.draw_sequences(ro, seqs, obs_format="rgb"))
    got["draw_sequences: too few records"] = outcome(lambda: env.draw_sequences(ro.frames[:2], seqs, sel=[0]))
    got["draw_sequences: a float out"] = outcome(lambda: env.draw_sequences(ro, seqs, sel=[0, 1], out=f32(2, 2, 84, 84, 3)))
    got["draw_sequences: out of three rows"] = outcome(lambda: env.draw_sequences(ro, seqs, sel=[0, 1], out=u8(3, 2, 84, 84, 3)))
    got["draw_sequences x2: a trace of three steps and an unknown format"] = outcome(lambda: env.draw_sequences(ro3, seqs, obs_format="rgb"))
    got["draw_sequences x2: an unknown format and too few records"] = outcome(lambda: env.draw_sequences(ro.frames[:2], seqs, sel=[0], obs_format="rgb"))
    got["draw_sequences x2: too few records and a float sel"] = outcome(lambda: env.draw_sequences(ro.frames[:2], seqs, sel=[0.5]))
    got["sequences.picks: sel and m"] = outcome(lambda: seqs.picks(sel=[0], m=1))
    got["sequences.picks: m -1"] = outcome(lambda: seqs.picks(m=-1))
    got["sequences.picks: m True"] = outcome(lambda: seqs.picks(m=True))
    got["sequences.picks: a float sel"] = outcome(lambda: seqs.picks(sel=[0.5]))
    got["sequences.picks x2: a float sel and m"] = outcome(lambda: seqs.picks(sel=[0.5], m=-1))
    got["windows.picks: sel and m"] = outcome(lambda: win.picks(sel=[0], m=1))
    got["windows.picks: m beyond the samples"] = outcome(lambda: win.picks(m=10))
    got["windows.picks: m -1"] = outcome(lambda: win.picks(m=-1))
    got["windows.picks: m 2.0"] = outcome(lambda: win.picks(m=2.0))
    got["windows.picks: sel in two dimensions"] = outcome(lambda: win.picks(sel=[[0, 1]]))
    got["draw_windows: a trace of three steps"] = outcome(lambda: env.draw_windows(ro3, win))
    got["draw_windows: an unknown format"] = outcome(lambda: env.draw_windows(ro, win, obs_format="rgb"))
    got["draw_windows: out of three columns"] = outcome(lambda: env.draw_windows(ro, win, sel=[0], out=u8(1, 3, 84, 84, 3)))
    got["draw_windows x2: an unknown format and a float sel"] = outcome(lambda: env.draw_windows(ro, win, sel=[0.5], obs_format="rgb"))
    got["draw_windows x2: a float sel and out of three columns"] = outcome(lambda: env.draw_windows(ro, win, sel=[0.5], out=u8(1, 3, 84, 84, 3)))
    got["gather_rows: x on the host"] = outcome(lambda: env.gather_rows(torch.zeros((4, 2)), [0]))

    # ---- the value paths behind shared helpers, against the expression written out
    sums = [("reward", torch.float64), ("episodes", torch.int32), ("episode_reward", torch.float64), ("episode_length", torch.int64)]
    sums += [(nm, torch.float64) for nm in env.info_names]
    _, st = env.advance(2, render=False)
    assert [(k, v.dtype, tuple(v.shape)) for k, v in st.items()] == [(k, dt, (3,)) for k, dt in sums]
    _, st = env.play(tape, render=False)
    assert [(k, v.dtype, tuple(v.shape)) for k, v in st.items()] == [(k, dt, (3,)) for k, dt in sums + [("steps", torch.int32)]]
    assert st["steps"].tolist() == [2, 2, 2]
    _, st = env.play(tape, render=False, trace=True)
    assert list(st)[-2:] == ["reward_trace", "done_trace"] and st["reward_trace"].dtype == torch.float32 and st["done_trace"].dtype == torch.bool
    assert env.advance(1, render=False, stats=False) == (None, None) and env.play(tape, render=False, stats=False) == (None, None)
    rec = env.save_frames()
    plain = env.draw_frames(rec)
    assert torch.equal(plain, env.draw_frames_padded(rec, torch.arange(3))) and torch.equal(plain, env.draw_frames_padded(rec, None))
    assert torch.equal(plain, env.redraw()) and plain.dtype == torch.uint8 and tuple(plain.shape) == (3, 84, 84, 3)
    none = torch.zeros(0, dtype=torch.int32, device=dev)
    got["an empty pick: draw_frames"] = outcome(lambda: env.draw_frames(rec, pick=none))
    got["an empty pick: draw_frames_padded"] = outcome(lambda: env.draw_frames_padded(rec, none))
    got["an empty pick: draw_debug_frames"] = outcome(lambda: env.draw_debug_frames(dbg, pick=none))
    got["an empty pick: gather_rows"] = outcome(lambda: env.gather_rows(plain, none))

    # ---- terminal observations are frames: no headless form
    fin = memory_gym_amd.make(env_id, num_envs=3, device=0, final_observation=True)
    fin.reset(seed=0)
    fsnap = fin.save_instances()
    got["final_observation: step(render=False)"] = outcome(lambda: fin.step(acts, render=False))
    got["final_observation: load_instances(render=False)"] = outcome(lambda: fin.load_instances(fsnap, render=False))
    got["final_observation x2: load_instances(render=False) of no snapshot"] = outcome(lambda: fin.load_instances(None, render=False))

    # ---- next-step auto-reset has neither a masked nor a headless form, and no terminal rows
    nxt = memory_gym_amd.make(env_id, num_envs=3, device=0, autoreset_mode="next_step")
    nxt.reset(seed=0)
    got["next_step: step(mask=...)"] = outcome(lambda: nxt.step(acts, mask=[1, 1, 1]))
    got["next_step: step(render=False)"] = outcome(lambda: nxt.step(acts, render=False))
    got["next_step: final_observation=True"] = outcome(lambda: memory_gym_amd.make(env_id, num_envs=3, device=0, autoreset_mode="next_step", final_observation=True))
    got["next_step x2: a mask of length 2 and render=False"] = outcome(lambda: nxt.step(acts, render=False, mask=[1, 1]))

    for handle in (env, fin, nxt):  # every rejected call has left its handle usable
        obs, reward, done, _, info = handle.step(acts)
        assert tuple(obs.shape) == (3, 84, 84, 3) and tuple(reward.shape) == (3,) and "done_mask" in info
        handle.check_errors()
        handle.close()
    return got


_BEFORE = "%s: before the first reset (or load_state_dict)"
_ALIGNED = "%s: %s must be a 16-byte aligned tensor on cuda:<i>"
_ALIGNED2 = "%s: records and out must be 16-byte aligned tensors on cuda:<i>"
_LAYOUT = ("%s: the records (layout 0x<layout>) were saved from another handle, or before something changed that they would draw differently "
           "(layout 0x<layout> now): %s records are valid for the handle and the atlas they were saved under")
_FORMATS = "%s: obs_format must be one of ['bf16_chw', 'f16_chw', 'f32_chw', 'u8_chw', 'u8_xyc']"
_TWICE = "save_debug_frames: idx names an instance more than once (entries must be distinct; negative entries are padding)"
_NEXT = "step(%s) on a handle with autoreset_mode='next_step': the mode has neither a masked nor a headless form"
_V = "ValueError"

# name -> (type, message) as recorded; {A} and {T} stand for the id's action shape and tape shape (IDS)
EXPECTED = {
    "before reset: advance_traced": (_V, _BEFORE % "advance_traced"),
    "before reset: play(trace=...)": (_V, _BEFORE % "play(trace=...)"),
    "before reset: save_instances": (_V, _BEFORE % "save_instances"),
    "before reset: load_instances": (_V, _BEFORE % "load_instances"),
    "before reset: copy_instances": (_V, _BEFORE % "copy_instances"),
    "before reset: save_frames": (_V, _BEFORE % "save_frames"),
    "before reset: draw_frames": (_V, _BEFORE % "draw_frames"),
    "before reset: draw_frames_padded": (_V, _BEFORE % "draw_frames_padded"),
    "before reset: split_episodes": (_V, _BEFORE % "split_episodes"),
    "before reset: draw_sequences": (_V, _BEFORE % "draw_sequences"),
    "before reset: episode_positions": (_V, _BEFORE % "episode_positions"),
    "before reset: episode_windows": (_V, _BEFORE % "episode_windows"),
    "before reset: draw_windows": (_V, _BEFORE % "draw_windows"),
    "before reset: save_debug_frames": (_V, _BEFORE % "save_debug_frames"),
    "before reset: draw_debug_frames": (_V, _BEFORE % "draw_debug_frames"),
    "misaligned: save_instances": (_V, _ALIGNED % ("save_instances", "out.records")),
    "misaligned: load_instances": (_V, _ALIGNED % ("load_instances", "snapshot.records")),
    "misaligned: save_frames": (_V, _ALIGNED % ("save_frames", "out")),
    "misaligned: save_debug_frames": (_V, _ALIGNED % ("save_debug_frames", "out")),
    "misaligned: draw_frames": (_V, _ALIGNED2 % "draw_frames"),
    "misaligned: draw_frames_padded": (_V, _ALIGNED2 % "draw_frames_padded"),
    "misaligned: draw_debug_frames": (_V, _ALIGNED2 % "draw_debug_frames"),
    "misaligned records: draw_frames": (_V, _ALIGNED2 % "draw_frames"),
    "step: a mask of length 2": (_V, "step(mask=...): the mask must have shape [3], got (2,)"),
    "step: a mask [3, 1]": (_V, "step(mask=...): the mask must have shape [3], got (3, 1)"),
    "play: a mask of length 2": (_V, "play(mask=...): the mask must have shape [3], got (2,)"),
    "play: a tape of the wrong rank": (_V, "play(actions): the tape must have shape {T} with K >= 1, got (3,)"),
    "play x2: a tape of the wrong rank and a mask of length 2": (_V, "play(actions): the tape must have shape {T} with K >= 1, got (3,)"),
    "play x2: a mask of length 2 and a trace of three steps": (_V, "play(mask=...): the mask must have shape [3], got (2,)"),
    "play: a trace of three steps": (_V, "play(trace=...): trace.frames must be a contiguous torch.uint8 tensor of shape (3, 3, 16) (a trace of 2 steps of 3 "
                                         "instances), got torch.uint8 (4, 3, 16)"),
    "advance_traced: no trace": (_V, "advance_traced: need the RolloutTrace new_rollout returned"),
    "expert_actions: a float out": (_V, "expert_actions: out must be a contiguous int32 tensor of shape {A} on cuda:<i>"),
    "use_obs_buffer: float32": (_V, "use_obs_buffer: need a contiguous tensor like env.obs"),
    "use_step_buffers: a float64 reward": (_V, "use_step_buffers: need contiguous float32 [N] / uint8 [N] tensors on the handle's device"),
    "use_step_buffers: an int32 done": (_V, "use_step_buffers: need contiguous float32 [N] / uint8 [N] tensors on the handle's device"),
    "load_state_dict: another capacity": (_V, "the checkpoint was taken with capacity={'commands': 1024}, this handle was made with {}"),
    "copy_instances: two lengths": (_V, "copy_instances: src and dst must have the same length, got 2 and 1"),
    "copy_instances: a float src": (_V, "copy_instances: src must hold integers, got dtype float64"),
    "draw_frames: a stale layout": (_V, _LAYOUT % ("draw_frames", "frame")),
    "draw_frames: debug-view records": (_V, "draw_frames: these are debug-view records (save_debug_frames): draw_debug_frames draws them"),
    "draw_frames_padded: an unknown format": (_V, _FORMATS % "draw_frames"),
    "draw_debug_frames: frame records": (_V, "draw_debug_frames: these are frame records (save_frames): draw_frames draws them"),
    "draw_debug_frames: a stale layout": (_V, _LAYOUT % ("draw_debug_frames", "debug-view")),
    "draw_debug_frames: size 100": (_V, "draw_debug_frames: size must be 84 or 336"),
    "draw_debug_frames: a float pick": (_V, "draw_debug_frames: pick must hold integers, got dtype float64"),
    "draw_debug_frames: a pick in two dimensions": (_V, "draw_debug_frames: pick must have one dimension, got shape (1, 2)"),
    "draw_debug_frames: records of another width": (_V, "draw_debug_frames: records must be a contiguous uint8 tensor [..., 16]"),
    "draw_debug_frames: no records": (_V, "draw_debug_frames: no records to draw from"),
    "draw_debug_frames: out of the small size": (_V, "draw_debug_frames: out must be a contiguous uint8 tensor of shape (3, 336, 336, 3)"),
    "draw_debug_frames x2: frame records and size 100": (_V, "draw_debug_frames: size must be 84 or 336"),
    "draw_debug_frames x2: a stale layout and a float pick": (_V, _LAYOUT % ("draw_debug_frames", "debug-view")),
    "draw_debug_frames x2: a float pick and out of the small size": (_V, "draw_debug_frames: pick must hold integers, got dtype float64"),
    "save_debug_frames: an instance named twice": (_V, _TWICE),
    "save_debug_frames: out holds frame records": (_V, "save_debug_frames: out holds frame records (save_frames), not debug-view records"),
    "save_debug_frames: out of two records": (_V, "save_frames: out holds 2 records, the call saves 3"),
    "save_debug_frames x2: named twice and out holds frame records": (_V, _TWICE),
    "save_frames: out of two records": (_V, "save_frames: out holds 2 records, the call saves 3"),
    "draw_sequences: no sequences": (_V, "draw_sequences: seqs must be the EpisodeSequences split_episodes returned"),
    "draw_sequences: a trace of three steps": (_V, "draw_sequences: the trace holds 3 steps of 3 instances, the sequences were cut from 2 steps of 3"),
    "draw_sequences: a trace without frames": (_V, "draw_sequences: the trace keeps no frames"),
    "draw_sequences: an unknown format": (_V, _FORMATS % "draw_sequences"),
    "draw_sequences: too few records": (_V, "draw_sequences: frames holds fewer than (2 + 1) * 3 records"),
    "draw_sequences: a float out": (_V, "draw_sequences: out must be a contiguous torch.uint8 tensor of shape (2, 2, 84, 84, 3)"),
    "draw_sequences: out of three rows": (_V, "draw_sequences: out must be a contiguous torch.uint8 tensor of shape (2, 2, 84, 84, 3)"),
    "draw_sequences x2: a trace of three steps and an unknown format": (_V, "draw_sequences: the trace holds 3 steps of 3 instances, the sequences were cut "
                                                                           "from 2 steps of 3"),
    "draw_sequences x2: an unknown format and too few records": (_V, _FORMATS % "draw_sequences"),
    "draw_sequences x2: too few records and a float sel": (_V, "draw_sequences: frames holds fewer than (2 + 1) * 3 records"),
    "sequences.picks: sel and m": (_V, "EpisodeSequences.picks: give sel or m, not both"),
    "sequences.picks: m -1": (_V, "EpisodeSequences.picks: m must be an integer >= 0, got -1"),
    "sequences.picks: m True": (_V, "EpisodeSequences.picks: m must be an integer >= 0, got True"),
    "sequences.picks: a float sel": (_V, "EpisodeSequences.picks: sel must hold integers, got dtype float64"),
    "sequences.picks x2: a float sel and m": (_V, "EpisodeSequences.picks: give sel or m, not both"),
    "windows.picks: sel and m": (_V, "EpisodeWindows.picks: give sel or m, not both"),
    "windows.picks: m beyond the samples": (_V, "EpisodeWindows.picks: m must be an integer in 0 .. 9, got 10"),
    "windows.picks: m -1": (_V, "EpisodeWindows.picks: m must be an integer in 0 .. 9, got -1"),
    "windows.picks: m 2.0": (_V, "EpisodeWindows.picks: m must be an integer in 0 .. 9, got 2.0"),
    "windows.picks: sel in two dimensions": (_V, "EpisodeWindows.picks: sel must have one dimension, got shape (1, 2)"),
    "draw_windows: a trace of three steps": (_V, "draw_windows: the trace holds 3 steps of 3 instances, the windows were made from 2 steps of 3"),
    "draw_windows: an unknown format": (_V, _FORMATS % "draw_windows"),
    "draw_windows: out of three columns": (_V, "draw_windows: out must be a contiguous torch.uint8 tensor of shape (1, 2, 84, 84, 3)"),
    "draw_windows x2: an unknown format and a float sel": (_V, _FORMATS % "draw_windows"),
    "draw_windows x2: a float sel and out of three columns": (_V, "EpisodeWindows.picks: sel must hold integers, got dtype float64"),
    "gather_rows: x on the host": (_V, "gather_rows: x is on cpu, the handle on cuda:<i>"),
    # (draw_frames hands the library an empty tensor's NULL address, which it refuses on the host; the other three return before their call)
    "an empty pick: draw_frames": ("RuntimeError", "mg_draw_frames failed (-1): mg_draw_frames: obs_dev is NULL or not 16-byte aligned"),
    "an empty pick: draw_frames_padded": ("accepted", "torch.uint8 (0, 84, 84, 3)"),
    "an empty pick: draw_debug_frames": ("accepted", "torch.uint8 (0, 336, 336, 3)"),
    "an empty pick: gather_rows": ("accepted", "torch.uint8 (0, 84, 84, 3)"),
    "final_observation: step(render=False)": (_V, "step(render=False) on a handle with final_observation=True: terminal observations are frames"),
    "final_observation: load_instances(render=False)": (_V, "load_instances(render=False) on a handle with final_observation=True: terminal observations are frames"),
    "final_observation x2: load_instances(render=False) of no snapshot": (_V, "load_instances(render=False) on a handle with final_observation=True: terminal "
                                                                             "observations are frames"),
    "next_step: step(mask=...)": (_V, _NEXT % "mask=..."),
    "next_step: step(render=False)": (_V, _NEXT % "render=False"),
    "next_step: final_observation=True": (_V, "autoreset_mode='next_step' together with final_observation=True / final_frames=True: there are no terminal rows in "
                                              "this mode, the observation of the step that ends an episode IS the terminal observation"),
    "next_step x2: a mask of length 2 and render=False": (_V, _NEXT % "mask=..."),
}


@pytest.mark.parametrize("env_id", sorted(IDS))
def test_every_refusal_keeps_its_type_and_its_message(env_id):
    got = collect(env_id)
    assert sorted(got) == sorted(EXPECTED)
    for name, (kind, text) in EXPECTED.items():
        for k, v in IDS[env_id].items():
            text = text.replace("{" + k + "}", v)
        assert got[name] == (kind, text), name


if __name__ == "__main__":
    import os
    import pprint

    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.environ.get("MEMGYM_PKG") or os.path.join(here, "endless-memory-gym_amd"))
    for env_id in sorted(IDS):
        print("# %s" % env_id)
        pprint.pprint(collect(env_id), width=200, sort_dicts=False)
