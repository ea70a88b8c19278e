"""Characterisation of the host side's refusals and of its Python surface (no GPU, no handle): a fixed list of bad calls to the argument checks that
need no handle, each compared with the exception type and the message it gave when the tables below were recorded -- for exact equality, so a call
that is wrong in two ways pins which check comes first -- and the signatures, slots and public names of the package.  The tables are output of this
project's own code: `python tests/test_host_messages.py` prints them as the code at hand gives them."""
import inspect
import sys

import numpy as np
import torch

K, N, B = 6, 70, 64
CUDA0 = torch.device("cuda", 0)  # (only compared with: no GPU is touched)


def cases():
    """name -> a call that must be refused"""
    from memory_gym_amd import vec_env as V

    c = {}
    z = torch.zeros
    # ---- load_instances / save_instances
    n, width, layout = 200, 448, (5 << 24) | 2
    snap = V.InstanceSnapshot(z((65, width), dtype=torch.uint8), layout)
    load = lambda **kw: V.check_instance_load(snap, layout, width, n, **kw)
    c["load: another handle"] = lambda: V.check_instance_load(snap, (6 << 24) | 2, width, n, idx=torch.arange(65))
    c["load: a stale layout"] = lambda: V.check_instance_load(snap, (5 << 24) | 3, width, n, idx=torch.arange(65))
    c["load: a wrong record width"] = lambda: V.check_instance_load(snap, layout, width + 16, n, idx=torch.arange(65))
    c["load: no snapshot"] = lambda: V.check_instance_load(snap.records, layout, width, n)
    c["load: float indices"] = lambda: load(idx=torch.arange(65).float())
    c["load: bool indices"] = lambda: load(idx=torch.ones(65, dtype=torch.bool))
    c["load: a list of floats"] = lambda: load(idx=[0.5, 1.0])
    c["load: two dimensions"] = lambda: load(idx=z((5, 13), dtype=torch.int32))
    c["load: rec of another length"] = lambda: load(idx=torch.arange(65), rec=torch.arange(64))
    c["load: more instances than records without rec"] = lambda: load(idx=torch.arange(66))
    c["load: all instances from 65 records"] = lambda: load()
    c["load: records of another dtype"] = lambda: V.check_instance_load(V.InstanceSnapshot(z((65, width), dtype=torch.int8), layout), layout, width, n, idx=torch.arange(65))
    c["load: set_of of another length"] = lambda: V.check_instance_load(V.InstanceSnapshot(snap.records, layout, z(64, dtype=torch.int32)), layout, width, n,
                                                                         idx=torch.arange(65))
    c["load x2: a stale layout and a wrong record width"] = lambda: V.check_instance_load(snap, (5 << 24) | 3, width + 16, n, idx=torch.arange(65))
    c["load x2: a wrong record width and float indices"] = lambda: V.check_instance_load(snap, layout, width + 16, n, idx=torch.arange(65).float())
    c["load x2: float idx and a two-dimensional rec"] = lambda: load(idx=torch.arange(65).float(), rec=z((5, 13), dtype=torch.int64))
    c["load x2: rec of another length and set_of of another length"] = lambda: V.check_instance_load(
        V.InstanceSnapshot(snap.records, layout, z(64, dtype=torch.int32)), layout, width, n, idx=torch.arange(65), rec=torch.arange(64))
    out3 = V.InstanceSnapshot(z((3, width), dtype=torch.uint8), 1)
    c["save: out of two records for three"] = lambda: V.check_instance_save(width, n, idx=[3, 4], out=out3)
    c["save: out of three records for all"] = lambda: V.check_instance_save(width, n, out=out3)
    c["save: out of another width"] = lambda: V.check_instance_save(width + 16, n, idx=[3, -1, 5], out=out3)
    c["save: out is a tensor"] = lambda: V.check_instance_save(width, n, idx=[3, -1, 5], out=out3.records)
    c["save: float idx"] = lambda: V.check_instance_save(width, n, idx=z(3))
    c["save x2: float idx and out is a tensor"] = lambda: V.check_instance_save(width, n, idx=z(3), out=out3.records)
    c["save x2: two-dimensional idx and out of another width"] = lambda: V.check_instance_save(width + 16, n, idx=z((2, 2), dtype=torch.int64), out=out3)
    # ---- save_frames
    fn, fw = 48, 16
    fstore = z((4, fn, fw), dtype=torch.uint8)
    c["frame_save: out of 48 records for two"] = lambda: V.check_frame_save(fw, fn, idx=[3, 4], out=fstore[0])
    c["frame_save: out of 40 records for all"] = lambda: V.check_frame_save(fw, fn, out=fstore[0, :40])
    c["frame_save: another width"] = lambda: V.check_frame_save(64, fn, out=fstore[0])
    c["frame_save: a strided block"] = lambda: V.check_frame_save(fw, fn, out=fstore[:, 0])
    c["frame_save: int32 out"] = lambda: V.check_frame_save(fw, fn, out=fstore[0].to(torch.int32))
    c["frame_save: float idx"] = lambda: V.check_frame_save(fw, fn, idx=z(3))
    c["frame_save: two-dimensional idx"] = lambda: V.check_frame_save(fw, fn, idx=z((2, 2), dtype=torch.int64))
    c["frame_save x2: float idx and another width"] = lambda: V.check_frame_save(64, fn, idx=z(3), out=fstore[0])
    c["frame_save x2: int32 out of another count"] = lambda: V.check_frame_save(fw, fn, idx=[3, 4], out=fstore[0].to(torch.int32))
    # ---- draw_frames
    dw, dl = 64, (1 << 63) | (5 << 24) | 2
    dstore = z((7, 48, dw), dtype=torch.uint8)
    recs = V.FrameRecords(dstore, dl)
    draw = lambda **kw: V.check_frame_draw(recs, dl, dw, **kw)
    u8 = lambda *s: z(s, dtype=torch.uint8)
    c["draw: a stale layout"] = lambda: V.check_frame_draw(recs, dl + 1, dw)
    c["draw: another handle"] = lambda: V.check_frame_draw(recs, dl + (1 << 24), dw)
    c["draw: records of another dtype"] = lambda: V.check_frame_draw(dstore.to(torch.int8), dl, dw)
    c["draw: records of another width"] = lambda: V.check_frame_draw(recs, dl, 128)
    c["draw: one dimension"] = lambda: V.check_frame_draw(u8(dw), dl, dw)
    c["draw: a strided view"] = lambda: V.check_frame_draw(dstore[:, ::2], dl, dw)
    c["draw: a column block"] = lambda: V.check_frame_draw(u8(8, 128)[:, :64], dl, dw)
    c["draw: no tensor"] = lambda: V.check_frame_draw(dstore.numpy(), dl, dw)
    c["draw: float picks"] = lambda: draw(pick=torch.arange(4).float())
    c["draw: bool picks"] = lambda: draw(pick=torch.ones(4, dtype=torch.bool))
    c["draw: picks in two dimensions"] = lambda: draw(pick=z((2, 2), dtype=torch.int32))
    c["draw: an unknown format"] = lambda: draw(obs_format="rgb")
    c["draw: a count beyond the records without a pick"] = lambda: draw(out=u8(337, 84, 84, 3))
    c["draw: out of another dtype"] = lambda: draw(out=z((336, 84, 84, 3), dtype=torch.float32))
    c["draw: out of another format's shape"] = lambda: draw(out=u8(336, 3, 84, 84))
    c["draw: out of another length than the pick"] = lambda: draw(pick=[1, 2], out=u8(3, 84, 84, 3))
    c["draw: a non-contiguous out"] = lambda: draw(pick=[1, 2], out=u8(4, 84, 84, 3)[::2])
    c["draw: a permuted out"] = lambda: draw(pick=[1, 2], out=u8(2, 3, 84, 84).permute(0, 3, 2, 1))
    c["draw: no records"] = lambda: V.check_frame_draw(u8(0, dw), dl, dw, pick=[0])
    c["draw: debug-view records"] = lambda: V.check_frame_draw(V.DebugFrameRecords(u8(3, 16), 5), 5, 16)
    c["draw x2: debug-view records of a stale layout"] = lambda: V.check_frame_draw(V.DebugFrameRecords(u8(3, 16), 5), 6, 16)
    c["draw x2: a stale layout and another width"] = lambda: V.check_frame_draw(recs, dl + 1, 128)
    c["draw x2: another width and an unknown format"] = lambda: V.check_frame_draw(recs, dl, 128, obs_format="rgb")
    c["draw x2: an unknown format and float picks"] = lambda: draw(obs_format="rgb", pick=torch.arange(4).float())
    c["draw x2: float picks and out of another dtype"] = lambda: draw(pick=torch.arange(4).float(), out=z((4, 84, 84, 3), dtype=torch.float32))
    c["draw x2: no records and out of another length"] = lambda: V.check_frame_draw(u8(0, dw), dl, dw, pick=[0], out=u8(2, 84, 84, 3))
    # ---- _distinct_host_index
    for name, bad in (("a list", [0, 7, 7]), ("an array", np.array([3, 2, 3])), ("a CPU tensor", torch.tensor([5, 5], dtype=torch.int32)), ("a tuple", (1, -1, 1))):
        c["distinct: " + name] = lambda bad=bad: V._distinct_host_index("save_debug_frames", bad)
    # ---- advance_traced / play(trace=...)
    def trace(adim=1, with_labels=True, **kw):
        acts = (K, N) if adim == 1 else (K, N, 2)
        ro = V.RolloutTrace(u8(K + 1, N, B), 5 << 24, z(acts, dtype=torch.int32), z(acts, dtype=torch.int32) if with_labels else None, z((K, N)),
                            z((K, N), dtype=torch.bool))
        for k, v in kw.items():
            setattr(ro, k, v)
        return ro

    buf = u8((K + 1) * N * B + 16)
    off = (-buf.data_ptr()) % 16 + 8  # 8 bytes behind a 16-byte boundary, wherever the allocator put the buffer
    skew = buf[off:off + (K + 1) * N * B].view(K + 1, N, B)
    tr = V.check_rollout_trace
    c["trace: another K"] = lambda: tr(trace(), K + 1, N, 1, B, True)
    c["trace: another N"] = lambda: tr(trace(), K, N + 1, 1, B, True)
    c["trace: another record width"] = lambda: tr(trace(), K, N, 1, 16, True)
    c["trace: frames without row 0"] = lambda: tr(trace(frames=u8(K, N, B)), K, N, 1, B, True)
    c["trace: misaligned frames"] = lambda: tr(trace(frames=skew), K, N, 1, B, False)
    c["trace: Discrete actions on a MultiDiscrete id"] = lambda: tr(trace(1), K, N, 2, B, True)
    c["trace: int64 actions"] = lambda: tr(trace(actions=z((K, N), dtype=torch.int64)), K, N, 1, B, True)
    c["trace: float labels"] = lambda: tr(trace(labels=z((K, N))), K, N, 1, B, True)
    c["trace: float64 reward"] = lambda: tr(trace(reward=z((K, N), dtype=torch.float64)), K, N, 1, B, False)
    c["trace: uint8 done"] = lambda: tr(trace(done=u8(K, N)), K, N, 1, B, False)
    c["trace: a strided view"] = lambda: tr(trace(reward=z((K, 2 * N))[:, ::2]), K, N, 1, B, False)
    c["trace: a numpy array"] = lambda: tr(trace(reward=z((K, N)).numpy()), K, N, 1, B, False)
    c["trace: another device"] = lambda: tr(trace(), K, N, 1, B, True, device=CUDA0)
    c["trace: FrameRecords"] = lambda: tr(V.FrameRecords(u8(K + 1, N, B), 0), K, N, 1, B, True)
    c["trace: True"] = lambda: tr(True, K, N, 1, B, False)
    c["trace x2: misaligned frames on another device"] = lambda: tr(trace(frames=skew), K, N, 1, B, False, device=CUDA0)
    c["trace x2: float64 reward and uint8 done"] = lambda: tr(trace(reward=z((K, N), dtype=torch.float64), done=u8(K, N)), K, N, 1, B, False)
    c["trace x2: uint8 done and int64 actions"] = lambda: tr(trace(done=u8(K, N), actions=z((K, N), dtype=torch.int64)), K, N, 1, B, True)
    # ---- RolloutTrace.draw (env=None would raise AttributeError if the handle were touched)
    c["trace.draw: t and i of two lengths"] = lambda: trace().draw(None, [0, 1], [0])
    c["trace.draw: a float t"] = lambda: trace().draw(None, [0.5], [0])
    c["trace.draw: no frames"] = lambda: trace(frames=None).draw(None, [0], [0])
    c["trace.draw: a store beyond an int32"] = lambda: trace(frames=u8(1).expand(1 << 16, 1 << 15, B)).draw(None, [0], [0])
    c["trace.draw x2: no frames and a float t"] = lambda: trace(frames=None).draw(None, [0.5], [0])
    c["trace.draw x2: a float t and two lengths"] = lambda: trace().draw(None, [0.5, 1.0], [0])
    c["trace.draw x2: a float i and a two-dimensional t"] = lambda: trace().draw(None, [[0, 1]], [0.5])
    # ---- split_episodes
    done = z((K, N), dtype=torch.bool)
    strided = z((K, 2 * N), dtype=torch.bool)[:, ::2]
    sp = V.check_split_episodes
    c["split: float done"] = lambda: sp(z((K, N)), 4, N)
    c["split: one-dimensional done"] = lambda: sp(z(K * N, dtype=torch.bool), 4, N)
    c["split: another N"] = lambda: sp(done, 4, N + 1)
    c["split: K = 0"] = lambda: sp(z((0, N), dtype=torch.bool), 4, N)
    c["split: a strided done"] = lambda: sp(strided, 4, N)
    c["split: a numpy done"] = lambda: sp(done.numpy(), 4, N)
    c["split: length 0"] = lambda: sp(done, 0, N)
    c["split: length 2.5"] = lambda: sp(done, 2.5, N)
    c["split: length True"] = lambda: sp(done, True, N)
    c["split: float steps"] = lambda: sp(done, 4, N, z(N))
    c["split: short steps"] = lambda: sp(done, 4, N, z(N - 1, dtype=torch.int32))
    c["split: int starts"] = lambda: sp(done, 4, N, None, z(N, dtype=torch.int32))
    c["split: short starts"] = lambda: sp(done, 4, N, None, z(N - 1, dtype=torch.bool))
    c["split: negative capacity"] = lambda: sp(done, 4, N, None, None, -1)
    c["split: float capacity"] = lambda: sp(done, 4, N, None, None, 3.0)
    c["split: another device"] = lambda: sp(done, 4, N, device=CUDA0)
    c["split: steps on another device"] = lambda: sp(done.to("meta"), 4, N, z(N, dtype=torch.int32), device=torch.device("meta"))
    c["split: starts on another device"] = lambda: sp(done.to("meta"), 4, N, None, z(N, dtype=torch.bool), device=torch.device("meta"))
    c["split: a broadcast view beyond an int32"] = lambda: sp(z(1, dtype=torch.bool).expand(4, 1 << 29), 4, 1 << 29)
    c["split x2: a float done of another N"] = lambda: sp(z((K, N)), 4, N + 1)
    c["split x2: length 0 with a strided done"] = lambda: sp(strided, 0, N)
    c["split x2: length 0 on another device"] = lambda: sp(done, 0, N, device=CUDA0)
    c["split x2: another device and float steps"] = lambda: sp(done, 4, N, z(N), device=CUDA0)
    c["split x2: float steps and int starts"] = lambda: sp(done, 4, N, z(N), z(N, dtype=torch.int32))
    c["split x2: short starts and a negative capacity"] = lambda: sp(done, 4, N, None, z(N - 1, dtype=torch.bool), -1)
    # ---- episode_positions / episode_windows
    ew = V.check_episode_windows
    c["windows: float done"] = lambda: ew(z((K, N)), 4, N)
    c["windows: one-dimensional done"] = lambda: ew(z(K * N, dtype=torch.bool), 4, N)
    c["windows: another N"] = lambda: ew(done, 4, N + 1)
    c["windows: K = 0"] = lambda: ew(z((0, N), dtype=torch.bool), 4, N)
    c["windows: a strided done"] = lambda: ew(strided, 4, N)
    c["windows: a numpy done"] = lambda: ew(done.numpy(), 4, N)
    c["windows: window 0"] = lambda: ew(done, 0, N)
    c["windows: window 2.5"] = lambda: ew(done, 2.5, N)
    c["windows: window True"] = lambda: ew(done, True, N)
    c["windows: lag -1"] = lambda: ew(done, 4, N, -1)
    c["windows: lag 1.0"] = lambda: ew(done, 4, N, 1.0)
    c["windows: back -1"] = lambda: ew(done, 4, N, 0, -1)
    c["windows: float steps"] = lambda: ew(done, 4, N, 0, 0, z(N))
    c["windows: short steps"] = lambda: ew(done, 4, N, 0, 0, z(N - 1, dtype=torch.int32))
    c["windows: float pos0"] = lambda: ew(done, 4, N, 0, 0, None, z(N))
    c["windows: pos0 [K + 1, N]"] = lambda: ew(done, 4, N, 0, 0, None, z((K + 1, N), dtype=torch.int32))
    c["windows: a back beyond the int32 of a pick"] = lambda: ew(done, 4, N, 0, 2**31 // N)
    c["windows: another device"] = lambda: ew(done, 4, N, device=CUDA0)
    c["windows: pos0 on another device"] = lambda: ew(done.to("meta"), 4, N, 0, 0, None, z(N, dtype=torch.int32), device=torch.device("meta"))
    c["windows: a broadcast view beyond an int32"] = lambda: ew(z(1, dtype=torch.bool).expand(4, 1 << 29), 4, 1 << 29)
    c["windows x2: a float done of another N"] = lambda: ew(z((K, N)), 4, N + 1)
    c["windows x2: window 0 with a strided done"] = lambda: ew(strided, 0, N)
    c["windows x2: lag -1 and back -1"] = lambda: ew(done, 4, N, -1, -1)
    c["windows x2: a strided done on another device"] = lambda: ew(strided, 4, N, device=CUDA0)
    c["windows x2: another device and float steps"] = lambda: ew(done, 4, N, 0, 0, z(N), device=CUDA0)
    c["windows x2: float steps and float pos0"] = lambda: ew(done, 4, N, 0, 0, z(N), z(N))
    # ---- gather_rows
    x = torch.arange(40, dtype=torch.float32).view(10, 2, 2)
    gr = V.check_gather_rows
    c["gather_rows: a strided x"] = lambda: gr(x[:, :, 0], [0])
    c["gather_rows: a scalar x"] = lambda: gr(z(()), [0])
    c["gather_rows: rows without a byte"] = lambda: gr(z((4, 0)), [0])
    c["gather_rows: a float pick"] = lambda: gr(x, z(3))
    c["gather_rows: a float list"] = lambda: gr(x, [0.5])
    c["gather_rows: a numpy x"] = lambda: gr(x.numpy(), [0])
    c["gather_rows: out of another dtype"] = lambda: gr(x, [0, 1], z((2, 2, 2), dtype=torch.float64))
    c["gather_rows: out of another shape"] = lambda: gr(x, [0, 1], z((3, 2, 2)))
    c["gather_rows: a strided out"] = lambda: gr(x, [0, 1], z((2, 2, 4))[:, :, ::2])
    c["gather_rows: another device"] = lambda: gr(x, [0], device=CUDA0)
    c["gather_rows x2: rows without a byte on another device"] = lambda: gr(z((4, 0)), [0], device=CUDA0)
    c["gather_rows x2: another device and a float pick"] = lambda: gr(x, z(3), device=CUDA0)
    c["gather_rows x2: a float pick and out of another dtype"] = lambda: gr(x, z(3), z((3, 2, 2), dtype=torch.float64))
    # ---- draw_windows' layout checks
    pos = torch.arange((K + 1) * N, dtype=torch.int32).view(K + 1, N)
    w0, w3 = V.EpisodeWindows(pos, 4, 0, 0, K, N), V.EpisodeWindows(pos, 4, 1, 3, K, N)
    frames = u8(K + 1, N, B)
    only = lambda f: V.RolloutTrace(f, 5, None, None, None, None)
    wf = V.check_window_frames
    c["window_frames: a trace with back > 0"] = lambda: wf(only(frames), w3, B)
    c["window_frames: a [K + 1] store with back > 0"] = lambda: wf(frames, w3, B)
    c["window_frames: a [back + K + 1] store with back = 0"] = lambda: wf(V.FrameRecords(u8(3 + K + 1, N, B), 5), w0, B)
    c["window_frames: a trace of another K"] = lambda: wf(only(u8(K + 2, N, B)), w0, B)
    c["window_frames: a trace of another N"] = lambda: wf(only(u8(K + 1, N + 1, B)), w0, B)
    c["window_frames: a trace without frames"] = lambda: wf(V.RolloutTrace(None, 5, None, None, z((K, N)), None), w0, B)
    c["window_frames: records of another width"] = lambda: wf(frames, w0, 16)
    c["window_frames: an int32 store"] = lambda: wf(frames.to(torch.int32), w0, B)
    c["window_frames: a strided store"] = lambda: wf(u8(K + 1, N, 2 * B)[:, :, ::2], w0, B)
    c["window_frames: sequences instead of windows"] = lambda: wf(frames, "windows", B)
    c["window_frames x2: no windows and a trace without frames"] = lambda: wf(V.RolloutTrace(None, 5, None, None, z((K, N)), None), "windows", B)
    c["window_frames x2: back > 0 and a trace without frames"] = lambda: wf(V.RolloutTrace(None, 5, None, None, z((K, N)), None), w3, B)
    c["window_frames x2: a trace of another K whose frames have two dimensions"] = lambda: wf(only(u8(K + 2, N)), w0, B)
    # ---- EpisodeSequences / EpisodeWindows without a handle
    seqs = V.EpisodeSequences(z((5, 4), dtype=torch.int32), torch.tensor([5], dtype=torch.int32), 4, K, N)
    over = V.EpisodeSequences(z((5, 4), dtype=torch.int32), torch.tensor([6], dtype=torch.int32), 4, K, N)
    c["sequences: len beyond the table"] = lambda: len(over)
    c["sequences.picks: no handle"] = lambda: seqs.picks()
    c["sequences.picks x2: no handle, sel and m"] = lambda: seqs.picks(sel=[0.5], m=True)
    c["sequences.gather: x of K + 2 rows"] = lambda: seqs.gather(z((K + 2, N)))
    c["sequences.gather: x of another N"] = lambda: seqs.gather(z((K, N + 1)))
    c["sequences.gather: a one-dimensional x"] = lambda: seqs.gather(z(K))
    c["sequences.gather: a numpy x"] = lambda: seqs.gather(z((K, N)).numpy())
    c["sequences.gather: no handle"] = lambda: seqs.gather(z((K, N)))
    c["sequences.gather x2: a wrong x and no handle"] = lambda: seqs.gather(z((K + 2, N)), sel=[0.5])
    xs = z((K + 1, N, 5))
    c["windows.picks: no handle"] = lambda: w0.picks()
    c["windows.picks x2: no handle, sel and m"] = lambda: w0.picks(sel=[0.5], m=-1)
    c["windows.store: back > 0 without a prefix"] = lambda: w3.store(xs)
    c["windows.store: a prefix of another length"] = lambda: w3.store(xs, z((2, N, 5)))
    c["windows.store: a prefix of another dtype"] = lambda: w3.store(xs, z((3, N, 5), dtype=torch.float64))
    c["windows.store: back = 0 with a prefix"] = lambda: w0.store(xs, z((3, N, 5)))
    c["windows.store: x of K + 2 rows"] = lambda: w0.store(z((K + 2, N)))
    c["windows.store: x of another N"] = lambda: w0.store(z((K, N + 1)))
    c["windows.store: a one-dimensional x"] = lambda: w0.store(z(K))
    c["windows.store x2: a wrong x and no prefix"] = lambda: w3.store(z((K + 2, N)))
    c["windows.gather: back > 0 without a prefix"] = lambda: w3.gather(xs)
    c["windows.gather: no handle"] = lambda: w3.gather(xs, prefix=z((3, N, 5)))
    c["windows.gather x2: a wrong prefix and no handle"] = lambda: w3.gather(xs, sel=[0.5], prefix=z((2, N, 5)))
    return c


def outcome(call):
    try:
        call()
    except Exception as e:  # (every one of them is expected to be a ValueError: the table says so)
        return (type(e).__name__, str(e))
    return ("accepted", "")


def _own(cls):
    """the public attributes a class gets from this package (its own and those of its bases here), name -> what it is"""
    out = {}
    for k in reversed(cls.__mro__):
        if not k.__module__.startswith("memory_gym_amd"):
            continue
        for name, v in vars(k).items():
            if name.startswith("_"):
                continue
            if isinstance(v, property):
                out[name] = "property"
            elif isinstance(v, (staticmethod, classmethod)) or callable(v):
                out[name] = str(inspect.signature(getattr(cls, name)))
            else:
                out[name] = "attribute"
    return out


def _public(module):
    return sorted(k for k, v in vars(module).items() if not k.startswith("_") and not inspect.ismodule(v))


def surface():
    import memory_gym_amd
    from memory_gym_amd import vec_env as V
    from memory_gym_amd.vector import GymnasiumVectorEnv

    values = (V.InstanceSnapshot, V.FrameRecords, V.DebugFrameRecords, V.RolloutTrace, V.EpisodeSequences, V.EpisodeWindows)
    s = {c.__name__: _own(c) for c in (V.VecMemoryGym, V.MemoryGymEnv, GymnasiumVectorEnv) + values}
    for c in (V.VecMemoryGym, V.MemoryGymEnv, GymnasiumVectorEnv) + values:
        s[c.__name__]["__init__"] = str(inspect.signature(c.__init__))
    s["__slots__"] = {c.__name__: tuple(c.__slots__) for c in values}
    s["memory_gym_amd"] = _public(memory_gym_amd)
    s["memory_gym_amd.vec_env"] = _public(V) + ["_distinct_host_index"]
    return s


_LOAD_LAYOUT = ("load_instances: the snapshot (layout 0x5000002) was taken from another handle, or before this handle's geometry was rebuilt (layout 0x%x): "
                "records are valid for the handle and the geometry they were saved under")
_DRAW_LAYOUT = ("draw_frames: the records (layout 0x8000000005000002) were saved from another handle, or before something changed that they would draw "
                "differently (layout 0x%x now): frame records are valid for the handle and the atlas they were saved under")
_TRACE = "%s: trace.%s must be a contiguous %s tensor of shape %s (a trace of %d steps of %d instances), got %s"
_DONE = "%s: done must be a contiguous bool or uint8 tensor [K, N]"
_FORMATS = "draw_frames: obs_format must be one of ['bf16_chw', 'f16_chw', 'f32_chw', 'u8_chw', 'u8_xyc']"
_TWICE = "save_debug_frames: idx names an instance more than once (entries must be distinct; negative entries are padding)"
_STEPS = "split_episodes: steps must be an int32 or int64 tensor [70] (e.g. what play() returned as steps_played)"
_STORE = "draw_windows: frames must be a contiguous uint8 store of shape %s (back + K + 1 rows of N records)"
_BACK3 = "draw_windows: back = 3: a trace holds no rows of the previous rollout; pass a FrameRecords / uint8 store of [3 + 6 + 1, 70, 64] rows"
_X = "%s: x must be a tensor [6 or 7, 70, ...]"
_PREFIX = "EpisodeWindows.gather: prefix must be a torch.float32 tensor of shape (3, 70, 5) on cpu"
_NEED_PREFIX = "EpisodeWindows.gather: back = 3: a prefix [3, 70, ...] is required (the last rows of the previous rollout)"

# name -> the message of the ValueError the call raised when this table was recorded (every one of the calls raised a ValueError)
EXPECTED = {
    "load: another handle": _LOAD_LAYOUT % 0x6000002,
    "load: a stale layout": _LOAD_LAYOUT % 0x5000003,
    "load: a wrong record width": "load_instances: snapshot.records must be a contiguous uint8 tensor [k, 464]",
    "load: no snapshot": "load_instances: need the InstanceSnapshot save_instances returned",
    "load: float indices": "load_instances: idx must be an int32 or int64 tensor, got torch.float32",
    "load: bool indices": "load_instances: idx must be an int32 or int64 tensor, got torch.bool",
    "load: a list of floats": "load_instances: idx must hold integers, got dtype float64",
    "load: two dimensions": "load_instances: idx must have one dimension, got shape (5, 13)",
    "load: rec of another length": "load_instances: rec must have one entry per loaded instance (65), got 64",
    "load: more instances than records without rec": "load_instances: 66 instances named, the snapshot holds 65 records (pass rec= to load a record into several instances)",
    "load: all instances from 65 records": "load_instances: 200 instances named, the snapshot holds 65 records (pass rec= to load a record into several instances)",
    "load: records of another dtype": "load_instances: snapshot.records must be a contiguous uint8 tensor [k, 448]",
    "load: set_of of another length": "load_instances: snapshot.set_of must have one entry per record",
    "load x2: a stale layout and a wrong record width": _LOAD_LAYOUT % 0x5000003,
    "load x2: a wrong record width and float indices": "load_instances: snapshot.records must be a contiguous uint8 tensor [k, 464]",
    "load x2: float idx and a two-dimensional rec": "load_instances: idx must be an int32 or int64 tensor, got torch.float32",
    "load x2: rec of another length and set_of of another length": "load_instances: rec must have one entry per loaded instance (65), got 64",
    "save: out of two records for three": "save_instances: out.records must be a contiguous uint8 tensor [2, 448]",
    "save: out of three records for all": "save_instances: out.records must be a contiguous uint8 tensor [200, 448]",
    "save: out of another width": "save_instances: out.records must be a contiguous uint8 tensor [3, 464]",
    "save: out is a tensor": "save_instances: out must be an InstanceSnapshot",
    "save: float idx": "save_instances: idx must be an int32 or int64 tensor, got torch.float32",
    "save x2: float idx and out is a tensor": "save_instances: idx must be an int32 or int64 tensor, got torch.float32",
    "save x2: two-dimensional idx and out of another width": "save_instances: idx must have one dimension, got shape (2, 2)",
    "frame_save: out of 48 records for two": "save_frames: out holds 48 records, the call saves 2",
    "frame_save: out of 40 records for all": "save_frames: out holds 40 records, the call saves 48",
    "frame_save: another width": "save_frames: out must be a contiguous uint8 tensor [..., 64]",
    "frame_save: a strided block": "save_frames: out must be a contiguous uint8 tensor [..., 16]",
    "frame_save: int32 out": "save_frames: out must be a contiguous uint8 tensor [..., 16]",
    "frame_save: float idx": "save_frames: idx must be an int32 or int64 tensor, got torch.float32",
    "frame_save: two-dimensional idx": "save_frames: idx must have one dimension, got shape (2, 2)",
    "frame_save x2: float idx and another width": "save_frames: idx must be an int32 or int64 tensor, got torch.float32",
    "frame_save x2: int32 out of another count": "save_frames: out must be a contiguous uint8 tensor [..., 16]",
    "draw: a stale layout": _DRAW_LAYOUT % 0x8000000005000003,
    "draw: another handle": _DRAW_LAYOUT % 0x8000000006000002,
    "draw: records of another dtype": "draw_frames: records must be a contiguous uint8 tensor [..., 64]",
    "draw: records of another width": "draw_frames: records must be a contiguous uint8 tensor [..., 128]",
    "draw: one dimension": "draw_frames: records must be a contiguous uint8 tensor [..., 64]",
    "draw: a strided view": "draw_frames: records must be a contiguous uint8 tensor [..., 64]",
    "draw: a column block": "draw_frames: records must be a contiguous uint8 tensor [..., 64]",
    "draw: no tensor": "draw_frames: records must be a contiguous uint8 tensor [..., 64]",
    "draw: float picks": "draw_frames: pick must be an int32 or int64 tensor, got torch.float32",
    "draw: bool picks": "draw_frames: pick must be an int32 or int64 tensor, got torch.bool",
    "draw: picks in two dimensions": "draw_frames: pick must have one dimension, got shape (2, 2)",
    "draw: an unknown format": _FORMATS,
    "draw: a count beyond the records without a pick": "draw_frames: out must be a contiguous torch.uint8 tensor of shape (336, 84, 84, 3)",
    "draw: out of another dtype": "draw_frames: out must be a contiguous torch.uint8 tensor of shape (336, 84, 84, 3)",
    "draw: out of another format's shape": "draw_frames: out must be a contiguous torch.uint8 tensor of shape (336, 84, 84, 3)",
    "draw: out of another length than the pick": "draw_frames: out must be a contiguous torch.uint8 tensor of shape (2, 84, 84, 3)",
    "draw: a non-contiguous out": "draw_frames: out must be a contiguous torch.uint8 tensor of shape (2, 84, 84, 3)",
    "draw: a permuted out": "draw_frames: out must be a contiguous torch.uint8 tensor of shape (2, 84, 84, 3)",
    "draw: no records": "draw_frames: no records to draw from",
    "draw: debug-view records": "draw_frames: these are debug-view records (save_debug_frames): draw_debug_frames draws them",
    "draw x2: debug-view records of a stale layout": "draw_frames: these are debug-view records (save_debug_frames): draw_debug_frames draws them",
    "draw x2: a stale layout and another width": _DRAW_LAYOUT % 0x8000000005000003,
    "draw x2: another width and an unknown format": "draw_frames: records must be a contiguous uint8 tensor [..., 128]",
    "draw x2: an unknown format and float picks": _FORMATS,
    "draw x2: float picks and out of another dtype": "draw_frames: pick must be an int32 or int64 tensor, got torch.float32",
    "draw x2: no records and out of another length": "draw_frames: no records to draw from",
    "distinct: a list": _TWICE,
    "distinct: an array": _TWICE,
    "distinct: a CPU tensor": _TWICE,
    "distinct: a tuple": _TWICE,
    "trace: another K": _TRACE % ("advance_traced", "frames", "torch.uint8", "(8, 70, 64)", 7, 70, "torch.uint8 (7, 70, 64)"),
    "trace: another N": _TRACE % ("advance_traced", "frames", "torch.uint8", "(7, 71, 64)", 6, 71, "torch.uint8 (7, 70, 64)"),
    "trace: another record width": _TRACE % ("advance_traced", "frames", "torch.uint8", "(7, 70, 16)", 6, 70, "torch.uint8 (7, 70, 64)"),
    "trace: frames without row 0": _TRACE % ("advance_traced", "frames", "torch.uint8", "(7, 70, 64)", 6, 70, "torch.uint8 (6, 70, 64)"),
    "trace: misaligned frames": "play(trace=...): trace.frames must be 16-byte aligned",
    "trace: Discrete actions on a MultiDiscrete id": _TRACE % ("advance_traced", "actions", "torch.int32", "(6, 70, 2)", 6, 70, "torch.int32 (6, 70)"),
    "trace: int64 actions": _TRACE % ("advance_traced", "actions", "torch.int32", "(6, 70)", 6, 70, "torch.int64 (6, 70)"),
    "trace: float labels": _TRACE % ("advance_traced", "labels", "torch.int32", "(6, 70)", 6, 70, "torch.float32 (6, 70)"),
    "trace: float64 reward": _TRACE % ("play(trace=...)", "reward", "torch.float32", "(6, 70)", 6, 70, "torch.float64 (6, 70)"),
    "trace: uint8 done": _TRACE % ("play(trace=...)", "done", "torch.bool", "(6, 70)", 6, 70, "torch.uint8 (6, 70)"),
    "trace: a strided view": _TRACE % ("play(trace=...)", "reward", "torch.float32", "(6, 70)", 6, 70, "torch.float32 (6, 70)"),
    "trace: a numpy array": _TRACE % ("play(trace=...)", "reward", "torch.float32", "(6, 70)", 6, 70, "ndarray"),
    "trace: another device": "advance_traced: trace.frames is on cpu, the handle on cuda:0",
    "trace: FrameRecords": "advance_traced: need the RolloutTrace new_rollout returned",
    "trace: True": "play(trace=...): need the RolloutTrace new_rollout returned",
    "trace x2: misaligned frames on another device": "play(trace=...): trace.frames is on cpu, the handle on cuda:0",
    "trace x2: float64 reward and uint8 done": _TRACE % ("play(trace=...)", "reward", "torch.float32", "(6, 70)", 6, 70, "torch.float64 (6, 70)"),
    "trace x2: uint8 done and int64 actions": _TRACE % ("advance_traced", "done", "torch.bool", "(6, 70)", 6, 70, "torch.uint8 (6, 70)"),
    "trace.draw: t and i of two lengths": "RolloutTrace.draw: t and i must have one length, got 2 and 1",
    "trace.draw: a float t": "RolloutTrace.draw: t must hold integers, got dtype float64",
    "trace.draw: no frames": "RolloutTrace.draw: frames must be a uint8 tensor [K + 1, N, frame_record_bytes] (this trace keeps no frames?)",
    "trace.draw: a store beyond an int32": "RolloutTrace.draw: the store holds 65536 x 32768 records, draw_frames takes at most 2147483647: draw from slices of `frames`",
    "trace.draw x2: no frames and a float t": "RolloutTrace.draw: frames must be a uint8 tensor [K + 1, N, frame_record_bytes] (this trace keeps no frames?)",
    "trace.draw x2: a float t and two lengths": "RolloutTrace.draw: t must hold integers, got dtype float64",
    "trace.draw x2: a float i and a two-dimensional t": "RolloutTrace.draw: t must have one dimension, got shape (1, 2)",
    "split: float done": _DONE % "split_episodes",
    "split: one-dimensional done": _DONE % "split_episodes",
    "split: another N": "split_episodes: done is (6, 70), need [K >= 1, 71] (the handle's instances)",
    "split: K = 0": "split_episodes: done is (0, 70), need [K >= 1, 70] (the handle's instances)",
    "split: a strided done": _DONE % "split_episodes",
    "split: a numpy done": _DONE % "split_episodes",
    "split: length 0": "split_episodes: length must be an integer >= 1, got 0",
    "split: length 2.5": "split_episodes: length must be an integer >= 1, got 2.5",
    "split: length True": "split_episodes: length must be an integer >= 1, got True",
    "split: float steps": _STEPS,
    "split: short steps": _STEPS,
    "split: int starts": "split_episodes: starts must be a contiguous bool or uint8 tensor [70]",
    "split: short starts": "split_episodes: starts must be a contiguous bool or uint8 tensor [70]",
    "split: negative capacity": "split_episodes: capacity must be an integer >= 0, got -1",
    "split: float capacity": "split_episodes: capacity must be an integer >= 0, got 3.0",
    "split: another device": "split_episodes: done is on cpu, the handle on cuda:0",
    "split: steps on another device": "split_episodes: steps is on cpu, the handle on meta",
    "split: starts on another device": "split_episodes: starts is on cpu, the handle on meta",
    "split: a broadcast view beyond an int32": "split_episodes: (K + 1) * N = 2684354560 does not fit the int32 of a pick: split slices of the rollout",
    "split x2: a float done of another N": _DONE % "split_episodes",
    "split x2: length 0 with a strided done": _DONE % "split_episodes",
    "split x2: length 0 on another device": "split_episodes: length must be an integer >= 1, got 0",
    "split x2: another device and float steps": "split_episodes: done is on cpu, the handle on cuda:0",
    "split x2: float steps and int starts": _STEPS,
    "split x2: short starts and a negative capacity": "split_episodes: starts must be a contiguous bool or uint8 tensor [70]",
    "windows: float done": _DONE % "episode_windows",
    "windows: one-dimensional done": _DONE % "episode_windows",
    "windows: another N": "episode_windows: done is (6, 70), need [K >= 1, 71] (the handle's instances)",
    "windows: K = 0": "episode_windows: done is (0, 70), need [K >= 1, 70] (the handle's instances)",
    "windows: a strided done": _DONE % "episode_windows",
    "windows: a numpy done": _DONE % "episode_windows",
    "windows: window 0": "episode_windows: window must be an integer >= 1, got 0",
    "windows: window 2.5": "episode_windows: window must be an integer >= 1, got 2.5",
    "windows: window True": "episode_windows: window must be an integer >= 1, got True",
    "windows: lag -1": "episode_windows: lag must be an integer >= 0, got -1",
    "windows: lag 1.0": "episode_windows: lag must be an integer >= 0, got 1.0",
    "windows: back -1": "episode_windows: back must be an integer >= 0, got -1",
    "windows: float steps": "episode_windows: steps must be an int32 or int64 tensor [70]",
    "windows: short steps": "episode_windows: steps must be an int32 or int64 tensor [70]",
    "windows: float pos0": "episode_windows: pos0 must be an int32 or int64 tensor [70]",
    "windows: pos0 [K + 1, N]": "episode_windows: pos0 must be an int32 or int64 tensor [70]",
    "windows: a back beyond the int32 of a pick": "episode_windows: (back + K + 1) * N = 2147484080 does not fit the int32 of a pick: take slices of the rollout",
    "windows: another device": "episode_windows: done is on cpu, the handle on cuda:0",
    "windows: pos0 on another device": "episode_windows: pos0 is on cpu, the handle on meta",
    "windows: a broadcast view beyond an int32": "episode_windows: (back + K + 1) * N = 2684354560 does not fit the int32 of a pick: take slices of the rollout",
    "windows x2: a float done of another N": _DONE % "episode_windows",
    "windows x2: window 0 with a strided done": "episode_windows: window must be an integer >= 1, got 0",
    "windows x2: lag -1 and back -1": "episode_windows: lag must be an integer >= 0, got -1",
    "windows x2: a strided done on another device": _DONE % "episode_windows",
    "windows x2: another device and float steps": "episode_windows: done is on cpu, the handle on cuda:0",
    "windows x2: float steps and float pos0": "episode_windows: steps must be an int32 or int64 tensor [70]",
    "gather_rows: a strided x": "gather_rows: x must be a contiguous tensor [R, ...]",
    "gather_rows: a scalar x": "gather_rows: x must be a contiguous tensor [R, ...]",
    "gather_rows: rows without a byte": "gather_rows: a row of x (4, 0) holds no byte",
    "gather_rows: a float pick": "gather_rows: pick must be an int32 or int64 tensor, got torch.float32",
    "gather_rows: a float list": "gather_rows: pick must hold integers, got dtype float64",
    "gather_rows: a numpy x": "gather_rows: x must be a contiguous tensor [R, ...]",
    "gather_rows: out of another dtype": "gather_rows: out must be a contiguous torch.float32 tensor of shape (2, 2, 2) on cpu",
    "gather_rows: out of another shape": "gather_rows: out must be a contiguous torch.float32 tensor of shape (2, 2, 2) on cpu",
    "gather_rows: a strided out": "gather_rows: out must be a contiguous torch.float32 tensor of shape (2, 2, 2) on cpu",
    "gather_rows: another device": "gather_rows: x is on cpu, the handle on cuda:0",
    "gather_rows x2: rows without a byte on another device": "gather_rows: a row of x (4, 0) holds no byte",
    "gather_rows x2: another device and a float pick": "gather_rows: x is on cpu, the handle on cuda:0",
    "gather_rows x2: a float pick and out of another dtype": "gather_rows: pick must be an int32 or int64 tensor, got torch.float32",
    "window_frames: a trace with back > 0": _BACK3,
    "window_frames: a [K + 1] store with back > 0": _STORE % "(10, 70, 64)",
    "window_frames: a [back + K + 1] store with back = 0": _STORE % "(7, 70, 64)",
    "window_frames: a trace of another K": "draw_windows: the trace holds 7 steps of 70 instances, the windows were made from 6 steps of 70",
    "window_frames: a trace of another N": "draw_windows: the trace holds 6 steps of 71 instances, the windows were made from 6 steps of 70",
    "window_frames: a trace without frames": "draw_windows: the trace keeps no frames",
    "window_frames: records of another width": _STORE % "(7, 70, 16)",
    "window_frames: an int32 store": _STORE % "(7, 70, 64)",
    "window_frames: a strided store": _STORE % "(7, 70, 64)",
    "window_frames: sequences instead of windows": "draw_windows: windows must be the EpisodeWindows episode_windows returned",
    "window_frames x2: no windows and a trace without frames": "draw_windows: windows must be the EpisodeWindows episode_windows returned",
    "window_frames x2: back > 0 and a trace without frames": _BACK3,
    "window_frames x2: a trace of another K whose frames have two dimensions": "draw_windows: the trace keeps no frames",
    "sequences: len beyond the table": "EpisodeSequences: the rollout has 6 sequences, the table holds 5: split again with capacity >= 6",
    "sequences.picks: no handle": "EpisodeSequences.picks: these sequences belong to no handle",
    "sequences.picks x2: no handle, sel and m": "EpisodeSequences.picks: these sequences belong to no handle",
    "sequences.gather: x of K + 2 rows": _X % "EpisodeSequences.gather",
    "sequences.gather: x of another N": _X % "EpisodeSequences.gather",
    "sequences.gather: a one-dimensional x": _X % "EpisodeSequences.gather",
    "sequences.gather: a numpy x": _X % "EpisodeSequences.gather",
    "sequences.gather: no handle": "EpisodeSequences.picks: these sequences belong to no handle",
    "sequences.gather x2: a wrong x and no handle": _X % "EpisodeSequences.gather",
    "windows.picks: no handle": "EpisodeWindows.picks: these windows belong to no handle",
    "windows.picks x2: no handle, sel and m": "EpisodeWindows.picks: these windows belong to no handle",
    "windows.store: back > 0 without a prefix": _NEED_PREFIX,
    "windows.store: a prefix of another length": _PREFIX,
    "windows.store: a prefix of another dtype": _PREFIX,
    "windows.store: back = 0 with a prefix": "EpisodeWindows.gather: back = 0: there is no room for a prefix",
    "windows.store: x of K + 2 rows": _X % "EpisodeWindows.gather",
    "windows.store: x of another N": _X % "EpisodeWindows.gather",
    "windows.store: a one-dimensional x": _X % "EpisodeWindows.gather",
    "windows.store x2: a wrong x and no prefix": _X % "EpisodeWindows.gather",
    "windows.gather: back > 0 without a prefix": _NEED_PREFIX,
    "windows.gather: no handle": "EpisodeWindows.gather: these windows belong to no handle",
    "windows.gather x2: a wrong prefix and no handle": _PREFIX,
}

_RECORD_CALLS = {"frame_record_bytes": "property", "frame_layout": "(self)", "save_frames": "(self, idx=None, out=None)",
                 "draw_frames": "(self, records, pick=None, out=None, obs_format=None)",
                 "split_episodes": "(self, done, length, steps=None, starts=None, capacity=None)",
                 "draw_frames_padded": "(self, records, pick, out=None, obs_format=None)",
                 "draw_sequences": "(self, frames, seqs, sel=None, out=None, obs_format=None)", "episode_positions": "(self, done, steps=None, pos0=None)",
                 "episode_windows": "(self, done, window, lag=0, back=0, steps=None, pos0=None)", "gather_rows": "(self, x, pick, out=None)",
                 "draw_windows": "(self, frames, windows, sel=None, out=None, obs_format=None)", "DEBUG_SIZES": "attribute",
                 "save_debug_frames": "(self, idx=None, out=None)", "draw_debug_frames": "(self, records, pick=None, out=None, size=336)"}
_KEPT = {"new_rollout": "(self, steps, labels=False)", "advance": "(self, steps, eps=0.0, seed=0, step=None, render=True, stats=True)",
         "advance_traced": "(self, trace, eps=0.0, seed=0, step=None, render=True, stats=True)",
         "play": "(self, actions, until_done=False, mask=None, render=True, stats=True, trace=False)",
         "expert_actions": "(self, eps=0.0, seed=0, step=None, out=None)", "save_instances": "(self, idx=None, out=None)",
         "load_instances": "(self, snap, idx=None, rec=None, render=True)", "copy_instances": "(self, src, dst, render=True)", "redraw": "(self)"}
_FORWARDED = ("split_episodes", "draw_frames_padded", "draw_sequences", "episode_positions", "episode_windows", "gather_rows", "draw_windows")

# what surface() gave when this table was recorded
SURFACE = {
    "VecMemoryGym": dict(_RECORD_CALLS, **_KEPT, **{
        "metadata": "attribute", "OBS_FORMATS": "attribute", "AUTORESET_MODES": "attribute",
        "reset": "(self, seed=None, return_info=True, options=None, mask=None)", "step": "(self, actions, render=True, mask=None)",
        "autoreset_mode": "property", "instance_bytes": "property", "instance_layout": "property", "new_obs_buffer": "(self)",
        "use_obs_buffer": "(self, tensor)", "use_step_buffers": "(self, reward, done_u8)", "render": "(self)", "render_debug": "(self)",
        "state_dict": "(self)", "load_state_dict": "(self, sd)", "set_profiling": "(self, every)", "get_profile": "(self, kind)",
        "CAPACITY_BITS": "attribute", "ERROR_BITS": "attribute", "check_errors": "(self)", "rng_words": "(self, i)",
        "set_rng_words": "(self, i, words)", "debug_counter": "(self, name)", "close": "(self)",
        "__init__": "(self, env_id, num_envs=1, device=None, render_mode=None, obs_format='u8_xyc', final_observation=False, obs_buffer=None, "
                    "obs_placement=None, ground_truth64=False, on_capacity='raise', capacity=None, autoreset_mode='same_step', final_frames=False)"}),
    "MemoryGymEnv": {
        "metadata": "attribute", "spec": "attribute", "env_id": "attribute", "unwrapped": "property", "np_random": "property",
        "max_episode_steps": "property", "reset": "(self, seed=None, return_info=True, options=None)", "step": "(self, action)",
        "expert_action": "(self, eps=0.0, seed=0, step=None)", "render": "(self)", "state_dict": "(self)", "load_state_dict": "(self, sd)",
        "snapshot": "(self)", "restore": "(self, snap)", "close": "(self)",
        "__init__": "(self, env_id=None, device=None, render_mode=None, capacity=None)"},
    "GymnasiumVectorEnv": dict({k: _RECORD_CALLS[k] for k in _FORWARDED}, **_KEPT, **{
        "reset": "(self, seed=None, options=None)", "step": "(self, actions)", "final_observations": "(self, info, out=None, obs_format=None)",
        "step_async": "(self, actions)", "step_wait": "(self)", "reset_async": "(self, seed=None, options=None)",
        "reset_wait": "(self, seed=None, options=None)", "close": "(self, **kwargs)", "close_extras": "(self, **kwargs)", "unwrapped": "property",
        "__init__": "(self, env_id, num_envs, device=None, obs_format='u8_xyc', as_numpy=False, on_capacity='raise', capacity=None, "
                    "autoreset_mode='same_step', final_frames=False)"}),
    "InstanceSnapshot": {"count": "property", "layout": "attribute", "records": "attribute", "set_of": "attribute",
                         "__init__": "(self, records, layout, set_of=None)"},
    "FrameRecords": {"count": "property", "layout": "attribute", "records": "attribute", "__init__": "(self, records, layout)"},
    "DebugFrameRecords": {"count": "property", "layout": "attribute", "records": "attribute", "__init__": "(self, records, layout)"},
    "RolloutTrace": {"steps": "property", "num_envs": "property", "draw": "(self, env, t, i, out=None, obs_format=None)", "actions": "attribute",
                     "done": "attribute", "frame_layout": "attribute", "frames": "attribute", "labels": "attribute", "reward": "attribute",
                     "__init__": "(self, frames, frame_layout, actions, labels, reward, done)"},
    "EpisodeSequences": {"capacity": "property", "picks": "(self, sel=None, m=None)", "gather": "(self, x, sel=None)", "count": "attribute",
                         "length": "attribute", "num_envs": "attribute", "steps": "attribute", "table": "attribute",
                         "__init__": "(self, table, count, length, steps, num_envs, env=None)"},
    "EpisodeWindows": {"carry": "property", "picks": "(self, sel=None, m=None)", "store": "(self, x, prefix=None)",
                       "gather": "(self, x, sel=None, prefix=None)", "back": "attribute", "lag": "attribute", "num_envs": "attribute",
                       "pos": "attribute", "steps": "attribute", "window": "attribute",
                       "__init__": "(self, pos, window, lag, back, steps, num_envs, env=None)"},
    "__slots__": {"InstanceSnapshot": ("records", "layout", "set_of"), "FrameRecords": ("records", "layout"), "DebugFrameRecords": (),
                  "RolloutTrace": ("frames", "frame_layout", "actions", "labels", "reward", "done"),
                  "EpisodeSequences": ("table", "count", "length", "steps", "num_envs", "_env"),
                  "EpisodeWindows": ("pos", "window", "lag", "back", "steps", "num_envs", "_env")},
    "memory_gym_amd": ["DEFAULTS", "DebugFrameRecords", "ENV_IDS", "EpisodeSequences", "EpisodeWindows", "FrameRecords", "GymnasiumVectorEnv",
                       "InstanceSnapshot", "MemoryGymEnv", "RolloutTrace", "VecMemoryGym", "alloc_obs_buffer", "make", "process_reset_params"],
    "memory_gym_amd.vec_env": ["DEFAULTS", "DebugFrameRecords", "ENV_IDS", "EpisodeSequences", "EpisodeWindows", "FrameRecords", "InstanceSnapshot",
                               "MAX_DRAW_RECORDS", "MAX_PICK", "MemoryGymEnv", "RolloutTrace", "VecMemoryGym", "alloc_obs_buffer",
                               "calc_max_episode_steps", "check_episode_windows", "check_frame_draw", "check_frame_save", "check_gather_rows",
                               "check_instance_load", "check_instance_save", "check_rollout_trace", "check_split_episodes", "check_window_frames",
                               "is_balanced_buffer", "process_reset_params", "_distinct_host_index"],
}


def test_every_refusal_keeps_its_type_and_its_message():
    got = {name: outcome(call) for name, call in cases().items()}
    assert sorted(got) == sorted(EXPECTED)
    for name, want in EXPECTED.items():
        assert got[name] == ("ValueError", want), name


def test_the_surface_is_what_it_was():
    got = surface()
    for name, want in SURFACE.items():
        if name == "memory_gym_amd.vec_env":  # (what the module imports for its own use may change; every name it had stays)
            assert set(want) <= set(got[name]), sorted(set(want) - set(got[name]))
        else:
            assert got[name] == want, name


def test_the_names_of_vec_env_are_the_objects_of_their_homes():
    import memory_gym_amd
    from memory_gym_amd import vec_env as V

    for name in SURFACE["memory_gym_amd.vec_env"]:
        obj = getattr(V, name)
        home = sys.modules.get(getattr(obj, "__module__", None) or "")
        if home is not None and home is not V:  # a class or a function defined in another module of the package
            assert getattr(home, name) is obj, name
        if hasattr(memory_gym_amd, name):
            assert getattr(memory_gym_amd, name) is obj, name
    assert V.VecMemoryGym.OBS_FORMATS is getattr(sys.modules[V.check_frame_draw.__module__], "OBS_FORMATS", V.VecMemoryGym.OBS_FORMATS)
    assert V.ENV_IDS == list(memory_gym_amd.DEFAULTS)


if __name__ == "__main__":
    import os
    import pprint

    sys.path.insert(0, os.environ.get("MEMGYM_PKG") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "endless-memory-gym_amd"))
    print("EXPECTED = \\")
    pprint.pprint({k: outcome(c) for k, c in cases().items()}, width=160, sort_dicts=False)
    print("\nSURFACE = \\")
    pprint.pprint(surface(), width=160, sort_dicts=False)
