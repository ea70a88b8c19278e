"""The handle's calls over kept rollouts -- frame records, episode sequences, memory windows, debug-view records -- as the base class of VecMemoryGym.
They read the handle (`_h`, `_stream()`, `device`, `num_envs`, `obs_format`, `_require_started`) and change nothing in it."""
import torch

from . import _native
from ._args import aligned_on, ptr
from .episodes import EpisodeSequences, EpisodeWindows, check_episode_windows, check_gather_rows, check_split_episodes, check_window_frames
from .records import (OBS_FORMATS, DebugFrameRecords, FrameRecords, RolloutTrace, _distinct_host_index, _pick_count, _record_rows, check_frame_draw,
                      check_frame_save, trace_frame_records)


class RecordCalls:
    # ------------------------------------------------------------------ frame records
    @property
    def frame_record_bytes(self):
        return int(_native.LIB.mg_frame_record_bytes(self._h))

    def frame_layout(self):
        return int(_native.LIB.mg_frame_layout(self._h))

    def _save_records(self, what, save, cls, idx, out):
        """save_frames / save_debug_frames behind their first checks: `save` is the library's call, `cls` the record class it fills"""
        nbytes = self.frame_record_bytes
        idx, k, rows = check_frame_save(nbytes, self.num_envs, idx, out, self.device)
        if rows is None:
            out = rows = torch.empty((k, nbytes), dtype=torch.uint8, device=self.device)
        aligned_on(what, "out", self.device, rows)
        with torch.cuda.device(self.device):
            _native.check(save(self._h, ptr(idx), k, rows.data_ptr(), self._stream()), "mg_" + what)
        if isinstance(out, cls):
            out.layout = self.frame_layout()
            return out
        return cls(out, self.frame_layout())

    def save_frames(self, idx=None, out=None):
        """Keep the CURRENT frames as their descriptors (include/memgym.h: mg_save_frames) -> FrameRecords over a uint8 tensor [k, frame_record_bytes]:
        16 / 64 / 128 bytes per frame instead of 21,168 and more.  After step(render=False) the records hold the frames the step would have drawn.
        idx: the instances, an integer tensor / list (None: all, in order); entries < 0 are skipped (their records keep their bytes).  out: a
        FrameRecords or a uint8 tensor [k, frame_record_bytes] to write into -- a row block store[t] of a larger [T, N, bytes] store, so one store is
        filled step by step.  One small launch on the current stream; nothing synchronises, nothing of the handle changes."""
        self._require_started("save_frames")
        return self._save_records("save_frames", _native.LIB.mg_save_frames, FrameRecords, idx, out)

    def _draw_records(self, what, draw, records, pick, out, obs_format, skip_empty):
        """draw_frames / draw_frames_padded: `draw` is the library's call; skip_empty: a draw of no rows returns before the alignment check and the call"""
        self._require_started(what)
        fmt = self.obs_format if obs_format is None else obs_format
        rows, pick, count, (dt, shape) = check_frame_draw(records, self.frame_layout(), self.frame_record_bytes, pick, out, fmt, self.device)
        if out is None:
            out = torch.empty((count,) + shape, dtype=dt, device=self.device)
        if skip_empty and count == 0:  # nothing to draw (an empty tensor has no address to hand to the library)
            return out
        aligned_on(what, "records and out", self.device, rows, out)
        with torch.cuda.device(self.device):
            _native.check(draw(self._h, rows.data_ptr(), rows.shape[0], ptr(pick), count, OBS_FORMATS[fmt][0], out.data_ptr(), self._stream()), "mg_" + what)
        return out

    def draw_frames(self, records, pick=None, out=None, obs_format=None):
        """Draw kept frames (include/memgym.h: mg_draw_frames): row j of the result is the frame of record pick[j] (pick=None: record j), in
        `obs_format` (default: the handle's) -- bit for bit what `obs` showed when the record was saved, or what a handle of that format would have
        shown.  records: a FrameRecords (its layout is checked: ValueError if stale, before anything is launched) or a plain uint8 tensor, viewed as
        [n_records, frame_record_bytes].  pick: an integer tensor / list of any length, duplicates allowed; an entry outside the records leaves its row
        untouched and raises error bit 512.  out: a contiguous tensor [count] + shape of the format to draw into (a network's input tensor).  One
        raster launch on the current stream; nothing synchronises, nothing of the handle changes."""
        return self._draw_records("draw_frames", _native.LIB.mg_draw_frames, records, pick, out, obs_format, False)

    def draw_frames_padded(self, records, pick, out=None, obs_format=None):
        """draw_frames with padding rows (include/memgym.h: mg_draw_frames_padded): a pick below 0 writes its row as zeros, every byte, and is no
        error.  Everything else -- the arguments, the checks, a pick at or beyond the records (row untouched, error bit 512), the single raster
        launch -- is draw_frames; pick=None equals it."""
        return self._draw_records("draw_frames_padded", _native.LIB.mg_draw_frames_padded, records, pick, out, obs_format, True)

    def _draw_picked(self, what, frames, picks, width, out, obs_format):
        """The tail of draw_sequences / draw_windows: picks() -> (pick [M, width], ...) once the format is known to exist; -> (obs [M, width] + shape
        of the format, drawn by draw_frames_padded, and what picks() returned behind the pick)."""
        fmt = self.obs_format if obs_format is None else obs_format
        if fmt not in OBS_FORMATS:
            raise ValueError("%s: obs_format must be one of %s" % (what, sorted(OBS_FORMATS)))
        _, dt, shape = OBS_FORMATS[fmt]
        pick, *rest = picks()
        M = int(pick.shape[0])
        if out is not None:
            if not (isinstance(out, torch.Tensor) and out.dtype == dt and tuple(out.shape) == (M, width) + shape and out.is_contiguous()):
                raise ValueError("%s: out must be a contiguous %s tensor of shape %s" % (what, dt, (M, width) + shape))
            out = out.view((M * width,) + shape)
        flat = self.draw_frames_padded(frames, pick.view(-1), out=out, obs_format=fmt)
        return (flat.view((M, width) + shape), *rest)

    # ------------------------------------------------------------------ episode sequences
    def split_episodes(self, done, length, steps=None, starts=None, capacity=None):
        """Cut a rollout into episode sequences on the device (include/memgym.h: mg_split_episodes) -> EpisodeSequences.  done: a bool or uint8 tensor
        [K, N], e.g. trace.done; every episode is cut at its done and chopped into sequences of at most `length` steps, ordered by (instance, t0).
        steps: an integer tensor [N], the steps instance i took (play()'s steps_played; clamped to 0 .. K), None: K for all.  starts: a bool / uint8
        tensor [N], whether the rollout's first step starts an episode of instance i (it only sets the flag of the first sequence), None: all do.
        capacity: the rows of the table.  None allocates N * ceil(K / length) + int(done.sum()), which always suffices -- and READS done.sum() ON THE
        HOST: the one place that synchronises.  An explicit capacity synchronises nothing; the count may then exceed it (len() raises, the table holds
        the first `capacity` sequences).  Three small launches on the current stream; the handle's first call allocates an int32 per instance and
        cannot be captured into a graph, every later one can."""
        self._require_started("split_episodes")
        d8, K, L, steps, starts, capacity = check_split_episodes(done, length, self.num_envs, steps, starts, capacity, self.device)
        if capacity is None:
            capacity = self.num_envs * ((K + L - 1) // L) + int(d8.sum())
        table = torch.empty((capacity, 4), dtype=torch.int32, device=self.device)
        count = torch.empty((1,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(_native.LIB.mg_split_episodes(self._h, d8.data_ptr(), K, ptr(steps), ptr(starts), L, table.data_ptr() if capacity else None,
                                                        capacity, count.data_ptr(), self._stream()), "mg_split_episodes")
        return EpisodeSequences(table, count, L, K, self.num_envs, self)

    def draw_sequences(self, frames, seqs, sel=None, out=None, obs_format=None):
        """Frames of a minibatch of sequences -> (obs [M, L] + shape of the format, mask bool [M, L]): row (j, l) is the observation step t0 + l of
        sequence sel[j] was played in (sel=None: all sequences, M = len(seqs)), zeros where the sequence is shorter than L and for entries of sel below
        0.  frames: the RolloutTrace the sequences were cut from, or a FrameRecords / uint8 tensor over its [K + 1, N] frame store; its layout is
        checked as draw_frames checks it, and a trace whose K or N is not the sequences' is refused.  out: a contiguous tensor [M, L] + shape to draw
        into.  Two launches on the current stream: the picks, and the PAD form of the gather raster."""
        what = "draw_sequences"
        self._require_started(what)
        if not isinstance(seqs, EpisodeSequences):
            raise ValueError("%s: seqs must be the EpisodeSequences split_episodes returned" % what)
        if isinstance(frames, RolloutTrace):
            frames = trace_frame_records(what, frames, seqs.steps, seqs.num_envs, "the sequences were cut from")

        def picks():
            n_rec = (frames.records if isinstance(frames, FrameRecords) else frames)
            if isinstance(n_rec, torch.Tensor) and n_rec.dim() >= 2 and n_rec.numel() // max(1, int(n_rec.shape[-1])) < (seqs.steps + 1) * seqs.num_envs:
                raise ValueError("%s: frames holds fewer than (%d + 1) * %d records" % (what, seqs.steps, seqs.num_envs))
            return seqs.picks(sel)
        return self._draw_picked(what, frames, picks, seqs.length, out, obs_format)

    # ------------------------------------------------------------------ memory windows
    def episode_positions(self, done, steps=None, pos0=None):
        """-> int32 [K + 1, N] (include/memgym.h: mg_episode_positions): row t holds the steps instance i's episode had already taken when frame t of
        the rollout's [K + 1, N] store was shown.  done: a bool or uint8 tensor [K, N], e.g. trace.done.  steps: an integer tensor [N], the steps
        instance i took (play()'s steps_played), None: K for all.  pos0: an integer tensor [N], the positions at the rollout's first frame -- row K of
        the previous rollout's result -- None: every instance starts an episode.  One small launch on the current stream; nothing synchronises,
        nothing is allocated in the handle."""
        self._require_started("episode_positions")
        d8, K, _, _, _, steps, pos0 = check_episode_windows(done, 1, self.num_envs, 0, 0, steps, pos0, self.device)
        pos = torch.empty((K + 1, self.num_envs), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(_native.LIB.mg_episode_positions(self._h, d8.data_ptr(), K, ptr(steps), ptr(pos0), pos.data_ptr(), self._stream()), "mg_episode_positions")
        return pos

    def episode_windows(self, done, window, lag=0, back=0, steps=None, pos0=None):
        """The sliding memory windows of a rollout (include/memgym.h: MEMORY WINDOWS) -> EpisodeWindows: episode_positions(done, steps, pos0) with the
        window's shape.  window: the rows of a window.  lag: 0 -- the window of sample (t, i) ends with its own row t (windows of frames); 1 -- one row
        earlier (memories of past hidden states).  back: how many rows of the previous rollout a window may reach into; its picks then index a store
        of [back + K + 1, N] rows.  One small launch."""
        self._require_started("episode_windows")
        d8, K, window, lag, back, steps, pos0 = check_episode_windows(done, window, self.num_envs, lag, back, steps, pos0, self.device)
        return EpisodeWindows(self.episode_positions(d8, steps, pos0), window, lag, back, K, self.num_envs, self)

    def gather_rows(self, x, pick, out=None):
        """Rows of a store by index, zero rows at the pads (include/memgym.h: mg_gather_rows_padded): x [R, ...] contiguous, of any dtype and row
        length; pick: integers of any shape, or None (row j) -> pick.shape + x.shape[1:].  A pick below 0 gives a row of zeros; a pick at or beyond
        R leaves its row as it was and raises error bit 512.  out: a contiguous tensor of the result's shape and x's dtype that shares no byte
        with x.  One launch on the current stream; nothing synchronises."""
        x, pick, shape, row_bytes = check_gather_rows(x, pick, out, self.device)
        if out is None:
            out = torch.empty(shape, dtype=x.dtype, device=self.device)
        count = int(x.shape[0]) if pick is None else pick.numel()
        if count:
            with torch.cuda.device(self.device):
                _native.check(_native.LIB.mg_gather_rows_padded(self._h, x.data_ptr(), int(x.shape[0]), row_bytes, ptr(pick), count, out.data_ptr(),
                                                                self._stream()), "mg_gather_rows_padded")
        return out

    def draw_windows(self, frames, windows, sel=None, out=None, obs_format=None):
        """Frames of a minibatch of windows -> (obs [M, W] + shape of the format, mask bool [M, W], len int32 [M]): row (j, l) is the l-th oldest frame
        of the window of sample sel[j] (sel=None: every sample), zeros behind the window's len and for entries of sel below 0.  frames: with
        back == 0 the RolloutTrace the windows were made from, or a FrameRecords / uint8 tensor [K + 1, N, frame_record_bytes]; with back > 0 a
        FrameRecords / uint8 store [back + K + 1, N, frame_record_bytes] whose first `back` rows are the previous rollout's frames[K_prev - back : K_prev].
        Its layout is checked as draw_sequences checks it.  out: a contiguous tensor [M, W] + shape to draw into.  Two launches on the current
        stream: the picks, and the PAD form of the gather raster."""
        what = "draw_windows"
        self._require_started(what)
        frames = check_window_frames(frames, windows, self.frame_record_bytes)
        return self._draw_picked(what, frames, lambda: windows.picks(sel), windows.window, out, obs_format)

    # ------------------------------------------------------------------ debug-view records
    DEBUG_SIZES = {84: (84, 84, 3), 336: (336, 336, 3)}  # draw_debug_frames: the debug surface [x][y][c], or the reference's debug_rgb_array [y][x][c]

    def save_debug_frames(self, idx=None, out=None):
        """Keep the GROUND-TRUTH (debug) view of a few instances as records (include/memgym.h: mg_save_debug_frames) -> DebugFrameRecords over a uint8
        tensor [k, frame_record_bytes]: what render_debug() would draw for instance idx[j] right now, as 16 / 64 / 128 bytes.  It counts as one debug
        render of the named instances and of no other (Mortar Mayhem ids: the view's clone of the command schedule advances for them alone).  idx: the
        instances, an integer tensor / list (None: all, in order); entries < 0 are skipped (their records keep their bytes); entries must be
        DISTINCT -- a list, array or CPU tensor that names an instance twice is refused, a device tensor is not looked at.  out: a
        DebugFrameRecords or a uint8 tensor [k, frame_record_bytes] to write into -- a row block store[t] of a larger [T, k, bytes] store.  One small
        launch on the current stream (Endless-MysteryPath-v0: behind the launch that generates owed path segments); nothing synchronises."""
        self._require_started("save_debug_frames")
        _distinct_host_index("save_debug_frames", idx)
        if out is not None and isinstance(out, FrameRecords) and not isinstance(out, DebugFrameRecords):
            raise ValueError("save_debug_frames: out holds frame records (save_frames), not debug-view records")
        return self._save_records("save_debug_frames", _native.LIB.mg_save_debug_frames, DebugFrameRecords, idx, out)

    def draw_debug_frames(self, records, pick=None, out=None, size=336):
        """Draw kept debug views (include/memgym.h: mg_draw_debug_frames): row j of the result is the view of record pick[j] (pick=None: record j).
        size=336: uint8 [count, 336, 336, 3], bit for bit the row render_debug() gave when the record was saved; size=84: uint8 [count, 84, 84, 3], the
        debug surface before its stretch, in the observation layout [x][y][c].  records: a DebugFrameRecords (its layout is checked: ValueError if
        stale, before anything is launched) or a plain uint8 tensor, viewed as [n_records, frame_record_bytes].  pick: an integer tensor / list of any
        length, duplicates allowed; an entry outside the records leaves its row untouched and raises error bit 512.  out: a contiguous uint8 tensor of
        the result's shape to draw into.  One raster launch on the current stream; nothing synchronises, nothing of the handle changes."""
        what = "draw_debug_frames"
        self._require_started(what)
        if size not in self.DEBUG_SIZES:
            raise ValueError("%s: size must be 84 or 336" % what)
        rows = _record_rows(what, records, self.frame_layout(), self.frame_record_bytes, debug=True)
        pick, count = _pick_count(what, rows, pick, self.device)
        shape = (count,) + self.DEBUG_SIZES[size]
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and tuple(out.shape) == shape and out.is_contiguous()):
            raise ValueError("%s: out must be a contiguous uint8 tensor of shape %s" % (what, shape))
        if count == 0:  # nothing to draw (an empty tensor has no address to hand to the library)
            return out
        aligned_on(what, "records and out", self.device, rows, out)
        with torch.cuda.device(self.device):
            _native.check(_native.LIB.mg_draw_debug_frames(self._h, rows.data_ptr(), rows.shape[0], ptr(pick), count, int(size), out.data_ptr(),
                                                           self._stream()), "mg_draw_debug_frames")
        return out
