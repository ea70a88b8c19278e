"""What the handle's record calls return and take -- instance snapshots, frame records, debug-view records, rollout traces -- with the argument checks
that need no handle."""
import numpy as np
import torch

from ._args import index_tensor, same_device

OBS_FORMATS = {"u8_xyc": (0, torch.uint8, (84, 84, 3)), "f32_chw": (1, torch.float32, (3, 84, 84)),
               "f16_chw": (2, torch.float16, (3, 84, 84)), "bf16_chw": (3, torch.bfloat16, (3, 84, 84)),
               "u8_chw": (4, torch.uint8, (3, 84, 84))}  # name -> (the library's code, dtype, shape of one observation); VecMemoryGym.OBS_FORMATS


class InstanceSnapshot:
    """What VecMemoryGym.save_instances returns: `records`, a uint8 tensor [k, instance_bytes] on the handle's device (record j = the j-th saved
    instance; the layout of a record is private), `layout`, the value of mg_instance_layout when it was taken (unique to the handle, new after every
    rebuild of its geometry: load_instances refuses a snapshot whose layout is not the handle's current one), and `set_of`, the saved instances'
    option-set indices (int32 [k]) or None where the handle had one option set."""
    __slots__ = ("records", "layout", "set_of")

    def __init__(self, records, layout, set_of=None):
        self.records, self.layout, self.set_of = records, int(layout), set_of

    @property
    def count(self):
        return int(self.records.shape[0])


def check_instance_load(snap, layout, instance_bytes, num_envs, idx=None, rec=None, device=None):
    """The argument checks of load_instances, which need no handle: -> (idx, rec) as int32 tensors or None.  ValueError for a snapshot of another
    handle or of an earlier geometry (`layout`), records of the wrong width, index tensors of the wrong dtype or length."""
    what = "load_instances"
    if not isinstance(snap, InstanceSnapshot):
        raise ValueError("%s: need the InstanceSnapshot save_instances returned" % what)
    if snap.layout != int(layout):
        raise ValueError("%s: the snapshot (layout 0x%x) was taken from another handle, or before this handle's geometry was rebuilt (layout 0x%x): "
                         "records are valid for the handle and the geometry they were saved under" % (what, snap.layout, int(layout)))
    r = snap.records
    if not (isinstance(r, torch.Tensor) and r.dtype == torch.uint8 and r.dim() == 2 and r.shape[1] == int(instance_bytes) and r.is_contiguous()):
        raise ValueError("%s: snapshot.records must be a contiguous uint8 tensor [k, %d]" % (what, int(instance_bytes)))
    if idx is not None:
        idx = index_tensor(what, "idx", idx, device)
    if rec is not None:
        rec = index_tensor(what, "rec", rec, device)
    m = num_envs if idx is None else idx.numel()
    if rec is not None and rec.numel() != m:
        raise ValueError("%s: rec must have one entry per loaded instance (%d), got %d" % (what, m, rec.numel()))
    if rec is None and m > snap.count:
        raise ValueError("%s: %d instances named, the snapshot holds %d records (pass rec= to load a record into several instances)" % (what, m, snap.count))
    if snap.set_of is not None and tuple(snap.set_of.shape) != (snap.count,):
        raise ValueError("%s: snapshot.set_of must have one entry per record" % what)
    return idx, rec


def check_instance_save(instance_bytes, num_envs, idx=None, out=None, device=None):
    """The argument checks of save_instances, which need no handle: -> (idx as an int32 tensor or None, number of records)."""
    what = "save_instances"
    if idx is not None:
        idx = index_tensor(what, "idx", idx, device)
    k = num_envs if idx is None else idx.numel()
    if out is not None:
        if not isinstance(out, InstanceSnapshot):
            raise ValueError("%s: out must be an InstanceSnapshot" % what)
        r = out.records
        if not (isinstance(r, torch.Tensor) and r.dtype == torch.uint8 and tuple(r.shape) == (k, int(instance_bytes)) and r.is_contiguous()):
            raise ValueError("%s: out.records must be a contiguous uint8 tensor [%d, %d]" % (what, k, int(instance_bytes)))
    return idx, k


class FrameRecords:
    """What VecMemoryGym.save_frames returns: `records`, a uint8 tensor [..., frame_record_bytes] on the handle's device (one row = the frame descriptor
    of one instance at one moment: 16 / 64 / 128 bytes, its layout private), and `layout`, the value of mg_frame_layout when it was taken (unique to the
    handle, new whenever a stored descriptor would draw differently: draw_frames refuses records whose layout is not the handle's current one).  A
    trainer that fills a [T, N, bytes] store step by step (save_frames(out=store[t])) wraps the whole store: FrameRecords(store, env.frame_layout())."""
    __slots__ = ("records", "layout")

    def __init__(self, records, layout):
        self.records, self.layout = records, int(layout)

    @property
    def count(self):
        return int(self.records.numel() // self.records.shape[-1])


class DebugFrameRecords(FrameRecords):
    """What VecMemoryGym.save_debug_frames returns: FrameRecords whose rows are DEBUG-VIEW descriptors (the same widths, another content: what
    render_debug() draws from, include/memgym.h mg_save_debug_frames).  draw_debug_frames draws them; draw_frames refuses them."""
    __slots__ = ()


def _distinct_host_index(what, idx):
    """idx as the caller gave it, where the host can see it (a list, an array, a CPU tensor): ValueError if an instance is named twice.  A device tensor
    is not looked at (no synchronisation): there a repeated index is the caller's to avoid (include/memgym.h)."""
    if idx is None or (isinstance(idx, torch.Tensor) and idx.device.type != "cpu"):
        return
    a = np.asarray(idx.numpy() if isinstance(idx, torch.Tensor) else idx)
    if a.dtype.kind in "iu" and a.ndim == 1:
        named = a[a >= 0]
        if np.unique(named).size != named.size:
            raise ValueError("%s: idx names an instance more than once (entries must be distinct; negative entries are padding)" % what)


def _frame_rows(what, name, t, record_bytes):
    """A tensor of frame records -> its view [n, record_bytes]; ValueError unless it is a contiguous uint8 tensor whose last dimension is one record."""
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() >= 2 and t.shape[-1] == int(record_bytes) and t.is_contiguous()):
        raise ValueError("%s: %s must be a contiguous uint8 tensor [..., %d]" % (what, name, int(record_bytes)))
    return t.view(-1, int(record_bytes))


def check_frame_save(record_bytes, num_envs, idx=None, out=None, device=None):
    """The argument checks of save_frames, which need no handle: -> (idx as an int32 tensor or None, number of records, out's records as [k, bytes] or
    None).  out: a FrameRecords or a plain uint8 tensor [k, record_bytes] -- e.g. the row block store[t] of a [T, N, bytes] store -- contiguous."""
    what = "save_frames"
    if idx is not None:
        idx = index_tensor(what, "idx", idx, device)
    k = num_envs if idx is None else idx.numel()
    rows = None
    if out is not None:
        rows = _frame_rows(what, "out", out.records if isinstance(out, FrameRecords) else out, record_bytes)
        if rows.shape[0] != k:
            raise ValueError("%s: out holds %d records, the call saves %d" % (what, rows.shape[0], k))
    return idx, k, rows


def _record_rows(what, records, layout, record_bytes, debug=False):
    """The records argument of draw_frames (debug=False) / draw_debug_frames (debug=True) -> its rows [n, bytes].  ValueError for records of the other
    kind, of another handle or an earlier layout (FrameRecords only: a plain tensor carries neither), of the wrong dtype / width / stride."""
    if isinstance(records, FrameRecords):
        if isinstance(records, DebugFrameRecords) != debug:
            raise ValueError(("%s: these are frame records (save_frames): draw_frames draws them" if debug else
                              "%s: these are debug-view records (save_debug_frames): draw_debug_frames draws them") % what)
        if records.layout != int(layout):
            raise ValueError("%s: the records (layout 0x%x) were saved from another handle, or before something changed that they would draw differently "
                             "(layout 0x%x now): %s records are valid for the handle and the atlas they were saved under"
                             % (what, records.layout, int(layout), "debug-view" if debug else "frame"))
        records = records.records
    return _frame_rows(what, "records", records, record_bytes)


def _pick_count(what, rows, pick, device):
    """The pick argument of a draw over `rows` -> (pick as an int32 tensor or None, the number of rows to draw); ValueError for a pick that is no
    one-dimensional integer tensor, and for rows to draw from no record."""
    if pick is not None:
        pick = index_tensor(what, "pick", pick, device)
    count = rows.shape[0] if pick is None else pick.numel()
    if count > 0 and rows.shape[0] < 1:
        raise ValueError("%s: no records to draw from" % what)
    return pick, count


def check_frame_draw(records, layout, record_bytes, pick=None, out=None, obs_format="u8_xyc", device=None):
    """The argument checks of draw_frames, which need no handle: -> (records as [n, bytes], pick as an int32 tensor or None, count, (dtype, shape) of
    one row).  ValueError for records of another handle or an earlier layout (FrameRecords only: a plain tensor carries none), of the wrong dtype /
    width / stride, a pick that is no one-dimensional integer tensor, more rows than records without a pick, an unknown format, an `out` of the wrong
    shape / dtype or one that is not contiguous."""
    what = "draw_frames"
    rows = _record_rows(what, records, layout, record_bytes)
    if obs_format not in OBS_FORMATS:
        raise ValueError("%s: obs_format must be one of %s" % (what, sorted(OBS_FORMATS)))
    _, dt, shape = OBS_FORMATS[obs_format]
    pick, count = _pick_count(what, rows, pick, device)
    if out is not None and not (isinstance(out, torch.Tensor) and out.dtype == dt and tuple(out.shape) == (count,) + shape and out.is_contiguous()):
        raise ValueError("%s: out must be a contiguous %s tensor of shape %s" % (what, dt, (count,) + shape))
    return rows, pick, count, (dt, shape)


MAX_DRAW_RECORDS = (1 << 31) - 1  # include/memgym.h: mg_draw_frames refuses n_records > INT32_MAX


class RolloutTrace:
    """What VecMemoryGym.new_rollout returns and advance_traced(ro) / play(trace=ro) fill (include/memgym.h: mg_advance_traced / mg_play_traced): K steps
    of N instances kept as
        frames   uint8   [K + 1, N, frame_record_bytes]   the frame records, and `frame_layout`, the value of mg_frame_layout they were filled under
        actions  int32   [K, N] or [K, N, 2]              the action played at step t (advance only; play leaves it alone: the tape is the caller's)
        labels   int32   same shape, or None              the teacher's answer at eps = 0 in the state the action was played in (new_rollout(labels=True))
        reward   float32 [K, N]                           done   bool [K, N]
    (any of them may be None: not kept -- e.g. RolloutTrace(frames, 0, None, None, None, None) keeps the frame records alone)
    in the gymnasium convention: frames[t] is the observation actions[t] / labels[t] belong to, frames[t + 1] the result of step t (the new episode's
    first frame where the step auto-reset the instance; for an instance that did not step, the frame it keeps).  draw() turns picks of it into frames."""
    __slots__ = ("frames", "frame_layout", "actions", "labels", "reward", "done")

    def __init__(self, frames, frame_layout, actions, labels, reward, done):
        self.frames, self.frame_layout, self.actions, self.labels, self.reward, self.done = frames, int(frame_layout), actions, labels, reward, done

    @property
    def steps(self):
        return int(self.frames.shape[0]) - 1 if self.frames is not None else int(next(t for t in (self.reward, self.done, self.actions) if t is not None).shape[0])

    @property
    def num_envs(self):
        return int(next(t for t in (self.frames, self.reward, self.done, self.actions) if t is not None).shape[1])

    def draw(self, env, t, i, out=None, obs_format=None):
        """Frames of the trace: row j of the result is frames[t[j], i[j]] drawn in `obs_format` (default: the handle's) -- draw_frames over the flattened
        store with pick = t * N + i.  t, i: integers, or integer tensors / lists of one length (t in 0 .. K, i in 0 .. N - 1).  ValueError, before anything
        is launched: a trace filled under another handle or an earlier frame layout, t and i of different lengths, a store of more records than
        mg_draw_frames accepts, and whatever draw_frames refuses about `out`."""
        what = "RolloutTrace.draw"
        if not (isinstance(self.frames, torch.Tensor) and self.frames.dim() == 3):
            raise ValueError("%s: frames must be a uint8 tensor [K + 1, N, frame_record_bytes] (this trace keeps no frames?)" % what)
        n = int(self.frames.shape[1])
        if int(self.frames.shape[0]) * n > MAX_DRAW_RECORDS:
            raise ValueError("%s: the store holds %d x %d records, draw_frames takes at most %d: draw from slices of `frames`"
                             % (what, int(self.frames.shape[0]), n, MAX_DRAW_RECORDS))
        dev = self.frames.device
        t, i = (index_tensor(what, nm, [v] if isinstance(v, (int, np.integer)) else v, dev) for nm, v in (("t", t), ("i", i)))
        if t.numel() != i.numel():
            raise ValueError("%s: t and i must have one length, got %d and %d" % (what, t.numel(), i.numel()))
        return env.draw_frames(FrameRecords(self.frames, self.frame_layout), pick=t * n + i, out=out, obs_format=obs_format)


def check_rollout_trace(ro, steps, num_envs, action_dim, record_bytes, teacher, device=None):
    """The argument checks of advance_traced(ro) / play(trace=ro), which need no handle: ValueError unless `ro` is a RolloutTrace whose tensors have the
    shapes and dtypes of RolloutTrace's docstring for K = steps and N = num_envs, are contiguous, lie on `device` (if given) and are aligned for the
    launches' vector stores (frames to 16 bytes, actions / labels to 8).  teacher=False (play): actions and labels are not looked at."""
    what = "advance_traced" if teacher else "play(trace=...)"
    if not isinstance(ro, RolloutTrace):
        raise ValueError("%s: need the RolloutTrace new_rollout returned" % what)
    K, N = int(steps), int(num_envs)
    acts = (K, N) if action_dim == 1 else (K, N, 2)
    want = [("frames", ro.frames, torch.uint8, (K + 1, N, int(record_bytes)), 16), ("reward", ro.reward, torch.float32, (K, N), 4), ("done", ro.done, torch.bool, (K, N), 1)]
    if teacher:
        want.append(("actions", ro.actions, torch.int32, acts, 8))
        if ro.labels is not None:
            want.append(("labels", ro.labels, torch.int32, acts, 8))
    for name, t, dt, shape, align in want:
        if t is None:  # not kept (include/memgym.h: every array may be NULL)
            continue
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous()):
            raise ValueError("%s: trace.%s must be a contiguous %s tensor of shape %s (a trace of %d steps of %d instances), got %s"
                             % (what, name, dt, shape, K, N, "%s %s" % (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
        same_device(what, "trace." + name, t, device)
        if t.data_ptr() % align:
            raise ValueError("%s: trace.%s must be %d-byte aligned" % (what, name, align))


def trace_frame_records(what, trace, steps, num_envs, origin):
    """A RolloutTrace as the FrameRecords over its frame store; ValueError unless it keeps frames and holds `steps` steps of `num_envs` instances.
    origin: how the message names what those two numbers come from ("the sequences were cut from")."""
    if not (isinstance(trace.frames, torch.Tensor) and trace.frames.dim() == 3):
        raise ValueError("%s: the trace keeps no frames" % what)
    if (trace.steps, trace.num_envs) != (steps, num_envs):
        raise ValueError("%s: the trace holds %d steps of %d instances, %s %d steps of %d" % (what, trace.steps, trace.num_envs, origin, steps, num_envs))
    return FrameRecords(trace.frames, trace.frame_layout)
