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
"""
import ctypes as C
import os
import weakref

import numpy as np
import torch

from . import _native
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


_BALANCED = weakref.WeakSet()  # live mg_obs_alloc buffers of this process


def is_balanced_buffer(tensor):
    """True if `tensor` lies in memory obtained from mg_obs_alloc (HIP virtual memory: physical pieces mapped into a reserved
    range).  Such memory has no IPC handle (hipIpcGetMemHandle needs a hipMalloc allocation): memory_gym_amd.dist.PeerObsBuffer
    refuses to export it; collectives (RCCL) and peer access work on it like on any device memory."""
    p = tensor.data_ptr()
    return any(o.ptr is not None and o.ptr <= p < o.ptr + o.nbytes for o in _BALANCED)


class _ObsMemory:
    """Owner of a device buffer obtained from mg_obs_alloc; tensors made from it keep it alive (CUDA array interface)."""

    def __init__(self, ptr, shape, typestr, info):
        self.ptr, self.info = ptr, info
        self.nbytes = int(np.prod(shape))
        _BALANCED.add(self)
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}

    def __del__(self):
        try:
            if self.ptr:
                _native.LIB.mg_obs_free(C.c_void_p(self.ptr))
                self.ptr = None
        except Exception:
            pass


def alloc_obs_buffer(shape, dtype, device, search_budget_bytes=None, frame_bytes=None):
    """A tensor of `shape` / `dtype` on `device` whose memory comes from mg_obs_alloc_for (pieces from two HBM zones, see
    include/memgym.h); returns (tensor, info dict).  The memory is released when the last tensor viewing it goes away.
    `frame_bytes`: bytes of one instance's observation (default: what `shape[1:]` and `dtype` say) -- the pieces are dealt to the zones
    by the raster launch's windows of 14,336 observations.
    MEMGYM_OBS_SEARCH_MS bounds the search in time (default 1,500 ms), MEMGYM_OBS_SEARCH_GB its transient filler allocations
    (default: half of the free memory, at
    most 128 GiB -- VRAM that other processes on the GPU cannot have for the few milliseconds the search lasts; 0 = do not
    search).  The buffer is accessible from this device and from every device with peer access to it."""
    device = torch.device(device)
    elem = torch.empty((), dtype=dtype).element_size()
    nbytes = int(np.prod(shape)) * elem
    if search_budget_bytes is None:
        e = os.environ.get("MEMGYM_OBS_SEARCH_GB")
        search_budget_bytes = _native.MG_OBS_SEARCH_DEFAULT if e is None else int(float(e) * (1 << 30))
    ms = os.environ.get("MEMGYM_OBS_SEARCH_MS")  # time bound of the search (default 1,500 ms; include/memgym.h: mg_obs_set_search_ms)
    if ms is not None and hasattr(_native.LIB, "mg_obs_set_search_ms"):
        _native.check(_native.LIB.mg_obs_set_search_ms(float(ms)), "mg_obs_set_search_ms")
    ptr, info = C.c_void_p(), _native.ObsAllocInfo()
    with torch.cuda.device(device):
        torch.cuda.current_stream().synchronize()
        if frame_bytes is None:
            frame_bytes = int(np.prod(shape[1:])) * elem if len(shape) > 1 else 84 * 84 * 3
        lab = os.environ.get("MEMGYM_OBS_FRAME_BYTES")  # tools/fmt_ab.sh: the piece order of another format (A/B of the window rule)
        if lab:
            frame_bytes = int(lab)
        if hasattr(_native.LIB, "mg_obs_alloc_for"):
            _native.check(_native.LIB.mg_obs_alloc_for(device.index or 0, nbytes, C.c_size_t(frame_bytes), C.c_size_t(search_budget_bytes), C.byref(ptr),
                                                       C.byref(info)), "mg_obs_alloc_for")
        else:  # (a build of an earlier round, loaded through MEMGYM_HIP_LIB by tools/)
            _native.check(_native.LIB.mg_obs_alloc(device.index or 0, nbytes, C.c_size_t(search_budget_bytes), C.byref(ptr), C.byref(info)), "mg_obs_alloc")
    # bfloat16 has no array-interface typestr: expose the bytes and view them
    owner = _ObsMemory(ptr.value, (nbytes,), "|u1", {k: getattr(info, k) for k, _ in info._fields_})
    t = torch.as_tensor(owner, device=device).view(dtype).view(tuple(shape))
    return t, owner.info


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


def _instance_index(what, name, t, device=None):
    """An index argument of save_instances / load_instances / copy_instances -> a contiguous int32 tensor [m] (on `device` if given).  Integer
    tensors, arrays and lists are taken; anything else, and anything that is not one-dimensional, is a ValueError."""
    if not isinstance(t, torch.Tensor):
        a = np.asarray(t)
        if a.dtype.kind not in "iu":
            raise ValueError("%s: %s must hold integers, got dtype %s" % (what, name, a.dtype))
        t = torch.as_tensor(a.astype(np.int64))
    if t.dtype not in (torch.int32, torch.int64):
        raise ValueError("%s: %s must be an int32 or int64 tensor, got %s" % (what, name, t.dtype))
    if t.dim() != 1:
        raise ValueError("%s: %s must have one dimension, got shape %s" % (what, name, tuple(t.shape)))
    t = t.to(dtype=torch.int32) if device is None else t.to(device=device, dtype=torch.int32)
    return t.contiguous()


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
        idx = _instance_index(what, "idx", idx, device)
    if rec is not None:
        rec = _instance_index(what, "rec", rec, device)
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
        idx = _instance_index(what, "idx", idx, device)
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
        idx = _instance_index(what, "idx", idx, device)
    k = num_envs if idx is None else idx.numel()
    rows = None
    if out is not None:
        rows = _frame_rows(what, "out", out.records if isinstance(out, FrameRecords) else out, record_bytes)
        if rows.shape[0] != k:
            raise ValueError("%s: out holds %d records, the call saves %d" % (what, rows.shape[0], k))
    return idx, k, rows


def check_frame_draw(records, layout, record_bytes, pick=None, out=None, obs_format="u8_xyc", device=None):
    """The argument checks of draw_frames, which need no handle: -> (records as [n, bytes], pick as an int32 tensor or None, count, (dtype, shape) of
    one row).  ValueError for records of another handle or an earlier layout (FrameRecords only: a plain tensor carries none), of the wrong dtype /
    width / stride, a pick that is no one-dimensional integer tensor, more rows than records without a pick, an unknown format, an `out` of the wrong
    shape / dtype or one that is not contiguous."""
    what = "draw_frames"
    if isinstance(records, DebugFrameRecords):
        raise ValueError("%s: these are debug-view records (save_debug_frames): draw_debug_frames draws them" % what)
    if isinstance(records, FrameRecords):
        if records.layout != int(layout):
            raise ValueError("%s: the records (layout 0x%x) were saved from another handle, or before something changed that they would draw differently "
                             "(layout 0x%x now): frame records are valid for the handle and the atlas they were saved under" % (what, records.layout, int(layout)))
        records = records.records
    rows = _frame_rows(what, "records", records, record_bytes)
    if obs_format not in VecMemoryGym.OBS_FORMATS:
        raise ValueError("%s: obs_format must be one of %s" % (what, sorted(VecMemoryGym.OBS_FORMATS)))
    _, dt, shape = VecMemoryGym.OBS_FORMATS[obs_format]
    if pick is not None:
        pick = _instance_index(what, "pick", pick, device)
    count = rows.shape[0] if pick is None else pick.numel()
    if count > 0 and rows.shape[0] < 1:
        raise ValueError("%s: no records to draw from" % what)
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
        t, i = (_instance_index(what, nm, [v] if isinstance(v, (int, np.integer)) else v, dev) for nm, v in (("t", t), ("i", i)))
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
        if device is not None and t.device != device:
            raise ValueError("%s: trace.%s is on %s, the handle on %s" % (what, name, t.device, device))
        if t.data_ptr() % align:
            raise ValueError("%s: trace.%s must be %d-byte aligned" % (what, name, align))


MAX_PICK = (1 << 31) - 1  # include/memgym.h: a pick is an int32 -- mg_split_episodes refuses (steps + 1) * num_envs beyond it


def check_split_episodes(done, length, num_envs, steps=None, starts=None, capacity=None, device=None):
    """The argument checks of split_episodes, which need no handle: -> (done as a uint8 view [K, N], K, length, steps as an int32 tensor [N] or None,
    starts as a uint8 view [N] or None, capacity as an int or None).  ValueError for a `done` that is no contiguous bool / uint8 tensor [K, N] with
    K >= 1 and N = num_envs, a length below 1, (K + 1) * N beyond an int32, `steps` that is no int32 / int64 tensor [N], `starts` that is no contiguous
    bool / uint8 tensor [N], a negative capacity, and anything that does not lie on `device` (if given)."""
    what = "split_episodes"
    if not (isinstance(done, torch.Tensor) and done.dtype in (torch.bool, torch.uint8) and done.dim() == 2):
        raise ValueError("%s: done must be a contiguous bool or uint8 tensor [K, N]" % what)
    K, N = int(done.shape[0]), int(done.shape[1])
    if N != int(num_envs) or K < 1:
        raise ValueError("%s: done is %s, need [K >= 1, %d] (the handle's instances)" % (what, tuple(done.shape), int(num_envs)))
    if (K + 1) * N > MAX_PICK:
        raise ValueError("%s: (K + 1) * N = %d does not fit the int32 of a pick: split slices of the rollout" % (what, (K + 1) * N))
    if not done.is_contiguous():
        raise ValueError("%s: done must be a contiguous bool or uint8 tensor [K, N]" % what)
    if isinstance(length, bool) or not isinstance(length, (int, np.integer)) or length < 1 or length > MAX_PICK:
        raise ValueError("%s: length must be an integer >= 1, got %r" % (what, length))
    if device is not None and done.device != device:
        raise ValueError("%s: done is on %s, the handle on %s" % (what, done.device, device))
    if steps is not None:
        if not (isinstance(steps, torch.Tensor) and steps.dtype in (torch.int32, torch.int64) and tuple(steps.shape) == (N,)):
            raise ValueError("%s: steps must be an int32 or int64 tensor [%d] (e.g. what play() returned as steps_played)" % (what, N))
        if device is not None and steps.device != device:
            raise ValueError("%s: steps is on %s, the handle on %s" % (what, steps.device, device))
        steps = steps.to(torch.int32).contiguous()
    if starts is not None:
        if not (isinstance(starts, torch.Tensor) and starts.dtype in (torch.bool, torch.uint8) and tuple(starts.shape) == (N,) and starts.is_contiguous()):
            raise ValueError("%s: starts must be a contiguous bool or uint8 tensor [%d]" % (what, N))
        if device is not None and starts.device != device:
            raise ValueError("%s: starts is on %s, the handle on %s" % (what, starts.device, device))
        starts = starts.view(torch.uint8)
    if capacity is not None:
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 0 or capacity > MAX_PICK:
            raise ValueError("%s: capacity must be an integer >= 0, got %r" % (what, capacity))
        capacity = int(capacity)
    return done.view(torch.uint8), K, int(length), steps, starts, capacity


class EpisodeSequences:
    """What VecMemoryGym.split_episodes returns (include/memgym.h: mg_split_episodes): a rollout of `steps` steps of `num_envs` instances cut into
    episodes at done and chopped into sequences of at most `length` steps.
        table    int32 [capacity, 4]   one row per sequence: instance, t0, len, flags (1: starts an episode, 2: ends with its episode's done), ordered
                                       by (instance, t0); rows from the count on are untouched
        count    int32 [1]             the true number of sequences, on the device (it may exceed the capacity: the table then holds the first `capacity`)
    len(seqs) reads the count (a synchronisation); picks() and gather() do not."""
    __slots__ = ("table", "count", "length", "steps", "num_envs", "_env")

    def __init__(self, table, count, length, steps, num_envs, env=None):
        self.table, self.count, self.length, self.steps, self.num_envs, self._env = table, count, int(length), int(steps), int(num_envs), env

    @property
    def capacity(self):
        return int(self.table.shape[0])

    def __len__(self):
        s = int(self.count.item())
        if s > self.capacity:
            raise ValueError("EpisodeSequences: the rollout has %d sequences, the table holds %d: split again with capacity >= %d" % (s, self.capacity, s))
        return s

    def picks(self, sel=None, m=None):
        """-> (pick int32 [M, L], mask bool [M, L]) (include/memgym.h: mg_sequence_picks): row j belongs to sequence sel[j] (sel=None: sequence j,
        M = m, default len(self) -- which synchronises; m = capacity does not, rows beyond the count are padding).  pick[j, l] = (t0 + l) * N + instance
        for l < len, -1 behind it: an index into the flattened [K + 1, N] frame store of the trace and into its flattened [K, N] action / label /
        reward / done rows.  sel: an integer tensor / list [M]; an entry < 0 gives a padding row, an entry at or beyond the number of sequences the
        table holds a padding row and error bit 512.  One launch on the current stream."""
        what = "EpisodeSequences.picks"
        env = self._env
        if env is None:
            raise ValueError("%s: these sequences belong to no handle" % what)
        if sel is not None:
            if m is not None:
                raise ValueError("%s: give sel or m, not both" % what)
            sel = _instance_index(what, "sel", sel, env.device)
            M = sel.numel()
        else:
            M = len(self) if m is None else m
            if isinstance(M, bool) or not isinstance(M, (int, np.integer)) or M < 0:
                raise ValueError("%s: m must be an integer >= 0, got %r" % (what, m))
            M = int(M)
        if M * self.length > MAX_PICK:
            raise ValueError("%s: %d rows of %d picks do not fit one call" % (what, M, self.length))
        pick = torch.empty((M, self.length), dtype=torch.int32, device=env.device)
        mask = torch.empty((M, self.length), dtype=torch.bool, device=env.device)
        if M:
            with torch.cuda.device(env.device):
                _native.check(_native.LIB.mg_sequence_picks(env._h, self.table.data_ptr() if self.capacity else None, self.count.data_ptr(), self.capacity,
                                                            None if sel is None else sel.data_ptr(), M, self.length, pick.data_ptr(), mask.data_ptr(),
                                                            env._stream()), "mg_sequence_picks")
        return pick, mask

    def gather(self, x, sel=None):
        """x [K, N, ...] (actions, labels, reward, done) or [K + 1, N, ...] (per-frame data) -> [M, L, ...], zero at the pads: x flattened over its
        first two dimensions, indexed with picks(sel)."""
        if not (isinstance(x, torch.Tensor) and x.dim() >= 2 and int(x.shape[0]) in (self.steps, self.steps + 1) and int(x.shape[1]) == self.num_envs):
            raise ValueError("EpisodeSequences.gather: x must be a tensor [%d or %d, %d, ...]" % (self.steps, self.steps + 1, self.num_envs))
        pick, mask = self.picks(sel)
        rows = x.reshape((-1,) + tuple(x.shape[2:]))[pick.clamp(min=0).long()]
        return torch.where(mask.reshape(mask.shape + (1,) * (x.dim() - 2)), rows, torch.zeros_like(rows))


def _plain_int(what, name, v, least):
    """v as an int; ValueError unless it is an integer (no bool, no float) in least .. MAX_PICK"""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least or v > MAX_PICK:
        raise ValueError("%s: %s must be an integer >= %d, got %r" % (what, name, least, v))
    return int(v)


def _per_instance_int32(what, name, t, n, device):
    """an int32 / int64 tensor [n] (on `device` if given) -> a contiguous int32 tensor; None stays None"""
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.dtype in (torch.int32, torch.int64) and tuple(t.shape) == (n,)):
        raise ValueError("%s: %s must be an int32 or int64 tensor [%d]" % (what, name, n))
    if device is not None and t.device != device:
        raise ValueError("%s: %s is on %s, the handle on %s" % (what, name, t.device, device))
    return t.to(torch.int32).contiguous()


def check_episode_windows(done, window, num_envs, lag=0, back=0, steps=None, pos0=None, device=None):
    """The argument checks of episode_positions / episode_windows, which need no handle: -> (done as a uint8 view [K, N], K, window, lag, back, steps as
    an int32 tensor [N] or None, pos0 as an int32 tensor [N] or None).  ValueError for a `done` that is no contiguous bool / uint8 tensor [K, N] with
    K >= 1 and N = num_envs, a window below 1, a negative lag or back, (back + K + 1) * N beyond an int32, `steps` / `pos0` that are no int32 / int64
    tensors [N], and anything that does not lie on `device` (if given)."""
    what = "episode_windows"
    if not (isinstance(done, torch.Tensor) and done.dtype in (torch.bool, torch.uint8) and done.dim() == 2):
        raise ValueError("%s: done must be a contiguous bool or uint8 tensor [K, N]" % what)
    K, N = int(done.shape[0]), int(done.shape[1])
    if N != int(num_envs) or K < 1:
        raise ValueError("%s: done is %s, need [K >= 1, %d] (the handle's instances)" % (what, tuple(done.shape), int(num_envs)))
    window, lag, back = _plain_int(what, "window", window, 1), _plain_int(what, "lag", lag, 0), _plain_int(what, "back", back, 0)
    if (back + K + 1) * N > MAX_PICK:
        raise ValueError("%s: (back + K + 1) * N = %d does not fit the int32 of a pick: take slices of the rollout" % (what, (back + K + 1) * N))
    if not done.is_contiguous():
        raise ValueError("%s: done must be a contiguous bool or uint8 tensor [K, N]" % what)
    if device is not None and done.device != device:
        raise ValueError("%s: done is on %s, the handle on %s" % (what, done.device, device))
    return (done.view(torch.uint8), K, window, lag, back, _per_instance_int32(what, "steps", steps, N, device),
            _per_instance_int32(what, "pos0", pos0, N, device))


def _pick_tensor(what, name, t, device=None):
    """An index argument of any shape -> a contiguous int32 tensor of that shape (on `device` if given); integer tensors, arrays and lists are taken"""
    if not isinstance(t, torch.Tensor):
        a = np.asarray(t)
        if a.dtype.kind not in "iu":
            raise ValueError("%s: %s must hold integers, got dtype %s" % (what, name, a.dtype))
        t = torch.as_tensor(a.astype(np.int64))
    if t.dtype not in (torch.int32, torch.int64):
        raise ValueError("%s: %s must be an int32 or int64 tensor, got %s" % (what, name, t.dtype))
    t = t.to(dtype=torch.int32) if device is None else t.to(device=device, dtype=torch.int32)
    return t.contiguous()


def check_gather_rows(x, pick, out=None, device=None):
    """The argument checks of gather_rows, which need no handle: -> (x, pick as a contiguous int32 tensor or None, the result's shape, bytes of a row).
    ValueError for an `x` that is no contiguous tensor [R, ...] with rows of at least one byte, a pick that holds no integers, more rows than x has
    without a pick, and an `out` of another shape / dtype / device than the result or one that is not contiguous."""
    what = "gather_rows"
    if not (isinstance(x, torch.Tensor) and x.dim() >= 1 and x.is_contiguous()):
        raise ValueError("%s: x must be a contiguous tensor [R, ...]" % what)
    row_bytes = int(np.prod(x.shape[1:], dtype=np.int64)) * x.element_size()
    if row_bytes < 1:
        raise ValueError("%s: a row of x %s holds no byte" % (what, tuple(x.shape)))
    if int(x.shape[0]) > MAX_PICK:
        raise ValueError("%s: x has %d rows, a pick is an int32" % (what, int(x.shape[0])))
    if device is not None and x.device != device:
        raise ValueError("%s: x is on %s, the handle on %s" % (what, x.device, device))
    if pick is not None:
        pick = _pick_tensor(what, "pick", pick, x.device)
    shape = ((int(x.shape[0]),) if pick is None else tuple(pick.shape)) + tuple(x.shape[1:])
    if (x.shape[0] if pick is None else pick.numel()) > MAX_PICK:
        raise ValueError("%s: more than %d rows in one call" % (what, MAX_PICK))
    if out is not None and not (isinstance(out, torch.Tensor) and out.dtype == x.dtype and tuple(out.shape) == shape and out.is_contiguous()
                                and out.device == x.device):
        raise ValueError("%s: out must be a contiguous %s tensor of shape %s on %s" % (what, x.dtype, shape, x.device))
    return x, pick, shape, row_bytes


class EpisodeWindows:
    """What VecMemoryGym.episode_windows returns (include/memgym.h: mg_episode_positions / mg_window_picks): the sliding memory windows of a rollout of
    `steps` steps of `num_envs` instances.
        pos      int32 [K + 1, N]   the steps instance i's episode had already taken at store row t (mg_episode_positions)
        window   W, the rows of a window;  lag: the window of sample (t, i) ends at row t - lag;  back: rows of the previous trace a window may reach into
    The window of sample s = t * N + i holds the rows max(t - pos[t, i], t - lag - W + 1, -back) .. t - lag, oldest first, pads behind them.  `carry`
    is the next call's pos0.  Nothing here synchronises."""
    __slots__ = ("pos", "window", "lag", "back", "steps", "num_envs", "_env")

    def __init__(self, pos, window, lag, back, steps, num_envs, env=None):
        self.pos, self.window, self.lag, self.back, self.steps, self.num_envs, self._env = pos, int(window), int(lag), int(back), int(steps), int(num_envs), env

    @property
    def carry(self):
        """row K of pos: the positions behind the rollout's last step -- the pos0 of the next rollout's episode_windows"""
        return self.pos[self.steps]

    def picks(self, sel=None, m=None):
        """-> (pick int32 [M, W], mask bool [M, W], len int32 [M]) (include/memgym.h: mg_window_picks): row j belongs to sample sel[j] = t * N + i
        (sel=None: sample j, M = m, default (K + 1) * N: every sample, the bootstrap row included).  pick[j, l] = (back + lo + l) * N + i for l < len,
        -1 behind it: an index into a flattened [back + K + 1, N] store whose first `back` rows are the last `back` rows of the previous rollout.
        sel: an integer tensor / list [M]; an entry < 0 gives a padding row, an entry at or beyond (K + 1) * N a padding row and error bit 512.  One
        launch on the current stream."""
        what = "EpisodeWindows.picks"
        env = self._env
        if env is None:
            raise ValueError("%s: these windows belong to no handle" % what)
        samples = (self.steps + 1) * self.num_envs
        if sel is not None:
            if m is not None:
                raise ValueError("%s: give sel or m, not both" % what)
            sel = _instance_index(what, "sel", sel, env.device)
            M = sel.numel()
        else:
            M = samples if m is None else m
            if isinstance(M, bool) or not isinstance(M, (int, np.integer)) or M < 0 or M > samples:
                raise ValueError("%s: m must be an integer in 0 .. %d, got %r" % (what, samples, m))
            M = int(M)
        if M * self.window > MAX_PICK:
            raise ValueError("%s: %d rows of %d picks do not fit one call" % (what, M, self.window))
        pick = torch.empty((M, self.window), dtype=torch.int32, device=env.device)
        mask = torch.empty((M, self.window), dtype=torch.bool, device=env.device)
        length = torch.empty((M,), dtype=torch.int32, device=env.device)
        if M:
            with torch.cuda.device(env.device):
                _native.check(_native.LIB.mg_window_picks(env._h, self.pos.data_ptr(), self.steps, None if sel is None else sel.data_ptr(), M, self.window,
                                                          self.lag, self.back, pick.data_ptr(), mask.data_ptr(), length.data_ptr(), env._stream()),
                              "mg_window_picks")
        return pick, mask, length

    def store(self, x, prefix=None):
        """The store the picks index, [(back + rows of x) * N, ...]: cat(prefix, x) flattened over its first two dimensions.  x: [K, N, ...] (actions,
        rewards: a pick of row K is then out of range) or [K + 1, N, ...] (per-frame data: hidden states, values).  prefix: [back, N, ...], the last
        `back` rows of the previous rollout's x in front of its row K_prev; required when back > 0.  ValueError otherwise."""
        what = "EpisodeWindows.gather"
        if not (isinstance(x, torch.Tensor) and x.dim() >= 2 and int(x.shape[0]) in (self.steps, self.steps + 1) and int(x.shape[1]) == self.num_envs):
            raise ValueError("%s: x must be a tensor [%d or %d, %d, ...]" % (what, self.steps, self.steps + 1, self.num_envs))
        if self.back > 0:
            if prefix is None:
                raise ValueError("%s: back = %d: a prefix [%d, %d, ...] is required (the last rows of the previous rollout)" % (what, self.back, self.back, self.num_envs))
            if not (isinstance(prefix, torch.Tensor) and prefix.dtype == x.dtype and prefix.device == x.device
                    and tuple(prefix.shape) == (self.back, self.num_envs) + tuple(x.shape[2:])):
                raise ValueError("%s: prefix must be a %s tensor of shape %s on %s" % (what, x.dtype, (self.back, self.num_envs) + tuple(x.shape[2:]), x.device))
            x = torch.cat((prefix, x), 0)
        elif prefix is not None and int(prefix.shape[0]) != 0:
            raise ValueError("%s: back = 0: there is no room for a prefix" % what)
        return x.contiguous().view((-1,) + tuple(x.shape[2:]))

    def gather(self, x, sel=None, prefix=None):
        """x [K, N, ...] or [K + 1, N, ...] -> [M, W, ...], zero rows at the pads: gather_rows on store(x, prefix), indexed with picks(sel).  One launch
        for the picks and one for the rows (include/memgym.h: mg_gather_rows_padded), on the current stream."""
        rows = self.store(x, prefix)
        if self._env is None:
            raise ValueError("EpisodeWindows.gather: these windows belong to no handle")
        return self._env.gather_rows(rows, self.picks(sel)[0])


def check_window_frames(frames, windows, record_bytes):
    """The layout checks of draw_windows, which need no handle: -> a FrameRecords or uint8 tensor for draw_frames_padded.  With back == 0 `frames` may be
    the RolloutTrace the windows were made from (its K and N are checked); with back > 0 it must be a FrameRecords / uint8 store of
    [back + K + 1, N, record_bytes] rows that the caller assembled.  ValueError otherwise."""
    what = "draw_windows"
    if not isinstance(windows, EpisodeWindows):
        raise ValueError("%s: windows must be the EpisodeWindows episode_windows returned" % what)
    if isinstance(frames, RolloutTrace):
        if windows.back > 0:
            raise ValueError("%s: back = %d: a trace holds no rows of the previous rollout; pass a FrameRecords / uint8 store of [%d + %d + 1, %d, %d] rows"
                             % (what, windows.back, windows.back, windows.steps, windows.num_envs, int(record_bytes)))
        if not (isinstance(frames.frames, torch.Tensor) and frames.frames.dim() == 3):
            raise ValueError("%s: the trace keeps no frames" % what)
        if (frames.steps, frames.num_envs) != (windows.steps, windows.num_envs):
            raise ValueError("%s: the trace holds %d steps of %d instances, the windows were made from %d steps of %d"
                             % (what, frames.steps, frames.num_envs, windows.steps, windows.num_envs))
        return FrameRecords(frames.frames, frames.frame_layout)
    rec = frames.records if isinstance(frames, FrameRecords) else frames
    want = (windows.back + windows.steps + 1, windows.num_envs, int(record_bytes))
    if not (isinstance(rec, torch.Tensor) and rec.dtype == torch.uint8 and tuple(rec.shape) == want and rec.is_contiguous()):
        raise ValueError("%s: frames must be a contiguous uint8 store of shape %s (back + K + 1 rows of N records)" % (what, want))
    return frames


class VecMemoryGym:
    metadata ={"render_modes": ["rgb_array", "debug_rgb_array"], "render_fps": 25}

    OBS_FORMATS = {"u8_xyc": (0, torch.uint8, (84, 84, 3)), "f32_chw": (1, torch.float32, (3, 84, 84)),
                   "f16_chw": (2, torch.float16, (3, 84, 84)), "bf16_chw": (3, torch.bfloat16, (3, 84, 84)),
                   "u8_chw": (4, torch.uint8, (3, 84, 84))}
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
        self._info = _native.InfoBuffers()
        self._info.struct_size = C.sizeof(_native.InfoBuffers)
        self._err = C.c_int(0)
        self._info.ep_reward_dev = self.ep_reward.data_ptr()
        self._info.ep_length_dev = self.ep_length.data_ptr()
        for k, t in enumerate(self.aux):
            self._info.aux_dev[k] = t.data_ptr()
        self._info.final_obs_dev = self.final_obs.data_ptr() if self.final_obs is not None else None
        self._info.reward64_dev = self.reward64.data_ptr()
        self._info.gt64_dev = self.gt64.data_ptr() if self.gt64 is not None else None
        # What happens when ONE instance reaches a capacity of this build (128 path segments, 128 fall-off cells, 512 commands, 16 live
        # spotlights; the reference's lists are unbounded).  The kernels end that instance's episode and raise a sticky error bit either
        # way.  "raise" (default): step() turns the bit into a RuntimeError -- nothing that differs from the reference goes unnoticed.
        # "truncate": step() reports the instance as truncated (`truncated[i]`, info["capacity_exceeded"][i]) and the batch goes on: one
        # instance of 262,144 that outlives a list does not abort a rollout (missing #1).
        if on_capacity not in ("raise", "truncate"):
            raise ValueError("on_capacity must be 'raise' or 'truncate'")
        self.on_capacity = on_capacity
        self.capacity_u8 = torch.zeros(N, dtype=torch.uint8, device=dev) if on_capacity == "truncate" else None
        self._info.capacity_dev = self.capacity_u8.data_ptr() if self.capacity_u8 is not None else None
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
            while len(self._set_params) <= k:
                self._set_params.append({})
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
            self._set_of = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
            _native.check(_native.LIB.mg_bind_option_sets(self._h, self._set_of.data_ptr()), "mg_bind_option_sets")
        self._set_of[mask.to(device=self.device, dtype=torch.bool)] = k

    def _apply_options(self, options):
        params = process_reset_params(self.env_id, options)
        self._write_set(0, params)
        if self._set_of is not None:
            # a reset of every instance: all of them run under these options.  The per-instance index is unbound again, so the
            # handle is back in its one-set launch arrangement (one-launch mortar step, fused resets, lazy segments), and the other
            # sets are forgotten: their geometry entries may be stale now, a later masked reset writes the set it needs in full.
            _native.check(_native.LIB.mg_bind_option_sets(self._h, None), "mg_bind_option_sets")
            self._set_of = None
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
            _native.check(_native.LIB.mg_reset(self._h, None if s is None else s.data_ptr(),
                                               None if m is None else m.data_ptr(), self.obs.data_ptr(),
                                               self.gt.data_ptr() if self.gt_dim else None, self._stream()), "mg_reset")
            if self.gt64 is not None:
                _native.check(_native.LIB.mg_ground_truth64(self._h, self.gt64.data_ptr(), self._stream()), "mg_ground_truth64")
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
            m = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(mask)
            if m.numel() != self.num_envs or m.dim() != 1:
                raise ValueError("step(mask=...): the mask must have shape [%d], got %s" % (self.num_envs, tuple(m.shape)))
            if m.dtype == torch.bool and m.device == self.device and m.is_contiguous():
                m = m.view(torch.uint8)  # (the same bytes: True is 1)
            elif not (m.dtype == torch.uint8 and m.device == self.device and m.is_contiguous()):
                m = (m != 0).to(device=self.device, dtype=torch.uint8).contiguous()
        a = actions
        if not (isinstance(a, torch.Tensor) and a.dtype == torch.int32 and a.device == self.device and a.is_contiguous()):
            a = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
            a = a.to(device=self.device, dtype=torch.int32).contiguous()
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
        ptr = lambda t: None if t is None else t.data_ptr()
        rows = _native.RolloutTraceRows()
        rows.struct_size = C.sizeof(_native.RolloutTraceRows)
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
            N, dev = self.num_envs, self.device
            t = {"reward": torch.zeros(N, dtype=torch.float64, device=dev), "episodes": torch.zeros(N, dtype=torch.int32, device=dev),
                 "episode_reward": torch.zeros(N, dtype=torch.float64, device=dev), "episode_length": torch.zeros(N, dtype=torch.int64, device=dev)}
            out = _native.AdvanceOut()
            out.struct_size = C.sizeof(_native.AdvanceOut)
            out.reward_sum_dev, out.episodes_dev = t["reward"].data_ptr(), t["episodes"].data_ptr()
            out.ep_reward_sum_dev, out.ep_length_sum_dev = t["episode_reward"].data_ptr(), t["episode_length"].data_ptr()
            for k, nm in enumerate(self.info_names):
                t[nm] = torch.zeros(N, dtype=torch.float64, device=dev)
                out.aux_sum_dev[k] = t[nm].data_ptr()
            self._adv = (t, out)
        mask = (1 << 64) - 1
        with torch.cuda.device(self.device):
            self._clear_pending()
            if trace is not None:
                rows = self._trace_rows(trace, True)
                _native.check(_native.LIB.mg_advance_traced(self._h, steps, float(eps), int(seed) & mask, int(self._expert_calls if step is None else step) & mask,
                                                            self._p_gt, C.byref(self._adv[1]) if stats else None, C.byref(rows), self._stream()), "mg_advance_traced")
            else:
                _native.check(_native.LIB.mg_advance(self._h, steps, float(eps), int(seed) & mask, int(self._expert_calls if step is None else step) & mask,
                                                     self._p_gt, C.byref(self._adv[1]) if stats else None, self._stream()), "mg_advance")
            if self.gt64 is not None:
                _native.check(_native.LIB.mg_ground_truth64(self._h, self.gt64.data_ptr(), self._stream()), "mg_ground_truth64")
        if step is None:
            self._expert_calls += steps
        self._stale = True
        _native.LIB.mg_peek_errors(self._h, self._p_err)  # host-mapped word: no synchronisation
        if self._err.value & ~self._tolerated:
            self.check_errors()
        return (self.redraw() if render else None), (dict(self._adv[0]) if stats else None)

    def _sum_tensors(self):
        """the [N] tensors of advance()'s / play()'s stats and the mg_advance_out over them"""
        N, dev = self.num_envs, self.device
        t = {"reward": torch.zeros(N, dtype=torch.float64, device=dev), "episodes": torch.zeros(N, dtype=torch.int32, device=dev),
             "episode_reward": torch.zeros(N, dtype=torch.float64, device=dev), "episode_length": torch.zeros(N, dtype=torch.int64, device=dev)}
        out = _native.AdvanceOut()
        out.struct_size = C.sizeof(_native.AdvanceOut)
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
            a = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
            a = a.to(device=self.device, dtype=torch.int32).contiguous()
        want = (self.num_envs,) if self.action_dim == 1 else (self.num_envs, 2)
        if a.dim() != len(want) + 1 or tuple(a.shape[1:]) != want or a.shape[0] < 1:
            raise ValueError("play(actions): the tape must have shape [K, %s] with K >= 1, got %s" % (", ".join(str(x) for x in want), tuple(a.shape)))
        K = int(a.shape[0])
        m = None
        if mask is not None:
            m = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(mask)
            if m.numel() != self.num_envs or m.dim() != 1:
                raise ValueError("play(mask=...): the mask must have shape [%d], got %s" % (self.num_envs, tuple(m.shape)))
            if m.dtype == torch.bool and m.device == self.device and m.is_contiguous():
                m = m.view(torch.uint8)  # (the same bytes: True is 1)
            elif not (m.dtype == torch.uint8 and m.device == self.device and m.is_contiguous()):
                m = (m != 0).to(device=self.device, dtype=torch.uint8).contiguous()
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
        with torch.cuda.device(self.device):
            self._clear_pending()
            if ro is not None:
                rows = self._trace_rows(ro, False)
                _native.check(_native.LIB.mg_play_traced(self._h, a.data_ptr(), K, _native.MG_PLAY_EPISODE if until_done else _native.MG_PLAY_THROUGH,
                                                         None if m is None else m.data_ptr(), sums["steps"].data_ptr() if stats else None, self._p_gt,
                                                         C.byref(out) if stats else None, C.byref(rows), self._stream()), "mg_play_traced")
            else:
                _native.check(_native.LIB.mg_play(self._h, a.data_ptr(), K, _native.MG_PLAY_EPISODE if until_done else _native.MG_PLAY_THROUGH,
                                                  None if m is None else m.data_ptr(), None if rt is None else rt.data_ptr(),
                                                  None if dt is None else dt.data_ptr(), sums["steps"].data_ptr() if stats else None, self._p_gt,
                                                  C.byref(out) if stats else None, self._stream()), "mg_play")
            if self.gt64 is not None:
                _native.check(_native.LIB.mg_ground_truth64(self._h, self.gt64.data_ptr(), self._stream()), "mg_ground_truth64")
        self._stale = True
        _native.LIB.mg_peek_errors(self._h, self._p_err)  # host-mapped word: no synchronisation
        if self._err.value & ~self._tolerated:
            self.check_errors()
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
        mask = (1 << 64) - 1
        with torch.cuda.device(self.device):
            _native.check(_native.LIB.mg_expert_actions(self._h, float(eps), int(seed) & mask, int(self._expert_calls if step is None else step) & mask,
                                                        out.data_ptr(), self._stream()), "mg_expert_actions")
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
        if records.device != self.device or records.data_ptr() % 16:
            raise ValueError("save_instances: out.records must be a 16-byte aligned tensor on %s" % (self.device,))
        with torch.cuda.device(self.device):
            _native.check(_native.LIB.mg_save_instances(self._h, None if idx is None else idx.data_ptr(), k, records.data_ptr(), self._stream()), "mg_save_instances")
            set_of = None
            if self._set_of is not None:  # the caller owns the set index (include/memgym.h): it travels beside the records
                set_of = self._set_of.clone() if idx is None else self._set_of[idx.clamp(0, self.num_envs - 1).long()]
        if out is not None:
            out.layout, out.set_of = self.instance_layout, set_of
            return out
        return InstanceSnapshot(records, self.instance_layout, set_of)

    # ------------------------------------------------------------------ frame records
    @property
    def frame_record_bytes(self):
        return int(_native.LIB.mg_frame_record_bytes(self._h))

    def frame_layout(self):
        return int(_native.LIB.mg_frame_layout(self._h))

    def save_frames(self, idx=None, out=None):
        """Keep the CURRENT frames as their descriptors (include/memgym.h: mg_save_frames) -> FrameRecords over a uint8 tensor [k, frame_record_bytes]:
        16 / 64 / 128 bytes per frame instead of 21,168 and more.  After step(render=False) the records hold the frames the step would have drawn.
        idx: the instances, an integer tensor / list (None: all, in order); entries < 0 are skipped (their records keep their bytes).  out: a
        FrameRecords or a uint8 tensor [k, frame_record_bytes] to write into -- a row block store[t] of a larger [T, N, bytes] store, so one store is
        filled step by step.  One small launch on the current stream; nothing synchronises, nothing of the handle changes."""
        self._require_started("save_frames")
        nbytes = self.frame_record_bytes
        idx, k, rows = check_frame_save(nbytes, self.num_envs, idx, out, self.device)
        if rows is None:
            out = rows = torch.empty((k, nbytes), dtype=torch.uint8, device=self.device)
        if rows.device != self.device or rows.data_ptr() % 16:
            raise ValueError("save_frames: out must be a 16-byte aligned tensor on %s" % (self.device,))
        with torch.cuda.device(self.device):
            _native.check(_native.LIB.mg_save_frames(self._h, None if idx is None else idx.data_ptr(), k, rows.data_ptr(), self._stream()), "mg_save_frames")
        if isinstance(out, FrameRecords):
            out.layout = self.frame_layout()
            return out
        return FrameRecords(out, self.frame_layout())

    def draw_frames(self, records, pick=None, out=None, obs_format=None):
        """Draw kept frames (include/memgym.h: mg_draw_frames): row j of the result is the frame of record pick[j] (pick=None: record j), in
        `obs_format` (default: the handle's) -- bit for bit what `obs` showed when the record was saved, or what a handle of that format would have
        shown.  records: a FrameRecords (its layout is checked: ValueError if stale, before anything is launched) or a plain uint8 tensor, viewed as
        [n_records, frame_record_bytes].  pick: an integer tensor / list of any length, duplicates allowed; an entry outside the records leaves its row
        untouched and raises error bit 512.  out: a contiguous tensor [count] + shape of the format to draw into (a network's input tensor).  One
        raster launch on the current stream; nothing synchronises, nothing of the handle changes."""
        self._require_started("draw_frames")
        fmt = self.obs_format if obs_format is None else obs_format
        rows, pick, count, (dt, shape) = check_frame_draw(records, self.frame_layout(), self.frame_record_bytes, pick, out, fmt, self.device)
        if out is None:
            out = torch.empty((count,) + shape, dtype=dt, device=self.device)
        if rows.device != self.device or out.device != self.device or rows.data_ptr() % 16 or out.data_ptr() % 16:
            raise ValueError("draw_frames: records and out must be 16-byte aligned tensors on %s" % (self.device,))
        with torch.cuda.device(self.device):
            _native.check(_native.LIB.mg_draw_frames(self._h, rows.data_ptr(), rows.shape[0], None if pick is None else pick.data_ptr(), count,
                                                     self.OBS_FORMATS[fmt][0], out.data_ptr(), self._stream()), "mg_draw_frames")
        return out

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
            _native.check(_native.LIB.mg_split_episodes(self._h, d8.data_ptr(), K, None if steps is None else steps.data_ptr(),
                                                        None if starts is None else starts.data_ptr(), L, table.data_ptr() if capacity else None,
                                                        capacity, count.data_ptr(), self._stream()), "mg_split_episodes")
        return EpisodeSequences(table, count, L, K, self.num_envs, self)

    def draw_frames_padded(self, records, pick, out=None, obs_format=None):
        """draw_frames with padding rows (include/memgym.h: mg_draw_frames_padded): a pick below 0 writes its row as zeros, every byte, and is no
        error.  Everything else -- the arguments, the checks, a pick at or beyond the records (row untouched, error bit 512), the single raster
        launch -- is draw_frames; pick=None equals it."""
        self._require_started("draw_frames_padded")
        fmt = self.obs_format if obs_format is None else obs_format
        rows, pick, count, (dt, shape) = check_frame_draw(records, self.frame_layout(), self.frame_record_bytes, pick, out, fmt, self.device)
        if out is None:
            out = torch.empty((count,) + shape, dtype=dt, device=self.device)
        if count == 0:  # nothing to draw (an empty tensor has no address to hand to the library)
            return out
        if rows.device != self.device or out.device != self.device or rows.data_ptr() % 16 or out.data_ptr() % 16:
            raise ValueError("draw_frames_padded: records and out must be 16-byte aligned tensors on %s" % (self.device,))
        with torch.cuda.device(self.device):
            _native.check(_native.LIB.mg_draw_frames_padded(self._h, rows.data_ptr(), rows.shape[0], None if pick is None else pick.data_ptr(), count,
                                                            self.OBS_FORMATS[fmt][0], out.data_ptr(), self._stream()), "mg_draw_frames_padded")
        return out

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
            if not (isinstance(frames.frames, torch.Tensor) and frames.frames.dim() == 3):
                raise ValueError("%s: the trace keeps no frames" % what)
            if (frames.steps, frames.num_envs) != (seqs.steps, seqs.num_envs):
                raise ValueError("%s: the trace holds %d steps of %d instances, the sequences were cut from %d steps of %d"
                                 % (what, frames.steps, frames.num_envs, seqs.steps, seqs.num_envs))
            frames = FrameRecords(frames.frames, frames.frame_layout)
        fmt = self.obs_format if obs_format is None else obs_format
        if fmt not in self.OBS_FORMATS:
            raise ValueError("%s: obs_format must be one of %s" % (what, sorted(self.OBS_FORMATS)))
        _, dt, shape = self.OBS_FORMATS[fmt]
        n_rec = (frames.records if isinstance(frames, FrameRecords) else frames)
        if isinstance(n_rec, torch.Tensor) and n_rec.dim() >= 2 and n_rec.numel() // max(1, int(n_rec.shape[-1])) < (seqs.steps + 1) * seqs.num_envs:
            raise ValueError("%s: frames holds fewer than (%d + 1) * %d records" % (what, seqs.steps, seqs.num_envs))
        pick, mask = seqs.picks(sel)
        M, L = int(pick.shape[0]), seqs.length
        if out is not None:
            if not (isinstance(out, torch.Tensor) and out.dtype == dt and tuple(out.shape) == (M, L) + shape and out.is_contiguous()):
                raise ValueError("%s: out must be a contiguous %s tensor of shape %s" % (what, dt, (M, L) + shape))
            flat = out.view((M * L,) + shape)
        else:
            flat = None
        flat = self.draw_frames_padded(frames, pick.view(-1), out=flat, obs_format=fmt)
        return flat.view((M, L) + shape), mask

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
            _native.check(_native.LIB.mg_episode_positions(self._h, d8.data_ptr(), K, None if steps is None else steps.data_ptr(),
                                                           None if pos0 is None else pos0.data_ptr(), pos.data_ptr(), self._stream()), "mg_episode_positions")
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
                _native.check(_native.LIB.mg_gather_rows_padded(self._h, x.data_ptr(), int(x.shape[0]), row_bytes, None if pick is None else pick.data_ptr(),
                                                                count, out.data_ptr(), self._stream()), "mg_gather_rows_padded")
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
        fmt = self.obs_format if obs_format is None else obs_format
        if fmt not in self.OBS_FORMATS:
            raise ValueError("%s: obs_format must be one of %s" % (what, sorted(self.OBS_FORMATS)))
        _, dt, shape = self.OBS_FORMATS[fmt]
        pick, mask, length = windows.picks(sel)
        M, W = int(pick.shape[0]), windows.window
        if out is not None:
            if not (isinstance(out, torch.Tensor) and out.dtype == dt and tuple(out.shape) == (M, W) + shape and out.is_contiguous()):
                raise ValueError("%s: out must be a contiguous %s tensor of shape %s" % (what, dt, (M, W) + shape))
            flat = out.view((M * W,) + shape)
        else:
            flat = None
        flat = self.draw_frames_padded(frames, pick.view(-1), out=flat, obs_format=fmt)
        return flat.view((M, W) + shape), mask, length

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
        nbytes = self.frame_record_bytes
        if out is not None and isinstance(out, FrameRecords) and not isinstance(out, DebugFrameRecords):
            raise ValueError("save_debug_frames: out holds frame records (save_frames), not debug-view records")
        idx, k, rows = check_frame_save(nbytes, self.num_envs, idx, out, self.device)
        if rows is None:
            out = rows = torch.empty((k, nbytes), dtype=torch.uint8, device=self.device)
        if rows.device != self.device or rows.data_ptr() % 16:
            raise ValueError("save_debug_frames: out must be a 16-byte aligned tensor on %s" % (self.device,))
        with torch.cuda.device(self.device):
            _native.check(_native.LIB.mg_save_debug_frames(self._h, None if idx is None else idx.data_ptr(), k, rows.data_ptr(), self._stream()),
                          "mg_save_debug_frames")
        if isinstance(out, DebugFrameRecords):
            out.layout = self.frame_layout()
            return out
        return DebugFrameRecords(out, self.frame_layout())

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
        if isinstance(records, FrameRecords):
            if not isinstance(records, DebugFrameRecords):
                raise ValueError("%s: these are frame records (save_frames): draw_frames draws them" % what)
            if records.layout != self.frame_layout():
                raise ValueError("%s: the records (layout 0x%x) were saved from another handle, or before something changed that they would draw differently "
                                 "(layout 0x%x now): debug-view records are valid for the handle and the atlas they were saved under"
                                 % (what, records.layout, self.frame_layout()))
            records = records.records
        rows = _frame_rows(what, "records", records, self.frame_record_bytes)
        if pick is not None:
            pick = _instance_index(what, "pick", pick, self.device)
        count = rows.shape[0] if pick is None else pick.numel()
        if count > 0 and rows.shape[0] < 1:
            raise ValueError("%s: no records to draw from" % what)
        shape = (count,) + self.DEBUG_SIZES[size]
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and tuple(out.shape) == shape and out.is_contiguous()):
            raise ValueError("%s: out must be a contiguous uint8 tensor of shape %s" % (what, shape))
        if count == 0:  # nothing to draw (an empty tensor has no address to hand to the library)
            return out
        if rows.device != self.device or out.device != self.device or rows.data_ptr() % 16 or out.data_ptr() % 16:
            raise ValueError("%s: records and out must be 16-byte aligned tensors on %s" % (what, self.device))
        with torch.cuda.device(self.device):
            _native.check(_native.LIB.mg_draw_debug_frames(self._h, rows.data_ptr(), rows.shape[0], None if pick is None else pick.data_ptr(), count,
                                                           int(size), out.data_ptr(), self._stream()), "mg_draw_debug_frames")
        return out

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
        if snap.records.device != self.device or snap.records.data_ptr() % 16:
            raise ValueError("load_instances: snapshot.records must be a 16-byte aligned tensor on %s" % (self.device,))
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
                _native.check(_native.LIB.mg_load_instances(self._h, None if ci is None else ci.data_ptr(), None if cr is None else cr.data_ptr(), k,
                                                            snap.records.data_ptr(), obs_ptr, self._stream()), "mg_load_instances")
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
        src = _instance_index("copy_instances", "src", src, self.device)
        dst = _instance_index("copy_instances", "dst", dst, self.device)
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
                    while len(self._set_params) <= k:
                        self._set_params.append({})
                    if k > 0 and p:  # (an empty entry: a slot that was never filled or half-written when the checkpoint was taken)
                        self._set_params[k] = {}
                        self._write_set(k, process_reset_params(self.env_id, {kk: vv for kk, vv in p.items() if kk in DEFAULTS[self.env_id]}))
                if self._set_of is None:
                    self._set_of = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
                    _native.check(_native.LIB.mg_bind_option_sets(self._h, self._set_of.data_ptr()), "mg_bind_option_sets")
                self._set_of.copy_(torch.as_tensor(np.asarray(sd["set_of"], dtype=np.int32), device=self.device))
            elif self._set_of is not None:  # the checkpoint was taken with one option set: back to that arrangement
                _native.check(_native.LIB.mg_bind_option_sets(self._h, None), "mg_bind_option_sets")
                self._set_of = None
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
        io = _native.SingleIO()
        io.struct_size = C.sizeof(_native.SingleIO)
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
