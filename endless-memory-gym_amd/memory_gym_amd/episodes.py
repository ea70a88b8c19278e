"""What split_episodes and episode_windows return -- a rollout's episode sequences and its sliding memory windows -- with the argument checks that
need no handle; and rollout_targets, the advantages and returns of a rollout, a function over the handle."""
import numpy as np
import torch

from . import _native
from ._args import MAX_PICK, done_rows, done_view, index_tensor, per_instance_int32, plain_int, ptr, same_device
from .records import FrameRecords, RolloutTrace, trace_frame_records


def _pick_rows(what, noun, env, sel, m, most):
    """The sel / m arguments of a picks() call -> (sel as an int32 tensor on the handle's device or None, the number of rows M).  The caller has put
    its default into `m` where both were None; most: the largest m it takes (None: any)."""
    if env is None:
        raise ValueError("%s: these %s belong to no handle" % (what, noun))
    if sel is not None:
        if m is not None:
            raise ValueError("%s: give sel or m, not both" % what)
        sel = index_tensor(what, "sel", sel, env.device)
        return sel, sel.numel()
    return None, plain_int(what, "m", m, 0, most, name_most=most is not None)


def _rollout_rows(what, x, steps, num_envs):
    """ValueError unless x is a tensor [K, N, ...] or [K + 1, N, ...] of the rollout"""
    if not (isinstance(x, torch.Tensor) and x.dim() >= 2 and int(x.shape[0]) in (steps, steps + 1) and int(x.shape[1]) == num_envs):
        raise ValueError("%s: x must be a tensor [%d or %d, %d, ...]" % (what, steps, steps + 1, num_envs))


def check_split_episodes(done, length, num_envs, steps=None, starts=None, capacity=None, device=None):
    """The argument checks of split_episodes, which need no handle: -> (done as a uint8 view [K, N], K, length, steps as an int32 tensor [N] or None,
    starts as a uint8 view [N] or None, capacity as an int or None).  ValueError for a `done` that is no contiguous bool / uint8 tensor [K, N] with
    K >= 1 and N = num_envs, a length below 1, (K + 1) * N beyond an int32, `steps` that is no int32 / int64 tensor [N], `starts` that is no contiguous
    bool / uint8 tensor [N], a negative capacity, and anything that does not lie on `device` (if given)."""
    what = "split_episodes"
    K, N = done_rows(what, done, num_envs)
    if (K + 1) * N > MAX_PICK:
        raise ValueError("%s: (K + 1) * N = %d does not fit the int32 of a pick: split slices of the rollout" % (what, (K + 1) * N))
    d8 = done_view(what, done)
    length = plain_int(what, "length", length, 1)
    same_device(what, "done", done, device)
    steps = per_instance_int32(what, "steps", steps, N, device, " (e.g. what play() returned as steps_played)")
    if starts is not None:
        if not (isinstance(starts, torch.Tensor) and starts.dtype in (torch.bool, torch.uint8) and tuple(starts.shape) == (N,) and starts.is_contiguous()):
            raise ValueError("%s: starts must be a contiguous bool or uint8 tensor [%d]" % (what, N))
        same_device(what, "starts", starts, device)
        starts = starts.view(torch.uint8)
    if capacity is not None:
        capacity = plain_int(what, "capacity", capacity, 0)
    return d8, K, length, steps, starts, capacity


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
        if env is not None and sel is None and m is None:
            m = len(self)
        sel, M = _pick_rows(what, "sequences", env, sel, m, None)
        if M * self.length > MAX_PICK:
            raise ValueError("%s: %d rows of %d picks do not fit one call" % (what, M, self.length))
        pick = torch.empty((M, self.length), dtype=torch.int32, device=env.device)
        mask = torch.empty((M, self.length), dtype=torch.bool, device=env.device)
        if M:
            with torch.cuda.device(env.device):
                _native.check(_native.LIB.mg_sequence_picks(env._h, self.table.data_ptr() if self.capacity else None, self.count.data_ptr(), self.capacity,
                                                            ptr(sel), M, self.length, pick.data_ptr(), mask.data_ptr(), env._stream()), "mg_sequence_picks")
        return pick, mask

    def gather(self, x, sel=None):
        """x [K, N, ...] (actions, labels, reward, done) or [K + 1, N, ...] (per-frame data) -> [M, L, ...], zero at the pads: x flattened over its
        first two dimensions, indexed with picks(sel)."""
        _rollout_rows("EpisodeSequences.gather", x, self.steps, self.num_envs)
        pick, mask = self.picks(sel)
        rows = x.reshape((-1,) + tuple(x.shape[2:]))[pick.clamp(min=0).long()]
        return torch.where(mask.reshape(mask.shape + (1,) * (x.dim() - 2)), rows, torch.zeros_like(rows))


def check_episode_windows(done, window, num_envs, lag=0, back=0, steps=None, pos0=None, device=None):
    """The argument checks of episode_positions / episode_windows, which need no handle: -> (done as a uint8 view [K, N], K, window, lag, back, steps as
    an int32 tensor [N] or None, pos0 as an int32 tensor [N] or None).  ValueError for a `done` that is no contiguous bool / uint8 tensor [K, N] with
    K >= 1 and N = num_envs, a window below 1, a negative lag or back, (back + K + 1) * N beyond an int32, `steps` / `pos0` that are no int32 / int64
    tensors [N], and anything that does not lie on `device` (if given)."""
    what = "episode_windows"
    K, N = done_rows(what, done, num_envs)
    window, lag, back = plain_int(what, "window", window, 1), plain_int(what, "lag", lag, 0), plain_int(what, "back", back, 0)
    if (back + K + 1) * N > MAX_PICK:
        raise ValueError("%s: (back + K + 1) * N = %d does not fit the int32 of a pick: take slices of the rollout" % (what, (back + K + 1) * N))
    d8 = done_view(what, done)
    same_device(what, "done", done, device)
    return d8, K, window, lag, back, per_instance_int32(what, "steps", steps, N, device), per_instance_int32(what, "pos0", pos0, N, device)


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
    same_device(what, "x", x, device)
    if pick is not None:
        pick = index_tensor(what, "pick", pick, x.device, one_dim=False)
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
        samples = (self.steps + 1) * self.num_envs
        if sel is None and m is None:
            m = samples
        sel, M = _pick_rows(what, "windows", env, sel, m, samples)
        if M * self.window > MAX_PICK:
            raise ValueError("%s: %d rows of %d picks do not fit one call" % (what, M, self.window))
        pick = torch.empty((M, self.window), dtype=torch.int32, device=env.device)
        mask = torch.empty((M, self.window), dtype=torch.bool, device=env.device)
        length = torch.empty((M,), dtype=torch.int32, device=env.device)
        if M:
            with torch.cuda.device(env.device):
                _native.check(_native.LIB.mg_window_picks(env._h, self.pos.data_ptr(), self.steps, ptr(sel), M, self.window, self.lag, self.back,
                                                          pick.data_ptr(), mask.data_ptr(), length.data_ptr(), env._stream()), "mg_window_picks")
        return pick, mask, length

    def store(self, x, prefix=None):
        """The store the picks index, [(back + rows of x) * N, ...]: cat(prefix, x) flattened over its first two dimensions.  x: [K, N, ...] (actions,
        rewards: a pick of row K is then out of range) or [K + 1, N, ...] (per-frame data: hidden states, values).  prefix: [back, N, ...], the last
        `back` rows of the previous rollout's x in front of its row K_prev; required when back > 0.  ValueError otherwise."""
        what = "EpisodeWindows.gather"
        _rollout_rows(what, x, self.steps, self.num_envs)
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


def _unit_interval(what, name, v):
    """v as a float; ValueError unless it is a number (no bool) in 0 .. 1"""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= 1.0:
        raise ValueError("%s: %s must be a number in 0 .. 1, got %r" % (what, name, v))
    return float(v)


def check_rollout_targets(reward, done, value, num_envs, gamma=0.99, lam=0.95, steps=None, skip=None, truncated=None, final_value=None, device=None):
    """The argument checks of rollout_targets, which need no handle: -> (reward, done as a uint8 view [K, N], value, K, gamma, lam, steps as an int32
    tensor [N] or None, skip and truncated as uint8 views [K, N] or None, final_value).  ValueError for a `done` that is no contiguous bool / uint8
    tensor [K, N] with K >= 1 and N = num_envs, (K + 1) * N beyond an int32, a `reward` / `final_value` that is no contiguous float32 tensor [K, N], a
    `value` that is no contiguous float32 tensor [K + 1, N], `skip` / `truncated` that are no contiguous bool / uint8 tensors [K, N], `steps` that is no
    int32 / int64 tensor [N], a final_value without truncated, gamma or lam outside 0 .. 1, and anything that does not lie on `device` (if given)."""
    what = "rollout_targets"
    K, N = done_rows(what, done, num_envs)
    if (K + 1) * N > MAX_PICK:
        raise ValueError("%s: (K + 1) * N = %d does not fit the int32 of a pick: take slices of the rollout" % (what, (K + 1) * N))
    d8 = done_view(what, done)
    same_device(what, "done", done, device)
    for name, t, rows in (("reward", reward, K), ("value", value, K + 1), ("final_value", final_value, K)):
        if t is None and name == "final_value":
            continue
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and tuple(t.shape) == (rows, N) and t.is_contiguous()):
            raise ValueError("%s: %s must be a contiguous float32 tensor [%d, %d]" % (what, name, rows, N))
        same_device(what, name, t, device)
    flags = []
    for name, t in (("skip", skip), ("truncated", truncated)):
        if t is not None:
            if not (isinstance(t, torch.Tensor) and t.dtype in (torch.bool, torch.uint8) and tuple(t.shape) == (K, N) and t.is_contiguous()):
                raise ValueError("%s: %s must be a contiguous bool or uint8 tensor [%d, %d]" % (what, name, K, N))
            same_device(what, name, t, device)
            t = t.view(torch.uint8)
        flags.append(t)
    if final_value is not None and truncated is None:
        raise ValueError("%s: final_value needs truncated (the ends that bootstrap from it)" % what)
    gamma, lam = _unit_interval(what, "gamma", gamma), _unit_interval(what, "lam", lam)
    return reward, d8, value, K, gamma, lam, per_instance_int32(what, "steps", steps, N, device), flags[0], flags[1], final_value


class RolloutTargets:
    """What rollout_targets returns (include/memgym.h: mg_rollout_targets / mg_sum_columns): the targets of a rollout of K steps of N
    instances.
        adv      float32 [K, N]   generalised advantage estimates, 0 where the row has no target
        ret      float32 [K, N]   adv + value, the critic's target (lam = 1: the discounted return-to-go)
        valid    bool    [K, N]   whether the row has a target
    and with moments=True
        columns  float64 [3, N]   per instance the count, the sum and the sum of squares of its valid advantages
        moments  float64 [3]      the same over all instances, summed in mg_sum_columns' fixed order
    mean() / std() / normalized() are torch expressions over `moments` on the device.  Nothing here synchronises."""
    __slots__ = ("adv", "ret", "valid", "columns", "moments")

    def __init__(self, adv, ret, valid, columns=None, moments=None):
        self.adv, self.ret, self.valid, self.columns, self.moments = adv, ret, valid, columns, moments

    def _need_moments(self, what):
        if self.moments is None:
            raise ValueError("RolloutTargets.%s: these targets were made without moments=True" % what)
        return self.moments

    def mean(self):
        """the mean of the valid advantages, a float64 scalar on the device (nan where no row is valid)"""
        m = self._need_moments("mean")
        return m[1] / m[0]

    def std(self):
        """the standard deviation of the valid advantages (the population's: divided by the count), a float64 scalar on the device"""
        m = self._need_moments("std")
        mean = m[1] / m[0]
        return (m[2] / m[0] - mean * mean).clamp(min=0.0).sqrt()

    def normalized(self, eps=1e-8):
        """(adv - mean()) / (std() + eps) as float32 [K, N], 0 where the row has no target"""
        self._need_moments("normalized")
        z = ((self.adv.double() - self.mean()) / (self.std() + eps)).float()
        return torch.where(self.valid, z, torch.zeros_like(z))


def check_targets_out(out, steps, num_envs, moments, device=None):
    """ValueError unless `out` is a RolloutTargets whose tensors have the shapes and dtypes of its docstring for K = steps and N = num_envs, are
    contiguous and lie on `device` (if given); with moments its columns and moments too."""
    what = "rollout_targets"
    if not isinstance(out, RolloutTargets):
        raise ValueError("%s: out must be a RolloutTargets (what an earlier call returned)" % what)
    want = [("adv", torch.float32, (steps, num_envs)), ("ret", torch.float32, (steps, num_envs)), ("valid", torch.bool, (steps, num_envs))]
    if moments:
        want += [("columns", torch.float64, (3, num_envs)), ("moments", torch.float64, (3,))]
    for name, dt, shape in want:
        t = getattr(out, name)
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous()):
            raise ValueError("%s: out.%s must be a contiguous %s tensor of shape %s" % (what, name, dt, shape))
        same_device(what, "out." + name, t, device)
    return out


def rollout_targets(env, reward, done, value, gamma=0.99, lam=0.95, steps=None, skip=None, truncated=None, final_value=None, out=None, moments=False):
    """Advantages, returns and their valid mask of a rollout (include/memgym.h: mg_rollout_targets) -> RolloutTargets.  env: the VecMemoryGym handle
    (of a GymnasiumVectorEnv: its `.env`).  reward: float32 [K, N] and
    done: bool / uint8 [K, N], e.g. trace.reward / trace.done; value: float32 [K + 1, N], the critic's value of row t of the rollout's [K + 1, N]
    frame store, row K the bootstrap value.  gamma, lam in 0 .. 1 (lam = 1: `ret` holds discounted returns-to-go).  steps: an integer tensor [N],
    the steps instance i took (play()'s steps_played), None: K for all; rows beyond it have no target.
    Same-step auto-reset needs nothing else: an episode that ends bootstraps from 0.  truncated: bool / uint8 [K, N], the ends that bootstrap from
    the terminal observation's value instead; final_value: float32 [K, N], that value (the critic on final_observations() / final_frames).  Under
    autoreset_mode="next_step" pass skip = the restart flags of step t (bool / uint8 [K, N]: the rows that reset instead of stepping have no
    target and cut the recursion) and truncated WITHOUT final_value: the terminal observation is frame row t + 1, value[t + 1] its value.
    moments=True also gives the per-instance and total count / sum / sum of squares of the valid advantages (a second small launch) for mean() /
    std() / normalized().  out: a RolloutTargets of an earlier call with the same K, N and moments, to write into.  One launch on the current
    stream; nothing synchronises, nothing is allocated in the handle: even the first call can be captured into a graph."""
    env._require_started("rollout_targets")
    reward, d8, value, K, gamma, lam, steps, skip, truncated, final_value = check_rollout_targets(reward, done, value, env.num_envs, gamma, lam, steps, skip,
                                                                                                  truncated, final_value, env.device)
    N = env.num_envs
    if out is None:
        adv, ret = (torch.empty((K, N), dtype=torch.float32, device=env.device) for _ in range(2))
        out = RolloutTargets(adv, ret, torch.empty((K, N), dtype=torch.bool, device=env.device))
        if moments:
            out.columns = torch.empty((3, N), dtype=torch.float64, device=env.device)
            out.moments = torch.empty((3,), dtype=torch.float64, device=env.device)
    else:
        check_targets_out(out, K, N, moments, env.device)
    with torch.cuda.device(env.device):
        _native.check(_native.LIB.mg_rollout_targets(env._h, reward.data_ptr(), d8.data_ptr(), value.data_ptr(), K, ptr(steps), ptr(skip), ptr(truncated),
                                                     ptr(final_value), gamma, lam, out.adv.data_ptr(), out.ret.data_ptr(), out.valid.data_ptr(),
                                                     out.columns.data_ptr() if moments else None, env._stream()), "mg_rollout_targets")
        if moments:
            _native.check(_native.LIB.mg_sum_columns(env._h, out.columns.data_ptr(), 3, out.moments.data_ptr(), env._stream()), "mg_sum_columns")
    return out


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
        return trace_frame_records(what, frames, windows.steps, windows.num_envs, "the windows were made from")
    rec = frames.records if isinstance(frames, FrameRecords) else frames
    want = (windows.back + windows.steps + 1, windows.num_envs, int(record_bytes))
    if not (isinstance(rec, torch.Tensor) and rec.dtype == torch.uint8 and tuple(rec.shape) == want and rec.is_contiguous()):
        raise ValueError("%s: frames must be a contiguous uint8 store of shape %s (back + K + 1 rows of N records)" % (what, want))
    return frames
