"""Shared referee of the image-order observation formats (bf16_chw, f16_chw, f32_chw, u8_chw): what tests/test_gpu_chw_final.py,
test_gpu_spot_chw.py, test_gpu_emp_chw.py, test_gpu_u8_chw.py, test_gpu_graph_capture.py and the worker tests/chw_worker.py have in common,
each written once.  A plain helper module like tests/gpu_parity.py: no tests of its own; tests/test_chw_referee.py shows without a GPU that
the comparisons here reject what they must.

Floats are compared EXACTLY: a float observation is the oracle's uint8 [x][y][c] frame / np.float32(255) transposed to [c][y][x], the 16-bit
formats that quotient rounded -- a table of 256 values (unit_values; tests/test_float_bytes.py), no tolerance."""
import functools

import numpy as np

CHW = ("bf16_chw", "f16_chw", "f32_chw", "u8_chw")
FLOATS = CHW[:3]
SENTINEL = {"u8_chw": 0x5A, "bf16_chw": -3.0, "f16_chw": -3.0, "f32_chw": -3.0}  # (no observation holds either value)

# reset options under which episodes end within a few steps (terminal observations, resets inside the run)
SHORT = {"MortarMayhem-Grid-v0": {"command_count": [2], "command_show_duration": [1], "command_show_delay": [0], "explosion_delay": [2],
                                  "explosion_duration": [1]},
         "Endless-MortarMayhem-v0": {"command_show_duration": [1], "command_show_delay": [0], "explosion_delay": [2], "explosion_duration": [1],
                                     "max_steps": 14},
         "MysteryPath-Grid-v0": {"max_steps": 7},
         "MysteryPath-v0": {"max_steps": 7},  # (max_steps, like the grid variant)
         "SearingSpotlights-v0": {"max_steps": 9, "agent_health": 1}}
SHORT["MortarMayhem-v0"] = SHORT["MortarMayhem-Grid-v0"]  # (the grid variant's)


# ---- the formats

def unit_values(fmt):
    """torch tensor [256]: what the format stores for the bytes 0 .. 255"""
    import torch

    q = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255))
    return q.to({"f32_chw": torch.float32, "f16_chw": torch.float16, "bf16_chw": torch.bfloat16}[fmt])


def float_rows_to_bytes(rows):
    """float tensor [k][3][84 y][84 x] (any of the three formats, any device) -> uint8 tensor [k][84 x][84 y][3], the oracle's frame order"""
    import torch

    return torch.round(rows.to(torch.float32) * 255.0).to(torch.uint8).permute(0, 3, 2, 1).contiguous()


def converted(fmt, frames):
    """uint8 [k][x][y][c] (numpy array or tensor, any device) -> what the format holds for these frames, a tensor [k][3][y][x] on the same
    device: the table's value for every byte (in chunks: the index tensor is 8 bytes per element)"""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(frames)) if isinstance(frames, np.ndarray) else frames
    t = t.permute(0, 3, 2, 1)
    if fmt == "u8_chw":
        return t.contiguous()
    lut = unit_values(fmt).to(t.device)
    out = torch.empty(t.shape, dtype=lut.dtype, device=t.device)
    for i in range(0, t.shape[0], 2048):
        out[i:i + 2048] = lut[t[i:i + 2048].long()]
    return out


def rows_to_bytes(fmt, rows):
    """rows in format `fmt` [k][3][y][x] -> uint8 [k][x][y][c], what tests/frame_digest.py digests"""
    return rows.permute(0, 3, 2, 1).contiguous() if fmt == "u8_chw" else float_rows_to_bytes(rows)


def exact_bytes(fmt, rows, what):
    """rows_to_bytes, exactly: every value must be the table's value of its byte"""
    import torch

    b = rows_to_bytes(fmt, rows)
    assert torch.equal(converted(fmt, b), rows), "%s hold a value no byte maps to" % what
    return b


def same_as_the_oracle(fmt, rows, frames, digest, what):
    """rows in format `fmt` against the oracle's frames, byte for byte, or (frames None) turned back into bytes, exactly, against its digests"""
    import frame_digest as fd
    import torch

    if frames is not None:
        assert torch.equal(rows.cpu(), converted(fmt, frames)), "%s differ from the oracle's" % what
    else:
        bad = fd.differing(fd.digest_torch(exact_bytes(fmt, rows, what)), digest)
        assert len(bad) == 0, "%s differ from the oracle's (rows %s)" % (what, bad[:8])


# ---- lock step with the oracle

def frozen(options):
    """reset options in a hashable form (oracle_run is cached on its arguments); dict(frozen(o)) holds o's lists as tuples"""
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in (options or {}).items()))


@functools.lru_cache(maxsize=1)
def oracle_run(env_id, n, steps, options, frames, seed0=31, action_seed=6):
    """The oracle's run of `steps` auto-reset steps of n instances under dict(options) (see frozen), seeds arange(n) + seed0, actions from
    PCG64(action_seed); computed once per case and shared by the formats, and nothing changes it afterwards.
    -> (seeds, first, run): first = (the reset frames or None, their digests); run = per step (actions, frames or None, digest, final_digest,
    reward, done, ground_truth float32 or None where the id has none).  frames=True: two batches in lock step, one returns the frames, one
    the digests."""
    import oracle_lib

    dig = oracle_lib.OracleBatch(env_id, n, options=dict(options))
    pix = oracle_lib.OracleBatch(env_id, n, options=dict(options)) if frames else None
    seeds = np.arange(n, dtype=np.int64) + seed0
    first = (pix.reset(seeds) if pix else None, dig.reset_digest(seeds))
    prng = np.random.Generator(np.random.PCG64(action_seed))
    run = []
    for _ in range(steps):
        a = (prng.integers(0, 4, n) if dig.discrete else prng.integers(0, 3, (n, 2))).astype(np.int32)
        dg, fdg, rew, done = dig.step_digest(a, autoreset=True)
        fr = None
        if pix:
            fr, rew2, done2 = pix.step(a, autoreset=True)
            assert np.array_equal(rew, rew2) and np.array_equal(done, done2)
        gt = np.stack([e.gt() for e in dig.envs]).astype(np.float32) if dig.envs[0].gt_dim else None
        run.append((a, fr, dg, fdg, rew, done, gt))
    dig.close()
    if pix:
        pix.close()
    return seeds, first, run


def check_step(what, fmt, t, got, want, final):
    """Step t of a handle against the oracle.  got = (obs, reward, done, info) as step() returned them (tensors on any device); want = the
    step's tuple of oracle_run.  final: info["final_observation"] held SENTINEL[fmt] in every row before the step.  -> the done flags, on the host"""
    obs, r, d, info = got
    _, frames, digest, final_digest, rew, done, gt = want
    d_host = d.cpu().numpy()
    assert np.array_equal(d_host, done.astype(bool)), "%s: dones differ at step %d" % (what, t)
    assert np.array_equal(r.cpu().numpy(), rew.astype(np.float32)), "%s: rewards differ at step %d" % (what, t)
    same_as_the_oracle(fmt, obs, frames, digest, "%s: frames at step %d" % (what, t))
    if gt is not None:
        assert np.array_equal(info["ground_truth"].cpu().numpy(), gt), "%s: ground truth differs at step %d" % (what, t)
    if final:
        rows = info["final_observation"]
        if d_host.any():
            same_as_the_oracle(fmt, rows[d], None, final_digest[d_host], "%s: terminal frames at step %d" % (what, t))
        assert bool((rows[~d] == SENTINEL[fmt]).all()), "%s: a row of a running instance was written at step %d" % (what, t)
    return d_host


def lock_step_with_the_oracle(env_id, fmt, n, steps, options, frames=True, final=True, make=None, **inputs):
    """Every step of a handle against oracle_run (`inputs`: its seed0 / action_seed): reset frames, dones, rewards, frames (frames=True: byte
    for byte, else by digest), ground truth where the id has one and, final=True, terminal rows by digest and sentinel rows.  `make`:
    memory_gym_amd.make, or a stand-in for it.  -> (finished rows seen, running rows seen, most finished in one step, the handle, still open)"""
    if make is None:
        import memory_gym_amd

        make = memory_gym_amd.make
    seeds, first, run = oracle_run(env_id, n, steps, frozen(options), frames, **inputs)
    env = make(env_id, num_envs=n, device=0, obs_format=fmt, final_observation=final)
    what = "%s %s" % (env_id, fmt)
    same_as_the_oracle(fmt, env.reset(seed=seeds, options=options)[0], first[0], first[1], "%s: reset frames" % what)
    n_done = n_running = most = 0
    for t, want in enumerate(run):
        if final:
            env.final_obs.fill_(SENTINEL[fmt])
        obs, r, d, _, info = env.step(want[0])
        k = int(check_step(what, fmt, t, (obs, r, d, info), want, final).sum())
        n_done, n_running, most = n_done + k, n_running + n - k, max(most, k)
    env.check_errors()
    return n_done, n_running, most, env


# ---- lock step with a u8_xyc handle of this library

def _split(obs):
    """MortarMayhemB* return the reference's Dict observation."""
    return (obs["visual_observation"], obs["vector_observation"]) if isinstance(obs, dict) else (obs, None)


def lock_step_with_a_twin(env_id, fmt, n, steps, options=None, final=True, seed=21, action_seed=4, between=None):
    """Two handles of one id, u8_xyc (the twin) and fmt, given the same actions, drawn on the device from Generator(action_seed): frames
    through converted (the vector observation too where there is one), rewards, dones and, final=True, the terminal rows of finished instances
    and the sentinel rows of running ones.  between(t, twin, env, generator) runs before step t.
    -> (finished instances step by step, the twin, the handle -- both still open)"""
    import memory_gym_amd
    import torch

    twin, env = (memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format=f, final_observation=final) for f in ("u8_xyc", fmt))
    g = torch.Generator(device="cuda").manual_seed(action_seed)
    what = "%s %s" % (env_id, fmt)

    def same_observations(o_x, o_c, where):
        (f_x, v_x), (f_c, v_c) = _split(o_x), _split(o_c)
        assert torch.equal(f_c, converted(fmt, f_x)), "%s: frames differ %s" % (what, where)
        assert v_x is None or torch.equal(v_c, v_x), "%s: vector observation differs %s" % (what, where)

    same_observations(twin.reset(seed=seed, options=options)[0], env.reset(seed=seed, options=options)[0], "after the reset")
    discrete = env.action_dim == 1
    finished = []
    for t in range(steps):
        if between:
            between(t, twin, env, g)
        a = torch.randint(0, 4 if discrete else 3, (n,) if discrete else (n, 2), device="cuda", generator=g, dtype=torch.int32)
        if final:
            env.final_obs.fill_(SENTINEL[fmt])
        (o_x, r_x, d_x, _, i_x), (o_c, r_c, d_c, _, i_c) = twin.step(a), env.step(a)
        assert torch.equal(r_x, r_c) and torch.equal(d_x, d_c), "%s: rewards / dones differ after step %d" % (what, t)
        same_observations(o_x, o_c, "after step %d" % t)
        if final:
            f_x, f_c = i_x["final_observation"], i_c["final_observation"]
            assert torch.equal(f_c[d_c], converted(fmt, f_x[d_x])), "%s: terminal frames differ after step %d" % (what, t)
            assert bool((f_c[~d_c] == SENTINEL[fmt]).all()), "%s: a row of a running instance was written at step %d" % (what, t)
        finished.append(int(d_c.sum()))
    return finished, twin, env


def two_option_sets_keep_the_generic_path(env_id, options, second_set, steps, counter):
    """Per-instance option sets (the second half of 64 instances runs under `second_set`): a bf16_chw handle and its twin keep terminal
    observations on mg_step's generic path, and the counters say so -- final_obs_generic_steps == steps, `counter` == 0."""
    import torch

    n = 64

    def second_half(t, twin, env, g):
        if t == 0:
            mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
            mask[n // 2:] = 1
            for e in (twin, env):
                e.reset(options=second_set, mask=mask)

    finished, twin, env = lock_step_with_a_twin(env_id, "bf16_chw", n, steps, options, seed=5, action_seed=7, between=second_half)
    assert sum(finished) > 0
    for e in (twin, env):
        assert e.debug_counter("final_obs_generic_steps") == steps
        assert e.debug_counter(counter) == 0
        e.check_errors()
        e.close()


# ---- graph capture

def clones(out, final=False):
    """what a graph test keeps of a step: (obs, reward, done) and, final=True, info["final_observation"], cloned"""
    return tuple(x.clone() for x in out[:3] + ((out[4]["final_observation"],) if final else ()))


def replay_captured(env, acts, keep, warmed_up=None):
    """torch's graph recipe on a handle that has been reset: one step as warm-up on a side stream, back to the snapshot, capture of
    keep(env.step(a)) for every a of acts, back to the snapshot (capture does not execute: the state is still the snapshot; made explicit),
    replay, synchronise.  warmed_up() runs right before the capture (for a counter's value then).  -> the kept outputs"""
    import torch

    snap = env.state_dict()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.step(acts[0])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    env.load_state_dict(snap)
    if warmed_up:
        warmed_up()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = [keep(env.step(a)) for a in acts]
    env.load_state_dict(snap)
    graph.replay()
    torch.cuda.synchronize()
    return outs


def same_steps(want, outs):
    """(obs, reward, done) of every replayed step equal the expected ones"""
    import torch

    assert len(want) == len(outs)
    for k, (w, o) in enumerate(zip(want, outs)):
        assert all(torch.equal(x, y) for x, y in zip(w[:3], o[:3])), "step %d of the replay differs" % k
