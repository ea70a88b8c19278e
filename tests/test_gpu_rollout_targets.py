"""GPU (-m gpu): rollout targets -- mg_rollout_targets / mg_sum_columns (include/memgym.h), memory_gym_amd.episodes.rollout_targets --
against the header's definition in numpy (tests/rollout_targets_definition.py).  Every comparison is bit for bit, on the raw integer views of the
floats: no tolerance anywhere.

Crafted columns need no stepping: one started handle per N.  Real rollouts: advance_traced at N = 200, K = 200, one id per family, and 150 expert steps
of a next-step handle."""

import numpy as np
import pytest

import rollout_targets_definition as rd

pytestmark = pytest.mark.gpu

F = np.float32
T = 16          # csrc/mg_targets.hpp TARGETS_T: the rows of a block of the walk
PATTERN = 0xA5  # every byte the device must not write
PAIRS = ((0.99, 0.95), (1.0, 1.0), (0.0, 0.5), (0.5, 0.0))
IDS = ("MortarMayhem-Grid-v0", "SearingSpotlights-v0", "Endless-MysteryPath-v0")  # one id per family
OUTPUTS = (("adv",), ("ret",), ("valid",), ("col",), ("adv", "ret", "valid", "col"))
OPTIONAL = ("steps_of", "skip", "trunc", "final_value")
_HANDLES = {}


def handle(n):
    """a started handle of n instances, shared by the tests of this module; the families take turns"""
    import memory_gym_amd

    if n not in _HANDLES:
        env = memory_gym_amd.make(IDS[len(_HANDLES) % len(IDS)], num_envs=n, device=0)
        env.reset(seed=np.arange(n, dtype=np.int64))
        _HANDLES[n] = env
    return _HANDLES[n]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for env in _HANDLES.values():
        env.check_errors()
        env.close()
    _HANDLES.clear()


def rollout_targets(env, *args, **kwargs):
    from memory_gym_amd.episodes import rollout_targets as call

    return call(env, *args, **kwargs)


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def combos():
    """every present / absent combination of steps_of, skip, trunc, final_value that is not refused"""
    return [dict(zip(OPTIONAL, (s, k, t, f))) for s in (False, True) for k in (False, True) for t, f in ((False, False), (True, False), (True, True))]


def done_patterns(K, N, g):
    at_first, at_last, edges = (np.zeros((K, N), np.uint8) for _ in range(3))
    at_first[0], at_last[K - 1] = 1, 1
    for t in range(K):  # the walk's blocks begin at t = K - 1, K - 1 - T, ...: the first row of every block, the row after it, and its last row
        if (K - 1 - t) % T in (0, 1, T - 1):
            edges[t] = 1
    return {"zeros": np.zeros((K, N), np.uint8), "ones": np.ones((K, N), np.uint8), "done at t = 0": at_first, "done at t = K - 1": at_last,
            "block edges": edges, "random": (g.random((K, N)) < 0.125).astype(np.uint8)}


def crafted(K, N, done, g):
    """finite inputs with the awkward values -- rewards 0.0, -0.0, a subnormal, 1e18, negatives; values normal with 1e18 and a subnormal -- and the
    optional arrays: flags set on done rows and elsewhere, steps_of with 0, 1, K, K + 5 and a negative entry"""
    reward = g.choice(np.array([0.0, -0.0, 1e-42, 1e18, -1.0, 0.25, -3.5, 1.0], F), size=(K, N)).astype(F)
    value = g.standard_normal((K + 1, N)).astype(F)
    value[g.random((K + 1, N)) < 0.05] = F(1e18)
    value[g.random((K + 1, N)) < 0.05] = F(1e-42)
    steps_of = g.integers(-3, K + 6, N).astype(np.int32)
    steps_of[:5] = [K, 0, 1, K + 5, -2][:N]
    return {"reward": reward, "done": done, "value": value, "steps_of": steps_of, "skip": (g.random((K, N)) < 0.1).astype(np.uint8),
            "trunc": ((g.random((K, N)) < 0.5) & ((done != 0) | (g.random((K, N)) < 0.1))).astype(np.uint8), "final_value": g.standard_normal((K, N)).astype(F)}


def c_targets(env, x, use, gamma, lam, outputs):
    """mg_rollout_targets through the C ABI.  Every output lies between two guard rows of PATTERN bytes; the outputs that are not in `outputs` are
    passed as NULL and their buffers stay where they are.  -> name -> the whole buffer on the host, guard rows included, as bytes [K + 2 or 5, ...]"""
    import torch
    from memory_gym_amd import _native

    K, N = x["reward"].shape
    ins = {k: dev(x[k]) for k in ("reward", "done", "value")}
    ins.update({k: dev(x[k]) for k in OPTIONAL if use[k]})
    bufs = {"adv": torch.full((K + 2, N * 4), PATTERN, dtype=torch.uint8, device="cuda"), "ret": torch.full((K + 2, N * 4), PATTERN, dtype=torch.uint8, device="cuda"),
            "valid": torch.full((K + 2, N), PATTERN, dtype=torch.uint8, device="cuda"), "col": torch.full((5, N * 8), PATTERN, dtype=torch.uint8, device="cuda")}
    p = lambda k: ins[k].data_ptr() if k in ins else None  # noqa: E731
    o = lambda k: bufs[k][1].data_ptr() if k in outputs else None  # noqa: E731
    rc = _native.LIB.mg_rollout_targets(env._h, p("reward"), p("done"), p("value"), K, p("steps_of"), p("skip"), p("trunc"), p("final_value"), gamma, lam,
                                        o("adv"), o("ret"), o("valid"), o("col"), env._stream())
    assert rc == 0, _native.last_error()
    torch.cuda.synchronize()
    return {k: b.cpu().numpy() for k, b in bufs.items()}


def compare(got, want, outputs, K, N, what):
    """the outputs that were asked for hold the definition's bits between untouched guard rows; the others are untouched altogether"""
    adv, ret, valid, col = want
    for name, ref, rows in (("adv", adv, K), ("ret", ret, K), ("valid", valid, K), ("col", col, 3)):
        buf = got[name]
        if name not in outputs:
            assert (buf == PATTERN).all(), "%s: %s was NULL and its neighbourhood was written" % (what, name)
            continue
        assert (buf[0] == PATTERN).all() and (buf[rows + 1:] == PATTERN).all(), "%s: a row around %s was written" % (what, name)
        body = np.ascontiguousarray(buf[1:rows + 1]).view(ref.dtype).reshape(ref.shape)
        if not rd.same_bits(body, ref):
            differs = (body.view(np.uint8).reshape(ref.shape + (-1,)) != np.ascontiguousarray(ref).view(np.uint8).reshape(ref.shape + (-1,))).any(-1)
            at = tuple(np.argwhere(differs)[0])
            pytest.fail("%s: %s differs in %d entries, first at %s: %r against %r" % (what, name, int(differs.sum()), at, body[at], ref[at]))


# ---- 1. crafted columns

@pytest.mark.parametrize("N", [1, 63, 64, 65, 200, 257])
def test_crafted_columns_equal_the_definition_bit_for_bit(N):
    env = handle(N)
    g = np.random.default_rng(977 * N)
    before = env.debug_counter("rollout_targets")
    calls, seen = 0, set()
    for ki, K in enumerate((1, 2, T - 1, T, T + 1, 2 * T + 1, 37, 1030)):
        for pi, (name, done) in enumerate(done_patterns(K, N, g).items()):
            x = crafted(K, N, done, g)
            n = ki * 6 + pi + N  # every K meets every pattern; the optional arrays, the pairs and the outputs take turns
            use, (gamma, lam), outputs = combos()[n % 12], PAIRS[(ki + pi + N) % 4], OUTPUTS[n % 5]
            opt = {k: (x[k] if use[k] else None) for k in OPTIONAL}
            want = rd.targets_rows(x["reward"], x["done"], x["value"], gamma, lam, **opt)
            what = "K %d, done %s, %s, gamma %g lam %g, outputs %s" % (K, name, sorted(k for k in use if use[k]), gamma, lam, outputs)
            compare(c_targets(env, x, use, gamma, lam, outputs), want, outputs, K, N, what)
            calls += 1
            seen.add((n % 12, n % 5))
    assert calls == 48 and len(seen) >= 40
    assert env.debug_counter("rollout_targets") == before + calls
    env.check_errors()


@pytest.mark.parametrize("pair", range(4), ids=["0.99_0.95", "1_1", "0_0.5", "0.5_0"])
def test_every_combination_of_the_optional_arrays_with_every_output_arrangement(pair):
    """K = 2T + 1 at N = 65: the twelve combinations x the five output arrangements, all bits, for one gamma / lam pair each"""
    K, N = 2 * T + 1, 65
    env = handle(N)
    g = np.random.default_rng(31 + pair)
    x = crafted(K, N, done_patterns(K, N, g)["random"], g)
    gamma, lam = PAIRS[pair]
    for use in combos():
        opt = {k: (x[k] if use[k] else None) for k in OPTIONAL}
        want = rd.targets_rows(x["reward"], x["done"], x["value"], gamma, lam, **opt)
        scalar = rd.targets_scalar(x["reward"][:, :3], x["done"][:, :3], x["value"][:, :3], gamma, lam,
                                   **{k: (None if v is None else v[:3] if k == "steps_of" else v[:, :3]) for k, v in opt.items()})
        assert all(rd.same_bits(a[:, :3], b) for a, b in zip(want, scalar))  # (the referee's own two forms, on three columns)
        for outputs in OUTPUTS:
            compare(c_targets(env, x, use, gamma, lam, outputs), want, outputs, K, N, "%s, outputs %s" % (sorted(k for k in use if use[k]), outputs))
    env.check_errors()


@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000])
def test_columns_and_their_sums_in_the_fixed_order(N):
    import torch
    from memory_gym_amd import _native

    env = handle(N)
    g = np.random.default_rng(5 * N)
    K = 37
    x = crafted(K, N, done_patterns(K, N, g)["random"], g)
    tg = rollout_targets(env, dev(x["reward"]), dev(x["done"]), dev(x["value"]), gamma=0.99, lam=0.95, steps=dev(x["steps_of"]), skip=dev(x["skip"]),
                             truncated=dev(x["trunc"]), final_value=dev(x["final_value"]), moments=True)
    adv, ret, valid, col = rd.targets_rows(x["reward"], x["done"], x["value"], 0.99, 0.95, **{k: x[k] for k in OPTIONAL})
    assert tg.valid.dtype == torch.bool and tg.columns.dtype == torch.float64 and tuple(tg.columns.shape) == (3, N) and tuple(tg.moments.shape) == (3,)
    assert rd.same_bits(tg.adv.cpu().numpy(), adv) and rd.same_bits(tg.ret.cpu().numpy(), ret) and np.array_equal(tg.valid.cpu().numpy(), valid != 0)
    assert rd.same_bits(tg.columns.cpu().numpy(), col) and rd.same_bits(tg.moments.cpu().numpy(), rd.sum_columns(col))
    # the torch expressions over them: no host round trip, the definition's numbers
    count, s, sq = rd.sum_columns(col)
    if count:
        # (a handful of double operations each, the device's division and square root among them: 1e-12 of the quantities' own scale is thousands of
        # roundings, and far below any mistake in a formula)
        mean, scale = s / count, np.sqrt(sq / count)
        std = np.sqrt(max(sq / count - mean * mean, 0.0))
        assert tg.mean().is_cuda and abs(float(tg.mean()) - mean) <= 1e-12 * scale and abs(float(tg.std()) - std) <= 1e-6 * scale
        z = tg.normalized(eps=1e-8)
        assert z.dtype == torch.float32 and z.is_cuda and not z.cpu().numpy()[valid == 0].any()
    # mg_sum_columns on its own: rows of doubles whose sum depends on the order (sixty binades), one row and five rows, guard entries around out
    rows = (g.standard_normal((5, N)) * np.exp2(g.integers(-30, 30, (5, N)))).astype(np.float64)
    rows[1] = -0.0
    for r in (1, 5):
        out = torch.full((r + 2,), 12345.0, dtype=torch.float64, device="cuda")
        assert _native.LIB.mg_sum_columns(env._h, dev(rows).data_ptr(), r, out[1:].data_ptr(), env._stream()) == 0, _native.last_error()
        got = out.cpu().numpy()
        assert got[0] == 12345.0 and got[r + 1] == 12345.0 and rd.same_bits(got[1:r + 1], rd.sum_columns(rows[:r])), (N, r)
    env.check_errors()


# ---- 2. the full size

def test_the_full_size_with_every_optional_array():
    import torch

    K, N = 128, 65536
    env = handle(N)
    g = np.random.default_rng(65536)
    x = crafted(K, N, (g.random((K, N)) < 0.125).astype(np.uint8), g)
    tg = rollout_targets(env, dev(x["reward"]), dev(x["done"]), dev(x["value"]), gamma=0.99, lam=0.95, steps=dev(x["steps_of"]), skip=dev(x["skip"]),
                             truncated=dev(x["trunc"]), final_value=dev(x["final_value"]), moments=True)
    torch.cuda.synchronize()
    adv, ret, valid, col = rd.targets_rows(x["reward"], x["done"], x["value"], 0.99, 0.95, **{k: x[k] for k in OPTIONAL})
    assert rd.same_bits(tg.adv.cpu().numpy(), adv) and rd.same_bits(tg.ret.cpu().numpy(), ret) and np.array_equal(tg.valid.cpu().numpy(), valid != 0)
    assert rd.same_bits(tg.columns.cpu().numpy(), col) and rd.same_bits(tg.moments.cpu().numpy(), rd.sum_columns(col))
    env.check_errors()


# ---- 3. real rollouts

@pytest.mark.parametrize("env_id", IDS)
def test_the_targets_of_a_traced_rollout(env_id):
    import memory_gym_amd
    import torch

    N, K = 200, 200
    env = memory_gym_amd.make(env_id, num_envs=N, device=0)
    env.reset(seed=np.arange(N, dtype=np.int64))
    ro = env.new_rollout(K)
    env.advance_traced(ro, eps=0.1, seed=3, step=0, render=False, stats=False)
    value = torch.randn((K + 1, N), generator=torch.Generator().manual_seed(7)).cuda()
    reward, done = ro.reward.cpu().numpy(), ro.done.cpu().numpy()
    assert done.any() and (reward != 0).any(), "the trace holds no ended episode or no reward: it tests nothing"
    tg = rollout_targets(env, ro.reward, ro.done, value, moments=True)
    adv, ret, valid, col = rd.targets_rows(reward, done, value.cpu().numpy(), 0.99, 0.95)
    assert rd.same_bits(tg.adv.cpu().numpy(), adv) and rd.same_bits(tg.ret.cpu().numpy(), ret) and tg.valid.all()
    assert rd.same_bits(tg.columns.cpu().numpy(), col) and rd.same_bits(tg.moments.cpu().numpy(), rd.sum_columns(col))
    # discounted returns-to-go at lam = 1, into the same tensors
    again = rollout_targets(env, ro.reward, ro.done, value, gamma=0.5, lam=1.0, out=tg, moments=True)
    assert again is tg and rd.same_bits(tg.ret.cpu().numpy(), rd.targets_rows(reward, done, value.cpu().numpy(), 0.5, 1.0)[1])
    env.check_errors()
    env.close()


def test_a_next_step_handle_skips_its_reset_rows():
    import memory_gym_amd
    import torch

    N, K = 48, 150
    env = memory_gym_amd.make("MortarMayhem-Grid-v0", num_envs=N, device=0, autoreset_mode="next_step")
    env.reset(seed=np.arange(N, dtype=np.int64))
    reward = torch.zeros((K, N), dtype=torch.float32, device="cuda")
    done, restart = (torch.zeros((K, N), dtype=torch.bool, device="cuda") for _ in range(2))
    pending = env.done_u8.view(torch.bool).clone()  # the instances the next call restarts
    for t in range(K):
        restart[t] = pending
        _, r, d, _, _ = env.step(env.expert_actions(0.0, 0, t))
        reward[t], done[t] = r, d
        pending = d.clone()
    value = torch.randn((K + 1, N), generator=torch.Generator().manual_seed(11)).cuda()
    assert bool(done.any()) and bool(restart.any()) and bool((reward != 0).any())
    for truncated in (None, done):
        tg = rollout_targets(env, reward, done, value, skip=restart, truncated=truncated)
        want = rd.targets_rows(reward.cpu().numpy(), done.cpu().numpy(), value.cpu().numpy(), 0.99, 0.95, skip=restart.cpu().numpy(),
                               trunc=None if truncated is None else truncated.cpu().numpy())
        adv, ret, valid = tg.adv.cpu().numpy(), tg.ret.cpu().numpy(), tg.valid.cpu().numpy()
        assert rd.same_bits(adv, want[0]) and rd.same_bits(ret, want[1]) and np.array_equal(valid, want[2] != 0)
        skipped = restart.cpu().numpy()
        assert np.array_equal(valid, ~skipped) and not adv[skipped].any() and not ret[skipped].any()
    env.check_errors()
    env.close()


# ---- 4. a captured graph

def test_the_first_call_of_a_handle_can_be_captured():
    import memory_gym_amd
    import torch

    K, N = 37, 130
    env = memory_gym_amd.make(IDS[1], num_envs=N, device=0)
    env.reset(seed=np.arange(N, dtype=np.int64))
    g = np.random.default_rng(99)
    first = crafted(K, N, (g.random((K, N)) < 0.125).astype(np.uint8), g)
    second = crafted(K, N, (g.random((K, N)) < 0.3).astype(np.uint8), g)
    reward, done, value = dev(first["reward"]), dev(first["done"]), dev(first["value"])
    assert env.debug_counter("rollout_targets") == 0
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            tg = rollout_targets(env, reward, done, value, gamma=0.99, lam=0.95, moments=True)
    for x in (first, second):
        reward.copy_(dev(x["reward"]))
        done.copy_(dev(x["done"]))
        value.copy_(dev(x["value"]))
        graph.replay()
        torch.cuda.synchronize()
        adv, ret, valid, col = rd.targets_rows(x["reward"], x["done"], x["value"], 0.99, 0.95)
        assert rd.same_bits(tg.adv.cpu().numpy(), adv) and rd.same_bits(tg.ret.cpu().numpy(), ret) and tg.valid.all()
        assert rd.same_bits(tg.columns.cpu().numpy(), col) and rd.same_bits(tg.moments.cpu().numpy(), rd.sum_columns(col))
    env.check_errors()
    env.close()


# ---- 5. refusals

def test_refusals_return_minus_one_with_their_message_and_launch_nothing():
    import memory_gym_amd
    import torch
    from memory_gym_amd import _native
    from memory_gym_amd.episodes import RolloutTargets

    lib, last = _native.LIB, _native.last_error
    K, N = 6, 64
    env = handle(N)
    z = lambda rows, dt: torch.zeros((rows, N), dtype=dt, device="cuda")  # noqa: E731
    reward, done, value, flags, final = z(K, torch.float32), z(K, torch.uint8), z(K + 1, torch.float32), z(K, torch.uint8), z(K, torch.float32)
    steps_of = torch.zeros(N, dtype=torch.int32, device="cuda")
    outs = {"adv": torch.full((K, N), 7.0, device="cuda"), "ret": torch.full((K, N), 7.0, device="cuda"),
            "valid": torch.full((K, N), 7, dtype=torch.uint8, device="cuda"), "col": torch.full((3, N), 7.0, dtype=torch.float64, device="cuda")}

    def call(h=None, **kw):
        a = dict(reward=reward.data_ptr(), done=done.data_ptr(), value=value.data_ptr(), steps=K, steps_of=None, skip=None, trunc=None, final=None, gamma=0.99, lam=0.95,
                 adv=outs["adv"].data_ptr(), ret=outs["ret"].data_ptr(), valid=outs["valid"].data_ptr(), col=outs["col"].data_ptr())
        a.update(kw)
        return lib.mg_rollout_targets(env._h if h is None else h, a["reward"], a["done"], a["value"], a["steps"], a["steps_of"], a["skip"], a["trunc"], a["final"],
                                      a["gamma"], a["lam"], a["adv"], a["ret"], a["valid"], a["col"], env._stream())

    fresh = memory_gym_amd.make(IDS[0], num_envs=N, device=0)
    assert call(h=fresh._h) == -1 and "before the first" in last() and "mg_rollout_targets" in last()
    fresh.close()
    before = env.debug_counter("rollout_targets")
    nan = float("nan")
    cases = [("reward_dev is NULL", dict(reward=None)), ("done_dev is NULL", dict(done=None)), ("value_dev is NULL", dict(value=None)),
             ("all NULL", dict(adv=None, ret=None, valid=None, col=None)), ("steps < 1", dict(steps=0)), ("steps < 1", dict(steps=-2)),
             ("INT32_MAX", dict(steps=(2**31 - 1) // N)), ("gamma outside [0, 1]", dict(gamma=-0.5)), ("gamma outside [0, 1]", dict(gamma=1.5)),
             ("gamma outside [0, 1]", dict(gamma=nan)), ("lambda outside [0, 1]", dict(lam=-0.5)), ("lambda outside [0, 1]", dict(lam=1.5)),
             ("lambda outside [0, 1]", dict(lam=nan)), ("final_value_dev without trunc_dev", dict(final=final.data_ptr())),
             ("adv_dev and reward_dev overlap", dict(adv=reward.data_ptr())), ("ret_dev and value_dev overlap", dict(ret=value.data_ptr() + 4 * N)),
             ("valid_dev and done_dev overlap", dict(valid=done.data_ptr())), ("col_dev and value_dev overlap", dict(col=value.data_ptr() + 8)),
             ("adv_dev and steps_of_dev overlap", dict(steps_of=outs["adv"].data_ptr() + 4 * N)), ("ret_dev and skip_dev overlap", dict(skip=outs["ret"].data_ptr())),
             ("valid_dev and trunc_dev overlap", dict(trunc=outs["valid"].data_ptr())),
             ("col_dev and final_value_dev overlap", dict(trunc=flags.data_ptr(), final=outs["col"].data_ptr())),
             ("adv_dev and ret_dev overlap", dict(ret=outs["adv"].data_ptr()))]
    for what, kw in cases:
        assert call(**kw) == -1 and what in last() and "mg_rollout_targets" in last(), (what, last())
    col = outs["col"]
    total = torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
    for what, args in (("rows < 1", (col.data_ptr(), 0, total.data_ptr())), ("rows < 1", (col.data_ptr(), -1, total.data_ptr())),
                       ("col_dev is NULL", (None, 3, total.data_ptr())), ("out_dev is NULL", (col.data_ptr(), 3, None))):
        assert lib.mg_sum_columns(env._h, *args, env._stream()) == -1 and what in last() and "mg_sum_columns" in last(), (what, last())
    torch.cuda.synchronize()
    # nothing was launched: the counter stands and no output byte changed
    assert env.debug_counter("rollout_targets") == before
    assert all(bool((t == 7).all()) for t in outs.values()) and bool((total == 7).all())
    # what lies right beside an input is taken
    assert call(trunc=flags.data_ptr(), final=final.data_ptr(), skip=flags.data_ptr(), steps_of=steps_of.data_ptr()) == 0, last()
    assert env.debug_counter("rollout_targets") == before + 1
    # the Python mirror names the argument before the library is asked
    with pytest.raises(ValueError, match="rollout_targets: gamma"):
        rollout_targets(env, reward, done, value, gamma=1.5)
    with pytest.raises(ValueError, match="rollout_targets: out.adv"):
        rollout_targets(env, reward, done, value, out=RolloutTargets(value, value, value))
    fresh = memory_gym_amd.make(IDS[0], num_envs=N, device=0)
    with pytest.raises(Exception, match="rollout_targets"):
        rollout_targets(fresh, reward, done, value)
    fresh.close()
    env.check_errors()
