"""CPU tests of the rollout targets' boundary (no GPU): the two forms of the definition (tests/rollout_targets_definition.py) agree bit for bit and have
the properties a trainer relies on -- exact integer returns at gamma = lam = 1, the one-step form at lam = 0, rows that next-step auto-reset skips
can be deleted, truncated ends bootstrap from the right value; the Python argument check refuses each bad argument by name; the library exports the two
calls; and the host half of csrc/mg_targets.hpp -- refusals, the overlap check, the column walk the kernel runs -- passes its stand-alone program
under the sanitizers against bits written here from the definition."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import rollout_targets_definition as rd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PAIRS = ((0.99, 0.95), (1.0, 1.0), (0.0, 0.5), (0.5, 0.0))


def crafted(K, N, seed, rate=0.125):
    """-> dict of finite inputs with the awkward values: rewards 0.0, -0.0, a subnormal, 1e18, negatives; values normal with 1e18 and a subnormal"""
    g = np.random.default_rng(seed)
    reward = g.choice(np.array([0.0, -0.0, 1e-42, 1e18, -1.0, 0.25, -3.5, 1.0], F), size=(K, N)).astype(F)
    value = g.standard_normal((K + 1, N)).astype(F)
    value[g.random((K + 1, N)) < 0.05] = F(1e18)
    value[g.random((K + 1, N)) < 0.05] = F(1e-42)
    done = (g.random((K, N)) < rate).astype(np.uint8)
    skip = np.zeros((K, N), np.uint8)
    for t in range(1, K):  # a reset row follows an end, and is itself no end
        skip[t] = done[t - 1] & (g.random(N) < 0.7)
        done[t] &= 1 - skip[t]
    trunc = (done & (g.random((K, N)) < 0.5)).astype(np.uint8)
    final = g.standard_normal((K, N)).astype(F)
    steps_of = g.choice(np.array([0, 1, K, K + 5, -3, K // 2]), size=N).astype(np.int32)
    return {"reward": reward, "done": done, "value": value, "skip": skip, "trunc": trunc, "final_value": final, "steps_of": steps_of}


def combos():
    """every present / absent combination of steps_of, skip, trunc, final_value that is not refused"""
    for steps_of in (False, True):
        for skip in (False, True):
            for trunc, final in ((False, False), (True, False), (True, True)):
                yield {"steps_of": steps_of, "skip": skip, "trunc": trunc, "final_value": final}


def pick(x, use):
    return {k: (x[k] if on else None) for k, on in use.items()}


def test_the_two_forms_of_the_definition_agree_bit_for_bit():
    for (K, N, seed) in ((1, 3, 1), (2, 5, 2), (17, 9, 3), (40, 70, 4)):
        x = crafted(K, N, seed)
        for use in combos():
            for gamma, lam in PAIRS:
                a = rd.targets_scalar(x["reward"], x["done"], x["value"], gamma, lam, **pick(x, use))
                b = rd.targets_rows(x["reward"], x["done"], x["value"], gamma, lam, **pick(x, use))
                for name, p, q in zip(("adv", "ret", "valid", "col"), a, b):
                    assert rd.same_bits(p, q), (name, K, N, use, gamma, lam)
    # the sum's order: small integers are exact in any order, 2^53 and ones are not
    col = np.arange(1, 601, dtype=np.float64)[None, :]
    assert rd.sum_columns(col[:, :257])[0] == 33153.0 and rd.sum_columns(col)[0] == 180300.0
    row = np.ones(300)
    row[0] = 2.0 ** 53
    by_hand = np.zeros(256)
    for i in range(300):
        by_hand[i % 256] = by_hand[i % 256] + row[i]
    h = 128
    while h:
        for l in range(h):
            by_hand[l] = by_hand[l] + by_hand[l + h]
        h //= 2
    assert rd.sum_columns(row[None, :])[0] == by_hand[0] != np.cumsum(row)[-1]


def test_exact_integer_returns_at_gamma_one_lambda_one():
    """gamma = lam = 1, small integer rewards and values: every intermediate is an exactly representable integer, so ret is the integer return-to-go
    of the episode, plus the bootstrap value where the column ends open, and adv is that minus value -- no tolerance."""
    g = np.random.default_rng(5)
    K, N = 60, 40
    reward = g.integers(-4, 5, (K, N)).astype(F)
    value = g.integers(-8, 9, (K + 1, N)).astype(F)
    done = g.random((K, N)) < 0.1
    adv, ret, valid, col = rd.targets_rows(reward, done, value, 1.0, 1.0)
    assert valid.all()
    want = np.zeros((K, N), np.int64)
    for i in range(N):
        togo = int(value[K, i])  # the column ends open: the bootstrap value
        for t in range(K - 1, -1, -1):
            if done[t, i]:
                togo = 0
            togo += int(reward[t, i])
            want[t, i] = togo
    assert np.array_equal(ret.astype(np.int64), want) and np.array_equal(ret, want.astype(F))
    assert np.array_equal(adv, (want - value[:K].astype(np.int64)).astype(F))
    assert np.array_equal(col[0], np.full(N, K)) and np.array_equal(col[1], adv.astype(np.float64).sum(0)) and np.array_equal(col[2], (adv.astype(np.float64) ** 2).sum(0))
    assert rd.sum_columns(col)[0] == K * N and rd.sum_columns(col)[1] == adv.astype(np.int64).sum()


def test_lambda_zero_is_the_one_step_form():
    x = crafted(30, 50, 6)
    for gamma in (0.99, 0.5):
        adv, ret, valid, _ = rd.targets_rows(x["reward"], x["done"], x["value"], gamma, 0.0)
        nv = np.where(x["done"] != 0, F(0.0), x["value"][1:])
        with np.errstate(all="ignore"):
            delta = (x["reward"] + F(gamma) * nv) - x["value"][:-1]
        assert valid.all() and np.array_equal(adv, delta)  # (gl * carry is a zero of either sign: equal values, a zero's sign apart)


def test_rows_that_follow_an_end_can_be_skipped_or_deleted():
    """A column in which every skip row follows a done row: deleting the skip rows and their value rows gives the same adv / ret bits on the rows that
    remain (next-step auto-reset seen as same-step auto-reset with the terminal observation's value as final_value)."""
    K, N = 80, 1
    hits = 0
    for seed in range(12):
        x = crafted(K, N, 100 + seed, rate=0.2)
        skip, done, trunc = x["skip"][:, 0] != 0, x["done"][:, 0], x["trunc"][:, 0]
        assert all(done[t - 1] for t in range(K) if skip[t])
        keep = ~skip
        keep_v = np.append(keep, True)
        for gamma, lam in PAIRS:
            # ends that bootstrap from 0: the rows are deleted, nothing else is needed
            adv, ret, valid, _ = rd.targets_scalar(x["reward"], x["done"], x["value"], gamma, lam, skip=x["skip"])
            adv2, ret2, valid2, _ = rd.targets_scalar(x["reward"][keep], x["done"][keep], x["value"][keep_v], gamma, lam)
            assert valid2.all() and np.array_equal(valid[:, 0] != 0, keep) and not adv[skip].any() and not ret[skip].any()
            assert rd.same_bits(adv[keep], adv2) and rd.same_bits(ret[keep], ret2), (seed, gamma, lam)
            # truncated ends: the terminal observation of an end at t is frame row t + 1, which the deletion may remove -- its value is handed over
            # as final_value
            adv, ret, valid, _ = rd.targets_scalar(x["reward"], x["done"], x["value"], gamma, lam, skip=x["skip"], trunc=x["trunc"])
            adv2, ret2, valid2, _ = rd.targets_scalar(x["reward"][keep], x["done"][keep], x["value"][keep_v], gamma, lam, trunc=x["trunc"][keep],
                                                      final_value=x["value"][1:][keep])
            assert valid2.all() and np.array_equal(valid[:, 0] != 0, keep) and not adv[skip].any() and not ret[skip].any()
            assert rd.same_bits(adv[keep], adv2) and rd.same_bits(ret[keep], ret2), (seed, gamma, lam)
        hits += int(skip.sum())
        assert (trunc != 0).any()
    assert hits > 40


def test_truncated_ends_bootstrap_from_the_right_value():
    reward = np.array([[1.0], [2.0], [4.0]], F)
    value = np.array([[10.0], [20.0], [30.0], [40.0]], F)
    done = np.array([[0], [1], [0]], np.uint8)
    trunc = np.array([[0], [1], [0]], np.uint8)
    final = np.array([[7.0], [100.0], [9.0]], F)
    g = 0.5
    plain = rd.targets_scalar(reward, done, value, g, 0.0)[0][:, 0]
    by_next = rd.targets_scalar(reward, done, value, g, 0.0, trunc=trunc)[0][:, 0]
    by_final = rd.targets_scalar(reward, done, value, g, 0.0, trunc=trunc, final_value=final)[0][:, 0]
    unflagged = rd.targets_scalar(reward, done, value, g, 0.0, trunc=np.zeros_like(trunc), final_value=final)[0][:, 0]
    assert plain.tolist() == [1 + 10 - 10, 2 + 0 - 20, 4 + 20 - 30]
    assert by_next.tolist() == [1.0, 2 + 15 - 20, -6.0] and by_final.tolist() == [1.0, 2 + 50 - 20, -6.0] and unflagged.tolist() == plain.tolist()
    # a truncation flag on a row that is not done changes nothing
    stray = rd.targets_scalar(reward, done, value, g, 0.0, trunc=np.array([[1], [0], [1]], np.uint8), final_value=final)[0][:, 0]
    assert stray.tolist() == plain.tolist()
    # -0.0 on a terminal row: r + gamma * 0 is +0.0
    r0 = rd.targets_scalar(np.array([[-0.0]], F), np.array([[1]], np.uint8), np.array([[0.0], [5.0]], F), 1.0, 1.0)
    assert rd.same_bits(r0[0], np.array([[0.0]], F)) and not np.signbit(r0[0][0, 0])


def test_exports_and_the_null_handle():
    from memory_gym_amd import _native

    v, i32, f = C.c_void_p, C.c_int32, C.c_float
    want = {"mg_rollout_targets": [v, v, v, v, i32, v, v, v, v, f, f, v, v, v, v, v], "mg_sum_columns": [v, v, i32, v, v]}
    for name, argtypes in want.items():
        assert hasattr(_native.LIB, name), "libmemgym_hip.so does not export " + name
        assert list(getattr(_native.LIB, name).argtypes) == argtypes, name
    assert _native.LIB.mg_rollout_targets(None, None, None, None, 1, None, None, None, None, 0.9, 0.9, None, None, None, None, None) == -1
    assert "null handle" in _native.last_error()
    assert _native.LIB.mg_sum_columns(None, None, 3, None, None) == -1 and "null handle" in _native.last_error()
    header = open(os.path.join(ROOT, "include", "memgym.h")).read()
    for words in ("int mg_rollout_targets(", "int mg_sum_columns(", "ROLLOUT TARGETS", "delta = (r + gamma * nv) - v", "#define MG_STATE_VERSION 8u", "next-step auto-reset",
                  "lambda = 1 gives", "h = 128, 64, ..., 1", "OUT OF SCOPE: values in bf16 / f16", "V-trace", "\"rollout_targets\""):
        assert words in header, words


def test_python_surface():
    import inspect

    from memory_gym_amd import episodes, vec_env

    assert vec_env.RolloutTargets is episodes.RolloutTargets and vec_env.rollout_targets is episodes.rollout_targets
    assert vec_env.check_rollout_targets is episodes.check_rollout_targets
    assert episodes.RolloutTargets.__slots__ == ("adv", "ret", "valid", "columns", "moments")
    p = inspect.signature(episodes.rollout_targets).parameters
    assert list(p) == ["env", "reward", "done", "value", "gamma", "lam", "steps", "skip", "truncated", "final_value", "out", "moments"]
    assert [p[k].default for k in list(p)[4:]] == [0.99, 0.95, None, None, None, None, None, False]
    assert list(inspect.signature(episodes.check_rollout_targets).parameters)[:4] == ["reward", "done", "value", "num_envs"]


def test_the_moments_of_rollout_targets_are_torch_expressions():
    import torch
    from memory_gym_amd.vec_env import RolloutTargets

    g = np.random.default_rng(8)
    adv = g.standard_normal((6, 9)).astype(F)
    valid = g.random((6, 9)) < 0.7
    adv[~valid] = 0.0
    a64 = adv.astype(np.float64)
    col = np.stack([valid.sum(0).astype(np.float64), a64.sum(0), (a64 * a64).sum(0)])
    tg = RolloutTargets(torch.from_numpy(adv), torch.from_numpy(adv + 1), torch.from_numpy(valid), torch.from_numpy(col), torch.from_numpy(rd.sum_columns(col)))
    picked = a64[valid]
    assert abs(float(tg.mean()) - picked.mean()) < 1e-12 and abs(float(tg.std()) - picked.std()) < 1e-12
    z = tg.normalized(eps=0.0).numpy()
    assert not z[~valid].any() and np.allclose(z[valid], (picked - picked.mean()) / picked.std(), rtol=1e-6, atol=1e-6)
    bare = RolloutTargets(tg.adv, tg.ret, tg.valid)
    for call in (bare.mean, bare.std, bare.normalized):
        with pytest.raises(ValueError, match="moments=True"):
            call()


def test_check_rollout_targets_refuses_each_bad_argument_by_name():
    import torch
    from memory_gym_amd.vec_env import RolloutTargets, check_rollout_targets
    from memory_gym_amd.episodes import check_targets_out

    K, N = 6, 70
    reward, value = torch.zeros((K, N)), torch.zeros((K + 1, N))
    done = torch.zeros((K, N), dtype=torch.bool)
    flags, final = torch.zeros((K, N), dtype=torch.uint8), torch.zeros((K, N))
    r, d8, v, k, gamma, lam, steps, skip, trunc, fv = check_rollout_targets(reward, done, value, N)
    assert r is reward and v is value and d8.dtype == torch.uint8 and d8.data_ptr() == done.data_ptr() and (k, gamma, lam) == (K, 0.99, 0.95)
    assert steps is None and skip is None and trunc is None and fv is None
    _, _, _, _, gamma, lam, steps, skip, trunc, fv = check_rollout_targets(reward, done.view(torch.uint8), value, N, 1, np.float32(0.5), torch.zeros(N, dtype=torch.int64),
                                                                         done, flags, final)
    assert (gamma, lam) == (1.0, 0.5) and steps.dtype == torch.int32 and skip.dtype == torch.uint8 and trunc.data_ptr() == flags.data_ptr() and fv is final
    ok = (reward, done, value, N)
    bad = {"reward": [lambda: check_rollout_targets(reward.double(), done, value, N), lambda: check_rollout_targets(torch.zeros((K + 1, N)), done, value, N),
                      lambda: check_rollout_targets(torch.zeros((K, 2 * N))[:, ::2], done, value, N), lambda: check_rollout_targets(reward.numpy(), done, value, N),
                      lambda: check_rollout_targets(None, done, value, N)],
           "done": [lambda: check_rollout_targets(reward, reward, value, N), lambda: check_rollout_targets(reward, done.view(-1), value, N),
                    lambda: check_rollout_targets(reward, done, value, N + 1), lambda: check_rollout_targets(reward, torch.zeros((K, 2 * N), dtype=torch.bool)[:, ::2], value, N),
                    lambda: check_rollout_targets(reward, done, value, N, device=torch.device("cuda", 0))],
           "value": [lambda: check_rollout_targets(reward, done, reward, N), lambda: check_rollout_targets(reward, done, value.half(), N),
                     lambda: check_rollout_targets(reward, done, torch.zeros((K + 2, N)), N)],
           "gamma": [lambda: check_rollout_targets(*ok, gamma=-0.1), lambda: check_rollout_targets(*ok, gamma=1.5), lambda: check_rollout_targets(*ok, gamma=float("nan")),
                     lambda: check_rollout_targets(*ok, gamma=True), lambda: check_rollout_targets(*ok, gamma="0.9")],
           "lam": [lambda: check_rollout_targets(*ok, lam=-1), lambda: check_rollout_targets(*ok, lam=2), lambda: check_rollout_targets(*ok, lam=float("nan")),
                   lambda: check_rollout_targets(*ok, lam=None)],
           "steps": [lambda: check_rollout_targets(*ok, steps=torch.zeros(N)), lambda: check_rollout_targets(*ok, steps=torch.zeros(N - 1, dtype=torch.int32)),
                     lambda: check_rollout_targets(*ok, steps=[K] * N)],
           "skip": [lambda: check_rollout_targets(*ok, skip=final), lambda: check_rollout_targets(*ok, skip=torch.zeros((K + 1, N), dtype=torch.bool)),
                    lambda: check_rollout_targets(*ok, skip=torch.zeros((K, 2 * N), dtype=torch.bool)[:, ::2])],
           "truncated": [lambda: check_rollout_targets(*ok, truncated=final), lambda: check_rollout_targets(*ok, truncated=torch.zeros((K, N - 1), dtype=torch.uint8)),
                         lambda: check_rollout_targets(*ok, truncated=flags.numpy())],
           "final_value": [lambda: check_rollout_targets(*ok, truncated=flags, final_value=flags), lambda: check_rollout_targets(*ok, truncated=flags, final_value=value),
                           lambda: check_rollout_targets(*ok, final_value=final)]}
    for name, calls in bad.items():
        for n, call in enumerate(calls):
            with pytest.raises(ValueError, match=r"^rollout_targets: " + name + " "):
                call()
                pytest.fail("%s, case %d, was accepted" % (name, n))
    with pytest.raises(ValueError, match="int32 of a pick"):
        check_rollout_targets(reward, torch.zeros(1, dtype=torch.bool).expand(4, 1 << 29), value, 1 << 29)  # (a broadcast view, 1 byte of memory)

    out = RolloutTargets(torch.zeros((K, N)), torch.zeros((K, N)), torch.zeros((K, N), dtype=torch.bool), torch.zeros((3, N), dtype=torch.float64),
                         torch.zeros(3, dtype=torch.float64))
    assert check_targets_out(out, K, N, True) is out and check_targets_out(RolloutTargets(out.adv, out.ret, out.valid), K, N, False)
    bad_out = {"out must": lambda: check_targets_out((out.adv, out.ret, out.valid), K, N, False),
               "out.adv": lambda: check_targets_out(RolloutTargets(out.adv.double(), out.ret, out.valid), K, N, False),
               "out.ret": lambda: check_targets_out(RolloutTargets(out.adv, torch.zeros((K + 1, N)), out.valid), K, N, False),
               "out.valid": lambda: check_targets_out(RolloutTargets(out.adv, out.ret, out.valid.view(torch.uint8)), K, N, False),
               "out.columns": lambda: check_targets_out(RolloutTargets(out.adv, out.ret, out.valid), K, N, True),
               "out.moments": lambda: check_targets_out(RolloutTargets(out.adv, out.ret, out.valid, out.columns, torch.zeros(3)), K, N, True)}
    for name, call in bad_out.items():
        with pytest.raises(ValueError, match=r"^rollout_targets: " + name + " "):
            call()
            pytest.fail(name + " was accepted")


def write_cases(path):
    """the cases of tests/host/rollout_targets_check.cpp's file: inputs, then the definition's bits"""
    cases = []
    for K, N, seed in ((1, 1, 11), (2, 3, 12), (15, 5, 13), (16, 7, 14), (17, 4, 15), (33, 6, 16), (37, 65, 17), (5, 300, 18)):
        x = crafted(K, N, seed)
        for n, use in enumerate(combos()):
            gamma, lam = PAIRS[(n + seed) % len(PAIRS)]
            opt = pick(x, use)
            adv, ret, valid, col = rd.targets_rows(x["reward"], x["done"], x["value"], gamma, lam, **opt)
            head = np.array([K, N] + [int(opt[k] is not None) for k in ("steps_of", "skip", "trunc", "final_value")], np.int32).tobytes() + np.array([gamma, lam], F).tobytes()
            arrays = [x["reward"], x["done"], x["value"]] + [opt[k] for k in ("steps_of", "skip", "trunc", "final_value") if opt[k] is not None]
            arrays += [adv, ret, valid, col, rd.sum_columns(col)]
            cases.append(head + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays))
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], np.int32).tobytes() + b"".join(cases))
    return len(cases)


def test_the_host_half_of_the_kernels_header_under_the_sanitizers(tmp_path):
    """tests/host/rollout_targets_check.cpp, a stand-alone program (its own main) over the host half of csrc/mg_targets.hpp, built with
    -ffp-contract=off -fsanitize=address,undefined and run as a program: the refusals, the overlap check, and the kernel's column walk over buffers
    of exactly the ABI's sizes against the definition's bits."""
    if not shutil.which("g++"):
        pytest.skip("g++ not installed")
    exe = tmp_path / "rollout_targets_check"
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "host", "rollout_targets_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert write_cases(tmp_path / "cases.bin") == 8 * 12
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
