"""CPU (-m "not gpu"): the frame digest with which the oracle referees every frame of every step of the full-batch GPU runs
(tests/frame_digest.py, oracle/mgo_api.c mgo_batch_step_digest; used by tests/test_gpu_full_batch.py).  Pinned here: the oracle's digest
step is mgo_batch_step in everything but its output; its digests are those of the frames a twin batch hands out, terminal frames
included; numpy, torch and exact Python integers agree; one changed byte anywhere, swapped words and swapped frames are seen; the
result does not depend on the number of OpenMP threads."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import frame_digest as fd
import oracle_lib

# (env id, options, steps): random play, long enough that episodes end at a few dozen instances
IDS = [("MortarMayhem-Grid-v0", None, 90), ("MortarMayhem-v0", None, 120), ("Endless-MortarMayhem-v0", None, 120),
       ("MortarMayhemB-Grid-v0", None, 60), ("MortarMayhemB-v0", None, 80),
       ("MysteryPath-v0", dict(max_steps=24), 80), ("Endless-MysteryPath-v0", None, 150), ("MysteryPath-Grid-v0", dict(max_steps=24), 80),
       ("SearingSpotlights-v0", dict(max_steps=40), 130), ("Endless-SearingSpotlights-v0", None, 200)]
N = 36


def _actions(g, disc):
    return g.integers(0, 4 if disc else 3, (N,) if disc else (N, 2)).astype(np.int32)


@pytest.mark.parametrize("env_id,options,steps", IDS, ids=[c[0] for c in IDS])
def test_digest_step_is_the_batch_step(env_id, options, steps):
    a_ref = oracle_lib.OracleBatch(env_id, N, options=options)   # digests
    twin = oracle_lib.OracleBatch(env_id, N, options=options)    # frames: step without auto-reset, then the per-instance reset(None)
    seeds = np.arange(N, dtype=np.int64) + 11
    assert np.array_equal(a_ref.reset_digest(seeds), fd.digest_numpy(twin.reset(seeds)))
    g = np.random.Generator(np.random.PCG64(5))
    finals = 0
    for t in range(steps):
        a = _actions(g, a_ref.discrete)
        dg, fdg, rew, done = a_ref.step_digest(a, autoreset=True)
        obs, rew2, done2 = twin.step(a, autoreset=False)
        assert np.array_equal(rew, rew2) and np.array_equal(done, done2), "%s step %d" % (env_id, t)
        d = done.astype(bool)
        terminal = fd.digest_numpy(obs)
        assert np.array_equal(fdg[d], terminal[d]), "%s: terminal digests at step %d" % (env_id, t)
        assert not fdg[~d].any(), "final_digest is written only where done"
        for i in np.nonzero(d)[0]:
            obs[i] = twin.envs[i].reset(None)
        finals += int(d.sum())
        assert np.array_equal(dg, fd.digest_numpy(obs)), "%s: digests at step %d" % (env_id, t)
        if t % 16 == 0:  # what lies on the screens is what was digested
            which = [0, N // 2, N - 1]
            assert np.array_equal(a_ref.frames(which), obs[which])
    assert finals > 0, "no episode ended: the terminal digests were never compared"
    for i in range(N):
        assert np.array_equal(a_ref.envs[i].rng_words(), twin.envs[i].rng_words()), "%s: RNG words of instance %d" % (env_id, i)
    # without auto-reset the digest is the terminal frame's and final_digest stays untouched
    a = _actions(g, a_ref.discrete)
    dg, fdg, _, done = a_ref.step_digest(a, autoreset=False)
    obs, _, done2 = twin.step(a, autoreset=False)
    assert np.array_equal(done, done2) and np.array_equal(dg, fd.digest_numpy(obs)) and not fdg.any()
    a_ref.close()
    twin.close()


def _frames(env_id="Endless-SearingSpotlights-v0", n=12, steps=30):
    ref = oracle_lib.OracleBatch(env_id, n)
    ref.reset(np.arange(n, dtype=np.int64))
    g = np.random.Generator(np.random.PCG64(2))
    for _ in range(steps):
        obs, _, _ = ref.step(g.integers(0, 3, (n, 2)).astype(np.int32))
    ref.close()
    return obs


def test_numpy_torch_and_exact_integers_agree():
    import torch

    obs = _frames()
    want = fd.digest_numpy(obs)
    assert [int(x) for x in want[:3]] == [fd.digest_exact(obs[i]) for i in range(3)]
    t = torch.from_numpy(obs)
    assert np.array_equal(fd.as_uint64(fd.digest_torch(t)), want)
    assert np.array_equal(fd.as_uint64(fd.digest_torch(t, chunk=5)), want)            # chunk boundaries inside the batch
    assert np.array_equal(fd.as_uint64(fd.digest_torch(t[1::2])), want[1::2])         # a sliced batch: rows not back to back
    assert np.array_equal(fd.as_uint64(fd.digest_torch(t[1::2], chunk=2)), want[1::2])
    mask = torch.tensor([i % 3 == 0 for i in range(len(obs))])
    assert np.array_equal(fd.as_uint64(fd.digest_torch(t[mask])), want[mask.numpy()])
    assert np.array_equal(fd.digest_numpy(obs[::-1]), want[::-1])
    extreme = np.full((2, 84, 84, 3), 255, np.uint8)                                  # every word 0xFFFFFFFF: sign and carry handling
    extreme[1, :, :, :] = 0x80
    assert [int(x) for x in fd.digest_numpy(extreme)] == [fd.digest_exact(extreme[0]), fd.digest_exact(extreme[1])]
    assert np.array_equal(fd.as_uint64(fd.digest_torch(torch.from_numpy(extreme))), fd.digest_numpy(extreme))
    with pytest.raises(ValueError):
        fd.digest_torch(t.to(torch.float32))
    with pytest.raises(ValueError):
        fd.digest_torch(t[:, :, :, :1][:, :1, :1])                                    # one byte per frame: no whole word
    c = fd.coefficients(5292)
    assert (c & np.uint64(1)).all() and len(np.unique(c)) == len(c)                   # all odd, all different


def test_one_byte_swapped_words_and_swapped_frames_are_seen():
    import torch

    obs = _frames()
    want = fd.digest_numpy(obs)
    nbytes = 84 * 84 * 3
    positions = [0, 1, 2, 3, 4, nbytes // 2, nbytes - 5, nbytes - 4, nbytes - 1] + list(range(7, nbytes, 1013))
    for k, pos in enumerate(positions):
        for delta in (1, 128, 255):
            bad = obs.copy()
            i = k % len(obs)
            flat = bad[i].reshape(-1)
            flat[pos] = (int(flat[pos]) + delta) & 0xFF
            assert list(fd.differing(fd.digest_numpy(bad), want)) == [i], "byte %d + %d" % (pos, delta)
            assert list(fd.differing(fd.digest_torch(torch.from_numpy(bad)), want)) == [i]
    words = obs[0].reshape(-1).view("<u4")
    j, k = 0, int(np.nonzero(words != words[0])[0][0])    # two unequal words of one frame
    for a, b in ((j, k), (k, len(words) - 1 if words[-1] != words[k] else j)):
        bad = obs.copy()
        w = bad[0].reshape(-1).view("<u4")
        w[a], w[b] = words[b], words[a]
        assert list(fd.differing(fd.digest_numpy(bad), want)) == [0]
    bad = obs.copy()
    bad[[2, 7]] = obs[[7, 2]]                              # the frames of two instances swapped
    assert not np.array_equal(obs[2], obs[7])
    assert list(fd.differing(fd.digest_numpy(bad), want)) == [2, 7]
    assert list(fd.differing(fd.digest_torch(torch.from_numpy(bad)), want)) == [2, 7]
    assert list(fd.differing(fd.digest_numpy(bad), want, mask=np.arange(len(obs)) != 7)) == [2]
    assert len(fd.differing(fd.digest_numpy(obs), want)) == 0


_WORKER = """
import hashlib, sys
import numpy as np
sys.path.insert(0, %r)
import oracle_lib
h = hashlib.sha256()
for env_id, adim in (("MortarMayhem-Grid-v0", 1), ("Endless-MysteryPath-v0", 1), ("SearingSpotlights-v0", 2)):
    n = 67
    ref = oracle_lib.OracleBatch(env_id, n)
    h.update(ref.reset_digest(np.arange(n, dtype=np.int64)).tobytes())
    g = np.random.Generator(np.random.PCG64(3))
    for t in range(60):
        a = g.integers(0, 4 if adim == 1 else 3, (n,) if adim == 1 else (n, 2)).astype(np.int32)
        for x in ref.step_digest(a):
            h.update(x.tobytes())
    ref.close()
print("sha", h.hexdigest())
"""


def test_digests_do_not_depend_on_the_number_of_threads():
    def run(threads):
        env = dict(os.environ)
        env.pop("OMP_NUM_THREADS", None)
        if threads:
            env["OMP_NUM_THREADS"] = str(threads)
        r = subprocess.run([sys.executable, "-c", _WORKER % os.path.dirname(os.path.abspath(__file__))], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return [ln for ln in r.stdout.splitlines() if ln.startswith("sha ")]
    one = run(1)
    assert len(one) == 1 and one == run(None) == run(5)
    assert hashlib.sha256().hexdigest() not in one[0]
