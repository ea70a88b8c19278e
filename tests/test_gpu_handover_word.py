"""GPU (-m gpu): the 64-bit hand-over word of the mortar family's one-launch step (csrc/mg_mortar_handover.hpp, mortar_step_raster_kernel).

A step lane hands its instance's frame descriptor to the frame workgroup of the same launch in ONE 64-bit word (sprite position, template,
sprite, glyph, the FINAL marker, an epoch byte); the 16-byte descriptor in memory is still written for every other consumer.  Against the CPU
oracle, every frame of every step:
  * 300 steps pass the epoch's wrap 255 -> 1; n = 1, 63, 65: partial waves; n = 2049: more frames than resident frame workgroups' first round
    of a small grid, and a last slot of one instance;
  * Endless-MortarMayhem-v0: negative sprite coordinates (the screen-wrap controller) and frames without a sprite (0xFF);
  * step -> render() -> masked reset -> step: mg_render and the masked reset's sparse raster read the 16-byte descriptors the one-launch step left;
  * final_observation kept: the terminal frame's word, announced by the reset frame's word (the FINAL instantiation)."""
import numpy as np
import pytest

import gpu_parity

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("env_id,n,steps", [("MortarMayhem-Grid-v0", 1, 300), ("MortarMayhem-Grid-v0", 63, 300), ("MortarMayhem-Grid-v0", 65, 300),
                                            ("MortarMayhem-Grid-v0", 2049, 300), ("Endless-MortarMayhem-v0", 2049, 300), ("MortarMayhem-v0", 1025, 120)])
def test_every_frame_against_the_oracle(env_id, n, steps):
    finished = gpu_parity.run_parity(env_id, None, n, steps, check_every=1, want_counters=("one_launch_steps",))
    assert finished > 0 or n == 1


def test_render_and_masked_reset_read_the_descriptors_the_one_launch_step_left():
    import memory_gym_amd
    import oracle_lib
    import torch
    from memory_gym_amd import _native

    env_id, n = "MortarMayhem-Grid-v0", 2049
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    ref = oracle_lib.OracleBatch(env_id, n)
    seeds = np.arange(n, dtype=np.int64) + 11
    obs, _ = env.reset(seed=seeds)
    assert np.array_equal(obs.cpu().numpy(), ref.reset(seeds))
    prng = np.random.Generator(np.random.PCG64(6))
    everyone = np.arange(n, dtype=np.int32)
    again = torch.empty_like(obs)
    for t in range(40):
        a = prng.integers(0, 4, n).astype(np.int32)
        obs, rew, done, _, _ = env.step(a)
        want, r2, d2 = ref.step(a, autoreset=True)
        assert np.array_equal(obs.cpu().numpy(), want), "step %d" % t
        assert np.array_equal(rew.cpu().numpy(), r2.astype(np.float32)) and np.array_equal(done.cpu().numpy(), d2.astype(bool))
        again.fill_(7)
        _native.check(_native.LIB.mg_render(env._h, again.data_ptr(), env._stream()), "mg_render")
        assert torch.equal(again, obs), "mg_render after step %d" % t
        mask = prng.random(n) < 0.3
        mask[n - 1] = t % 2 == 0  # (the one instance of the last slot, every other round)
        obs, _ = env.reset(mask=torch.from_numpy(mask))
        for i in np.nonzero(mask)[0]:
            ref.envs[i].reset(None, want_obs=False)
        assert np.array_equal(obs.cpu().numpy(), ref.frames(everyone)), "masked reset after step %d" % t
    assert env.debug_counter("one_launch_steps") == 40
    for i in (0, n // 2, n - 1):
        assert np.array_equal(env.rng_words(i), ref.envs[i].rng_words())
    env.check_errors()
    env.close()
    ref.close()


def test_terminal_frames_kept_by_the_one_launch_step():
    """final_observation=True: for every instance that finishes, infos["final_observation"] is the frame the oracle's instance showed at its last
    step and obs the first frame after its reset (tests/test_gpu_vector_api.py's comparison, every instance of every step)."""
    import memory_gym_amd
    import oracle_lib

    env_id, n, steps = "MortarMayhem-Grid-v0", 2049, 120
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, final_observation=True)
    ref = oracle_lib.OracleBatch(env_id, n)
    seeds = np.arange(n, dtype=np.int64) + 100
    obs, _ = env.reset(seed=seeds)
    assert np.array_equal(obs.cpu().numpy(), ref.reset(seeds))
    prng = np.random.Generator(np.random.PCG64(8))
    n_final = 0
    for t in range(steps):
        a = prng.integers(0, 4, n).astype(np.int32)
        obs, rew, done, _, info = env.step(a)
        want, r2, d2 = ref.step(a, autoreset=False)  # the terminal frames where done ...
        d2 = d2.astype(bool)
        assert np.array_equal(done.cpu().numpy(), d2) and np.array_equal(rew.cpu().numpy(), r2.astype(np.float32)), "step %d" % t
        if d2.any():
            fin = info["final_observation"].cpu().numpy()
            assert np.array_equal(fin[d2], want[d2]), "terminal frames differ at step %d: instances %s" % (
                t, np.nonzero(d2)[0][(fin[d2] != want[d2]).reshape(int(d2.sum()), -1).any(1)][:8])
            for i in np.nonzero(d2)[0]:  # ... and the first frames of their next episodes
                want[i] = ref.envs[i].reset(None)
            n_final += int(d2.sum())
        got = obs.cpu().numpy()
        assert np.array_equal(got, want), "frames differ at step %d: instances %s" % (t, np.nonzero((got != want).reshape(n, -1).any(1))[0][:8])
    assert n_final > n
    assert env.debug_counter("one_launch_steps") == steps
    for i in (0, n // 2, n - 1):
        assert np.array_equal(env.rng_words(i), ref.envs[i].rng_words())
    env.check_errors()
    env.close()
    ref.close()
