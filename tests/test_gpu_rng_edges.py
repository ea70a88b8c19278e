"""GPU (-m gpu): the device's restatements of numpy's PCG64 stream -- Pcg (mg_device.hpp), WaveRng (mg_mystery_path.hpp), the 16 outputs at
once of new_spots_at_reset (mg_spot_logic.hpp), the lane generator of the larger Endless-MysteryPath launches and the position sampler
(mg_spot_sampler.hpp) -- at REJECTED and EXTREME draws, bit-exact against the CPU oracle.

Streams that start at SeedSequence(seed) reject a bounded draw once in 10^7 (span 360) and never produce a word of 0 or 2^32 - 1 where it
matters.  PCG64 runs backwards (tests/rng_craft.py): instance i of a handle receives, through the test hook mg_debug_set_rng on the device
and mgo_rng_set_words on the oracle, a stream whose 64-bit output number p = i // 8 is all zeros (both halves rejected by every span that
can reject), zeros followed by 0xFFFFFFFF00000000 (three rejections in a row, then the maximal value), all ones (the maximal k, uniform()
at 1 - 2^-53) or the smallest accepted word twice (k = 0), with and without a buffered half.  The sweep of p covers the whole reset.

  a  explicit reset          seeded reset, inject, reset(seed=None): all ten ids
  b  reset inside a step     inject, step under auto-reset until every injected instance has finished: the resets of the one-launch mortar
                             step, of the fused spotlight raster / reset launch, of the Mystery Path step launches; twice with terminal frames
  c  draws during an episode inject mid-episode, 48 steps of the oracle's expert policy: spawns, coins, next commands, appended segments
  d  64-bit seeds            Pcg::seed with a second entropy word (seeds of 2^32 and more)

After every call: the digest of every frame (tests/frame_digest.py), rewards against the oracle's doubles, dones, the RNG words of every
injected instance and the device's error bits.  What a case exercised is read from the oracle's bookkeeping (oracle/mgo_rng.h) and asserted:
tests/test_rng_craft.py shows the same conditions on the oracle alone, without a GPU."""
import numpy as np
import pytest

import rng_craft as rc

pytestmark = pytest.mark.gpu


class Pair:
    """A HIP handle and an oracle batch in lock-step"""

    def __init__(self, env_id, n, options, final=False):
        import memory_gym_amd
        import oracle_lib

        self.env_id, self.n, self.options, self.final = env_id, n, options, final
        self.env = memory_gym_amd.make(env_id, num_envs=n, device=0, final_observation=final)
        self.ref = oracle_lib.OracleBatch(env_id, n, options=options)
        self.watch = []  # instances whose RNG words are compared after every call
        self.n_done = self.n_final = 0

    def close(self):
        self.env.close()
        self.ref.close()

    def plan(self, i):
        """(p, has, pattern) of the stream instance i received (tests/test_gpu_rng_edges_arrangements.py injects other instances than 0, 1, 2, ...)"""
        return rc.plan(i)

    @staticmethod
    def _visual(o):
        return o["visual_observation"] if isinstance(o, dict) else o

    def _frames(self, where, obs, want_dg, mask=None, what="frames"):
        import frame_digest as fd

        bad = fd.differing(fd.digest_torch(obs), want_dg, mask)
        if len(bad):
            self.env.check_errors()  # a capacity error flagged by the kernels explains a mismatch better than pixels do
            pixels = ""
            if what == "frames":  # (the oracle's screens still hold these; terminal frames are gone after its reset)
                pixels = ", %d pixels of instance %d" % (int((obs[int(bad[0])].cpu().numpy() != self.ref.frames(bad[:1])[0]).any(-1).sum()), bad[0])
            raise AssertionError("%s %s: %d of %d %s differ from the oracle's; instances %s (p, has, pattern: %s)%s" % (
                self.env_id, where, len(bad), self.n, what, bad[:8], [self.plan(int(i)) for i in bad[:4]], pixels))

    def _words(self, where):
        for i in self.watch:
            got, want = self.env.rng_words(i), self.ref.envs[i].rng_words()
            assert np.array_equal(got, want), "%s %s: RNG words of instance %d (p, has, pattern: %s): device %s, oracle %s" % (
                self.env_id, where, i, self.plan(i), [hex(int(x)) for x in got], [hex(int(x)) for x in want])
        self.env.check_errors()

    def reset(self, seeds, where):
        obs, _ = self.env.reset(seed=seeds, options=self.options)
        self._frames(where, self._visual(obs), self.ref.reset_digest(seeds))
        self._vector(obs, where)
        self._words(where)

    def _vector(self, obs, where):
        if isinstance(obs, dict):  # MortarMayhemB*: the one-hot command vector is drawn from the stream too
            want = np.stack([e.get_list("vec") for e in self.ref.envs]).astype(np.float32)
            assert np.array_equal(obs["vector_observation"].cpu().numpy(), want), "%s %s: vector_observation differs" % (self.env_id, where)

    def inject(self, n_injected):
        rc.inject(self.ref, self.env, n_injected)
        self.watch = list(range(n_injected))
        self._words("after the injection")

    def step_unwatched(self, actions, where):
        """A step before the injection (streams from ordinary seeds, which the rest of the suite referees): dones alone are compared."""
        done = self.env.step(actions)[2]
        want_done = self.ref.step(actions, autoreset=True, want_obs=False)[2]
        assert np.array_equal(done.cpu().numpy(), want_done.astype(bool)), "%s %s: done differs" % (self.env_id, where)

    def step(self, actions, where):
        """-> done (bool [n])"""
        obs, _, done, _, info = self.env.step(actions)
        want_dg, want_fdg, rew, want_done = self.ref.step_digest(actions, autoreset=True)
        d = done.cpu().numpy()
        assert np.array_equal(d, want_done.astype(bool)), "%s %s: done differs for instances %s" % (self.env_id, where, np.nonzero(d != want_done.astype(bool))[0][:8])
        r = self.env.reward64.cpu().numpy()
        assert np.array_equal(r, rew), "%s %s: reward differs for instances %s" % (self.env_id, where, np.nonzero(r != rew)[0][:8])
        self._frames(where, self._visual(obs), want_dg)
        if self.final:
            self._frames(where, info["final_observation"], want_fdg, mask=d, what="terminal frames")
            self.n_final += int(d.sum())
        self._vector(obs, where)
        self._words(where)
        self.n_done += int(d.sum())
        return d

    def coverage(self, label, n_injected, at_least=32):
        cov = rc.Coverage(self.env_id, self.ref, n_injected)
        print("\n%s: %s" % (label, cov.summary()))
        cov.assert_instances(label, at_least)
        return cov


def _seeds(n):
    return np.arange(n, dtype=np.int64) + 500


@pytest.mark.parametrize("env_id", rc.ALL_IDS)
def test_explicit_reset(env_id):
    n_inj = rc.injected(env_id)
    pair = Pair(env_id, rc.handle_size(n_inj), rc.RESET_OPTIONS[env_id])
    pair.reset(_seeds(pair.n), "seeded reset")
    pair.inject(n_inj)
    pair.reset(None, "reset(seed=None) on the crafted streams")
    label = env_id + " explicit reset"
    cov = pair.coverage(label, n_inj)
    cov.assert_every_rejectable_span_rejected(label)
    if env_id in rc.MYSTERY:
        rc.check_mystery_rejections(label, env_id, cov)
    if env_id in rc.SPOT:
        rc.check_spot_wirings(label, cov)
    for k in range(2):  # (a finite path takes 19 - 49 outputs: the later positions of the Mystery Path ids' sweep lie in the next paths)
        pair.reset(None, "reset(seed=None) number %d" % (k + 2))
    pair.close()


@pytest.mark.parametrize("env_id,final", [(e, False) for e in rc.ALL_IDS] + [("MortarMayhem-Grid-v0", True), ("SearingSpotlights-v0", True)])
def test_reset_inside_a_step(env_id, final):
    n_inj = rc.injected(env_id)
    pair = Pair(env_id, rc.handle_size(n_inj), rc.short_options(env_id), final=final)
    pair.reset(_seeds(pair.n), "seeded reset")
    pair.inject(n_inj)
    prng = np.random.Generator(np.random.PCG64(21))
    finished = np.zeros(pair.n, bool)
    steps = 0
    while not finished[:n_inj].all():
        finished |= pair.step(rc.random_actions(prng, pair.n, pair.ref.discrete), "step %d" % steps)
        steps += 1
        assert steps <= 64, "%s: %d injected instances have not finished after %d steps" % (env_id, int((~finished[:n_inj]).sum()), steps)
    pair.coverage("%s reset inside a step%s (%d steps)" % (env_id, ", terminal frames kept" if final else "", steps), n_inj)
    assert not final or (pair.n_final == pair.n_done and pair.n_final >= n_inj)
    if "MortarMayhem" in env_id:  # the one-launch step did the resets (its FINAL form where terminal frames are kept)
        assert pair.env.debug_counter("one_launch_steps") == steps
    pair.close()


@pytest.mark.parametrize("env_id,n_inj,size,warmup,options", rc.EPISODE_CASES)
def test_draws_during_an_episode(env_id, n_inj, size, warmup, options):
    n_inj = n_inj or rc.injected(env_id)
    pair = Pair(env_id, size or rc.handle_size(n_inj), options)
    pair.reset(_seeds(pair.n), "seeded reset")
    for t in range(warmup):
        pair.step_unwatched(pair.ref.expert_actions(rc.EPISODE_EPS, rc.EPISODE_POLICY_SEED, t), "step %d" % t)
    pair.inject(n_inj)
    emp = env_id == "Endless-MysteryPath-v0"
    ahead_at_injection = pair.env.debug_counter("emp_ahead_records") if emp else 0
    for t in range(warmup, warmup + rc.EPISODE_STEPS):
        pair.step(pair.ref.expert_actions(rc.EPISODE_EPS, rc.EPISODE_POLICY_SEED, t), "step %d" % t)
    pair.coverage("%s x%d draws during an episode" % (env_id, pair.n), n_inj)
    if emp:  # which generator ran: records ahead of time belong to the lane generator's arrangement.  (The counter is the handle's: that
        # it grew behind the injection shows the arrangement at work then, not which instance's stream a record continued.)
        ahead = pair.env.debug_counter("emp_ahead_records")
        assert (ahead_at_injection > 0) == (pair.n > 20480) and (ahead > ahead_at_injection) == (pair.n > 20480), (
            "%d records ahead of time at the injection, %d at the end, %d instances" % (ahead_at_injection, ahead, pair.n))
    pair.close()


SEEDS_64 = [0, 1, 2**31 - 1, 2**32 - 1, 2**32, 2**32 + 7, 123456789012, 2**63 - 1]


@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "MortarMayhemB-v0", "MysteryPath-v0", "Endless-SearingSpotlights-v0"])
def test_seeds_of_64_bits(env_id):
    """Pcg::seed's second entropy word (ent[1] != 0): the oracle's seeding is pinned to numpy's for these seeds by tests/test_oracle_rng.py"""
    n = 64 + 3
    seeds = np.array((SEEDS_64 * 9)[:n], dtype=np.int64)
    pair = Pair(env_id, n, None)
    pair.watch = list(range(n))
    pair.reset(seeds, "seeded reset")
    prng = np.random.Generator(np.random.PCG64(22))
    for t in range(10):
        pair.step(rc.random_actions(prng, n, pair.ref.discrete), "step %d" % t)
    pair.close()
