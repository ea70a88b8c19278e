"""Shared inputs of tests/test_gpu_next_step.py (a plain helper module like tests/masked_step_inputs.py: no tests of its own): the CPU oracle stepped one
instance at a time under restart flags, the action table of the rollouts, the option pairs of the two-set test and the episode counts the oracle ALONE
gives with exactly these inputs.  `python tests/next_step_inputs.py` (no GPU) recomputes and prints those counts."""
import numpy as np

import masked_step_inputs as mi

N, T = 67, 40  # four full 16-instance spotlight workgroups and three instances; one mortar wave and three lanes

# episodes that end in T next-step calls of N instances under mi.SHORT, seeds mi.seeds(N), actions rollout_actions(): measured by main() below
EPISODES = {"MortarMayhem-Grid-v0": 464, "MortarMayhem-v0": 322, "Endless-MortarMayhem-v0": 361, "MortarMayhemB-Grid-v0": 561, "MortarMayhemB-v0": 361,
            "MysteryPath-v0": 201, "MysteryPath-Grid-v0": 201, "Endless-MysteryPath-v0": 201, "SearingSpotlights-v0": 201, "Endless-SearingSpotlights-v0": 201}

TWO_SETS = {
    "SearingSpotlights-v0": (dict(num_coins=[3], use_exit=True, max_steps=12), dict(num_coins=[1, 2], use_exit=False, max_steps=9)),
    "MortarMayhem-Grid-v0": (dict(mi.SHORT["MortarMayhem-Grid-v0"]), dict(mi.SHORT["MortarMayhem-Grid-v0"], command_count=[3])),
}
# the halves of 64 instances (seeds arange(64) + 3) under TWO_SETS, T calls: measured by main() below
TWO_SET_EPISODES = {"SearingSpotlights-v0": (96, 128), "MortarMayhem-Grid-v0": (218, 173)}


def rollout_actions(discrete, t, n, seed=13):
    return mi.actions(np.random.default_rng(seed), discrete, t, n)


class NextOracle:
    """An OracleBatch whose envs[i] are driven one by one: envs[i].reset(None) where restart[i] is set (reward 0, done False), else envs[i].step(a[i]);
    nobody is reset in the step that ends its episode.  Keeps what a handle reports: reward64 / done of the call, the episode record where done."""

    def __init__(self, env_id, n, info_names, ref=None):
        """ref: an OracleBatch that has been reset already (otherwise one under the id's short-episode options, reset with mi.seeds(n))"""
        import oracle_lib

        self.n, self.names = n, tuple(info_names)
        self.ref = ref
        if ref is None:
            self.ref = oracle_lib.OracleBatch(env_id, n, options=mi.full(env_id, mi.SHORT[env_id]))
            self.ref.reset(mi.seeds(n))
        self.episodes = np.zeros(n, np.int64)

    def step(self, a, restart):
        """-> (reward float64 [n], done bool [n], info {name: float64 [n]}, valid where done)"""
        n = self.n
        reward, done = np.zeros(n), np.zeros(n, bool)
        info = {k: np.zeros(n) for k in ("reward", "length") + self.names}
        for i in range(n):
            e = self.ref.envs[i]
            if restart[i]:
                e.reset(None, want_obs=False)
                continue
            _, reward[i], d = e.step(a[i], want_obs=False)
            if d:
                done[i] = True
                for k in info:
                    info[k][i] = e.get("info_" + k)
        self.episodes += done
        return reward, done, info

    def frames(self):
        return self.ref.frames(range(self.n))

    def rng_words(self, i):
        return self.ref.envs[i].rng_words()

    def close(self):
        self.ref.close()


def two_set_oracles(env_id, n, info_names):
    """the two halves of the two-set test as oracle batches, reset the way the handle is (SearingSpotlights: every instance gets an exit under the
    defaults first -- use_exit = False keeps drawing the earlier one)"""
    import oracle_lib

    half = n // 2
    opt_a, opt_b = TWO_SETS[env_id]
    seeds = np.arange(n, dtype=np.int64) + 3
    ref_a = oracle_lib.OracleBatch(env_id, half, options=mi.full(env_id, opt_a))
    ref_b = oracle_lib.OracleBatch(env_id, half, options=mi.full(env_id, dict()))
    ref_b.reset(seeds[half:])
    ref_b.set_options(mi.full(env_id, opt_b))
    ref_a.reset(seeds[:half])
    ref_b.reset(seeds[half:])
    return [NextOracle(env_id, half, info_names, ref=r) for r in (ref_a, ref_b)]


def run(oracles, slices, discrete, n):
    act = rollout_actions(discrete, T, n)
    prev = np.zeros(n, bool)
    for t in range(T):
        prev = np.concatenate([o.step(act[t][sl], prev[sl])[1] for o, sl in zip(oracles, slices)])
    return [int(o.episodes.sum()) for o in oracles]


def main():
    import oracle_lib

    for env_id in mi.ALL_IDS:
        o = NextOracle(env_id, N, ())
        print(env_id, run([o], [slice(0, N)], o.ref.discrete, N))
        o.close()
    for env_id in TWO_SETS:
        os_ = two_set_oracles(env_id, 64, ())
        print(env_id, "two sets", run(os_, [slice(0, 32), slice(32, 64)], os_[0].ref.discrete, 64))


if __name__ == "__main__":
    import os
    import sys

    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(ROOT, "endless-memory-gym_amd"))
    main()
