"""Shared inputs of tests/test_gpu_masked_step.py (a plain helper module like tests/gpu_parity.py: no tests of its own): the reset options
under which episodes end inside every test, the action table and the masks, and the CPU oracle stepped one instance at a time under a mask.

Instance i's k-th ACTIVE step uses act[k, i], so an instance's action sequence does not depend on when it is active."""
import numpy as np

MORTAR = ("MortarMayhem-Grid-v0", "MortarMayhem-v0", "Endless-MortarMayhem-v0", "MortarMayhemB-Grid-v0", "MortarMayhemB-v0")
MYSTERY = ("MysteryPath-v0", "MysteryPath-Grid-v0", "Endless-MysteryPath-v0")
SPOT = ("SearingSpotlights-v0", "Endless-SearingSpotlights-v0")
ALL_IDS = MORTAR + MYSTERY + SPOT
ONE_PER_FAMILY = ("MortarMayhem-Grid-v0", "SearingSpotlights-v0", "MysteryPath-Grid-v0")

SHORT = {
    "MortarMayhem-Grid-v0": dict(command_count=[2], command_show_duration=[1], command_show_delay=[0], explosion_delay=[2], explosion_duration=[1]),
    "MortarMayhem-v0": dict(command_count=[2], command_show_duration=[1], command_show_delay=[0], explosion_delay=[4], explosion_duration=[2]),
    "Endless-MortarMayhem-v0": dict(command_show_duration=[1], command_show_delay=[0], explosion_delay=[4], explosion_duration=[2]),
    "MortarMayhemB-Grid-v0": dict(command_count=[2], explosion_delay=[2], explosion_duration=[1]),
    "MortarMayhemB-v0": dict(command_count=[2], explosion_delay=[4], explosion_duration=[2]),
}
for _e in MYSTERY + SPOT:
    SHORT[_e] = dict(max_steps=12)
SEED0 = 1000


def full(env_id, opts):
    from memory_gym_amd.reset_params import process_reset_params
    return process_reset_params(env_id, opts)


def seeds(n):
    return np.arange(n, dtype=np.int64) + SEED0


def actions(rng, discrete, t, n):
    """uniform actions from `rng`: int32 [t, n] for Discrete ids, [t, n, 2] otherwise"""
    return (rng.integers(0, 4, (t, n)) if discrete else rng.integers(0, 3, (t, n, 2))).astype(np.int32)


def bernoulli_inputs(discrete, t, n, seed=7, p=0.5):
    """(mask bool [t, n], act): first the mask, then the actions, from one default_rng(seed)"""
    rng = np.random.default_rng(seed)
    mask = rng.random((t, n)) < p
    return mask, actions(rng, discrete, t, n)


def block_masks(t, n):
    """whole waves and whole 16-lane groups go silent, beside partial ones at the seam: with ph = (t // 8) & 1, instance idx < n / 2 is active
    iff ((idx // 64) & 1) == ph, the others iff ((idx // 16) & 1) == ph"""
    idx = np.arange(n)
    unit = np.where(idx < n // 2, (idx // 64) & 1, (idx // 16) & 1)
    ph = (np.arange(t) // 8) & 1
    return unit[None, :] == ph[:, None]


def sparse_masks(t, n):
    """one instance in eight, rows 5 and 6 all False, rows 50 and 51 all True"""
    m = np.random.default_rng(11).random((t, n)) < 0.125
    m[5:7] = False
    m[50:52] = True
    return m


def pick(act, counts):
    """the actions of this call: row counts[i] of instance i's column"""
    return np.ascontiguousarray(act[counts, np.arange(len(counts))])


class MaskedOracle:
    """An OracleBatch whose envs[i] are stepped one by one: envs[i].step runs for active i only, envs[i].reset(None) follows where done
    (same-call auto-reset).  Keeps what a handle reports: reward64 / done of the call, the episode record and the named aux infos where done."""

    def __init__(self, env_id, n, options, info_names, ref=None):
        """ref: an OracleBatch that has been reset already (otherwise one under full(env_id, options), reset with seeds(n))"""
        import oracle_lib

        self.n, self.names = n, tuple(info_names)
        self.ref = ref
        if ref is None:
            self.ref = oracle_lib.OracleBatch(env_id, n, options=full(env_id, options))
            self.ref.reset(seeds(n))
        self.discrete = self.ref.discrete
        self.episodes = np.zeros(n, np.int64)
        self.active_steps = np.zeros(n, np.int64)

    def step(self, a, active, autoreset=True):
        """-> (reward float64 [n], done bool [n], info {name: float64 [n]}, valid where done)"""
        n = self.n
        reward, done = np.zeros(n), np.zeros(n, bool)
        info = {k: np.zeros(n) for k in ("reward", "length") + self.names}
        for i in np.nonzero(active)[0]:
            e = self.ref.envs[i]
            _, reward[i], d = e.step(a[i], want_obs=False)
            if d:
                done[i] = True
                for k in info:
                    info[k][i] = e.get("info_" + k)
                if autoreset:
                    e.reset(None, want_obs=False)
        self.episodes += done
        self.active_steps += np.asarray(active, bool)
        return reward, done, info

    def frames(self, which):
        return self.ref.frames(which)

    def rng_words(self, i):
        return self.ref.envs[i].rng_words()

    def close(self):
        self.ref.close()
