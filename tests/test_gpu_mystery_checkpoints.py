"""GPU (-m gpu): checkpoints of the three Mystery Path ids written by an EARLIER commit's build (tests/golden/mystery_checkpoints.npz,
tests/golden/make_mystery_checkpoints.py; the commit's id is in the fixture) still load, and a fresh handle that was never reset computes
from them what that build computed: every step's rewards, dones, ground truth and info records, the stored frames and the RNG words,
bit for bit.  The state's payload -- which blobs, in which order, of which sizes -- is what mg_set_state checks and what a
change of the host classes can silently move."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mystery_checkpoints.npz")
ENV_IDS = {"mp": "MysteryPath-v0", "mpg": "MysteryPath-Grid-v0", "emp": "Endless-MysteryPath-v0", "emp_cap7": "Endless-MysteryPath-v0"}


@pytest.fixture(scope="module")
def stored():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", sorted(ENV_IDS))
def test_earlier_checkpoint_loads_and_replays(stored, case):
    import memory_gym_amd

    assert sorted(stored["cases"].tolist()) == sorted(ENV_IDS)
    get = lambda key: stored[case + "/" + key]
    env_id, n = ENV_IDS[case], get("actions").shape[1]
    capacity = json.loads(str(get("capacity")))
    assert n == 3 and capacity == ({"path_segments": 7} if case == "emp_cap7" else {})
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, capacity=capacity or None)
    blob = get("blob")
    assert len(env.state_dict()["blob"]) == len(blob), "%s: the state's payload changed its size" % case
    env.load_state_dict({"env_id": env_id, "num_envs": n, "blob": blob, "options": json.loads(str(get("options"))),
                         "capacity": capacity, "seeded": bool(get("seeded"))})  # no reset on this handle
    actions, frames = get("actions"), get("frames")
    steps = len(actions)
    assert steps >= 40 and get("done").any(), "%s: the fixture must hold an episode's end" % case
    for t in range(steps):
        obs, rew, done, _, info = env.step(actions[t])
        d = done.cpu().numpy()
        assert np.array_equal(d, get("done")[t]), "%s: dones differ at replayed step %d" % (case, t)
        assert rew.cpu().numpy().tobytes() == get("reward")[t].tobytes(), "%s: rewards differ at replayed step %d" % (case, t)
        if env.gt_dim:
            assert info["ground_truth"].cpu().numpy().tobytes() == get("ground_truth")[t].tobytes(), "%s: ground truth differs at replayed step %d" % (case, t)
        for nm in ["reward", "length"] + list(env.info_names):
            v = info[nm].cpu().numpy()
            assert np.where(d, v, np.zeros_like(v)).tobytes() == get("info_" + nm)[t].tobytes(), "%s: info[%r] differs at replayed step %d" % (case, nm, t)
        if t == 0 or t == steps - 1:
            assert np.array_equal(obs.cpu().numpy(), frames[0 if t == 0 else 1]), "%s: the frame after replayed step %d differs" % (case, t)
    assert np.array_equal(np.stack([env.rng_words(i) for i in range(n)]), get("rng_words")), "%s: RNG words differ after the replay" % case
    env.check_errors()
    env.close()
