"""CPU: the referee refereed.  tests/chw_referee.py decides a hundred GPU cases; a slip in it (a tensor compared with itself, say) would let
them all pass.  Here its comparisons meet what they must accept and, one alteration at a time, what they must reject -- without a GPU: a
stand-in handle replays the oracle's own frames through converted() on CPU tensors, and tests/frame_digest.py digests CPU tensors as well.

The smallest shapes at which it can go wrong: 8 instances, 12 steps, max_steps = 9 (every episode ends within the run, so finished and
running rows both occur; in which steps: test_the_runs_hold_what_the_cases_need), an id without ground truth and one with."""
import numpy as np
import pytest

import frame_digest as fd
from chw_referee import CHW, FLOATS, SENTINEL, check_step, converted, frozen, lock_step_with_the_oracle, oracle_run, unit_values
from test_emp_chw_inputs import ENV_ID as EMP
from test_emp_chw_inputs import SHORT as EMP_SHORT
from test_spot_chw_inputs import IDS as SPOT_IDS
from test_spot_chw_inputs import SHORT as SPOT_SHORT

N, STEPS = 8, 12
AT, WHO = 5, 2  # the step and the instance of every alteration
OPTIONS = {SPOT_IDS[0]: SPOT_SHORT[SPOT_IDS[0]], EMP: EMP_SHORT}  # SearingSpotlights-v0: no ground truth; Endless-MysteryPath-v0: has one
IDS = tuple(OPTIONS)


def the_run(env_id):
    return oracle_run(env_id, N, STEPS, frozen(OPTIONS[env_id]), True)


def a_step_with(env_id, kind):
    """the first step of the run with "finished" / "running" rows; one with rows of both kinds where the run has such a step"""
    counts = [int(s[5].sum()) for s in the_run(env_id)[2]]
    steps = [t for t, k in enumerate(counts) if (k > 0 if kind == "finished" else k < N)]
    return min(steps, key=lambda t: (not 0 < counts[t] < N, t))


def test_the_runs_hold_what_the_cases_need():
    """From the oracle alone.  Both runs see finished rows and running rows.  Endless-MysteryPath-v0's has them in ONE step (6 of 8 finish in
    step 2: stamina), which is where its cases below look.  SearingSpotlights-v0's has not: at 8 instances no agent dies early, all eight
    are truncated in step 8 and none in any other step -- its cases look at step 8 for terminal rows and at step 0 for running rows.
    Ground truth on one id only; a step AT to alter."""
    for env_id in IDS:
        run = the_run(env_id)[2]
        counts = [int(s[5].sum()) for s in run]
        assert len(run) == STEPS > AT and max(counts) > 0 and min(counts) < N, counts
        assert (run[AT][6] is not None) == (env_id == EMP)
    counts = [int(s[5].sum()) for s in the_run(EMP)[2]]
    assert 0 < counts[a_step_with(EMP, "finished")] < N and 0 < counts[a_step_with(EMP, "running")] < N, counts


class Replay:
    """Stand-in for a handle: every step returns what the oracle said, frames through converted(fmt, .), after alter(t, step) had its way
    with copies of the oracle's arrays (step: dict of frames uint8 [n][x][y][c], reward, done, gt)."""

    def __init__(self, env_id, fmt, alter):
        _, (self.first, _), self.run = the_run(env_id)
        self.fmt, self.alter, self.t = fmt, alter, 0

    def reset(self, seed, options):
        return converted(self.fmt, self.first), {}

    def step(self, actions):
        import torch

        a, frames, _, _, rew, done, gt = self.run[self.t]
        assert actions is a
        s = dict(frames=frames.copy(), reward=rew.astype(np.float32), done=done.astype(bool), gt=None if gt is None else gt.copy())
        if self.alter:
            self.alter(self.t, s)
        self.t += 1
        info = {} if gt is None else {"ground_truth": torch.from_numpy(s["gt"])}
        return converted(self.fmt, s["frames"]), torch.from_numpy(s["reward"]), torch.from_numpy(s["done"]), None, info

    def check_errors(self):
        pass


def replay(env_id, fmt, alter=None):
    def make(env_id, num_envs, device, obs_format, final_observation):
        assert num_envs == N and not final_observation
        return Replay(env_id, obs_format, alter)

    return lock_step_with_the_oracle(env_id, fmt, N, STEPS, OPTIONS[env_id], final=False, make=make)


@pytest.mark.parametrize("env_id,fmt", [(e, f) for e in IDS for f in CHW])  # (id by id: oracle_run is shared)
def test_the_oracles_own_frames_pass(env_id, fmt):
    n_done, n_running, most, _ = replay(env_id, fmt)
    run = the_run(env_id)[2]
    assert n_done == sum(int(s[5].sum()) for s in run) > 0 and n_done + n_running == N * STEPS
    assert most == max(int(s[5].sum()) for s in run)


def one_byte(t, s):
    if t == AT:
        s["frames"][WHO, 40, 41, 1] ^= 1


def one_done_flag(t, s):
    if t == AT:
        s["done"][WHO] ^= True


def one_reward(t, s):
    if t == AT:
        s["reward"][WHO] += np.float32(0.5)


def one_ground_truth_entry(t, s):
    if t == AT:
        s["gt"][WHO, 0] += np.float32(1)


ALTERATIONS = ([(e, f, one_byte, "frames") for e in IDS for f in CHW]
               + [(e, f, a, w) for e in IDS for f in ("bf16_chw", "u8_chw") for a, w in ((one_done_flag, "dones"), (one_reward, "rewards"))]
               + [(EMP, f, one_ground_truth_entry, "ground truth") for f in ("bf16_chw", "u8_chw")])


@pytest.mark.parametrize("env_id,fmt,alter,what", ALTERATIONS, ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_one_alteration_is_rejected(env_id, fmt, alter, what):
    with pytest.raises(AssertionError, match="%s .* step %d" % (what, AT)):
        replay(env_id, fmt, alter)


def a_step_with_terminal_rows(env_id, fmt, by_digest, kind="finished"):
    """-> (t, got, want, an instance of that kind) for check_step(final=True) at a_step_with(env_id, kind): the rows of finished
    instances hold converted(fmt, .) of this step's frames (oracle frames as good as any), want's final digests are digest_numpy of those
    frames, every other row holds the sentinel.  by_digest: want carries no frames, as in a run of oracle_run(frames=False)."""
    import torch

    t = a_step_with(env_id, kind)
    a, frames, dg, _, rew, done, gt = the_run(env_id)[2][t]
    d = done.astype(bool)
    rows = torch.full((N, 3, 84, 84), SENTINEL[fmt], dtype=converted(fmt, frames[:1]).dtype)
    rows[torch.from_numpy(d)] = converted(fmt, frames[d])
    final_digest = np.zeros(N, np.uint64)
    if d.any():
        final_digest[d] = fd.digest_numpy(frames[d])
    info = {"final_observation": rows}
    if gt is not None:
        info["ground_truth"] = torch.from_numpy(gt.copy())
    got = (converted(fmt, frames), torch.from_numpy(rew.astype(np.float32)), torch.from_numpy(d), info)
    want = (a, None if by_digest else frames, dg, final_digest, rew, done, gt)
    return t, got, want, int(np.nonzero(d if kind == "finished" else ~d)[0][0])


STEP_CASES = [(e, f, b) for e in IDS for f in CHW for b in (False, True)]


@pytest.mark.parametrize("kind", ["finished", "running"])
@pytest.mark.parametrize("env_id,fmt,by_digest", STEP_CASES)
def test_a_step_with_terminal_rows_passes(env_id, fmt, by_digest, kind):
    t, got, want, _ = a_step_with_terminal_rows(env_id, fmt, by_digest, kind)
    assert np.array_equal(check_step("case", fmt, t, got, want, final=True), want[5].astype(bool))


def another_value(fmt, x):
    """a value of the format that differs from x: the next byte's"""
    if fmt == "u8_chw":
        return int(x) ^ 1
    lut = unit_values(fmt)
    return lut[(int((lut == x).nonzero()[0, 0]) + 1) % 256]


@pytest.mark.parametrize("env_id,fmt,by_digest", STEP_CASES)
def test_one_altered_value_in_a_frame_is_rejected_by_either_comparison(env_id, fmt, by_digest):
    t, got, want, _ = a_step_with_terminal_rows(env_id, fmt, by_digest)
    got[0][WHO, 1, 41, 40] = another_value(fmt, got[0][WHO, 1, 41, 40])
    with pytest.raises(AssertionError, match="frames at step %d differ" % t):
        check_step("case", fmt, t, got, want, final=True)


@pytest.mark.parametrize("env_id,fmt", [(e, f) for e in IDS for f in CHW])
def test_one_altered_value_in_a_terminal_row_is_rejected(env_id, fmt):
    t, got, want, finished = a_step_with_terminal_rows(env_id, fmt, False)
    rows = got[3]["final_observation"]
    rows[finished, 2, 7, 70] = another_value(fmt, rows[finished, 2, 7, 70])
    with pytest.raises(AssertionError, match="terminal frames at step %d differ" % t):
        check_step("case", fmt, t, got, want, final=True)


@pytest.mark.parametrize("env_id,fmt", [(e, f) for e in IDS for f in FLOATS])
def test_a_value_between_two_table_entries_is_rejected(env_id, fmt):
    """Halfway between the values of bytes 1 and 2 (there every format has values in between): round(x * 255) names a byte, the byte's value
    is not x."""
    t, got, want, finished = a_step_with_terminal_rows(env_id, fmt, False)
    lut = unit_values(fmt)
    mid = ((lut[1].float() + lut[2].float()) / 2).to(lut.dtype)
    assert lut[1] < mid < lut[2]
    got[3]["final_observation"][finished, 0, 0, 0] = mid
    with pytest.raises(AssertionError, match="terminal frames at step %d hold a value no byte maps to" % t):
        check_step("case", fmt, t, got, want, final=True)


@pytest.mark.parametrize("env_id,fmt", [(e, f) for e in IDS for f in CHW])
def test_one_value_written_to_a_running_row_is_rejected(env_id, fmt):
    t, got, want, running = a_step_with_terminal_rows(env_id, fmt, False, "running")
    got[3]["final_observation"][running, 1, 83, 83] = 0
    with pytest.raises(AssertionError, match="a row of a running instance was written at step %d" % t):
        check_step("case", fmt, t, got, want, final=True)
