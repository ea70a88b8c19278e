"""The inputs of tests/test_gpu_emp_chw.py (Endless-MysteryPath-v0's fused raster / service launch in the image-order formats) and what the
oracle alone says about them (no GPU): that the runs reach what the GPU tests are about -- terminal rows and running rows in the same steps, a
step with more finished instances than one service round of the small launch takes (EMP_SVC_WGS_SMALL x 4 waves = 3,072), and, in the lane
regime (more than 20,480 instances), a step with more than EMP_SVC_WGS_PRE x 4 = 256 of them.

The oracle's runs are computed once per case and shared by the formats (tests/chw_referee.py oracle_run: seeds arange(n) + 31, actions from
PCG64(6)); nothing changes them afterwards."""
from chw_referee import frozen, oracle_run

ENV_ID = "Endless-MysteryPath-v0"
# Episodes that end within nine steps: max_steps truncates, three points of stamina let an agent off the path end them earlier (both kinds of ending in one run).
SHORT = {"max_steps": 9, "stamina_level": 3}
# The same truncation with the default stamina (20): nearly every instance ends in the SAME step (9, 18).
IN_STEP = {"max_steps": 9}

TERMINAL = dict(n=48, steps=60)        # case 1
ROUNDS = dict(n=4163, steps=20)        # case 2: no multiple of 64
ONE_ROUND = 768 * 4                    # EMP_SVC_WGS_SMALL x the four service waves of a workgroup (csrc/mg_mystery_endless_launch.hpp)
# case 3: beyond 20,480 instances the handle leaves bg_coop (lane generator, background workgroups, records ahead of time, plain stores); no multiple
# of 64 or 256.  20 steps, not tuned on the code under test: a u8_xyc handle of the parent commit on these inputs shows records ahead of time from
# its second step on ("emp_ahead_records": 1,623 after two steps, 11,930 when 19,279 instances finish in step 9, 16,296 after twenty).
LANES = dict(n=20481, steps=20)
ONE_ROUND_PRE = 64 * 4                 # EMP_SVC_WGS_PRE x 4
FORCED = dict(n=96, steps=40)          # case 4


def most_in_one_step(run):
    return max(int(s[5].sum()) for s in run)


def test_case_1_sees_terminal_and_running_rows():
    n, steps = TERMINAL["n"], TERMINAL["steps"]
    run = oracle_run(ENV_ID, n, steps, frozen(SHORT), False)[2]
    n_done = sum(int(s[5].sum()) for s in run)
    n_running = sum(int((s[5] == 0).sum()) for s in run)
    assert n_done >= 6 * n, n_done  # max_steps = 9 over 60 steps: six endings per instance at the least
    assert n_running >= n, n_running


def test_case_2_fills_more_than_one_service_round():
    assert ROUNDS["n"] % 64 != 0
    run = oracle_run(ENV_ID, ROUNDS["n"], ROUNDS["steps"], frozen(IN_STEP), False)[2]
    assert most_in_one_step(run) > ONE_ROUND, most_in_one_step(run)


def test_case_3_fills_more_than_one_service_round_of_the_lane_regime():
    assert LANES["n"] > 20480 and LANES["n"] % 64 != 0 and LANES["n"] % 256 != 0
    run = oracle_run(ENV_ID, LANES["n"], LANES["steps"], frozen(IN_STEP), False)[2]
    assert most_in_one_step(run) > ONE_ROUND_PRE, most_in_one_step(run)


def test_case_4_resets_instances():
    run = oracle_run(ENV_ID, FORCED["n"], FORCED["steps"], frozen(SHORT), False)[2]
    assert sum(int(s[5].sum()) for s in run) > FORCED["n"]
