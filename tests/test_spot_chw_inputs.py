"""The inputs of tests/test_gpu_spot_chw.py (the spotlight family's fused raster / reset launch in the image-order formats) and what the oracle
alone says about them (no GPU): that the runs reach what the GPU tests are about -- terminal rows and running rows in the same steps, and a
step with more finished instances than one service round of the launch takes (512 workgroups x 8 = 4,096).

The oracle's runs are computed once per (id, case) and shared by the formats (tests/chw_referee.py oracle_run: seeds arange(n) + 31, actions
from PCG64(6)); nothing changes them afterwards."""
from chw_referee import frozen, oracle_run

IDS = ("SearingSpotlights-v0", "Endless-SearingSpotlights-v0")
# Episodes that end within nine steps: max_steps truncates, one point of health lets a spotlight end them earlier (both kinds of ending in one run).
SHORT = {env_id: {"max_steps": 9, "agent_health": 1} for env_id in IDS}
# The same truncation with an agent no spotlight kills within nine steps: nearly every instance ends in the SAME step (9, 18).
# (use_exit on the finite id stays on: an agent that reaches the exit within nine steps leaves early -- few do; the assert below counts.)
IN_STEP = {env_id: {"max_steps": 9, "agent_health": 100} for env_id in IDS}

TERMINAL = dict(n=48, steps=60)            # case 1
ROUNDS = dict(n=4096 + 67, steps=20)       # case 2: no multiple of 64
ONE_ROUND = 512 * 8                        # SPOT_SVC_WGS x SPOT_SVC_BATCH (csrc/mg_spot_serve.hpp)
FORCED = dict(n=96, steps=40)              # case 4


def test_case_1_sees_terminal_and_running_rows():
    for env_id in IDS:
        n, steps = TERMINAL["n"], TERMINAL["steps"]
        run = oracle_run(env_id, n, steps, frozen(SHORT[env_id]), False)[2]
        n_done = sum(int(s[5].sum()) for s in run)
        n_running = sum(int((s[5] == 0).sum()) for s in run)
        assert n_done >= 6 * n, (env_id, n_done)  # max_steps = 9 over 60 steps: six endings per instance at the least
        assert n_running >= n, (env_id, n_running)


def test_case_2_fills_more_than_one_service_round():
    for env_id in IDS:
        run = oracle_run(env_id, ROUNDS["n"], ROUNDS["steps"], frozen(IN_STEP[env_id]), False)[2]
        most = max(int(s[5].sum()) for s in run)
        assert most > ONE_ROUND, (env_id, most)


def test_case_4_resets_instances():
    for env_id in IDS:
        run = oracle_run(env_id, FORCED["n"], FORCED["steps"], frozen(SHORT[env_id]), False)[2]
        assert sum(int(s[5].sum()) for s in run) > FORCED["n"]
