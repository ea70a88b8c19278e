"""CPU: the crafted PCG64 streams of tests/rng_craft.py against numpy itself (bit_generator.state assigned), the oracle's stream from
crafted words against numpy under spans that reject every second draw, and -- the oracle alone -- the injection plan of
tests/test_gpu_rng_edges.py with its coverage conditions, so that they are known to hold before anyone visits a GPU."""
import numpy as np
import pytest

import oracle_lib
import rng_craft as rc


@pytest.mark.parametrize("has", [0, 1])
def test_crafted_streams_produce_the_chosen_outputs(has):
    g = np.random.Generator(np.random.PCG64(11))
    for p in range(141):
        o1, o2 = int(g.integers(0, 1 << 64, dtype=np.uint64)), int(g.integers(0, 1 << 64, dtype=np.uint64))
        buf = int(g.integers(0, 1 << 32))
        w = rc.craft(p, o1, o2, has, buf, g)
        assert w[3] & 1 and all(0 <= x <= rc.M64 for x in w)
        ng = rc.numpy_generator(w)
        if has:  # the buffered half comes first and does not move the stream
            assert int(ng.integers(0, 1 << 32, dtype=np.uint32)) == buf
        raw = ng.bit_generator.random_raw(p + 2)
        assert int(raw[p]) == o1 and int(raw[p + 1]) == o2, "position %d" % p
        w1 = rc.craft(p, o1, None, has, buf, g)  # the second output left to chance
        assert int(rc.numpy_generator(w1).bit_generator.random_raw(p + 1)[p]) == o1


def test_the_patterns_do_what_the_plan_says():
    """numpy itself: 0 then 0xFFFFFFFF00000000 rejects three words of integers(0, 360) and returns 359; the L word gives 0; M gives
    n - 1 and a double of 1 - 2^-53."""
    g = np.random.Generator(np.random.PCG64(12))
    assert rc.threshold(360) == 256 and rc.L_WORD == 1 and rc.threshold(100) == 96 and rc.threshold(7) == 4 and rc.threshold(3) == 1
    assert rc.threshold(8) == 0 and rc.threshold(2) == 0
    for p in (0, 5):
        ng = rc.numpy_generator(rc.craft(p, 0, 0xFFFFFFFF00000000, 0, 0, g))
        ng.bit_generator.random_raw(p)
        assert int(ng.integers(0, 360)) == 359
        assert ng.bit_generator.state["has_uint32"] == 0  # four words: both outputs used up
        ng = rc.numpy_generator(rc.craft(p, rc.pattern_outputs("L")[0], None, 0, 0, g))
        ng.bit_generator.random_raw(p)
        assert [int(ng.integers(0, 360)), int(ng.integers(0, 360))] == [0, 0]
        ng = rc.numpy_generator(rc.craft(p, rc.M64, rc.M64, 0, 0, g))
        ng.bit_generator.random_raw(p)
        assert int(ng.integers(0, 360)) == 359 and int(ng.integers(0, 7056)) == 7055
        assert ng.random() == 1.0 - 2.0 ** -53


REJECTING = [2**31 + 1, 3 * 2**30, 2**32 - 1]  # thresholds 2^31 - 1, 2^30 and 1
ENV_SPANS = [3, 5, 9, 25, 36, 90, 270, 360, 7056, 7055, 7053, 7049, 7040]


@pytest.mark.parametrize("case", range(12))
def test_oracle_from_crafted_words_matches_numpy(case):
    """mgo_test_rng_words: the mixed integers / random / raw / uniform ops of tests/test_oracle_rng.py from crafted words, with the spans
    the environments draw and three that reject often.  numpy's own stream is asked first whether the inputs are what they claim: at
    least a quarter of the draws with the first two spans rejected there (arithmetic says a half and a quarter)."""
    L = oracle_lib.lib()
    n = 6000
    prng = np.random.default_rng(1000 + case)
    ops = prng.integers(0, 4, n).astype(np.int32)
    lo = prng.integers(-200, 200, n).astype(np.int64)
    span = prng.choice(ENV_SPANS + REJECTING * 4, n).astype(np.int64)
    hi = lo + span
    p = [0, 1, 7, 63, 64, 140][case % 6]
    name = rc.PATTERNS[case % 4]
    o1, o2 = rc.pattern_outputs(name)
    words = rc.craft(p, o1, o2, case & 1, int(prng.integers(0, 1 << 32)), prng)
    g = rc.numpy_generator(words)
    exp = np.empty(n)
    numpy_rejected = np.zeros(n, bool)
    for i in range(n):
        if ops[i] == 0:
            # how many words numpy itself takes for this draw: the raw stream of a twin that stands where g stands
            twin = rc.numpy_generator(_words_of(g))
            exp[i] = g.integers(lo[i], hi[i])
            numpy_rejected[i] = _words_between(twin, g) > 1
        elif ops[i] == 1:
            exp[i] = g.random()
        elif ops[i] == 2:
            exp[i] = int(g.bit_generator.random_raw()) >> 11
        else:
            exp[i] = g.uniform(lo[i] / 1e6, hi[i] / 1e6)
    # (arithmetic: (2^31 - 1) / 2^32 of the words for the first span, exactly a quarter -- the words divisible by four -- for the second)
    sel = (ops == 0) & ((span == REJECTING[0]) | (span == REJECTING[1]))
    assert sel.sum() > 300 and numpy_rejected[sel].mean() >= 0.25, "numpy rejected %.3f of the draws with the first two spans" % numpy_rejected[sel].mean()
    for sp in REJECTING:
        assert numpy_rejected[(ops == 0) & (span == sp)].any() or sp == REJECTING[2]
    out = np.empty(n)
    rej = np.zeros(n, np.uint32)
    w = np.array(words, dtype=np.uint64)
    total = L.mgo_test_rng_words(w.ctypes.data, ops.ctypes.data, lo.ctypes.data, hi.ctypes.data, n, out.ctypes.data, rej.ctypes.data)
    assert np.array_equal(out, exp)
    assert total == int(rej.sum()) and not rej[ops != 0].any()
    # the oracle's counter says the same as numpy's stream, op by op: a rejection where and only where numpy took more than one word
    assert np.array_equal(rej > 0, numpy_rejected)
    assert (rej[sel] > 0).mean() >= 0.25
    out2 = np.empty(n)  # (without the per-op counts: one run)
    assert L.mgo_test_rng_words(w.ctypes.data, ops.ctypes.data, lo.ctypes.data, hi.ctypes.data, n, out2.ctypes.data, None) == total
    assert np.array_equal(out2, exp)


def _words_of(g):
    st = g.bit_generator.state
    return [st["state"]["state"] >> 64, st["state"]["state"] & rc.M64, st["state"]["inc"] >> 64, st["state"]["inc"] & rc.M64,
            st["has_uint32"], st["uinteger"]]


def _words_between(before, after):
    """32-bit words a generator consumed between two of its positions"""
    wb, wa = _words_of(before), _words_of(after)
    return 2 * rc.outputs_between(wb, wa) + int(wb[4]) - int(wa[4])


def test_env_hooks_set_and_report():
    """mgo_rng_set_words is the mirror of mgo_rng_words, makes reset(seed=None) legal, and the bookkeeping alters no draw."""
    g = np.random.Generator(np.random.PCG64(13))
    words = rc.craft(3, 0, None, 1, 77, g)
    a, b = oracle_lib.OracleEnv("Endless-SearingSpotlights-v0"), oracle_lib.OracleEnv("Endless-SearingSpotlights-v0")
    a.set_rng_words(words)
    assert [int(x) for x in a.rng_words()] == words
    f1 = a.reset(None)
    st = a.rng_stats()
    assert st["rejected"] >= 1 and 360 in st["spans"] and st["outputs"] == rc.outputs_between(words, a.rng_words())
    assert all(o == 3 for o, _ in st["rej_at"]) and {h for _, h in st["rej_at"]} <= {0, 1}
    assert a.rng_stats(clear=True)["rejected"] == st["rejected"] and a.rng_stats()["rejected"] == 0
    # the same stream entered by seeding somewhere else and assigning the words afterwards: the same frame, the same end state
    b.reset(5)
    b.set_rng_words(words)
    f2 = b.reset(None)
    assert np.array_equal(f1, f2) and np.array_equal(a.rng_words(), b.rng_words())
    a.close()
    b.close()


# ---- the injection plan of tests/test_gpu_rng_edges.py on the oracle alone ----------------------------------------------------------------
# (`pytest -s` prints what the oracle's bookkeeping saw per id and case: profiles/rng_edges.md)

@pytest.mark.parametrize("env_id", rc.ALL_IDS)
def test_plan_explicit_reset(env_id):
    n_inj = rc.injected(env_id)
    assert 8 * rc.P_MARGIN < n_inj <= 640
    n = rc.handle_size(n_inj)
    assert n % 64 == 3
    ref = oracle_lib.OracleBatch(env_id, n, options=rc.RESET_OPTIONS[env_id])
    ref.reset_digest(np.arange(n, dtype=np.int64) + 500)
    rc.inject(ref, None, n_inj)
    ref.reset_digest(None)
    cov = rc.Coverage(env_id, ref, n_inj)
    print("\n%s explicit reset, P = %d: %s" % (env_id, n_inj // 8, cov.summary()))
    cov.assert_instances(env_id + " explicit reset")
    cov.assert_every_rejectable_span_rejected(env_id + " explicit reset")
    if env_id in rc.MYSTERY:
        print("   last rejection / most outputs behind the hand-over: %s" % (rc.check_mystery_rejections(env_id, env_id, cov),))
    if env_id in rc.SPOT:
        rc.check_spot_wirings(env_id, cov)
    ref.close()


@pytest.mark.parametrize("env_id", rc.ALL_IDS)
def test_plan_reset_inside_a_step(env_id):
    n_inj = rc.injected(env_id)
    n = rc.handle_size(n_inj)
    ref = oracle_lib.OracleBatch(env_id, n, options=rc.short_options(env_id))
    ref.reset_digest(np.arange(n, dtype=np.int64) + 500)
    rc.inject(ref, None, n_inj)
    prng = np.random.Generator(np.random.PCG64(21))
    finished = np.zeros(n, bool)
    steps = 0
    while not finished[:n_inj].all():
        finished |= ref.step_digest(rc.random_actions(prng, n, ref.discrete), autoreset=True)[3].astype(bool)
        steps += 1
        assert steps <= 64, "%d injected instances have not finished after %d steps" % (int((~finished[:n_inj]).sum()), steps)
    cov = rc.Coverage(env_id, ref, n_inj)
    print("\n%s reset inside a step (%d steps): %s" % (env_id, steps, cov.summary()))
    cov.assert_instances(env_id + " reset inside a step")
    ref.close()


@pytest.mark.parametrize("env_id,n_inj,size,warmup,options", rc.EPISODE_CASES)
def test_plan_draws_during_an_episode(env_id, n_inj, size, warmup, options):
    """(instances do not interact: the oracle's plan check of the 20,481-instance case runs the injected instances and a few more)"""
    n_inj = n_inj or rc.injected(env_id)
    n = rc.handle_size(n_inj)
    ref = oracle_lib.OracleBatch(env_id, n, options=options)
    ref.reset_digest(np.arange(n, dtype=np.int64) + 500)
    for t in range(warmup + rc.EPISODE_STEPS):
        if t == warmup:
            rc.inject(ref, None, n_inj)
        ref.step_digest(ref.expert_actions(rc.EPISODE_EPS, rc.EPISODE_POLICY_SEED, t), autoreset=True)
    cov = rc.Coverage(env_id, ref, n_inj)
    print("\n%s x%s draws during an episode: %s" % (env_id, size or n, cov.summary()))
    cov.assert_instances("%s x%s draws during an episode" % (env_id, size or n))
    ref.close()


# ---- the arrangement cases of tests/test_gpu_rng_edges_arrangements.py on the oracle alone -------------------------------------------------

def test_second_option_sets_have_other_spans_that_can_reject():
    """list lengths 3 against 5 or 6, radius spans 7 against 5: every threshold non-zero; the two dictionaries of an id name the same
    keys or keys no handle treats as geometry (lists, radii, max_steps, health, a reward)"""
    assert all(rc.threshold(s) > 0 for s in (3, 5, 6, 7))
    geometry = ("arena_size", "agent_scale", "agent_speed", "coin_scale", "show_last_action", "initial_spawn_interval", "spawn_interval_threshold",
                "exit_scale", "camera_offset_scale")
    for env_id, (a, b) in rc.TWO_SETS.items():
        assert a != b and not any(k in geometry for k in list(a) + list(b)), env_id
        own = rc.TWO_SETS_OWN_SPANS[env_id]
        if own is not None:
            assert not (own[0] & own[1]) and all(rc.threshold(s) > 0 for s in own[0] | own[1]), env_id


def test_arrangement_table_sizes():
    """no case above 1,300 instances or 200 calls; every size leaves the last wave partial (n % 64 == 3, twice that for two sets)"""
    seen = set()
    for case in rc.ARRANGEMENT_CASES:
        env_id, arr, n_inj, size, _, cap = case
        n = size or rc.handle_size(n_inj or rc.injected(env_id))
        n *= 2 if arr.endswith("sets") else 1
        assert n <= 1300 and 1 <= cap <= 200 and n % 64 in (3, 6), case
        assert rc.case_id(case) not in seen
        seen.add(rc.case_id(case))
    assert {c[0] for c in rc.ARRANGEMENT_CASES if c[1] in ("headless", "masked", "masked-reset")} == set(rc.ALL_IDS)


@pytest.mark.parametrize("case", rc.ARRANGEMENT_CASES, ids=rc.case_id)
def test_plan_arrangement(case):
    """The oracle needs exactly the calls of the row's cap (so it stays within it) and its books show the case's conditions (rc.check_arrangement): 32 injected instances with
    a rejection (per set where there are two), each set's own span, both has_uint32 values behind the lane generator's hand-over."""
    side, calls, covs = rc.run_arrangement(case, lambda env_id, n, options, final=False, autoreset=True, sets=None: rc.OracleSide(env_id, n, options, sets=sets))
    rc.check_arrangement(case, side, calls, covs, exact=True)
    side.close()
