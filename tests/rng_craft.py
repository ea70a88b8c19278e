"""PCG64 run backwards -- test infrastructure: streams whose 64-bit outputs at a chosen position are chosen values, so that a rejected
bounded draw (Lemire's loop, 6e-8 per draw for a span of 360) or an extreme word happens WHERE a test wants it instead of once in 10^7.

PCG64 (numpy's: the 128-bit LCG  s' = s * A + inc  with the XSL-RR output  ror64(hi ^ lo, hi >> 58)  of the state AFTER the step):
    * the output fixes only hi ^ lo once hi is chosen: choose hi freely, lo = rol64(output, hi >> 58) ^ hi;
    * two consecutive states s1, s2 fix the increment: inc = s2 - s1 * A  (mod 2^128), a legal one if it is odd -- half of all
      choices of the two high words; retry with other ones;
    * the LCG steps backwards with A^-1 (A is odd): s = (s' - inc) * A^-1.
craft() returns the stream in the six words of rng_words() / mg_debug_rng: {state_hi, state_lo, inc_hi, inc_lo, has_uint32, uinteger}.

The second half is the INJECTION PLAN that tests/test_rng_craft.py (the oracle alone, no GPU) and tests/test_gpu_rng_edges.py (HIP against
the oracle) share: which instance receives which stream, per env id the options and the sweep of positions, and the coverage conditions
read from the oracle's bookkeeping (oracle/mgo_rng.h mgo_rng_book).  The third part, "the arrangement axis", is the table, the driver and the
conditions that tests/test_gpu_rng_edges_arrangements.py shares with tests/test_rng_craft.py in the same way."""
import numpy as np

M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
PCG_MULT = (0x2360ED051FC65DA4 << 64) | 0x4385DF649FCCF645
PCG_MULT_INV = pow(PCG_MULT, -1, 1 << 128)


def rol64(x, r):
    r &= 63
    return ((x << r) | (x >> ((64 - r) & 63))) & M64 if r else x


def output_of(state):
    """XSL-RR 128/64 of a state (the state AFTER its step)"""
    hi, lo = state >> 64, state & M64
    x, r = hi ^ lo, hi >> 58
    return ((x >> r) | (x << ((64 - r) & 63))) & M64 if r else x


def step(state, inc):
    return (state * PCG_MULT + inc) & M128


def step_back(state, inc):
    return ((state - inc) * PCG_MULT_INV) & M128


def state_with_output(hi, out):
    return (hi << 64) | (rol64(out, hi >> 58) ^ hi)


def craft(p, o1, o2, has, buf, rng):
    """Six words of a stream whose 64-bit outputs number p and p + 1 (0 = the first one drawn from these words) are o1 and o2;
    o2 None: left to chance.  has / buf: has_uint32 and the buffered half, consumed before output 0 by a 32-bit draw.  rng: the
    numpy Generator every free choice comes from.  Plain Python integers throughout."""
    assert p >= 0 and 0 <= o1 <= M64 and (o2 is None or 0 <= o2 <= M64)
    while True:
        s1 = state_with_output(int(rng.integers(0, 1 << 64, dtype=np.uint64)), o1)
        hi2 = int(rng.integers(0, 1 << 64, dtype=np.uint64))
        s2 = state_with_output(hi2, o2) if o2 is not None else (hi2 << 64) | int(rng.integers(0, 1 << 64, dtype=np.uint64))
        inc = (s2 - s1 * PCG_MULT) & M128
        if inc & 1:
            break
    s = s1
    for _ in range(p + 1):
        s = step_back(s, inc)
    return [s >> 64, s & M64, inc >> 64, inc & M64, 1 if has else 0, int(buf) & 0xFFFFFFFF]


def numpy_generator(words):
    """np.random.Generator(PCG64) standing at the six words (bit_generator.state assigned)"""
    bg = np.random.PCG64(0)
    bg.state = {"bit_generator": "PCG64", "state": {"state": (int(words[0]) << 64) | int(words[1]), "inc": (int(words[2]) << 64) | int(words[3])},
                "has_uint32": int(words[4]), "uinteger": int(words[5])}
    return np.random.Generator(bg)


def outputs_between(start_words, end_words, limit=1 << 16):
    """How many 64-bit outputs lie between two rng_words() of one stream: the start state stepped until it equals the end state."""
    s, inc = (int(start_words[0]) << 64) | int(start_words[1]), (int(start_words[2]) << 64) | int(start_words[3])
    end = (int(end_words[0]) << 64) | int(end_words[1])
    assert inc == (int(end_words[2]) << 64) | int(end_words[3]), "two streams"
    for k in range(limit):
        if s == end:
            return k
        s = step(s, inc)
    raise AssertionError("the end state is not within %d outputs of the start state" % limit)


def threshold(span):
    """Lemire's rejection threshold of a bounded 32-bit draw: a word w is rejected iff (w * span) mod 2^32 < threshold(span)"""
    return ((1 << 32) - span) % span


def smallest_accepted_word(span):
    w = 0
    while ((w * span) & 0xFFFFFFFF) < threshold(span):
        w += 1
    return w


# ---- the injection plan ----------------------------------------------------------------------------------------------------------------
# Instance i receives a stream crafted at output position p = i // 8, with has_uint32 = i & 1 and pattern (i >> 1) & 3:
#   Z   o_p = 0                                   both halves rejected wherever they feed a span that can reject
#   ZM  o_p = 0, o_(p+1) = 0xFFFFFFFF00000000     up to three rejections in a row across two outputs, then the maximal value
#   M   o_p = 2^64 - 1                            the maximal k of every span; uniform() at 1 - 2^-53
#   L   both halves of o_p = the smallest word a span-360 draw accepts: k = 0
# Everything not chosen comes from a fixed numpy generator.
PATTERNS = ("Z", "ZM", "M", "L")
L_WORD = smallest_accepted_word(360)


def plan(i):
    """-> (p, has, pattern name) of injected instance i"""
    return i // 8, i & 1, PATTERNS[(i >> 1) & 3]


def pattern_outputs(name):
    return {"Z": (0, None), "ZM": (0, 0xFFFFFFFF00000000), "M": (M64, None), "L": ((L_WORD << 32) | L_WORD, None)}[name]


def plan_words(n_injected, seed=20240607):
    """The six words of every injected instance, in order (deterministic: both sides of a test and both test files get the same)."""
    g = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i in range(n_injected):
        p, has, name = plan(i)
        o1, o2 = pattern_outputs(name)
        out.append(craft(p, o1, o2, has, int(g.integers(0, 1 << 32)), g))
    return out


ALL_IDS = ["MortarMayhem-Grid-v0", "MortarMayhem-v0", "Endless-MortarMayhem-v0", "MortarMayhemB-Grid-v0", "MortarMayhemB-v0",
           "MysteryPath-v0", "MysteryPath-Grid-v0", "Endless-MysteryPath-v0", "SearingSpotlights-v0", "Endless-SearingSpotlights-v0"]
MYSTERY = ("MysteryPath-v0", "MysteryPath-Grid-v0", "Endless-MysteryPath-v0")
SPOT = ("SearingSpotlights-v0", "Endless-SearingSpotlights-v0")
P_MYSTERY = 80  # a finite path takes 19 .. 49 outputs, an endless reset's three segments 71 .. 122: 80 positions reach into the third
P_MARGIN = 8

# case a (explicit reset): options under which every `choice` has a span that can reject (3 entries: threshold 2^32 mod 3 = 1), the
# spotlight radius range is no power of two (7 .. 13: span 7) and both forms of the coin sampler run (num_coins 1 and 3 or more).
# The command lists are long (18 - 20 commands; MortarMayhemB's limit is 20): a mortar reset with the default ten draws a dozen outputs,
# and a sweep that short leaves fewer than 32 instances with a rejection.
_MM_LISTS = {"command_count": [18, 19, 20], "explosion_duration": [1, 2, 3], "explosion_delay": [2, 3, 4]}
_MM_SHOW = {"command_show_duration": [1, 2, 3], "command_show_delay": [0, 1, 2]}
RESET_OPTIONS = {
    "MortarMayhem-Grid-v0": dict(_MM_LISTS, **_MM_SHOW),
    "MortarMayhem-v0": dict(_MM_LISTS, **_MM_SHOW),
    "Endless-MortarMayhem-v0": dict({k: v for k, v in _MM_LISTS.items() if k != "command_count"}, initial_command_count=20, **_MM_SHOW),
    "MortarMayhemB-Grid-v0": dict(_MM_LISTS),
    "MortarMayhemB-v0": dict(_MM_LISTS),
    "MysteryPath-v0": {"cardinal_origin_choice": [0, 2, 3]},
    "MysteryPath-Grid-v0": {"cardinal_origin_choice": [1, 2, 3]},
    "Endless-MysteryPath-v0": {},
    "SearingSpotlights-v0": {"spot_min_radius": 7.0, "spot_max_radius": 13.0, "num_coins": [1, 3, 5]},
    "Endless-SearingSpotlights-v0": {"spot_min_radius": 7.0, "spot_max_radius": 13.0},
}

# The spans whose VALUE is fixed by the options, per family; every other span an instance draws depends on the state -- the number of
# outer-wall candidates of a path (mg_mystery_path.hpp: integers(0, n_outer)), the free cells of the position sampler
# (mg_spot_sampler.hpp: integers(0, free_total)) -- and belongs to ONE draw in the code however many values it takes: a class.
# (3: the finite Mystery Path ids' cardinal choice and SearingSpotlights-v0's num_coins list under RESET_OPTIONS)
FIXED_SPANS = {"mystery": {2, 3, 7, 8, 100}, "Endless-MysteryPath-v0": {2, 7, 8, 100}, "spot": {2, 3, 7, 8, 90, 270, 360, 7056}}


def span_class(env_id, span):
    """the span itself, or the name of the state-dependent draw it belongs to.  (A state-dependent span that happens to equal a fixed one
    -- 7 or 8 outer-wall candidates -- is counted with the fixed span: the books know spans, not call sites.)"""
    if env_id in MYSTERY:
        return span if span in FIXED_SPANS.get(env_id, FIXED_SPANS["mystery"]) else "outer-wall candidates"
    if env_id in SPOT:
        return span if span in FIXED_SPANS["spot"] else "free cells"
    return span


# case b (reset inside a step): short episodes, as the options of tests/test_gpu_u8_chw.py SHORT (one step of showing and no delay per
# command, explosions after two steps for one step; max_steps 14 / 7 / 9 with one point of health), for all ten ids.  The mortar ids take
# three-entry lists and 10 - 12 commands (the endless id: twenty initial commands) where SHORT has single entries and one or two commands:
# a reset that draws four outputs leaves a handful of instances with a rejection, not 32.
_MM_SHORT = {"command_count": [10, 11, 12], "command_show_duration": [1, 1, 1], "command_show_delay": [0, 0, 0], "explosion_delay": [2, 2, 2],
             "explosion_duration": [1, 1, 1]}
_MMB_SHORT = {k: _MM_SHORT[k] for k in ("command_count", "explosion_delay", "explosion_duration")}
SHORT_OPTIONS = {
    "MortarMayhem-Grid-v0": _MM_SHORT, "MortarMayhem-v0": _MM_SHORT, "MortarMayhemB-Grid-v0": _MMB_SHORT, "MortarMayhemB-v0": _MMB_SHORT,
    "Endless-MortarMayhem-v0": dict({k: v for k, v in _MM_SHORT.items() if k != "command_count"}, max_steps=14, initial_command_count=20),
    "MysteryPath-v0": {"max_steps": 7}, "MysteryPath-Grid-v0": {"max_steps": 7}, "Endless-MysteryPath-v0": {"max_steps": 8},
    "SearingSpotlights-v0": {"max_steps": 9, "agent_health": 1}, "Endless-SearingSpotlights-v0": {"max_steps": 9, "agent_health": 1},
}


def short_options(env_id):
    return dict(SHORT_OPTIONS[env_id])


# case c (draws during an episode): (env id, injected instances or None = the id's sweep, handle size or None = handle_size(),
# steps played before the injection, options).  The spotlight ids spawn every six steps, so that 48 steps hold several new_spot calls
# per instance; Endless-MysteryPath is injected at step 72, when the experts reach the last-but-one of the three initial segments and
# the appends begin (before that no instance draws at all).
EPISODE_STEPS, EPISODE_EPS, EPISODE_POLICY_SEED = 48, 0.1, 4711
# (spotlights that cross within 20 - 50 steps: with the default speeds a spawn every six steps would keep 25 alive, the build holds 16)
_FAST_SPOTS = {"spot_min_speed": 0.02, "spot_max_speed": 0.05}
EPISODE_CASES = [
    ("Endless-SearingSpotlights-v0", None, None, 12, dict(_FAST_SPOTS, spawn_interval=6, steps_per_coin=40)),
    ("SearingSpotlights-v0", None, None, 12, dict(_FAST_SPOTS, initial_spawn_interval=6, num_coins=[3])),
    ("Endless-MortarMayhem-v0", None, None, 12, {"command_show_duration": [1], "command_show_delay": [0], "explosion_delay": [3], "explosion_duration": [1]}),
    ("Endless-MysteryPath-v0", 320, None, 72, {}),     # the co-operative generator through the queue
    ("Endless-MysteryPath-v0", 640, 20481, 72, {}),   # the smallest size with the lane generator and records ahead of time (mg_mystery.hip: bg_coop, EMP_PRE)
]

_POSITIONS = {}


def positions(env_id):
    """P of the sweep p = 0 .. P - 1: the Mystery Path ids P_MYSTERY; the others as many 64-bit outputs as the oracle's reset consumes
    under RESET_OPTIONS (the largest over 64 instances, counted by stepping the start state until it equals the end state) plus
    P_MARGIN, at most 80."""
    if env_id in MYSTERY:
        return P_MYSTERY
    if env_id not in _POSITIONS:
        import oracle_lib

        ref = oracle_lib.OracleBatch(env_id, 64, options=RESET_OPTIONS[env_id])
        ref.reset(np.arange(64, dtype=np.int64) + 500)
        before = [e.rng_words() for e in ref.envs]
        for e in ref.envs:
            e.rng_stats(clear=True)
        ref.reset(None)
        used = [outputs_between(b, e.rng_words()) for b, e in zip(before, ref.envs)]
        assert used == [e.rng_stats()["outputs"] for e in ref.envs]  # (the oracle's own count of outputs says the same)
        ref.close()
        _POSITIONS[env_id] = min(80, max(used) + P_MARGIN)
    return _POSITIONS[env_id]


def injected(env_id):
    return 8 * positions(env_id)


def handle_size(n_injected):
    """instances of a case's handles: the injected ones rounded up to a multiple of 64, plus 3 (the last claim slot and wave are partial)"""
    return (n_injected + 63) // 64 * 64 + 3


def inject(ref, env, n_injected):
    """The plan's streams into the first n_injected instances of the oracle batch and -- env not None -- of the HIP handle; the oracle's
    bookkeeping of ALL instances starts over."""
    for i, w in enumerate(plan_words(n_injected)):
        ref.envs[i].set_rng_words(w)
        if env is not None:
            env.set_rng_words(i, w)
    for e in ref.envs[:n_injected]:
        e.rng_stats(clear=True)


class Coverage:
    """What the oracle's bookkeeping says a case exercised, gathered after the case has run (rng_stats of the injected instances)."""

    def __init__(self, env_id, ref, n_injected):
        self.env_id = env_id
        self.stats = [ref.envs[i].rng_stats() for i in range(n_injected)]
        assert not any(s["spans_lost"] for s in self.stats), "the oracle's table of spans overflowed: the books are incomplete"
        self.rejecting = [i for i, s in enumerate(self.stats) if s["rejected"] > 0]
        self.spans = {}  # span or class -> (draws, words rejected, can reject)
        for s in self.stats:
            for span, (draws, rej) in s["spans"].items():
                k = span_class(env_id, span)
                d, r, c = self.spans.get(k, (0, 0, False))
                self.spans[k] = (d + draws, r + rej, c or threshold(span) > 0)

    def summary(self):
        spans = ", ".join("%s: %d / %d" % (k, d, r) for k, (d, r, _) in sorted(self.spans.items(), key=lambda kv: str(kv[0]).rjust(8)))
        return "%d of %d injected instances rejected, %d words; span: draws / words rejected {%s}" % (
            len(self.rejecting), len(self.stats), sum(s["rejected"] for s in self.stats), spans)

    def assert_instances(self, label, at_least=32):
        assert len(self.rejecting) >= at_least, "%s: only %d injected instances took a rejection; %s" % (label, len(self.rejecting), self.summary())

    def assert_every_rejectable_span_rejected(self, label):
        """case a: every span with a non-zero threshold that any injected instance drew also rejected in some instance -- the state-
        dependent spans as one class each (span_class): their values are drawn once or twice each, and they are one draw in the code."""
        missed = [k for k, (d, r, can) in self.spans.items() if can and r == 0]
        assert not missed, "%s: spans %s can reject and never did; %s" % (label, missed, self.summary())

    def rejected_outputs(self, i):
        """indices (counted from the injection) of the 64-bit outputs instance i rejected a word of"""
        return {o for o, _ in self.stats[i]["rej_at"] if o >= 0}


def handover_outputs(env_id, has):
    """Mystery Path ids: 64-bit outputs an injected instance's reset draws before the path generator takes the stream over (the wave
    generator's batch of 64 starts there, mg_mystery_path.hpp WaveRng::take).  The finite ids draw the cardinal choice and two rows /
    columns first -- three words: a buffered half and one output, or two outputs of which the second's high half stays buffered; the
    endless id hands over at once."""
    return 0 if env_id == "Endless-MysteryPath-v0" else (1 if has else 2)


PATH_WORDS_MAX = 2 + 16 + 1 + 8 + 84  # rows, inner walls, the choice of 4 or 8, outer walls, A* noise: see check_mystery_rejections


def check_mystery_rejections(label, env_id, cov):
    """Mystery Path ids, explicit reset.  The plan was to show an instance that rejected a word of output 63 or 64 counted from the
    hand-over, on either side of the wave generator's refill (mg_mystery_path.hpp WaveRng: a batch is 64 outputs, 128 words).  No stream
    can deliver that.  WaveRng::take runs once per path, and a path draws at most PATH_WORDS_MAX = 111 words plus what Lemire's loop
    rejects: two rows, 16 inner walls (span 100), the choice of 4 or 8, up to 8 outer walls, and the A* noise integers(1, 9) -- drawn
    when a node is expanded, for each neighbour that is not closed yet; the expanded node is closed afterwards, so every EDGE of the
    7 x 7 grid draws at most once: 2 * 7 * 6 = 84 words.  Rejections are possible only among the first 27 words (the noise has span 8,
    threshold 0), and a crafted stream holds at most three rejected words there (pattern ZM).  111 + 3 < 128: the refill beyond the
    first batch is never reached, and a word of output 63 behind the hand-over is never fed to a span that can reject.
    Asserted from the oracle's books, so that the argument stays true of the code: no injected instance rejected a word more than
    14 outputs (27 words and three rejected ones) behind its hand-over, and no path consumed more than (111 + 3 + 1) // 2 = 57 outputs
    -- the finite ids behind their hand-over; the endless id, which hands over anew for each of a reset's three segments, in all three
    together no more than 3 * 57."""
    per_path = (PATH_WORDS_MAX + 3 + 1) // 2
    assert per_path < 64
    if env_id == "Endless-MysteryPath-v0":
        most = max(st["outputs"] for st in cov.stats)
        assert most <= 3 * per_path, "%s: a reset consumed %d outputs" % (label, most)
        return None, most
    last, most = -1, 0
    for i, st in enumerate(cov.stats):
        h = handover_outputs(env_id, plan(i)[1])
        last = max([last] + [o - h for o in cov.rejected_outputs(i)])
        most = max(most, st["outputs"] - h)
    assert 0 <= last <= 14, "%s: a rejection %d outputs behind the hand-over" % (label, last)
    assert most <= per_path, "%s: a path consumed %d outputs behind the hand-over" % (label, most)
    return last, most


SPOTLIGHT_SPANS = (7, 360, 90, 270)  # radius (7 .. 13 under RESET_OPTIONS), start angle, target and offset: drawn by Spotlight.__init__ alone


def check_spot_wirings(label, cov):
    """spotlight ids, explicit reset: among the instances whose rejection fell inside the spotlights' outputs (five per spotlight,
    drawn 16 at once on the device with two wirings of halves to draws; a rejection sends the group back to the one-after-another form,
    mg_spot_logic.hpp new_spots_at_reset), both has_uint32 values occur.  An instance counts when its books show a rejected word under
    one of the spans only a spotlight draws (the agent, coins and exit, drawn before and after the spotlights, use 7056, the free-cell
    counts, 2, 3 and 8)."""
    seen = {0: 0, 1: 0}
    for i, st in enumerate(cov.stats):
        if any(st["spans"].get(sp, (0, 0))[1] for sp in SPOTLIGHT_SPANS):
            seen[plan(i)[1]] += 1
    assert seen[0] and seen[1], "%s: instances with a rejection inside the spotlights' draws, by has_uint32: %s" % (label, seen)
    return seen


def random_actions(prng, n, discrete):
    return (prng.integers(0, 4, n) if discrete else prng.integers(0, 3, (n, 2))).astype(np.int32)


# ---- the arrangement axis ---------------------------------------------------------------------------------------------------------------
# The cases above reach every draw through the launches a default handle takes.  The same draws sit in other kernels too -- the headless
# step, the masked step and the masked resets, the per-set <PS> instantiations, mg_advance, the finite ids' lane generator -- and
# ARRANGEMENT_CASES sends the crafted streams through each of them (tests/test_gpu_rng_edges_arrangements.py; the oracle alone:
# tests/test_rng_craft.py).  One driver, run_arrangement(), plays a case on whatever `make` returns: OracleSide below (no GPU), or the GPU
# test's pair of a handle and an OracleSide, whose methods make the device call, let the OracleSide do the oracle's and compare.  Both
# therefore see the same injection, actions and masks.

# The second option set of the two-set case: list lengths 5 and 6 (thresholds 2^32 mod 5 = 1, mod 6 = 4) where the first set has 3
# (threshold 1), a radius range of span 5 (7 .. 11) where the first has 7 (7 .. 13: threshold 4).  No geometry key differs, so a handle
# accepts both sets side by side.  Endless-MysteryPath-v0 has no option that sets a span: its sets differ in max_steps and a reward.
_MM_SECOND = {"command_count": [8, 9, 10, 11, 12], "command_show_duration": [1] * 5, "command_show_delay": [0] * 5, "explosion_delay": [2] * 6,
              "explosion_duration": [1] * 6}
TWO_SETS = {
    "MortarMayhem-v0": (_MM_SHORT, _MM_SECOND),
    "MysteryPath-v0": (dict(SHORT_OPTIONS["MysteryPath-v0"], **RESET_OPTIONS["MysteryPath-v0"]), {"max_steps": 7, "cardinal_origin_choice": [0, 1, 2, 3, 1]}),
    "Endless-MysteryPath-v0": ({"max_steps": 8}, {"max_steps": 9, "reward_fall_off": -0.2}),
    "SearingSpotlights-v0": (dict(SHORT_OPTIONS["SearingSpotlights-v0"], **RESET_OPTIONS["SearingSpotlights-v0"]),
                             dict(SHORT_OPTIONS["SearingSpotlights-v0"], spot_min_radius=7.0, spot_max_radius=11.0, num_coins=[1, 2, 3, 4, 5])),
    "Endless-SearingSpotlights-v0": (dict(SHORT_OPTIONS["Endless-SearingSpotlights-v0"], **RESET_OPTIONS["Endless-SearingSpotlights-v0"]),
                                     dict(SHORT_OPTIONS["Endless-SearingSpotlights-v0"], spot_min_radius=7.0, spot_max_radius=11.0)),
}
# spans only ONE of the two sets draws (the condition "each set rejected under a span the other does not draw"); None: no such span exists.
# (MortarMayhem-v0 draws a span of 6 under either set -- the second set's lists of six share it --, so 5 alone is its own.  MysteryPath-v0:
# the number of outer-wall candidates takes the values 3 and 5 too, in either set, and the books know spans, not call sites; there the
# choice is the reset's FIRST draw, and check_arrangement asks for a rejected word of output 0 in plan instance 0 (p 0, no buffered
# half, pattern Z: a word of 0, which 3 and 5 both reject) instead of for a span the other set never drew.)
TWO_SETS_OWN_SPANS = {"MortarMayhem-v0": ({3}, {5}), "MysteryPath-v0": ({3}, {5}), "Endless-MysteryPath-v0": None,
                      "SearingSpotlights-v0": ({7, 3}, {5}), "Endless-SearingSpotlights-v0": ({7}, {5})}

MORTAR = tuple(e for e in ALL_IDS if "Mortar" in e)
ADVANCE_EPS, ADVANCE_SEED = 0.3, 4711
LANE_N, LANE_INJECTED, LANE_WARMUP, LANE_EXPERT_STEPS = 1091, 8 * 60, 6, 4  # 17 waves + 3, more than PATH_MASS = 1,024 (mg_mystery_finite.hpp)
EPISODE_WARMUP = {c[0]: c[3] for c in EPISODE_CASES}


def _cases():
    """(env id, arrangement, injected instances or None = the id's sweep, handle size or None = handle_size(), options, step cap).
    The caps are MEASURED: the calls the oracle alone needs under the case's inputs (tests/test_rng_craft.py asserts that it stays within
    them, the GPU test that the handle needs exactly as many); where the arrangement fixes the number of calls, that number."""
    caps = {
        "headless": [24, 19, 14, 15, 9, 7, 7, 8, 9, 9], "masked": [50, 54, 50, 28, 22, 27, 27, 29, 35, 32],
        "masked-reset": [24, 19, 14, 15, 9, 7, 7, 8, 9, 9], "masked-blocks": [15, 15, 16, 25, 25],
    }
    rows = []
    for k, e in enumerate(ALL_IDS):
        rows.append((e, "headless", None, None, short_options(e), caps["headless"][k]))
    for e, n_inj, _, _, options in EPISODE_CASES[:3]:
        rows.append((e, "headless-episode", n_inj, None, options, EPISODE_STEPS))
    rows.append(("Endless-MysteryPath-v0", "headless-episode", 320, 323, {}, EPISODE_STEPS))
    for k, e in enumerate(ALL_IDS):
        rows.append((e, "masked", None, None, short_options(e), caps["masked"][k]))
    for k, e in enumerate(MYSTERY + SPOT):
        rows.append((e, "masked-blocks", None, None, short_options(e), caps["masked-blocks"][k]))
    for k, e in enumerate(ALL_IDS):
        rows.append((e, "masked-reset", None, None, short_options(e), caps["masked-reset"][k]))
    for e in ("MortarMayhem-Grid-v0", "SearingSpotlights-v0"):
        rows.append((e, "masked-reset-final", None, None, short_options(e), caps["masked-reset"][ALL_IDS.index(e)]))
    rows.append(("Endless-MysteryPath-v0", "masked-reset-sets", None, None, None, 9))
    for e, cap in zip(TWO_SETS, (23, 7, 9, 9, 9)):
        rows.append((e, "two-sets", None, None, None, cap))
    for e, cap in zip(MORTAR + ("MysteryPath-Grid-v0", "SearingSpotlights-v0"), (35, 24, 14, 30, 12, 7, 9)):
        rows.append((e, "advance", None, None, short_options(e), cap))
    for e in ("MysteryPath-Grid-v0", "MysteryPath-v0"):
        rows.append((e, "lane-generator", LANE_INJECTED, LANE_N, {"max_steps": 7}, 1))
    return rows


ARRANGEMENT_CASES = _cases()
MEASURE_LIMIT = 200  # run_arrangement(cap=None): how long a measuring run may last
MASK_ROWS = 200      # rows of the masked cases' mask and action tables, whatever the cap (bernoulli_inputs draws the actions behind the mask: another
                     # number of rows is another table)


def case_id(case):
    return "%s-%s" % (case[1], case[0])


def inject_at(ref, env, instances, plan_ids=None):
    """The stream of plan(plan_ids[k]) into instance instances[k] of the oracle batch and -- env not None -- of the HIP handle, at whatever
    point of a run; the oracle's books of these instances start over.  plan_ids None: 0, 1, 2, ..."""
    instances = [int(i) for i in instances]
    plan_ids = list(range(len(instances))) if plan_ids is None else [int(p) for p in plan_ids]
    words = plan_words(max(plan_ids) + 1)
    for i, p in zip(instances, plan_ids):
        ref.envs[i].set_rng_words(words[p])
        if env is not None:
            env.set_rng_words(i, words[p])
        ref.envs[i].rng_stats(clear=True)


class _Some:
    """the chosen instances of an oracle batch, where Coverage looks for `envs`"""

    def __init__(self, ref, instances):
        self.envs = [ref.envs[int(i)] for i in instances]


def coverage_of(env_id, ref, instances):
    """Coverage over the listed instances; entry k of its stats belongs to instances[k]"""
    return Coverage(env_id, _Some(ref, instances), len(instances))


class OracleSide:
    """The oracle's part of every call of an arrangement case.  Alone it is the CPU form of a case; the GPU test wraps it.  Each stepping
    method returns done (bool [n]) and leaves the call's rewards in `reward`."""

    def __init__(self, env_id, n, options=None, sets=None, ref=None):
        import oracle_lib

        self.env_id, self.n = env_id, n
        self.ref = ref if ref is not None else oracle_lib.OracleBatch(env_id, n, options=options)
        self.discrete = self.ref.discrete
        self.reward = np.zeros(n)
        self.plan_id = {}  # instance -> index into the plan
        self._masked = None
        if sets is not None:  # instance i runs under sets[i & 1]: the reference's options belong to ONE instance, the oracle's too
            for i, e in enumerate(self.ref.envs):
                e.set_options(sets[i & 1])

    def close(self):
        self.ref.close()

    def counter(self, name):
        return None  # (a handle's debug counter; the oracle has none)

    def reset(self, seeds, where=""):
        self.ref.reset_digest(seeds)

    reset_sets = reset

    def inject_at(self, instances, plan_ids=None):
        inject_at(self.ref, None, instances, plan_ids)
        self._injected(instances, plan_ids)

    def _injected(self, instances, plan_ids):
        self.plan_id = dict(zip([int(i) for i in instances], range(len(instances)) if plan_ids is None else [int(p) for p in plan_ids]))

    def step_unwatched(self, a, where=""):
        return self.ref.step(a, autoreset=True, want_obs=False)[2].astype(bool)

    def step(self, a, where="", autoreset=True):
        _, rew, done = self.ref.step(a, autoreset=autoreset, want_obs=False)
        self.reward = rew
        return done.astype(bool)

    headless = step

    def noreset_step(self, a, where=""):
        return self.step(a, where, autoreset=False)

    def masked(self, a, m, where=""):
        if self._masked is None:
            import masked_step_inputs as mi

            self._masked = mi.MaskedOracle(self.env_id, self.n, None, (), ref=self.ref)
        self.reward, done, _ = self._masked.step(a, m)
        return done

    def masked_reset(self, m, where=""):
        for i in np.nonzero(m)[0]:
            self.ref.envs[i].reset(None, want_obs=False)

    def advance(self, steps, eps, seed, step0, where=""):
        """-> episodes ended (int [n]); `reward`: the step rewards added in step order"""
        total, episodes = np.zeros(self.n), np.zeros(self.n, np.int32)
        for t in range(steps):
            _, r, d = self.ref.step(self.ref.expert_actions(eps, seed, step0 + t), autoreset=True, want_obs=False)
            total += r
            episodes += d.astype(np.int32)
        self.reward = total
        return episodes

    def redraw(self, where=""):
        pass

    def expert(self, eps, seed, t, where=""):
        return self.ref.expert_actions(eps, seed, t)

    def screens(self):
        """uint64 [n]: the digest of what lies on every instance's screen"""
        import frame_digest as fd

        return fd.digest_numpy(self.ref.frames(range(self.n)))

    def vector(self):
        return np.stack([e.get_list("vec") for e in self.ref.envs]).astype(np.float32)


def _seeds(n):
    return np.arange(n, dtype=np.int64) + 500


def run_arrangement(case, make, cap=-1):
    """Play one row of ARRANGEMENT_CASES on make(env_id, n, options, final=..., autoreset=..., sets=...) -> a side.
    -> (side, calls, [(label, instances, Coverage)]): the caller asserts the cap and the conditions, then closes the side.
    cap: the row's by default; None = a measuring run (up to MEASURE_LIMIT calls)."""
    import masked_step_inputs as mi

    env_id, arr, n_inj, size, options, row_cap = case
    cap = row_cap if cap == -1 else cap
    limit = MEASURE_LIMIT if cap is None else cap
    n_inj = n_inj or injected(env_id)
    n = size or handle_size(n_inj)
    who = np.arange(n_inj)
    label = "%s %s" % (env_id, arr)
    prng = np.random.Generator(np.random.PCG64(21))
    finished = np.zeros(2 * n if arr == "two-sets" else n, bool)
    calls = 0

    def unfinished():
        return "%s: %d injected instances have not finished after %d calls" % (label, int((~finished[who]).sum()), calls)

    if arr in ("headless", "headless-episode"):
        side = make(env_id, n, options)
        side.reset(_seeds(n), "seeded reset")
        t0 = 0
        if arr == "headless-episode":  # as case c: the warm-up drawn, under the oracle's expert
            t0 = EPISODE_WARMUP[env_id]
            for t in range(t0):
                side.step_unwatched(side.expert(EPISODE_EPS, EPISODE_POLICY_SEED, t), "step %d" % t)
        side.inject_at(who)
        c0 = side.counter("headless_steps")
        while (calls < limit) if arr == "headless-episode" else not finished[who].all():
            assert calls < limit, unfinished()
            a = side.expert(EPISODE_EPS, EPISODE_POLICY_SEED, t0 + calls) if arr == "headless-episode" else random_actions(prng, n, side.discrete)
            finished |= side.headless(a, "headless step %d" % calls)
            calls += 1
        assert c0 is None or side.counter("headless_steps") - c0 == calls, "%s: headless_steps grew by %d in %d calls" % (label, side.counter("headless_steps") - c0, calls)
        side.redraw("redraw() after the headless steps")
        side.step(random_actions(prng, n, side.discrete), "the drawn step at the end")
    elif arr in ("masked", "masked-blocks"):
        side = make(env_id, n, options)
        side.reset(_seeds(n), "seeded reset")
        side.inject_at(who)
        if arr == "masked":
            mask, act = mi.bernoulli_inputs(side.discrete, MASK_ROWS, n)
        else:
            mask, act = mi.block_masks(MASK_ROWS, n), mi.actions(np.random.default_rng(7), side.discrete, MASK_ROWS, n)
        counts = np.zeros(n, np.int64)
        c0 = side.counter("masked_steps")
        while not finished[who].all():
            assert calls < limit, unfinished()
            finished |= side.masked(mi.pick(act, counts), mask[calls], "masked step %d" % calls)
            counts += mask[calls]
            calls += 1
        assert c0 is None or side.counter("masked_steps") - c0 == calls
    elif arr in ("masked-reset", "masked-reset-final", "masked-reset-sets"):
        if arr.endswith("sets"):  # (Endless-MysteryPath-v0: with option sets a masked reset goes through the queue server)
            n, who = 2 * n, np.arange(2 * n_inj)
            finished = np.zeros(n, bool)
            side = make(env_id, n, None, autoreset=False, sets=TWO_SETS[env_id])
            side.reset_sets(_seeds(n), "seeded resets under the two sets")
            side.inject_at(who, who >> 1)
        else:
            side = make(env_id, n, options, final=arr.endswith("final"), autoreset=False)
            side.reset(_seeds(n), "seeded reset")
            side.inject_at(who)
        while not finished[who].all():  # (finished: has been reset by a masked reset)
            assert calls < limit, unfinished()
            d = side.noreset_step(random_actions(prng, n, side.discrete), "step %d without auto-reset" % calls)
            if d.any():
                side.masked_reset(d, "reset(seed=None, mask=done) after step %d" % calls)
            finished |= d
            calls += 1
    elif arr == "two-sets":
        n, who = 2 * n, np.arange(2 * n_inj)
        side = make(env_id, n, None, sets=TWO_SETS[env_id])
        side.reset_sets(_seeds(n), "seeded resets under the two sets")
        side.inject_at(who, who >> 1)  # (each set's instances take the whole sweep: instance i runs under set i & 1)
        while not finished[who].all():
            assert calls < limit, unfinished()
            finished |= side.step(random_actions(prng, n, side.discrete), "step %d" % calls)
            calls += 1
        cov = [("%s, set %d" % (label, s), who[s::2], coverage_of(env_id, side.ref, who[s::2])) for s in (0, 1)]
        return side, calls, cov
    elif arr == "advance":
        side = make(env_id, n, options)
        side.reset(_seeds(n), "seeded reset")
        side.inject_at(who)
        c0 = side.counter("advance_fused_steps")
        first = limit // 2
        for steps, step0 in ((first, 0), (limit - first, first)):
            finished |= side.advance(steps, ADVANCE_EPS, ADVANCE_SEED, step0, "advance(%d) from step %d" % (steps, step0)) > 0
        calls = limit
        assert c0 is None or side.counter("advance_fused_steps") - c0 == (calls if env_id in MORTAR else 0)
        assert finished[who].all(), unfinished()
    elif arr == "lane-generator":
        side = make(env_id, n, options)
        side.reset(_seeds(n), "seeded reset")
        for t in range(LANE_WARMUP):
            d = side.step_unwatched(random_actions(prng, n, side.discrete), "step %d" % t)
            assert not d.any(), "%s: an instance finished before the truncation" % label
        side.inject_at(who)
        c0 = side.counter("path_lane_paths")
        finished |= side.step(random_actions(prng, n, side.discrete), "the step that truncates everybody")
        calls = 1
        assert finished.all(), "%s: %d of %d instances were truncated" % (label, int(finished.sum()), n)
        if c0 is not None:  # more than PATH_MASS paths in the queue, the injected instances' among them: the lane generator made (nearly) all
            grew = side.counter("path_lane_paths") - c0
            assert grew > 1024 and grew >= n_inj, "%s: the lane generator made %d of %d paths" % (label, grew, n)
        for t in range(LANE_EXPERT_STEPS):  # the expert is the only reader of path_order
            side.step(side.expert(0.0, ADVANCE_SEED, t, "expert_actions %d steps behind the truncation" % t), "step %d behind the truncation" % t)
    else:
        raise ValueError(arr)
    return side, calls, [(label, who, coverage_of(env_id, side.ref, who))]


def check_arrangement(case, side, calls, covs, exact):
    """The conditions of a case, from the oracle's books: the cap (exact: as many calls as the row says, otherwise no more), 32 injected
    instances with a rejection per Coverage, and what the arrangement adds."""
    env_id, arr, cap = case[0], case[1], case[5]
    assert calls == cap if exact else calls <= cap, "%s %s: %d calls, the row says %d" % (env_id, arr, calls, cap)
    for label, _, cov in covs:
        print("\n%s (%d calls): %s" % (label, calls, cov.summary()))
        cov.assert_instances(label)
    if arr == "two-sets" and TWO_SETS_OWN_SPANS[env_id] is not None:
        for s, own in enumerate(TWO_SETS_OWN_SPANS[env_id]):
            label, cov, other = covs[s][0], covs[s][2], covs[1 - s][2]
            rejected = {sp for st in cov.stats for sp, (_, r) in st["spans"].items() if r}
            drawn_by_other = {sp for st in other.stats for sp in st["spans"]}
            assert rejected & own, "%s: rejected under %s, none of its own spans %s" % (label, sorted(rejected), sorted(own))
            if env_id in MYSTERY:
                assert 0 in cov.rejected_outputs(0), "%s: plan instance 0 rejected no word of the reset's first output (the cardinal choice)" % label
            else:
                assert not (own & drawn_by_other), "%s: the other set drew %s too" % (label, sorted(own & drawn_by_other))
    if arr == "lane-generator":  # both has_uint32 values with a rejection behind the hand-over to the path generator
        (label, who, cov), = covs
        seen = {0: 0, 1: 0}
        for k in range(len(who)):
            has = plan(k)[1]
            seen[has] += any(o >= handover_outputs(env_id, has) for o in cov.rejected_outputs(k))
        assert seen[0] and seen[1], "%s: instances with a rejection behind the hand-over, by has_uint32: %s" % (label, seen)
        print("   rejections behind the hand-over, by has_uint32: %s" % seen)
