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
read from the oracle's bookkeeping (oracle/mgo_rng.h mgo_rng_book)."""
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
