/* oracle/mgo_rng.h -- TEST INFRASTRUCTURE (CPU oracle), not product code.
 *
 * Restatement of the numpy random stream the reference consumes through
 * gymnasium.Env.reset(seed) -> np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed))).
 * The algorithm lives in third-party numpy (unpinned by the reference; validated here against
 * numpy 2.2.6, see tests/test_oracle_rng.py) -- call sites in the reference:
 *   memory_gym/mortar_mayhem_grid.py:181,186,244,253,254,268,269 and the list in SURVEY.md 8(a).
 * Published algorithms restated: SeedSequence (M.E. O'Neill seed_seq_fe128 variant used by numpy),
 * PCG64 XSL-RR 128/64, Lemire's nearly-divisionless bounded integers (numpy _bounded_integers),
 * next_double = (u64 >> 11) * 2^-53, 32-bit draws buffered LOW half first.
 *
 * Bookkeeping (mgo_rng_stats): which spans were drawn, how many 32-bit words Lemire's loop rejected and from which 64-bit
 * outputs they came.  It is written beside the draws and read by nothing that draws: a test that claims to have exercised a
 * rejection asks here whether it did (tests/test_rng_craft.py, tests/test_gpu_rng_edges.py).
 */
#ifndef MGO_RNG_H
#define MGO_RNG_H
#include <stdint.h>

typedef unsigned __int128 mgo_u128;

#define MGO_RNG_SPANS 32   /* distinct spans remembered per stream (the environments draw fewer than that per option set) */
#define MGO_RNG_REJ_AT 8   /* rejected words whose origin is remembered */

typedef struct {
    int on;                               /* books are kept from the first mgo_rng_set_words / mgo_rng_stats of the stream on: every other run of the oracle pays one test per draw */
    uint64_t rejected;                    /* 32-bit words Lemire's loop threw away */
    uint64_t outputs;                     /* 64-bit outputs generated since the stream was seeded / set */
    int n_spans, spans_lost;              /* spans_lost: distinct spans that found the table full */
    uint32_t span[MGO_RNG_SPANS];         /* distinct spans drawn (hi - lo; span 1 draws nothing and is not listed) */
    uint32_t span_draws[MGO_RNG_SPANS];   /* integers() calls with that span */
    uint32_t span_rejected[MGO_RNG_SPANS];/* words rejected under that span */
    uint32_t n_rej_at;                    /* min(rejected, MGO_RNG_REJ_AT) */
    uint32_t rej_at[MGO_RNG_REJ_AT];      /* the first rejected words: 2 * (index of the 64-bit output, counted from 0 at the seeding) + (1 = its high half) */
} mgo_rng_book;

typedef struct {
    mgo_u128 state, inc;
    int has_u32;
    uint32_t buf;
    mgo_rng_book book;
} mgo_rng;

static inline int mgo_rng_book_span(mgo_rng* r, uint32_t span) {
    mgo_rng_book* b = &r->book;
    for (int k = 0; k < b->n_spans; k++)
        if (b->span[k] == span) return k;
    if (b->n_spans == MGO_RNG_SPANS) {
        b->spans_lost++;
        return -1;
    }
    b->span[b->n_spans] = span;
    b->span_draws[b->n_spans] = 0;
    b->span_rejected[b->n_spans] = 0;
    return b->n_spans++;
}
static inline void mgo_rng_book_reject(mgo_rng* r, int k) {
    mgo_rng_book* b = &r->book;
    b->rejected++;
    if (k >= 0) b->span_rejected[k]++;
    /* the word just drawn: the buffered high half if nothing is buffered now, else the low half of the newest output */
    if (b->n_rej_at < MGO_RNG_REJ_AT)  /* (0xFFFFFFFF: the half that was buffered already when the stream was set) */
        b->rej_at[b->n_rej_at++] = b->outputs ? (uint32_t)(2 * (b->outputs - 1) + (r->has_u32 ? 0 : 1)) : 0xFFFFFFFFu;
}

static inline void mgo_seedseq_state(uint64_t seed, uint64_t out64[4]) {
    const uint32_t INIT_A = 0x43b0d7e5u, MULT_A = 0x931e8875u, INIT_B = 0x8b51f9ddu, MULT_B = 0x58f38dedu;
    const uint32_t MIX_L = 0xca01f9ddu, MIX_R = 0x4973f715u;
    uint32_t ent[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    int n_ent = ent[1] ? 2 : 1;
    uint32_t pool[4], hc = INIT_A;
#define MGO_HASHMIX(v_in, res) do { uint32_t v_ = (v_in); v_ ^= hc; hc *= MULT_A; v_ *= hc; v_ ^= v_ >> 16; (res) = v_; } while (0)
#define MGO_MIX(x, y, res) do { uint32_t r_ = MIX_L * (x) - MIX_R * (y); r_ ^= r_ >> 16; (res) = r_; } while (0)
    for (int i = 0; i < 4; i++) {
        uint32_t e = i < n_ent ? ent[i] : 0u;
        MGO_HASHMIX(e, pool[i]);
    }
    for (int s = 0; s < 4; s++)
        for (int d = 0; d < 4; d++)
            if (s != d) {
                uint32_t h;
                MGO_HASHMIX(pool[s], h);
                MGO_MIX(pool[d], h, pool[d]);
            }
    /* entropy longer than the pool (never the case for 64-bit seeds: n_ent <= 2) would be mixed here */
    uint32_t w32[8];
    hc = INIT_B;
    for (int i = 0; i < 8; i++) {
        uint32_t d = pool[i % 4] ^ hc;
        hc *= MULT_B;
        d *= hc;
        d ^= d >> 16;
        w32[i] = d;
    }
    for (int k = 0; k < 4; k++) out64[k] = (uint64_t)w32[2 * k] | ((uint64_t)w32[2 * k + 1] << 32);
#undef MGO_HASHMIX
#undef MGO_MIX
}

#define MGO_PCG_MULT ((((mgo_u128)0x2360ED051FC65DA4ull) << 64) | (mgo_u128)0x4385DF649FCCF645ull)

static inline void mgo_rng_seed(mgo_rng* r, uint64_t seed) {
    uint64_t w[4];
    mgo_seedseq_state(seed, w);
    mgo_u128 initstate = ((mgo_u128)w[0] << 64) | w[1];
    mgo_u128 initseq = ((mgo_u128)w[2] << 64) | w[3];
    r->inc = (initseq << 1) | 1u;
    r->state = 0;
    r->state = r->state * MGO_PCG_MULT + r->inc;
    r->state += initstate;
    r->state = r->state * MGO_PCG_MULT + r->inc;
    r->has_u32 = 0;
    r->buf = 0;
    r->book.outputs = 0;  /* (the other counters run on: a test clears them through mgo_rng_stats) */
}

static inline uint64_t mgo_next_u64(mgo_rng* r) {
    r->book.outputs++;
    r->state = r->state * MGO_PCG_MULT + r->inc;
    uint64_t hi = (uint64_t)(r->state >> 64), lo = (uint64_t)r->state;
    uint64_t x = hi ^ lo;
    unsigned rot = (unsigned)(hi >> 58);
    return (x >> rot) | (x << ((64 - rot) & 63));
}

static inline uint32_t mgo_next_u32(mgo_rng* r) {
    if (r->has_u32) {
        r->has_u32 = 0;
        return r->buf;
    }
    uint64_t v = mgo_next_u64(r);
    r->has_u32 = 1;
    r->buf = (uint32_t)(v >> 32);
    return (uint32_t)v;
}

static inline double mgo_next_double(mgo_rng* r) { return (double)(mgo_next_u64(r) >> 11) * (1.0 / 9007199254740992.0); }

/* Generator.integers(lo, hi) with int64 dtype, endpoint=False; lo/hi already truncated toward zero.
 * Only ranges < 2^32 occur on the hot path. */
static inline int64_t mgo_integers(mgo_rng* r, int64_t lo, int64_t hi) {
    uint64_t rng = (uint64_t)(hi - 1 - lo);
    if (rng == 0) return lo;
    uint32_t rng_excl = (uint32_t)rng + 1u;
    const int book = r->book.on ? mgo_rng_book_span(r, rng_excl) : -1;
    if (book >= 0) r->book.span_draws[book]++;
    uint64_t m = (uint64_t)mgo_next_u32(r) * rng_excl;
    uint32_t left = (uint32_t)m;
    if (left < rng_excl) {
        uint32_t thr = (0xFFFFFFFFu - (uint32_t)rng) % rng_excl;
        while (left < thr) {
            if (r->book.on) mgo_rng_book_reject(r, book);
            m = (uint64_t)mgo_next_u32(r) * rng_excl;
            left = (uint32_t)m;
        }
    }
    return lo + (int64_t)(m >> 32);
}

/* Generator.choice(list) == list[integers(0, len)] (a 1-element list consumes nothing) */
static inline int mgo_choice_index(mgo_rng* r, int n) { return (int)mgo_integers(r, 0, n); }

static inline double mgo_uniform(mgo_rng* r, double a, double b) { return a + (b - a) * mgo_next_double(r); }

#endif
