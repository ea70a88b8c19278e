// mg_mystery_path.hpp -- the reference's MysteryPath.__init__ (pygame_assets.py:606-724: 33 % inner walls, 4 or 8 outer walls, A* with integers(1, 9) noise on every
// relaxation) twice, and nothing of the environments that ask for paths.  Both generators take the same draws in the same order from the instance's stream, keep the
// reference's Python-list semantics (ties broken by list order; the `neighbor.g = g` typo: a node's g_cost never changes once it has entered the open set) and return
// the path END first.  They differ in who does the work:
//   coop_path (PathWS, WaveRng)  one path by a whole wave in 25-33 us: the lower latency.  A step's resets and due segments (serve_mp, serve_emp).
//   lane_path (LaneWS)           one path per lane, ~105 us for 64 of them: twice the throughput where many paths are due at once and nobody waits for one -- mass
//                                resets, Endless-MysteryPath's background jobs.  Compares f-costs through the integer keys that tests/test_path_keys.py checks.
#pragma once
#include "mg_mystery_types.hpp"

namespace mg {
__device__ __forceinline__ int nb_of(int idx, int k) {  // Node.add_neighbors order: x+1, x-1, y+1, y-1
    int x = idx / G, y = idx - x * G;
    if (k == 0) return x < G - 1 ? idx + G : -1;
    if (k == 1) return x > 0 ? idx - G : -1;
    if (k == 2) return y < G - 1 ? idx + 1 : -1;
    return y > 0 ? idx - 1 : -1;
}
__device__ __forceinline__ int diag_of(int idx, int k) {
    int x = idx / G, y = idx - x * G;
    if (k == 0) return (x < G - 1 && y < G - 1) ? idx + G + 1 : -1;
    if (k == 1) return (x > 0 && y > 0) ? idx - G - 1 : -1;
    if (k == 2) return (x < G - 1 && y > 0) ? idx + G - 1 : -1;
    return (x > 0 && y < G - 1) ? idx - G + 1 : -1;
}

// ---- Wave-cooperative path generation -------------------------------------------------------------------------
// The environments are stepped one LANE per instance, but generating a path (walls + noisy A*) is a long serial job:
// run by the single lane that happens to reset it took 70-300 us and was the tail of every launch in which any
// instance reset.  Instead, instances that need a path are served one at a time by their whole WAVE at a converged
// point of the kernel (serve_*): the requesting lane's inputs and RNG state are broadcast, all 64 lanes execute the
// same (uniform) control flow with node n's A* record living in lane n's registers and the ordered open list living
// one position per lane, so that the reference's list operations are O(1):
//   selection  "first index i >= 1 with f(open[i]) < f(open[0]) else 0"  = one shuffle of f + one ballot
//   removal    list.pop(i)                                                = one shuffle down
//   membership / closed / walls                                           = uniform 64-bit masks
// LDS: the heuristic table sqrt(0..79) for the block and 64 staging bytes per wave for the finished path.
constexpr int WS_SQRT = 0;                        // double sqrt_tab[80]
constexpr int WS_STAGE = 80 * 8;                  // uint8 stage[4 waves][64]
constexpr int WS_BYTES = WS_STAGE + 4 * 64;

struct PathWS {
    uint8_t* base;
    const uint4* jump;  // WaveRng's per-lane jump constants
    unsigned long long* stats;  // MysteryIO::stats or NULL
    __device__ __forceinline__ double h(int d2) const { return reinterpret_cast<const double*>(base + WS_SQRT)[d2]; }
    __device__ __forceinline__ uint8_t* stage() const { return base + WS_STAGE + (threadIdx.x >> 6) * 64; }
};

__device__ __forceinline__ void path_ws_init(uint8_t* smem) {  // all threads of the block, before any path is generated
    if (threadIdx.x < 80) reinterpret_cast<double*>(smem + WS_SQRT)[threadIdx.x] = sqrt((double)threadIdx.x);
    __syncthreads();
}

__device__ __forceinline__ int bcast(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ Pcg bcast(const Pcg& g, int lane) {
    Pcg b;
    uint32_t w[9] = {(uint32_t)g.state, (uint32_t)(g.state >> 32), (uint32_t)(g.state >> 64), (uint32_t)(g.state >> 96),
                     (uint32_t)g.inc,   (uint32_t)(g.inc >> 32),   (uint32_t)(g.inc >> 64),   (uint32_t)(g.inc >> 96), g.buf};
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = (uint32_t)__builtin_amdgcn_readlane((int)w[k], lane);
    b.state = ((u128)w[3] << 96) | ((u128)w[2] << 64) | ((u128)w[1] << 32) | w[0];
    b.inc = ((u128)w[7] << 96) | ((u128)w[6] << 64) | ((u128)w[5] << 32) | w[4];
    b.buf = w[8];
    b.has = __builtin_amdgcn_readlane(g.has ? 1 : 0, lane) != 0;
    return b;
}

// ---- the instance's RNG stream, generated 64 outputs at a time by the whole wave ------------------------------------------
// A path draws 40 - 100 32-bit numbers (at most 111 and what Lemire's loop rejects: fewer than one batch of 128); drawn one by one from wave-uniform state, every PCG64 step is a 128 x 128-bit multiply on
// the scalar unit (~45 scalar instructions per 64-bit output) inside a kernel that is bound by scalar issue -- a third of a
// path's instructions.  An LCG can be jumped: s_k = A^k s_0 + S_k inc with S_k = 1 + A + ... + A^(k-1), so lane k computes
// step k + 1 directly (two 128-bit multiplies on the vector unit, all 64 lanes at once) and a draw is one v_readlane.  The
// 32-bit draws are numpy's: low half, then the buffered high half of each 64-bit output (Pcg::next32), a half buffered
// before the hand-over first.  jump[k] = {A^(k+1), S_(k+1)} is built on the host (MysteryFamily).
struct WaveRng {
    u128 M, S;        // per lane: A^(lane + 1), S_(lane + 1)
    u128 st;          // per lane: the state after lane + 1 steps from `base`
    uint32_t lo, hi;  // per lane: that step's output
    u128 base, inc;   // uniform
    int cursor;       // uniform: 32-bit draws taken from the current batch (0 .. 128)
    bool pre_has;     // uniform: the stream was handed over with a buffered half, not consumed yet
    uint32_t pre_buf;

    __device__ __forceinline__ void load_jump(const uint4* jump) {
        const int lane = threadIdx.x & 63;
        const uint4 m = jump[2 * lane], q = jump[2 * lane + 1];
        M = ((u128)m.w << 96) | ((u128)m.z << 64) | ((u128)m.y << 32) | m.x;
        S = ((u128)q.w << 96) | ((u128)q.z << 64) | ((u128)q.y << 32) | q.x;
    }
    __device__ __forceinline__ void refill() {
        st = M * base + S * inc;
        const uint64_t h = (uint64_t)(st >> 64), l = (uint64_t)st, x = h ^ l;
        const unsigned rot = (unsigned)(h >> 58);
        const uint64_t o = (x >> rot) | (x << ((64 - rot) & 63));
        lo = (uint32_t)o;
        hi = (uint32_t)(o >> 32);
        cursor = 0;
    }
    static __device__ __forceinline__ u128 lane128(u128 v, int lane) {
        const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
        const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 64), lane);
        const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 96), lane);
        return ((u128)d << 96) | ((u128)c << 64) | ((u128)b << 32) | a;
    }
    // g: wave-uniform (a broadcast copy of the requesting lane's stream)
    __device__ __forceinline__ void take(const Pcg& g) {
        base = g.state;
        inc = g.inc;
        pre_has = g.has;
        pre_buf = g.buf;
        refill();
    }
    // the stream as it stands after the draws taken (uniform)
    __device__ __forceinline__ void give(Pcg& g) const {
        const int m = (cursor + 1) >> 1;  // 64-bit outputs consumed from this batch
        g.inc = inc;
        if (m == 0) {
            g.state = base;
            g.has = pre_has;
            g.buf = pre_buf;
        } else {
            g.state = lane128(st, m - 1);
            g.has = (cursor & 1) != 0;
            g.buf = (uint32_t)__builtin_amdgcn_readlane((int)hi, m - 1);  // numpy keeps the last buffered half also once it is used
        }
    }
    __device__ __forceinline__ uint32_t next32() {
        if (pre_has) {
            pre_has = false;
            return pre_buf;
        }
        if (cursor == 128) {
            base = lane128(st, 63);
            refill();
        }
        const int idx = cursor >> 1;
        const uint32_t v = (cursor & 1) ? (uint32_t)__builtin_amdgcn_readlane((int)hi, idx) : (uint32_t)__builtin_amdgcn_readlane((int)lo, idx);
        ++cursor;
        return v;
    }
    // Generator.integers(lo, hi): Lemire bounded draw on the 32-bit path; span 1 consumes nothing (Pcg::integers)
    __device__ __forceinline__ int integers(int lo_, int hi_) {
        const uint32_t rng = (uint32_t)(hi_ - 1 - lo_);
        if (rng == 0) return lo_;
        const uint32_t n = rng + 1u;
        uint64_t m = (uint64_t)next32() * n;
        uint32_t left = (uint32_t)m;
        if (left < n) {
            const uint32_t thr = (0xFFFFFFFFu - rng) % n;
            while (left < thr) {
                m = (uint64_t)next32() * n;
                left = (uint32_t)m;
            }
        }
        return lo_ + (int)(m >> 32);
    }
};

// MysteryPath.__init__ (pygame_assets.py:606-724) + Node (:438-493), every argument wave-uniform, called by all 64
// lanes.  Returns the path length (-1 = "No valid path found"); lane k < len receives the k-th path node (flat index
// x*7+y, END FIRST like the reference's list) in out_node, path_mask has one bit per path node.
__device__ int coop_path(WaveRng& g, const PathWS& W, int sx, int sy, int ex, int ey, int& out_node, uint64_t& path_mask, uint64_t& wall_out) {
    const int lane = threadIdx.x & 63;
    uint64_t wall = 0, closed = 0, in_open = 0;
    for (int i = 0; i < G; ++i)
        for (int j = 0; j < G; ++j)
            if (i > 0 && i < G - 2 && j > 0 && j < G - 2)
                if (g.integers(0, 100) < 33) wall |= 1ull << (i * G + j);
    const int start = sx * G + sy, end = ex * G + ey;
    // outer wall candidates, in the reference's (i, j) order == increasing flat index: one node per lane
    uint64_t outer;
    {
        const int idx = lane < G * G ? lane : 0;
        const int i = idx / G, j = idx - i * G;
        bool ok = lane < G * G && (i == 0 || i == G - 1 || j == 0 || j == G - 1) && idx != start && idx != end;
        for (int k = 0; k < 4; ++k) ok = ok && nb_of(start, k) != idx && nb_of(end, k) != idx;
        for (int k = 0; k < 4; ++k) {
            int q = nb_of(idx, k);
            if (q >= 0 && ((wall >> q) & 1ull)) ok = false;
            q = diag_of(idx, k);
            if (q >= 0 && ((wall >> q) & 1ull)) ok = false;
        }
        outer = __ballot(ok);
    }
    int n_outer = __popcll(outer);
    const int n_iter = g.integers(0, 2) == 0 ? 4 : 8;  // rng.choice([4, 8])
    for (int it = 0; it < n_iter; ++it) {
        if (n_outer > 0) {
            int k = g.integers(0, n_outer);
            uint64_t m = outer;
            for (int q = 0; q < k; ++q) m &= m - 1;  // k-th remaining candidate (list order)
            const int idx = __ffsll((unsigned long long)m) - 1;
            wall |= 1ull << idx;
            outer &= ~(1ull << idx);
            --n_outer;
        }
    }
    wall_out = wall;  // (the debug view draws the walls)
    // per-node record in lane n; f = g_cost + h is only ever evaluated for nodes in the open set, and the reference's
    // `neighbor.g = g` typo means g_cost never changes once a node has entered it
    int gval = 0, prev = -1;
    double hval = 0.0;
    {
        const int idx = lane < G * G ? lane : 0;
        const int ax = idx / G, ay = idx - ax * G;
        hval = W.h((ax - ex) * (ax - ex) + (ay - ey) * (ay - ey));
    }
    int lst = 0, n_open = 0;  // lane p: node at position p of the ordered open list
    if (lane == 0) lst = start;
    n_open = 1;
    in_open |= 1ull << start;
    for (;;) {
        if (n_open == 0) return -1;
        const double fnode = (double)gval + hval;
        const double f_at = __shfl(fnode, lst & 63);
        const double f0 = __shfl(f_at, 0);
        const uint64_t better = __ballot(lane >= 1 && lane < n_open && f_at < f0);
        const int w = better ? __ffsll((unsigned long long)better) - 1 : 0;  // first strictly better than open[0]
        const int cur = bcast(lst, w);
        if (cur == end) {
            int len = 0, t = cur;
            path_mask = 0;
            for (;;) {
                if (lane == len) out_node = t;
                path_mask |= 1ull << t;
                ++len;
                const int pv = bcast(prev, t);
                if (pv < 0) break;
                t = pv;
            }
            return len;
        }
        {  // open_set.remove(current)
            const int nxt = __shfl_down(lst, 1);
            if (lane >= w) lst = nxt;
            --n_open;
        }
        in_open &= ~(1ull << cur);
        closed |= 1ull << cur;
        const int gcur = bcast(gval, cur);
        // Node.add_neighbors order x+1, x-1, y+1, y-1 (-1 = outside).  Everything about WHICH neighbours are evaluated,
        // the draws and the list order is wave-uniform (scalar); the per-node updates are done by the node's own lane,
        // all four at once.  integers(1, 9) has a span of 8: Lemire never rejects, the draw is 1 + (word >> 29).
        const int cx = cur / G, cy = cur - cx * G;
        const int nb[4] = {cx < G - 1 ? cur + G : -1, cx > 0 ? cur - G : -1, cy < G - 1 ? cur + 1 : -1, cy > 0 ? cur - 1 : -1};
        const uint64_t blocked = closed | wall;
        int gg = 0;
        bool mine = false;
        int pos = n_open;
        const uint64_t was_open = in_open;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool valid = nb[k] >= 0 && !((blocked >> (nb[k] & 63)) & 1ull);
            if (!valid) continue;  // uniform
            const int cost = gcur + 1 + (int)(g.next32() >> 29);
            if (lane == nb[k]) {
                mine = true;
                gg = cost;
            }
            if (!((was_open >> nb[k]) & 1ull)) {  // open_set.append(neighbor)
                if (lane == pos) lst = nb[k];
                ++pos;
                in_open |= 1ull << nb[k];
            }
        }
        n_open = pos;
        if (mine) {
            if ((was_open >> lane) & 1ull) {
                if (gg < gval) prev = cur;  // `neighbor.g = g` typo: g_cost is NOT updated
            } else {
                gval = gg;
                prev = cur;
            }
        }
    }
}

// ---- Lane-per-job path generation ---------------------------------------------------------------------------------
// The wave-cooperative generator above finishes ONE path in ~25-33 us, as a chain of ~10,000 wave-uniform (scalar)
// instructions; a full reset of 32,768 instances (98,304 paths) keeps every SIMD's scalar issue busy for 1.25 ms.  Here
// every LANE generates its own path: the same algorithm with the per-node records and the open list in LDS (one column
// per lane) -- ~105 us per path (~1,100 vector instructions per expansion, one wave per SIMD), 64 paths per wave: a
// full reset in three rounds of 512 waves.  Used where many paths are due at once and nothing else runs (mg_reset of all
// instances); a step's few thousand queue entries stay with the cooperative generator, whose latency is lower
// (profiles/r02_emp.md).
//   * open list: every node enters it at most once and its f never changes afterwards (the reference's `neighbor.g = g`
//     typo), so the list is append-only with a 64-bit mask of the positions still in it; "first i >= 1 with f[i] < f[0]"
//     walks the set bits.
//   * f = g_cost + sqrt(d2) is compared through an integer key (g_cost << 17) + round(sqrt(d2) * 2^17): over all g_cost
//     <= 459 and all 27 values of d2 the keys order exactly like the doubles and are equal exactly where those are
//     (distinct sums differ by >= 2.5e-3; tests/test_path_keys.py checks every pair).
constexpr int LW_KEY = 0;                          // uint32 key[52][64]: (fkey << 6) | node, by list position; later the path
constexpr int LW_NODE = LW_KEY + 52 * 64 * 4;      // uint16 rec[49][64]: g_cost | previous_node << 9 (63 = none), by node
constexpr int LW_HFIX = LW_NODE + 49 * 64 * 2;     // uint32 hfix[80]
constexpr int LW_BYTES = LW_HFIX + 80 * 4;
struct LaneWS {
    uint8_t* base;
    int lane;
    __device__ __forceinline__ uint32_t& key(int p) const { return reinterpret_cast<uint32_t*>(base + LW_KEY)[p * 64 + lane]; }
    __device__ __forceinline__ uint16_t& rec(int n) const { return reinterpret_cast<uint16_t*>(base + LW_NODE)[n * 64 + lane]; }
    __device__ __forceinline__ uint32_t hfix(int d2) const { return reinterpret_cast<const uint32_t*>(base + LW_HFIX)[d2]; }
};
__device__ __forceinline__ void lane_ws_init(uint8_t* smem) {  // all threads of the block
    for (int d = threadIdx.x; d < 80; d += blockDim.x)
        reinterpret_cast<uint32_t*>(smem + LW_HFIX)[d] = (uint32_t)__double2ll_rn(sqrt((double)d) * 131072.0);
    __syncthreads();
}
constexpr uint64_t grid_mask(int which) {  // 0: y == 0, 1: y == 6, 2: border
    uint64_t m = 0;
    for (int x = 0; x < G; ++x)
        for (int y = 0; y < G; ++y)
            if ((which == 0 && y == 0) || (which == 1 && y == G - 1) || (which == 2 && (x == 0 || x == G - 1 || y == 0 || y == G - 1)))
                m |= 1ull << (x * G + y);
    return m;
}
constexpr uint64_t GM_Y0 = grid_mask(0), GM_Y6 = grid_mask(1), GM_BORDER = grid_mask(2), GM_ALL = (1ull << (G * G)) - 1;
__device__ __forceinline__ uint64_t cells_around4(uint64_t m) {
    return (((m << 1) & ~GM_Y0) | ((m >> 1) & ~GM_Y6) | (m << G) | (m >> G)) & GM_ALL;
}
__device__ __forceinline__ uint64_t cells_around8(uint64_t m) {  // m itself included
    const uint64_t v = m | ((m << 1) & ~GM_Y0) | ((m >> 1) & ~GM_Y6);
    return (v | (v << G) | (v >> G)) & GM_ALL;
}

// MysteryPath.__init__ (pygame_assets.py:606-724) by one lane.  Returns the path length (-1: none); W.key(k), k < len, is
// the k-th path node (flat index x*7+y, END first like the reference's list).
__device__ int lane_path(Pcg& g, const LaneWS& W, int sx, int sy, int ex, int ey, uint64_t& path_mask, uint64_t& wall_out) {
    uint64_t wall = 0;
    for (int i = 1; i < G - 2; ++i)
        for (int j = 1; j < G - 2; ++j)
            if (g.integers(0, 100) < 33) wall |= 1ull << (i * G + j);
    const int start = sx * G + sy, end = ex * G + ey;
    const uint64_t ends = (1ull << start) | (1ull << end);
    uint64_t outer = GM_BORDER & ~ends & ~cells_around4(ends) & ~cells_around8(wall);
    int n_outer = __popcll(outer);
    const int n_iter = g.integers(0, 2) == 0 ? 4 : 8;  // rng.choice([4, 8])
    for (int it = 0; it < n_iter; ++it) {
        if (n_outer > 0) {
            const int k = g.integers(0, n_outer);
            uint64_t m = outer;
            for (int q = 0; q < k; ++q) m &= m - 1;
            const uint64_t bit = m & (~m + 1);
            wall |= bit;
            outer &= ~bit;
            --n_outer;
        }
    }
    wall_out = wall;
    uint64_t closed = 0, in_open = 1ull << start, live = 1;
    int n_pos = 1;
    W.key(0) = (uint32_t)start;  // (only the order of the keys matters: the start is alone in the list when it is taken)
    W.rec(start) = (uint16_t)(63u << 9);
    // "first i >= 1 with f[i] < f[0], else 0": while open[0] stays, the positions before the last hit are known not to beat
    // it (keys never change), so the walk resumes behind the hit; four keys are fetched per round trip to LDS
    int head = -1, scan = 0;
    uint32_t khead = 0;
    for (;;) {
        if (!live) return -1;
        const int p0 = __ffsll((unsigned long long)live) - 1;
        if (p0 != head) {
            head = p0;
            khead = W.key(p0);
            scan = p0 + 1;
        }
        const uint32_t k0 = khead >> 6;
        int w = p0;
        uint32_t kw = khead;
        for (int p = scan; p < n_pos && w == p0; p += 4) {
            const uint32_t a[4] = {W.key(p), W.key(p + 1), W.key(p + 2), W.key(p + 3)};
#pragma unroll
            for (int q = 3; q >= 0; --q)  // the lowest qualifying position wins
                if (p + q < n_pos && ((live >> (p + q)) & 1ull) && (a[q] >> 6) < k0) {
                    w = p + q;
                    kw = a[q];
                }
        }
        scan = w != p0 ? w + 1 : n_pos;
        const int cur = (int)(kw & 63u);
        if (cur == end) {
            int len = 0, t = cur;
            path_mask = 0;
            for (;;) {
                path_mask |= 1ull << t;
                const int pv = W.rec(t) >> 9;
                W.key(len++) = (uint32_t)t;
                if (pv == 63) break;
                t = pv;
            }
            return len;
        }
        live &= ~(1ull << w);
        in_open &= ~(1ull << cur);
        closed |= 1ull << cur;
        const int gcur = W.rec(cur) & 511;
        const int cx = cur / G, cy = cur - cx * G;
        const uint64_t blocked = closed | wall;
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // Node.add_neighbors order x+1, x-1, y+1, y-1
            const int nb = k == 0 ? (cx < G - 1 ? cur + G : -1) : k == 1 ? (cx > 0 ? cur - G : -1) : k == 2 ? (cy < G - 1 ? cur + 1 : -1) : (cy > 0 ? cur - 1 : -1);
            if (nb < 0 || ((blocked >> nb) & 1ull)) continue;
            const int cost = gcur + 1 + (int)(g.next32() >> 29);  // integers(1, 9): span 8, never rejects
            if ((in_open >> nb) & 1ull) {
                const uint16_t r = W.rec(nb);
                if (cost < (int)(r & 511)) W.rec(nb) = (uint16_t)((r & 511) | (cur << 9));  // `neighbor.g = g` typo: g_cost stays
            } else {
                W.rec(nb) = (uint16_t)(cost | (cur << 9));
                const int ax = nb / G - ex, ay = nb % G - ey;
                W.key(n_pos) = ((((uint32_t)cost << 17) + W.hfix(ax * ax + ay * ay)) << 6) | (uint32_t)nb;
                live |= 1ull << n_pos;
                ++n_pos;
                in_open |= 1ull << nb;
            }
        }
    }
}
}  // namespace mg
