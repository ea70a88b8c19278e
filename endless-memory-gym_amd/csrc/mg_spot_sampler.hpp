// mg_spot_sampler.hpp -- (included by mg_spot.hip only) the reference's GridPositionSampler.sample (pygame_assets.py:7-59) for the 16 lanes of a group, and nothing of the
// environments that ask for cells (of mg_spot_types.hpp it takes MAX_COINS, the size of the disc list): integer distance tests, the blocked discs in LDS (Discs), where a
// lane sits in its group (LaneCtx), a row's blocked cells as a 128-bit mask or as two spans, and sample_cell, the cooperative draw of the k-th free cell.
#pragma once
#include "mg_spot_types.hpp"

namespace mg {
// floor(sqrt(v)), v < 2^24: single-precision estimate (a double-precision square root is ~20 dependent f64 instructions on this
// chip), made exact by the two integer corrections.
__device__ __forceinline__ int isqrt_floor(int v) {
    int r = (int)__fsqrt_rn((float)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}
// sqrt(dx^2 + dy^2) <= R for integers (Coin / agent distance tests of the reference, computed there in doubles): the square root is
// correctly rounded and monotonic and sqrt(R^2) == R exactly, so the test is d2 <= R^2 -- without the f64 square root.
__device__ __forceinline__ bool within(int dx, int dy, int R) { return dx * dx + dy * dy <= R * R; }

// GridPositionSampler.sample: k-th un-blocked cell (row-major) of the 84x84 grid; discs: (x, y, r) with strict <.
// Each row's blocked set is a union of intervals [cx - hw, cx + hw] with hw = isqrt(r^2 - dy^2 - 1); rows are
// 84-bit masks built with shifts (no per-cell loops), free cells counted with popcounts.
typedef unsigned __int128 u128m;
// The blocked discs (agent, coins, exit; at most 1 + MAX_COINS + 1) of the instance a 16-lane group is resetting live in
// LDS (x[], y[], r[] of MAX_DISCS ints each in the group's DISC_INTS-int slot; all 16 lanes write the same values, each
// reads after its own write).  As register arrays -- compile-time indices under predicates -- they pushed the finite
// variant's fused raster / reset kernel 109 dwords past its 96 VGPRs: 436 B of scratch per lane, which a kernel pays for at
// EVERY wave launch (profiles/r02_spot_resets.md), and unrolled its loops over the discs.
constexpr int MAX_DISCS = 1 + MAX_COINS + 1;
constexpr int DISC_INTS = 3 * MAX_DISCS + MAX_COINS + 2;  // + the coins placed by a finite reset (spot_reset), 16-byte multiple
static_assert(DISC_INTS % 4 == 0, "group slots stay 16-byte aligned");
struct Discs {
    int* p;  // LDS slot of this lane's group
    int n;
    __device__ __forceinline__ void push(int X, int Y, int R) {
        p[n] = X;
        p[MAX_DISCS + n] = Y;
        p[2 * MAX_DISCS + n] = R;
        ++n;
    }
};
// the slot of the calling lane's group inside an array of (workgroup size / 16) * DISC_INTS ints
__device__ __forceinline__ int* disc_slot(int* lds, int grp) { return lds + grp * DISC_INTS; }
// Where a lane sits: its slot id, the group (= instance) of 16 lanes it belongs to within the workgroup, and that group's bit
// position in a wave ballot.
struct LaneCtx {
    int ls, grp, gshift;
};
__device__ __forceinline__ LaneCtx lane_ctx(int tix) { return LaneCtx{tix & 15, tix >> 4, ((tix >> 4) & 3) * 16}; }
__device__ __forceinline__ u128m row_mask(const Discs& D, int y) {
    u128m m = 0;
    for (int d = 0; d < D.n; ++d) {
        const int dx = D.p[d], dr = D.p[2 * MAX_DISCS + d];
        int ddy = y - D.p[MAX_DISCS + d], rem = dr * dr - ddy * ddy - 1;
        if (rem < 0) continue;
        int hw = isqrt_floor(rem);
        int a = dx - hw, b = dx + hw;
        a = a < 0 ? 0 : a;
        b = b > SCREEN - 1 ? SCREEN - 1 : b;
        if (a > b) continue;
        m |= (((u128m)1 << (b + 1)) - 1) ^ (((u128m)1 << a) - 1);
    }
    return m;
}
__device__ __forceinline__ int popc128(u128m m) { return __popcll((unsigned long long)m) + __popcll((unsigned long long)(m >> 64)); }

// Cooperative form: the 16 lanes of an instance call this together (same arguments, same RNG state in every lane).
// Lane ls owns the six rows [6 ls, 6 ls + 6) (lanes 14, 15 idle); free-cell counts are reduced / scanned across the
// group with shuffles, every lane performs the identical draw, and the lane whose rows contain the k-th free cell
// locates it.  A single lane walking all 84 rows twice took ~40 us (the tail of the whole step kernel whenever any
// instance re-spawned its coin).
constexpr int ROWS_PER_LANE = 6;
static_assert(ROWS_PER_LANE * 14 == SCREEN, "14 lanes x 6 rows cover the sampler grid");
// One row of the grid under one or two discs: the blocked cells as two sorted, disjoint intervals [a1, a1 + l1), [a2, a2 + l2)
// (a length of 0 = none; two overlapping or touching spans are returned as one).
__device__ __forceinline__ void row_spans(const Discs& D, int y, int& a1, int& l1, int& a2, int& l2) {
    int lo[2] = {0, 0}, hi[2] = {-1, -1};
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        if (d >= D.n) continue;
        const int dx = D.p[d], dr = D.p[2 * MAX_DISCS + d], ddy = y - D.p[MAX_DISCS + d], rem = dr * dr - ddy * ddy - 1;
        if (rem < 0) continue;
        const int hw = isqrt_floor(rem);
        lo[d] = dx - hw < 0 ? 0 : dx - hw;
        hi[d] = dx + hw > SCREEN - 1 ? SCREEN - 1 : dx + hw;
    }
    const bool e0 = hi[0] >= lo[0], e1 = hi[1] >= lo[1];
    if (e0 && e1 && lo[0] <= hi[1] + 1 && lo[1] <= hi[0] + 1) {  // one span
        a1 = lo[0] < lo[1] ? lo[0] : lo[1];
        l1 = (hi[0] > hi[1] ? hi[0] : hi[1]) - a1 + 1;
        a2 = SCREEN;
        l2 = 0;
        return;
    }
    const bool first0 = e0 && (!e1 || lo[0] < lo[1]);  // which span comes first (an empty one goes last)
    const int fa = first0 ? lo[0] : lo[1], fb = first0 ? hi[0] : hi[1], sa = first0 ? lo[1] : lo[0], sb = first0 ? hi[1] : hi[0];
    const bool fe = first0 ? e0 : e1, se = first0 ? e1 : e0;
    a1 = fe ? fa : SCREEN;
    l1 = fe ? fb - fa + 1 : 0;
    a2 = se ? sa : SCREEN;
    l2 = se ? sb - sa + 1 : 0;
}

__device__ __forceinline__ int sample_cell(Pcg& g, const Discs& D, const LaneCtx& L, int* ox, int* oy) {
    const int ls = L.ls;
    if (D.n == 0) {  // empty mask: cell k itself
        int k = g.integers(0, SCREEN * SCREEN);
        *oy = k / SCREEN;
        *ox = k - *oy * SCREEN;
        return SCREEN * SCREEN;
    }
    const int y0 = ls * ROWS_PER_LANE;
    // One or two discs (the endless variant's coin re-sampling: the collected coin; the finite variant's first coin and, with one
    // coin, its exit: agent, agent + coin): a row's blocked cells are at most two spans -- no 128-bit masks, the k-th free cell by
    // comparisons (round 4; SearingSpotlights-v0 at 4,096 instances, where the launch is as long as one reset: 126 -> 135 M
    // env-steps/s with the one-disc form alone).
    const bool few = D.n <= 2;
    int local_free = 0;
    if (ls < 14) {
        if (few) {
            for (int j = 0; j < ROWS_PER_LANE; ++j) {
                int a1, l1, a2, l2;
                row_spans(D, y0 + j, a1, l1, a2, l2);
                local_free += SCREEN - l1 - l2;
            }
        } else {
            for (int j = 0; j < ROWS_PER_LANE; ++j) local_free += SCREEN - popc128(row_mask(D, y0 + j));
        }
    }
    // inclusive scan over the 16 lanes of the group (width-16 shuffles stay inside the instance's lanes)
    int incl = local_free;
    for (int off = 1; off < 16; off <<= 1) {
        int v = __shfl_up(incl, off, 16);
        if (ls >= off) incl += v;
    }
    const int free_total = __shfl(incl, 15, 16);
    int k = g.integers(0, free_total);  // identical in all 16 lanes
    const int excl = incl - local_free;
    int fx = -1, fy = -1;
    if (few && k >= excl && k < incl) {  // exactly one lane
        int kk = k - excl;
        for (int j = 0; j < ROWS_PER_LANE; ++j) {
            int a1, l1, a2, l2;
            row_spans(D, y0 + j, a1, l1, a2, l2);
            const int fr = SCREEN - l1 - l2;
            if (kk < fr) {
                int x = kk;
                if (x >= a1) x += l1;
                if (x >= a2) x += l2;
                fx = x;
                fy = y0 + j;
                break;
            }
            kk -= fr;
        }
    } else if (k >= excl && k < incl) {  // exactly one lane
        int kk = k - excl;
        for (int j = 0; j < ROWS_PER_LANE; ++j) {
            u128m m = row_mask(D, y0 + j);
            int fr = SCREEN - popc128(m);
            if (kk < fr) {
                // kk-th free cell of this row: skip whole bytes, then single bits
                int x = 0;
                for (;; x += 8) {
                    int zb = 8 - __popc((unsigned)(m >> x) & 0xFFu);
                    if (x + 8 > SCREEN) zb -= x + 8 - SCREEN;  // bits beyond the grid are not cells
                    if (kk < zb) break;
                    kk -= zb;
                }
                for (;; ++x) {
                    if (!((m >> x) & 1)) {
                        if (kk == 0) break;
                        --kk;
                    }
                }
                fx = x;
                fy = y0 + j;
                break;
            }
            kk -= fr;
        }
    }
    const int owner = __ffs((unsigned)(__ballot(fx >= 0) >> L.gshift) & 0xFFFFu) - 1;
    *ox = __shfl(fx, owner, 16);
    *oy = __shfl(fy, owner, 16);
    return free_total;
}
}  // namespace mg
