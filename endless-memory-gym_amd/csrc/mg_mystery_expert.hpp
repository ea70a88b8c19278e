// mg_mystery_expert.hpp -- Mystery Path family (included by mg_mystery.hip only): the scripted teacher of its three ids -- follow the path --, oracle/mgo_mystery.c
// mpf_expert / emp_expert restated on MysteryCore, the finite variants' stored path order (path_order) and the endless variant's segment store.
#pragma once
#include "mg_expert.hpp"
#include "mg_mystery_endless.hpp"
#include "mg_mystery_types.hpp"

namespace mg {
// MysteryPath-v0, MysteryPath-Grid-v0: towards the node that FOLLOWS the agent's tile in the reference's path list.  The list is kept as it was generated
// (path_order: end first), not rebuilt from path_mask: a path can have a chord -- two cells adjacent in the grid but not consecutive in the list, the
// `neighbor.g = g` typo of the reference's A* -- and then the mask does not say which neighbour comes next.
__device__ __forceinline__ void mpf_expert(const MysteryParams& P, const MysteryIO& io, int i, const MysteryCore& s, int& a0, int& a1) {
    typedef uint32_t q4 __attribute__((ext_vector_type(4)));
    const q4* op = reinterpret_cast<const q4*>(path_order(io, i));
    const q4 o0 = op[0], o1 = op[1], o2 = op[2], o3 = op[3];  // (49 nodes at most; the four loads are in flight together)
    const uint32_t w[16] = {o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w, o2.x, o2.y, o2.z, o2.w, o3.x, o3.y, o3.z, o3.w};
    const int nx = s.ax / P.tile, ny = s.ay / P.tile;  // (ax, ay >= 0: the finite variants clamp the agent to the screen)
    const uint32_t cell = (uint32_t)(nx * G + ny);
    int idx = -1, next = 0;  // a path holds a cell once: the first match is the only one
#pragma unroll
    for (int k = 63; k >= 1; --k) {
        const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
        if (k < (int)s.path_len && b == cell) {
            idx = k;
            next = (int)((w[(k - 1) >> 2] >> (8 * ((k - 1) & 3))) & 0xFFu);
        }
    }
    a0 = a1 = 0;
    if (idx <= 0) return;  // off the path (the next step puts the agent back), or on the goal (index 0)
    const int tx = next / G, ty = next - tx * G;
    if (P.grid) {
        a0 = expert_grid_action(s.rot8 * 45, expert_grid_facing(tx - nx, ty - ny));
        return;
    }
    a0 = expert_axis_action(tx * P.tile + P.tile / 2 - s.ax, 1);
    a1 = expert_axis_action(ty * P.tile + P.tile / 2 - s.ay, 1);
}

// Endless-MysteryPath-v0: towards the node behind cur_node (vertically first, then to the right).
__device__ __forceinline__ int emp_expert(const MysteryParams& P, const MysteryIO& io, int i, MysteryCore& s) {  // (s: read only; EMP_AX wants an lvalue)
    const uint8_t* rec = seg_ptr(io, i, s.cur_node_seg);
    int nseg = s.cur_node_seg, nidx = s.cur_node_idx + 1;
    if (nidx >= rec[0]) {  // (byte 0: the record's node count, the transition node at x = 7 included)
        nseg++;
        nidx = 0;
    }
    // The node behind cur_node is always generated when a step has returned, although segments may still be OWED (lazy initial segments, lazy appends):
    // cur_node is a node the agent has stood on, and nothing is generated in this kernel.  It is the LAST node of the last generated segment only if it
    // is that segment's transition node, in column 8 num_seg - 1.  The step that put the agent there had nx >= 8 num_seg - 2 and something owed (the
    // reference holds at least cur_seg + 2 segments, emp_step_a's `cur_seg > num_seg + owed - 2`, and cur_seg = num_seg - 1 here), so emp_step_a
    // returned EMP_DUE and the owed segment was generated inside that step's launches before emp_step_b ran -- num_seg has grown past nseg.  With
    // nothing owed the reference itself holds no further node (a full segment store: that step ended the episode), which is the oracle's
    // `k + 1 >= epath_len`: no action, as here.
    if (s.off || nseg >= s.num_seg) return 0;
    const uint8_t nb = seg_ptr(io, i, nseg)[1 + nidx];
    const int dx = node_x(nseg, nb) * P.tile + P.tile / 2 - EMP_AX(s), dy = node_y(nb) * P.tile + P.tile / 2 - s.ay;
    return dy < 0 ? 2 : (dy > 0 ? 3 : (dx > 0 ? 1 : 0));
}

__global__ __launch_bounds__(EXPERT_BLOCK) void mystery_expert_kernel(MysteryParams P0, MysteryIO io, ExpertArgs x) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P0.n) return;
    const MysteryParams& P = io.set_of ? io.sets[set_index(io.set_of, i)] : P0;
    MysteryCore s = load_core(io.core + i);
    int a0 = 0, a1 = 0;
    if (P.endless) a0 = emp_expert(P, io, i, s);
    else mpf_expert(P, io, i, s, a0, a1);
    expert_store(x, i, P.endless || P.grid, a0, a1);
}
}  // namespace mg
