// st_search.h -- the bit-set search helpers k_reachable (st_reachable.hip),
// k_routes (st_routes.hip) and k_locks (st_locks.hip) share: a slot's free
// rows, the occluded fills down and up, the result-word and route constants.
// Included behind st_kernels.hip (with ST_SIDE_TU), whose piece table it uses.
#pragma once

namespace st {
namespace {

// ---------------------------------------------------------------- reachability
// st_reachable / st_route_actions: which placement slots of st_afterstates the
// live piece can really be locked in under TetrisEngine.step
// (tetris_env.py:243-304), in how many steps, and the first action of a
// shortest way there (simpletetris.h, "Reachability").  A breadth-first search
// over the piece states (rot, x, y, l) with the board fixed, whole sets at a
// time: one wave per env, a lane per slot (rot, x) as in k_afterstates,
// ceil(S / 64) slots a lane; a lane's 32-bit word is a set of anchor rows y
// (never negative, below H <= 28).
//   free[rot, x]  bit y: the piece at (x, y) is not is_occupied (:29-36) -- the
//                 four box columns shifted by each cell's dy, ORed, inverted;
//                 rows above 0 shift in zeros (free, :32-33), rows past the
//                 field read the floor bits, columns past it the walls.  Every
//                 shape holds cell (0, 0), so no bit y >= H and no column
//                 outside [0, W) is ever free: nothing crosses a row's edge.
//   sets          A[tag][l][slot] in LDS, l = the lock counter's plane; two
//                 copies, read one / write the other, one wave_sync a layer.
// One layer = one step applied to a whole set: every action's destinations
// (a neighbouring lane's word & free for left / right / the two rotations,
// (A << 1) & free for soft drop, an occluded fill downward -- Kogge-Stone,
// five rounds -- for hard drop, A itself for idle and for every refused
// action), then gravity (:247-250), then _has_dropped and the lock counter
// (:259-262) across the planes.  Sets are cumulative, so the first layer whose
// lock set holds a slot's landing bit is its distance; the loop ends on a
// wave-uniform ballot when no set grew (then no lock set can grow either), and
// in every case after 4 * (W + 6) * H * (L + 1) layers, the number of states.
// TAGGED: seven sets, started from the seven successors of the start state
// (layer 1, computed by lanes 0..6 on the start state alone); the lowest tag
// that reaches a slot at its first layer is `first`.  ROUTE: the tagged search
// with one target slot an env, ended as soon as any tag reaches it.
__device__ __forceinline__ uint32_t reach_free(const uint32_t *C, int W, int id, int s) {
    const int per = W + 6;
    const int r = (s >= per) + (s >= 2 * per) + (s >= 3 * per), x = s - r * per - 3;
    const uint32_t m = c_tab_m[id * 4 + r], g = c_tab_g[id * 4 + r];
    const int x0 = box_x0(g, x);  // in [-6, W + 2]
    uint32_t occ = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t col = C[x0 + j], byte = (m >> (8 * j)) & 0xFFu;
#pragma unroll
        for (int b = 0; b < 7; ++b)  // bit b: a cell at dy = b - 3
            if ((byte >> b) & 1u) occ |= b >= 3 ? col >> (b - 3) : col << (3 - b);
    }
    return ~occ;
}

// Every row a set's pieces can fall to (hard_drop's loop, :54-59, on all of
// them at once): bit y + 1 joins while its row is free.
__device__ __forceinline__ uint32_t reach_fall(uint32_t a, uint32_t free) {
    uint32_t gen = a, pro = free;
    gen |= pro & (gen << 1);
    pro &= pro << 1;
    gen |= pro & (gen << 2);
    pro &= pro << 2;
    gen |= pro & (gen << 4);
    pro &= pro << 4;
    gen |= pro & (gen << 8);
    pro &= pro << 8;
    gen |= pro & (gen << 16);
    return gen;
}

constexpr uint32_t kReachNone = ~0u;  // a result word (layer << 3 | tag) not found yet

// ---------------------------------------------------------------- backward search
// What k_routes (st_routes.hip) and k_locks (st_locks.hip) share.
constexpr uint64_t kRouteNone = 0x7FFFFFFFFFFFFFFFull;  // every field 7, bit 63 clear
constexpr int kRoutePlanes = ST_REACH_MAX_LOCK + 1;

// Every row from which a hard drop lands in a row of `a` (rows of `a` are
// grounded): row y joins while row y + 1 is free (fd bit y) and has joined.
__device__ __forceinline__ uint32_t route_rise(uint32_t a, uint32_t fd) {
    uint32_t gen = a, pro = fd;
    gen |= pro & (gen >> 1);
    pro &= pro >> 1;
    gen |= pro & (gen >> 2);
    pro &= pro >> 2;
    gen |= pro & (gen >> 4);
    pro &= pro >> 4;
    gen |= pro & (gen >> 8);
    pro &= pro >> 8;
    gen |= pro & (gen >> 16);
    return gen;
}

}  // namespace
}  // namespace st
