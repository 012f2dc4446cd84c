// st_eval.h -- what the side units that evaluate placement slots share: the
// slot evaluators (eval_slot, eval_slot_set), the wave's column staging
// (stage_env_columns, also k_reachable's), the committed piece word, the linear
// score, the DPP wave reductions and the two-ply kernels' shape.  Included
// behind st_kernels.hip (with ST_SIDE_TU), whose helpers it uses; the library's
// own unit needs none of it.
#pragma once

namespace st {
namespace {

// ---------------------------------------------------------------- afterstates
// st_afterstates: what k_policy_greedy evaluates and throws away, as an
// output.  For env e's board and current piece id, every placement slot
// s = rot * (W + 6) + (x + 3) (k_policy_greedy's (rot, x) loop order): the
// piece at (x, 0) in rotation rot is valid iff not is_occupied
// (tetris_env.py:29-36), is hard-dropped (:54-59), set (_set_piece's
// clipping, :323-327) and the full rows are cleared (:205-216); the rows of
// st_after_feat and, optionally, the resulting board are written.  The
// piece's present rot, anchor and lock counter play no part, nor does
// lock_delay; no state is written.
// One wave per env, lane = slot, ceil(S / 64) passes.  The env's W column
// words are wave-uniform: lanes 0 .. W + 15 load one word each (floor bits,
// all-ones walls, as k_policy_greedy stages them) into W + 16 LDS words, and
// every later column read is a broadcast (all lanes one address) or, for the
// four box columns, at most W + 16 distinct addresses.  Outputs have the slot
// innermost, so each row leaves as one contiguous store per wave.
// REWARD is lock_score's -- the rules of the step that locks the piece there
// (:256-297) under the context's flags, from the env's holes and
// piece_height counters.
//
// One slot's evaluation, shared by k_afterstates and k_policy_linear: the
// collision test, the drop, the overlay, the clear, the column pass and
// lock_score.  C: the wave's column words, column c at C[c] (c in [-P, W + P));
// s: a slot in [0, S); f: the rows of st_after_feat as the slot has them if it
// is valid (the caller masks the rows of an invalid one); col_out(c, w, valid):
// column c of the board after the clear.  Returns the slot's validity.
template <class ColOut>
__device__ __forceinline__ bool eval_slot(const uint32_t *C, int W, int H, uint32_t flags, int id, int s,
                                          int32_t old_holes, int32_t old_height, int32_t (&f)[ST_AFTER_NFEAT],
                                          ColOut col_out) {
    const uint32_t hmask = (1u << H) - 1u, floorb = ~hmask;
    const int per = W + 6;
    const int r = (s >= per) + (s >= 2 * per) + (s >= 3 * per), x = s - r * per - 3;
    const uint32_t m = c_tab_m[id * 4 + r], g = c_tab_g[id * 4 + r];
    const int x0 = box_x0(g, x);
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = C[x0 + j];
    const bool valid = !collides_v(m, 0, v);
    const int y = valid ? drop_box(g, 0, v) : 0;
    bool above = false;
    uint32_t pb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t byte = (m >> (8 * j)) & 0xFFu;
        above = above || (byte != 0u && y + __builtin_ctz(byte) - 3 < 0);  // (a box column without cells)
        pb[j] = pc_bits(m, j, y) & hmask;
    }
    // the board with the piece: column c gets the bits of the box column at c
    uint32_t andv = hmask;
    for (int c = 0; c < W; ++c) {
        uint32_t w = C[c];
#pragma unroll
        for (int j = 0; j < 4; ++j) w |= x0 + j == c ? pb[j] : 0u;
        andv &= w;
    }
    const int32_t ncl = __builtin_popcount(andv);
    int32_t holes = 0, agg = 0, bump = 0, hprev = 0;
    uint32_t orv = 0;
    for (int c = 0; c < W; ++c) {
        uint32_t w = C[c] & hmask;
#pragma unroll
        for (int j = 0; j < 4; ++j) w |= x0 + j == c ? pb[j] : 0u;
        if (andv) w = compact(w, andv);
        const int32_t h = H - (int32_t)__builtin_ctz(w | floorb);  // the column's height
        holes += h - __builtin_popcount(w);
        agg += h;
        bump += c ? (h > hprev ? h - hprev : hprev - h) : 0;
        hprev = h;
        orv |= w;
        col_out(c, w, valid);
    }
    int32_t rew = (flags & ST_REWARD_STEP) ? 1 : 0;  // :256
    int32_t score = 0, lines = 0, nholes = 0, height = 0, deaths = 0;
    lock_score<false>(flags, ncl, orv, [&] { return holes; }, old_holes, old_height, rew, score, lines, nholes, height,
                      deaths);
    f[ST_AFTER_VALID] = 1;
    f[ST_AFTER_Y] = y;
    f[ST_AFTER_LINES] = ncl;
    f[ST_AFTER_HOLES] = holes;
    f[ST_AFTER_HEIGHT] = orv ? H - (int32_t)__builtin_ctz(orv) : 0;
    f[ST_AFTER_ROWS] = __builtin_popcount(orv);
    f[ST_AFTER_ABOVE] = above ? 1 : 0;
    f[ST_AFTER_DEAD] = (int32_t)(orv & 1u);
    f[ST_AFTER_REWARD] = rew;
    f[ST_AFTER_AGG_HEIGHT] = agg;
    f[ST_AFTER_BUMPINESS] = bump;
    return valid;
}

// eval_slot_set<SET>: eval_slot with the rows of a feature set, for the
// kernels of st_features.hip.  It restates eval_slot (which stays word for word
// what k_afterstates and k_policy_linear were compiled from: a set parameter
// on eval_slot itself, every extension statement under if constexpr, moved
// three instructions of theirs) and must follow it change for change; the
// tests hold the base rows of both against the same oracle.
// SET = ST_FEATS_BCTS adds the rows of st_after_ext (simpletetris.h, "Feature
// sets") behind st_after_feat's, from what the walks hold anyway: LANDING2 and
// ERODED from the piece's box bytes / box bits and the full-row mask, the
// other five from the column words of the second walk -- a column's word,
// its left neighbour's and the one before that (a well of column c - 1 is
// known once column c is), walls as all-ones words of H bits.
constexpr int feat_rows(int set) { return set == ST_FEATS_BCTS ? ST_AFTER_NFEAT + ST_AFTER_NEXT : ST_AFTER_NFEAT; }

// sum of d (d + 1) / 2 over the runs of set bits of m, d a run's length
__device__ __forceinline__ int32_t well_sum(uint32_t m) {
    int32_t sum = 0;
    while (m) {
        sum += __builtin_popcount(m);
        m &= m << 1;
    }
    return sum;
}

// the extension rows' state over the second walk: the two columns left of
// c and the sums of the per-column rows (nothing in the base set)
template <bool EXT>
struct ExtAcc {};
template <>
struct ExtAcc<true> {
    uint32_t w1, w2, hole_or = 0;
    int32_t rtr = 0, ctr = 0, wells = 0, hdepth = 0;
};

template <int SET, class ColOut>
__device__ __forceinline__ bool eval_slot_set(const uint32_t *C, int W, int H, uint32_t flags, int id, int s,
                                              int32_t old_holes, int32_t old_height,
                                              int32_t (&f)[feat_rows(SET)], ColOut col_out) {
    constexpr bool EXT = SET == ST_FEATS_BCTS;
    const uint32_t hmask = (1u << H) - 1u, floorb = ~hmask;
    const int per = W + 6;
    const int r = (s >= per) + (s >= 2 * per) + (s >= 3 * per), x = s - r * per - 3;
    const uint32_t m = c_tab_m[id * 4 + r], g = c_tab_g[id * 4 + r];
    const int x0 = box_x0(g, x);
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = C[x0 + j];
    const bool valid = !collides_v(m, 0, v);
    const int y = valid ? drop_box(g, 0, v) : 0;
    bool above = false;
    uint32_t pb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t byte = (m >> (8 * j)) & 0xFFu;
        above = above || (byte != 0u && y + __builtin_ctz(byte) - 3 < 0);  // (a box column without cells)
        pb[j] = pc_bits(m, j, y) & hmask;
    }
    // the board with the piece: column c gets the bits of the box column at c
    uint32_t andv = hmask;
    for (int c = 0; c < W; ++c) {
        uint32_t w = C[c];
#pragma unroll
        for (int j = 0; j < 4; ++j) w |= x0 + j == c ? pb[j] : 0u;
        andv &= w;
    }
    const int32_t ncl = __builtin_popcount(andv);
    int32_t holes = 0, agg = 0, bump = 0, hprev = 0;
    uint32_t orv = 0;
    ExtAcc<EXT> x_;
    if constexpr (EXT) x_.w1 = x_.w2 = hmask;  // the left wall
    for (int c = 0; c < W; ++c) {
        uint32_t w = C[c] & hmask;
#pragma unroll
        for (int j = 0; j < 4; ++j) w |= x0 + j == c ? pb[j] : 0u;
        if (andv) w = compact(w, andv);
        if constexpr (EXT) {
            x_.rtr += __builtin_popcount(x_.w1 ^ w);
            const uint32_t wf = w | (1u << H);  // the floor counts as filled
            x_.ctr += __builtin_popcount((wf ^ (wf >> 1)) & hmask);
            if (c) x_.wells += well_sum(~x_.w1 & x_.w2 & w & hmask);  // column c - 1
            const uint32_t top = w & (0u - w);                // the column's topmost cell (0: none)
            uint32_t hl = ~w & hmask & ~(top | (top - 1u));   // its holes: empty, below the top
            x_.hole_or |= hl;
            while (hl) {
                x_.hdepth += __builtin_popcount(w & ((hl & (0u - hl)) - 1u));  // the cells above this hole
                hl &= hl - 1u;
            }
            x_.w2 = x_.w1;
            x_.w1 = w;
        }
        const int32_t h = H - (int32_t)__builtin_ctz(w | floorb);  // the column's height
        holes += h - __builtin_popcount(w);
        agg += h;
        bump += c ? (h > hprev ? h - hprev : hprev - h) : 0;
        hprev = h;
        orv |= w;
        col_out(c, w, valid);
    }
    int32_t rew = (flags & ST_REWARD_STEP) ? 1 : 0;  // :256
    int32_t score = 0, lines = 0, nholes = 0, height = 0, deaths = 0;
    lock_score<false>(flags, ncl, orv, [&] { return holes; }, old_holes, old_height, rew, score, lines, nholes, height,
                      deaths);
    f[ST_AFTER_VALID] = 1;
    f[ST_AFTER_Y] = y;
    f[ST_AFTER_LINES] = ncl;
    f[ST_AFTER_HOLES] = holes;
    f[ST_AFTER_HEIGHT] = orv ? H - (int32_t)__builtin_ctz(orv) : 0;
    f[ST_AFTER_ROWS] = __builtin_popcount(orv);
    f[ST_AFTER_ABOVE] = above ? 1 : 0;
    f[ST_AFTER_DEAD] = (int32_t)(orv & 1u);
    f[ST_AFTER_REWARD] = rew;
    f[ST_AFTER_AGG_HEIGHT] = agg;
    f[ST_AFTER_BUMPINESS] = bump;
    if constexpr (EXT) {
        x_.rtr += __builtin_popcount(x_.w1 ^ hmask);    // the last column against the right wall
        x_.wells += well_sum(~x_.w1 & x_.w2 & hmask);   // column W - 1 (W >= 4: w2 is column W - 2)
        // the rows the piece spans, unclipped: bit dy + 3 of a box byte is row y + dy
        const uint32_t span = (m | m >> 8 | m >> 16 | m >> 24) & 0xFFu;
        const int32_t ymin = y + (int32_t)__builtin_ctz(span) - 3, ymax = y + 28 - (int32_t)__builtin_clz(span);
        int32_t gone = 0;  // cells of the piece, inside the board, in a row that was cleared
#pragma unroll
        for (int j = 0; j < 4; ++j) gone += __builtin_popcount(pb[j] & andv);
        f[ST_AFTER_NFEAT + ST_AFTER_EXT_LANDING2] = 2 * H - 1 - (ymin + ymax);
        f[ST_AFTER_NFEAT + ST_AFTER_EXT_ERODED] = ncl * gone;
        f[ST_AFTER_NFEAT + ST_AFTER_EXT_ROW_TRANS] = x_.rtr;
        f[ST_AFTER_NFEAT + ST_AFTER_EXT_COL_TRANS] = x_.ctr;
        f[ST_AFTER_NFEAT + ST_AFTER_EXT_WELLS] = x_.wells;
        f[ST_AFTER_NFEAT + ST_AFTER_EXT_HOLE_DEPTH] = x_.hdepth;
        f[ST_AFTER_NFEAT + ST_AFTER_EXT_HOLE_ROWS] = __builtin_popcount(x_.hole_or);
    }
    return valid;
}

// The wave's W + 2 * P column words (floor bits, all-ones walls): lanes
// 0 .. W + 2 * P - 1 write one word each.
constexpr int kAfterP = 8;  // wall columns each side: the box's columns span [-6, W + 5]
constexpr int kAfterCols = kMaxW + 2 * kAfterP;
__device__ __forceinline__ void stage_env_columns(uint32_t *L, const KParams &p, int64_t e, int lane) {
    if (lane < p.W + 2 * kAfterP) {
        const int c = lane - kAfterP;
        L[lane] = c >= 0 && c < p.W ? p.board[c * p.stride + e] | ~((1u << p.H) - 1u) : ~0u;
    }
}

// The piece word a committed slot gets (st_place; st_afterstates.hip, "placement step"): rotation rot, anchor
// (x, 0), lock counter lock_mod - 1.
__device__ __forceinline__ uint32_t placed_piece(int id, int rot, int x, int lock_mod) {
    return (uint32_t)id | (uint32_t)rot << 3 | (uint32_t)x << 5 | (uint32_t)(lock_mod - 1) << 17;  // anchor row 0
}

// ---------------------------------------------------------------- score, reductions
// The linear players' score (st_policy_linear; st_afterstates.hip, "linear feature player"):
// score = the float32 chain acc = acc + w[r] * (float)feat[r] over the rows
// of st_after_feat in enum order from acc = 0, every product and every sum
// rounded on its own.  No compiler flag can fuse the chain: lin_score passes
// every product through an empty asm statement before it is added, so the
// multiply and the add never meet in one expression the backend could
// contract (-ffp-contract=fast on the command line included, which overrides
// a `#pragma clang fp contract(off)`; __fmul_rn / __fadd_rn are plain * and +
// in this toolchain's headers and would contract too).  The statement emits
// no instruction.
template <int NF>
__device__ __forceinline__ float lin_score(const float (&w)[NF], const int32_t (&f)[NF]) {
#pragma clang fp contract(off)
    float acc = 0.0f;
#pragma unroll
    for (int r = 0; r < NF; ++r) {
        float prod = w[r] * (float)f[r];
        asm volatile("" : "+v"(prod));  // the rounded product, opaque to the add below
        acc = acc + prod;
    }
    return acc;
}

// op over the 64 lanes of a wave whose lanes are all active, in every lane:
// within each row of 16 by quad permutes and row rotations, then row_bcast:15
// into rows 1 and 3 and row_bcast:31 into rows 2 and 3 (gfx9 DPP), which leaves
// the result in lane 63.  A lane the controls do not write keeps its own value
// (old = x), and op(x, x) = x for the max / min this is used with.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ int dpp_from(int x) {
    return __builtin_amdgcn_update_dpp(x, x, CTRL, ROW_MASK, 0xF, false);
}
template <class Op>
__device__ __forceinline__ int wave_reduce(int x, Op op) {
    x = op(x, dpp_from<0xB1>(x));         // quad_perm:[1,0,3,2]
    x = op(x, dpp_from<0x4E>(x));         // quad_perm:[2,3,0,1]
    x = op(x, dpp_from<0x124>(x));        // row_ror:4
    x = op(x, dpp_from<0x128>(x));        // row_ror:8
    x = op(x, dpp_from<0x142, 0xA>(x));   // row_bcast:15 into rows 1, 3
    x = op(x, dpp_from<0x143, 0xC>(x));   // row_bcast:31 into rows 2, 3
    return __builtin_amdgcn_readlane(x, kWave - 1);
}

template <bool FIRST>
struct PassTag {
    static constexpr bool value = FIRST;
};

#ifndef ST_POLICY_WAVES
#define ST_POLICY_WAVES 4  // envs (waves) per workgroup: the block-shape A/B, DESIGN "Linear feature player"
#endif

// the two-ply kernels' shape (k_policy_lookahead, k_policy_expect): one first-ply
// slot per thread, the afterstate boards B1[s1][] in LDS at an odd row pitch
constexpr int kLaWaves = 4;
constexpr int kLaSlots = 4 * (kMaxW + 6);
static_assert(kLaSlots <= kLaWaves * kWave, "one first-ply slot per thread");
__host__ __device__ constexpr int la_pitch(int W) { return (W + 2 * kAfterP) | 1; }

}  // namespace
}  // namespace st
