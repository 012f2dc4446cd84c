// st_ntuple.hip -- k_ntuple_eval and k_policy_ntuple (st_ntuple_eval,
// st_policy_ntuple, st_play_ntuple: an n-tuple network as the afterstate value
// of every placement slot) as a translation unit of their own.  Entry points:
// launch_ntuple_eval, launch_policy_ntuple.  They use the evaluator
// (eval_slot_set), the chain (lin_score) and the reductions of st_eval.h and
// are compiled apart from every other kernel so that every other code object
// stays exactly as it was (st_kernels.hip, top).
#define ST_SIDE_TU 1
#include "st_kernels.hip"
#include "st_eval.h"

namespace st {
namespace {

// ---------------------------------------------------------------- n-tuple network
// simpletetris.h, "N-tuple network".  A tuple's six words (x, y, w, h, flip,
// base) are wave-uniform: every lane walks the same tuple at the same time, on
// a board of its own.  st_ntuple_set has validated them against W, H, so
// col(c) is asked for c in [0, W) only and base + idx < table_len.
//
// base_t + idx_t: column i of the window (mirrored under flip) contributes its
// h bits from row y at bit i * h.
template <class Col>
__device__ __forceinline__ int32_t tuple_index(const int32_t *__restrict__ d, Col col) {
    const int x = d[0], y = d[1], w = d[2], h = d[3], flip = d[4];
    const uint32_t hm = (1u << h) - 1u;
    const int c0 = flip ? x + w - 1 : x, dc = flip ? -1 : 1;
    uint32_t idx = 0;
    for (int i = 0; i < w; ++i) idx |= ((col(c0 + dc * i) >> y) & hm) << (i * h);
    return d[5] + (int32_t)idx;
}

// N(B): acc = acc + table[base_t + idx_t(B)] over the tuples in order from
// 0.0f, every add rounded on its own (nothing here can be contracted; the
// pragma keeps the unit's rule visible).
template <class Col>
__device__ __forceinline__ float ntuple_value(const int32_t *__restrict__ desc, int T, const float *__restrict__ table,
                                              Col col) {
#pragma clang fp contract(off)
    float acc = 0.0f;
    for (int t = 0; t < T; ++t) acc = acc + table[tuple_index(desc + 6 * t, col)];
    return acc;
}

// st_ntuple_eval: one lane per board; boards uint32 [W][pitch], board b at
// column stride `pitch` (m for caller boards, the state's stride for the
// context's own).  A tuple's w <= 16 column words are loaded as it is walked,
// coalesced across the lanes; values float [m] and index int32 [T][m], either
// null.
__global__ __launch_bounds__(256) void k_ntuple_eval(const int32_t *__restrict__ desc, int T,
                                                     const float *__restrict__ table,
                                                     const uint32_t *__restrict__ boards, int64_t pitch, int64_t m,
                                                     float *__restrict__ values, int32_t *__restrict__ index) {
#pragma clang fp contract(off)
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= m) return;
    const uint32_t *mine = boards + b;
    float acc = 0.0f;
    for (int t = 0; t < T; ++t) {
        const int32_t at = tuple_index(desc + 6 * t, [&](int c) { return mine[(int64_t)c * pitch]; });
        if (index) index[(int64_t)t * m + b] = at;
        if (values) acc = acc + table[at];
    }
    if (values) values[b] = acc;
}

// st_policy_ntuple: k_policy_linear_set's shape -- one wave per env, WAVES envs
// per workgroup, lane = slot, ceil(S / 64) passes, no workgroup barrier, the
// same two wave_reduces, the winning lane writes -- with the network behind the
// chain.  A lane cannot index up to 32 column words in registers without
// scratch, so eval_slot_set's col_out stores the slot's afterstate board to the
// lane's own row of the wave's LDS slice rows[64][la_pitch(W)] (the odd pitch
// k_policy_lookahead keeps B1[s1][] at: lanes on distinct banks), rewritten
// every pass; the tuple walk reads it back, w reads, one gather and one add
// per tuple.  Lanes whose slot is no candidate or is dead skip the walk (the
// loop bound is wave-uniform, the skip is a divergent branch around it).
// index (int32 [T][n], base_t + idx_t of the chosen slot's board): after the
// reduction the whole wave shares the work, lane l taking tuples l, l + 64, ...
// on the winner's row, which every lane reads at one address (a broadcast).
// With one pass the winner's row still holds its board.  With more, it holds
// the lane's last slot, so where the winner is of an earlier pass the wave
// evaluates that one slot again (wave-uniform) and lane 0 stores its columns to
// row 0 -- this costs a slot evaluation for such envs when index is asked for,
// and saves the second LDS row per lane a kept copy of the best board needs
// (at 32 columns the two would not fit four waves into 64 KiB).
template <int WAVES, bool COMMIT, int SET>
__global__ __launch_bounds__(WAVES *kWave) void k_policy_ntuple(
    KParams p, const float *__restrict__ wts, int64_t n_w, const int32_t *__restrict__ desc, int T,
    const float *__restrict__ table, float dead_value, const int32_t *__restrict__ allowed,
    int32_t *__restrict__ slots, uint8_t *__restrict__ actions, float *__restrict__ scores,
    float *__restrict__ values, int32_t *__restrict__ best, int32_t *__restrict__ index,
    float *__restrict__ values_all) {
#pragma clang fp contract(off)
    __shared__ uint32_t Lall[WAVES * kAfterCols];
    extern __shared__ uint32_t Rall[];  // [WAVES][kWave][la_pitch(W)]
    constexpr int NF = feat_rows(SET);
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t e = (int64_t)blockIdx.x * WAVES + wave;
    if (e >= p.n) return;  // (wave-uniform; the kernel has no workgroup barrier)
    uint32_t *L = Lall + wave * kAfterCols;
    const int64_t sd = p.stride;
    const int W = p.W, H = p.H;
    const int per = W + 6, S = 4 * per, pitch = la_pitch(W);
    uint32_t *rows = Rall + wave * (kWave * pitch);
    uint32_t *row = rows + lane * pitch;
    stage_env_columns(L, p, e, lane);
    const uint32_t pw = p.piece[e];
    const uint32_t pid = pw & 7u;
    const int id = (int)(pid < 7u ? pid : 6u);  // (a host-written id 7 stays inside the table)
    const int32_t old_holes = p.stats[ST_STAT_HOLES * sd + e];
    const int32_t old_height = p.stats[ST_STAT_PIECE_HEIGHT * sd + e];
    float w[NF];
    if (wts) {
        // e < 2^24 (st_create), so the row index is 32-bit arithmetic
        const uint32_t wrow = n_w > e ? (uint32_t)e : (uint32_t)e % (uint32_t)n_w;
#pragma unroll
        for (int r = 0; r < NF; ++r) w[r] = wts[(size_t)wrow * NF + r];
    } else {
#pragma unroll
        for (int r = 0; r < NF; ++r) w[r] = 0.0f;
    }
    wave_sync();
    // the lane's candidate: its best slot so far (-1: none), that slot's score, value, death and rows
    int32_t bslot;
    float bscore, bval;
    bool bdead;
    int32_t bf[NF];
    auto pass = [&](int s0, auto first) {
        const int s = s0 + lane;
        const bool live = s < S;
        int32_t f[NF];
        bool valid = eval_slot_set<SET>(L + kAfterP, W, H, p.flags, id, live ? s : S - 1, old_holes, old_height, f,
                                        [&](int c, uint32_t cw, bool) { row[c] = cw; });
        valid = valid && live;
        // (a slot the mask refuses is no candidate: from here on, as if invalid)
        if (allowed) valid = valid && allowed[(size_t)e * S + s] != 0;
        const bool dead = f[ST_AFTER_DEAD] != 0;
        float v = dead_value;
        if (valid && !dead) v = ntuple_value(desc, T, table, [&](int c) { return row[c]; });
        if (live && values_all) values_all[(size_t)e * S + s] = valid ? v : 0.0f;
        const float s1 = wts ? lin_score(w, f) : 0.0f;
        const float sc = s1 + v;
        if constexpr (decltype(first)::value) {  // (score, value and rows are read only where bslot >= 0)
            bslot = valid ? s : -1;
            bscore = sc;
            bval = v;
            bdead = dead;
#pragma unroll
            for (int r = 0; r < NF; ++r) bf[r] = f[r];
        } else if (valid && (bslot < 0 || sc > bscore)) {
            bslot = s;
            bscore = sc;
            bval = v;
            bdead = dead;
#pragma unroll
            for (int r = 0; r < NF; ++r) bf[r] = f[r];
        }
    };
    pass(0, PassTag<true>{});
    for (int s0 = kWave; s0 < S; s0 += kWave) pass(s0, PassTag<false>{});
    // k_policy_linear_set's reductions: the wave's maximum over the candidates,
    // then the lowest slot that reaches it; a NaN score equals nothing, and then
    // every candidate counts as reaching it, so that the slot stays a valid one.
    const bool has = bslot >= 0;
    const float top = __int_as_float(wave_reduce(__float_as_int(has ? bscore : -__builtin_inff()), [](int a, int b) {
        return __float_as_int(__builtin_fmaxf(__int_as_float(a), __int_as_float(b)));
    }));
    bool tied = has && bscore == top;
    if (__ballot(tied) == 0) tied = has;
    const int32_t win = wave_reduce(tied ? bslot : INT32_MAX, [](int a, int b) { return a < b ? a : b; });
    const bool none = win == INT32_MAX;  // no candidate: lane 0 writes slot -1, action 2, score 0, value 0, zero rows
    const bool winner = none ? lane == 0 : tied && bslot == win;
    if (winner) {
        if (slots) slots[e] = none ? -1 : win;
        if (scores) scores[e] = none ? 0.0f : bscore;
        if (values) values[e] = none ? 0.0f : bval;
        if (actions) {
            const int rot = (int)((pw >> 3) & 3u), ax = (int)((pw >> 5) & 63u);
            const int trot = (win >= per) + (win >= 2 * per) + (win >= 3 * per), tx = win - trot * per - 3;
            // k_placement_actions's rule
            actions[e] = (uint8_t)(none ? 2u : rot != trot ? 4u : (ax < tx ? 1u : (ax > tx ? 0u : 2u)));
        }
        if (best) {
#pragma unroll
            for (int r = 0; r < NF; ++r) best[(size_t)r * p.n + e] = none ? 0 : bf[r];
        }
        if constexpr (COMMIT) {
            if (!none) {
                const int trot = (win >= per) + (win >= 2 * per) + (win >= 3 * per), tx = win - trot * per - 3;
                p.piece[e] = placed_piece(id, trot, tx, p.lock_mod);
            }
        }
    }
    if (index) {
        // (exactly one lane is the winner; its death is the wave's)
        const bool skip = none || __ballot(winner && bdead) != 0;  // nothing was read from the table: -1 rows
        int wl = 0;
        if (!skip) {
            const int last0 = (S - 1) & ~(kWave - 1);  // the last pass's first slot
            if (win >= last0 || S <= kWave) {
                wl = win & (kWave - 1);  // the winner's row still holds its board
            } else {
                wave_sync();  // (every lane's walk of its row is over before row 0 is rewritten)
                int32_t f[NF];
                eval_slot_set<SET>(L + kAfterP, W, H, p.flags, id, win, old_holes, old_height, f,
                                   [&](int c, uint32_t cw, bool) {
                                       if (lane == 0) rows[c] = cw;
                                   });
            }
            wave_sync();
        }
        const uint32_t *wrow_ = rows + wl * pitch;
        for (int t = lane; t < T; t += kWave)
            index[(size_t)t * p.n + e] = skip ? -1 : tuple_index(desc + 6 * t, [&](int c) { return wrow_[c]; });
    }
}

}  // namespace

hipError_t launch_ntuple_eval(const int32_t *desc, int T, const float *table, const uint32_t *boards, int64_t pitch,
                              int64_t m, float *values, int32_t *index, hipStream_t s) {
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ntuple_eval, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, desc, T, table, boards, pitch,
                       m, values, index);
    return hipGetLastError();
}

hipError_t launch_policy_ntuple(const KParams &p, int set, bool commit, const float *weights, int64_t n_w,
                                const int32_t *desc, int T, const float *table, float dead_value,
                                const int32_t *allowed, int32_t *slots, uint8_t *actions, float *scores, float *values,
                                int32_t *best, int32_t *index, float *values_all, hipStream_t s) {
    if (set != ST_FEATS_BASE && set != ST_FEATS_BCTS) return hipErrorInvalidValue;
    constexpr int WV = ST_POLICY_WAVES;
    const dim3 grid((unsigned)((p.n + WV - 1) / WV)), block(WV * kWave);
    const size_t lds = sizeof(uint32_t) * (size_t)WV * kWave * (size_t)la_pitch(p.W);
#define ST_NT_ARGS \
    p, weights, n_w, desc, T, table, dead_value, allowed, slots, actions, scores, values, best, index, values_all
    if (set == ST_FEATS_BCTS && commit)
        hipLaunchKernelGGL((k_policy_ntuple<WV, true, ST_FEATS_BCTS>), grid, block, lds, s, ST_NT_ARGS);
    else if (set == ST_FEATS_BCTS)
        hipLaunchKernelGGL((k_policy_ntuple<WV, false, ST_FEATS_BCTS>), grid, block, lds, s, ST_NT_ARGS);
    else if (commit)
        hipLaunchKernelGGL((k_policy_ntuple<WV, true, ST_FEATS_BASE>), grid, block, lds, s, ST_NT_ARGS);
    else
        hipLaunchKernelGGL((k_policy_ntuple<WV, false, ST_FEATS_BASE>), grid, block, lds, s, ST_NT_ARGS);
#undef ST_NT_ARGS
    return hipGetLastError();
}

}  // namespace st
