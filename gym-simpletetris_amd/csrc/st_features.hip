// st_features.hip -- k_afterstates_set and k_policy_linear_set
// (st_afterstates_set, st_policy_linear_set, st_play_linear_set: the
// ST_FEATS_BCTS rows, and the slot mask) as a translation unit of their own.
// Entry points: launch_afterstates_set, launch_policy_linear_set.  Their
// evaluator eval_slot_set is in st_eval.h; they are compiled apart from the
// afterstates module so that the code objects of k_afterstates and
// k_policy_linear stay exactly as they were (st_kernels.hip, top).
#define ST_SIDE_TU 1
#include "st_kernels.hip"
#include "st_eval.h"

namespace st {
namespace {

// k_afterstates with the rows of SET: feat [n][feat_rows(SET)][S]
template <int SET>
__global__ __launch_bounds__(kWave) void k_afterstates_set(KParams p, int32_t *__restrict__ feat,
                                                           uint32_t *__restrict__ boards) {
    constexpr int NF = feat_rows(SET);
    __shared__ uint32_t L[kAfterCols];
    const int lane = threadIdx.x;
    const int64_t e = blockIdx.x;  // the grid is p.n waves: padding envs are not evaluated
    const int64_t sd = p.stride;
    const int W = p.W, H = p.H;
    const int S = 4 * (W + 6);
    stage_env_columns(L, p, e, lane);
    const uint32_t pid = p.piece[e] & 7u;
    const int id = (int)(pid < 7u ? pid : 6u);  // (a host-written id 7 stays inside the table)
    const int32_t old_holes = p.stats[ST_STAT_HOLES * sd + e];
    const int32_t old_height = p.stats[ST_STAT_PIECE_HEIGHT * sd + e];
    wave_sync();
    const size_t fbase = (size_t)e * NF * S, bbase = (size_t)e * W * S;
    for (int s0 = 0; s0 < S; s0 += kWave) {
        const int s = s0 + lane;
        const bool live = s < S;
        const int sc = live ? s : S - 1;  // (lanes past the last slot compute it again, store nothing)
        int32_t f[NF];
        const bool valid = eval_slot_set<SET>(L + kAfterP, W, H, p.flags, id, sc, old_holes, old_height, f,
                                          [&](int c, uint32_t w, bool ok) {
                                              if (boards && live) boards[bbase + (size_t)c * S + s] = ok ? w : 0u;
                                          });
        if (live) {
#pragma unroll
            for (int row = 0; row < NF; ++row) feat[fbase + (size_t)row * S + s] = valid ? f[row] : 0;
        }
    }
}

// k_policy_linear over the rows of SET (weights [n_w][NF], best [NF][n]) and
// with a slot mask: allowed int32 [n][S] or null; a slot is a candidate iff it
// is valid and its word is not 0.
template <int WAVES, bool COMMIT, int SET>
__global__ __launch_bounds__(WAVES *kWave) void k_policy_linear_set(KParams p, const float *__restrict__ wts,
                                                                    int64_t n_w, const int32_t *__restrict__ allowed,
                                                                    int32_t *__restrict__ slots,
                                                                    uint8_t *__restrict__ actions,
                                                                    float *__restrict__ scores,
                                                                    int32_t *__restrict__ best) {
    __shared__ uint32_t Lall[WAVES * kAfterCols];
    constexpr int NF = feat_rows(SET);
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t e = (int64_t)blockIdx.x * WAVES + wave;
    if (e >= p.n) return;  // (wave-uniform; the kernel has no workgroup barrier)
    uint32_t *L = Lall + wave * kAfterCols;
    const int64_t sd = p.stride;
    const int W = p.W, H = p.H;
    const int per = W + 6, S = 4 * per;
    stage_env_columns(L, p, e, lane);
    const uint32_t pw = p.piece[e];
    const uint32_t pid = pw & 7u;
    const int id = (int)(pid < 7u ? pid : 6u);  // (a host-written id 7 stays inside the table)
    const int32_t old_holes = p.stats[ST_STAT_HOLES * sd + e];
    const int32_t old_height = p.stats[ST_STAT_PIECE_HEIGHT * sd + e];
    // e < 2^24 (st_create), so the row index is 32-bit arithmetic
    const uint32_t wrow = n_w > e ? (uint32_t)e : (uint32_t)e % (uint32_t)n_w;
    float w[NF];
#pragma unroll
    for (int r = 0; r < NF; ++r) w[r] = wts[(size_t)wrow * NF + r];
    wave_sync();
    // the lane's candidate: its best slot so far (-1: none), that slot's score and rows
    int32_t bslot;
    float bscore;
    int32_t bf[NF];
    auto pass = [&](int s0, auto first) {
        const int s = s0 + lane;
        const bool live = s < S;
        int32_t f[NF];
        bool valid = eval_slot_set<SET>(L + kAfterP, W, H, p.flags, id, live ? s : S - 1, old_holes, old_height, f,
                                    [](int, uint32_t, bool) {});
        // (a slot the mask refuses is no candidate: from here on, as if invalid)
        if (allowed) valid = valid && live && allowed[(size_t)e * S + s] != 0;
        const float sc = lin_score(w, f);
        if constexpr (decltype(first)::value) {  // (score and rows are read only where bslot >= 0)
            bslot = live && valid ? s : -1;
            bscore = sc;
#pragma unroll
            for (int r = 0; r < NF; ++r) bf[r] = f[r];
        } else if (live && valid && (bslot < 0 || sc > bscore)) {
            bslot = s;
            bscore = sc;
#pragma unroll
            for (int r = 0; r < NF; ++r) bf[r] = f[r];
        }
    };
    pass(0, PassTag<true>{});
    for (int s0 = kWave; s0 < S; s0 += kWave) pass(s0, PassTag<false>{});
    // the wave's maximum over the candidates, then the lowest slot that reaches
    // it.  With finite weights some candidate equals the maximum; a NaN score
    // equals nothing, and then every candidate counts as reaching it, so that
    // the slot stays a valid one.
    const bool has = bslot >= 0;
    const float top = __int_as_float(wave_reduce(__float_as_int(has ? bscore : -__builtin_inff()), [](int a, int b) {
        return __float_as_int(__builtin_fmaxf(__int_as_float(a), __int_as_float(b)));
    }));
    bool tied = has && bscore == top;
    if (__ballot(tied) == 0) tied = has;
    const int32_t win = wave_reduce(tied ? bslot : INT32_MAX, [](int a, int b) { return a < b ? a : b; });
    const bool none = win == INT32_MAX;  // no valid slot: lane 0 writes slot -1, action 2, score 0, zero rows
    if (none ? lane == 0 : tied && bslot == win) {
        if (slots) slots[e] = none ? -1 : win;
        if (scores) scores[e] = none ? 0.0f : bscore;
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
}

}  // namespace

hipError_t launch_afterstates_set(const KParams &p, int set, int32_t *feat, uint32_t *boards, hipStream_t s) {
    if (set != ST_FEATS_BCTS) return hipErrorInvalidValue;  // (the base set is launch_afterstates)
    hipLaunchKernelGGL((k_afterstates_set<ST_FEATS_BCTS>), dim3((unsigned)p.n), dim3(kWave), 0, s, p, feat, boards);
    return hipGetLastError();
}

hipError_t launch_policy_linear_set(const KParams &p, int set, bool commit, const float *weights, int64_t n_w,
                                    const int32_t *allowed, int32_t *slots, uint8_t *actions, float *scores,
                                    int32_t *best, hipStream_t s) {
    constexpr int WV = ST_POLICY_WAVES;
    const dim3 grid((unsigned)((p.n + WV - 1) / WV)), block(WV * kWave);
#define ST_PL_ARGS p, weights, n_w, allowed, slots, actions, scores, best
    if (set == ST_FEATS_BCTS && commit)
        hipLaunchKernelGGL((k_policy_linear_set<WV, true, ST_FEATS_BCTS>), grid, block, 0, s, ST_PL_ARGS);
    else if (set == ST_FEATS_BCTS)
        hipLaunchKernelGGL((k_policy_linear_set<WV, false, ST_FEATS_BCTS>), grid, block, 0, s, ST_PL_ARGS);
    else if (set == ST_FEATS_BASE && !commit)  // (the base set without a mask is launch_policy_linear)
        hipLaunchKernelGGL((k_policy_linear_set<WV, false, ST_FEATS_BASE>), grid, block, 0, s, ST_PL_ARGS);
    else
        return hipErrorInvalidValue;
#undef ST_PL_ARGS
    return hipGetLastError();
}

}  // namespace st
