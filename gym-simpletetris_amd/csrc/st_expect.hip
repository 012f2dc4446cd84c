// st_expect.hip -- k_next_weights and k_policy_expect (st_next_weights,
// st_policy_expect, st_play_expect: the odds of the next piece as an output,
// and the expectimax player over them) as a translation unit of their own.
// Entry points: launch_next_weights, launch_policy_expect.  They use the
// evaluator (eval_slot_set), the chain (lin_score) and the reductions of
// st_eval.h and are compiled apart from every other kernel so that every other
// code object stays exactly as it was (st_kernels.hip, top).
#define ST_SIDE_TU 1
#include "st_kernels.hip"
#include "st_eval.h"

namespace st {
namespace {

// ---------------------------------------------------------------- piece odds, expectimax player
// st_next_weights: m of _choose_shape (tetris_env.py:186) from the counter rows
// of the moment, m[i] = 5 + max(counts) - counts[i] -- the odds of the piece the
// env's next _new_piece takes (shape_counts changes only at a spawn and clear()
// keeps it: k_next_piece's argument).  The MT row is not read.  Unsigned
// arithmetic: host-written counts of any size wrap, they do not trap.
__device__ __forceinline__ void next_odds(const int32_t (&cnt)[7], uint32_t (&m)[7]) {
    int32_t maxc = cnt[0];
#pragma unroll
    for (int i = 1; i < 7; ++i) maxc = cnt[i] > maxc ? cnt[i] : maxc;
#pragma unroll
    for (int i = 0; i < 7; ++i) m[i] = 5u + (uint32_t)maxc - (uint32_t)cnt[i];
}

// One lane per env; out int32 [7][n], env innermost.
__global__ __launch_bounds__(256) void k_next_weights(KParams p, int32_t *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.n) return;
    int32_t cnt[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) cnt[i] = p.stats[(ST_STAT_COUNT0 + i) * p.stride + e];
    uint32_t m[7];
    next_odds(cnt, m);
#pragma unroll
    for (int i = 0; i < 7; ++i) out[(int64_t)i * p.n + e] = (int32_t)m[i];
}

// E(s1) of st_policy_expect: acc = acc + (float)m[q] * T[q] over q = 0..6 from
// 0.0f, then acc / (float)M, every product, every sum and the division rounded
// on their own -- lin_score's precautions for the products; `/` is the
// correctly rounded division under the project's flags (v_div_scale /
// v_div_fmas / v_div_fixup in the code object; DESIGN.md "Expectimax player").
__device__ __forceinline__ float expect_chain(const uint32_t (&m)[7], uint32_t M, const float (&T)[7]) {
#pragma clang fp contract(off)
    float acc = 0.0f;
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        float prod = (float)m[q] * T[q];
        asm volatile("" : "+v"(prod));  // the rounded product, opaque to the add below
        acc = acc + prod;
    }
    float e = acc / (float)M;
    asm volatile("" : "+v"(e));  // the rounded quotient, opaque to the caller's add
    return e;
}

// st_policy_expect: the two-ply player over the odds of the next piece
// (simpletetris.h, "Expectimax player").  k_policy_lookahead's shape -- one
// workgroup of kLaWaves waves per env, the same staging, the same first ply
// with thread = s1 and B1[s1][] in LDS, the same live ballots -- with these
// differences:
//  - no preview is read: the seven counter rows give m (next_odds);
//  - second ply: the tasks are the pairs (live s1, q), q = 0..6, numbered
//    7 * k + q for the k-th live s1 in slot order and taken round-robin by the
//    waves (task i goes to wave i % kLaWaves); lane = s2, ceil(S / 64) passes of
//    eval_slot_set on B1[s1] with piece q (wave-uniform) and X(s1)'s counters,
//    lin_score, the two wave_reduces: T_q(s1) and its lowest s2 to sT / sSl2,
//    [7][kLaSlots] each;
//  - choose: after the barrier thread t reads its seven tails (dead_value where
//    s1 is dead or a piece has no valid s2), writes its table entries, runs
//    expect_chain and adds S1; the rest is k_policy_lookahead's.
template <int SET, bool COMMIT>
__global__ __launch_bounds__(kLaWaves *kWave) void k_policy_expect(
    KParams p, const float *__restrict__ wts1, const float *__restrict__ wts2, int64_t n_w, float dead_value,
    const int32_t *__restrict__ allowed, int32_t *__restrict__ slots, uint8_t *__restrict__ actions,
    float *__restrict__ scores, float *__restrict__ scores_all, float *__restrict__ tails,
    int32_t *__restrict__ slots2_all) {
    constexpr int NF = feat_rows(SET);
    // (the output pointers wait in vector registers for the last phase, as in k_policy_lookahead)
    asm volatile("" : "+v"(slots), "+v"(actions), "+v"(scores), "+v"(scores_all), "+v"(tails), "+v"(slots2_all));
    extern __shared__ uint32_t B1[];  // [S][la_pitch(W)]
    __shared__ uint32_t L[kAfterCols];
    __shared__ int32_t sHoles[kLaSlots], sHeight[kLaSlots], sSl2[7][kLaSlots];
    __shared__ float sT[7][kLaSlots];
    __shared__ uint32_t sLive[kLaWaves][2];
    __shared__ float sTop[kLaWaves];
    __shared__ int32_t sWin[kLaWaves];
    const int t = threadIdx.x, lane = t & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t e = blockIdx.x;  // the grid is p.n workgroups: padding envs are not evaluated
    const int64_t sd = p.stride;
    const int W = p.W, H = p.H;
    const int per = W + 6, S = 4 * per, pitch = la_pitch(W);
    const uint32_t floorb = ~((1u << H) - 1u);
    stage_env_columns(L, p, e, t);
    const uint32_t pw = p.piece[e];
    const uint32_t pid = pw & 7u;
    const int id = (int)(pid < 7u ? pid : 6u);  // (a host-written id 7 stays inside the table)
    const int32_t old_holes = p.stats[ST_STAT_HOLES * sd + e];
    const int32_t old_height = p.stats[ST_STAT_PIECE_HEIGHT * sd + e];
    // e < 2^24 (st_create), so the row index is 32-bit arithmetic
    const uint32_t wrow = n_w > e ? (uint32_t)e : (uint32_t)e % (uint32_t)n_w;
    __syncthreads();

    // ---- first ply: s1 = t (k_policy_lookahead's) ----
    const bool active = wave * kWave < S;  // (wave-uniform)
    bool cand = false, dead1 = false;
    float s1score = 0.0f;
    if (active) {
        const bool live = t < S;
        const int s1 = live ? t : S - 1;  // (threads past the last slot compute it again, store nothing)
        uint32_t *row = B1 + s1 * pitch;
        if (live) {
#pragma unroll
            for (int j = 0; j < kAfterP; ++j) row[j] = row[kAfterP + W + j] = ~0u;
        }
        int32_t f[NF];
        uint32_t orv = 0;
        const bool valid = eval_slot_set<SET>(L + kAfterP, W, H, p.flags, id, s1, old_holes, old_height, f,
                                              [&](int c, uint32_t w, bool) {
                                                  orv |= w;
                                                  if (live) row[kAfterP + c] = w | floorb;
                                              });
        cand = live && valid && (!allowed || allowed[(size_t)e * S + s1] != 0);
        // the counters the lock of s1 leaves (:283-297): lock_score's, on the slot's rows
        int32_t rew = 0, score = 0, lines = 0, holes1 = old_holes, height1 = old_height, deaths = 0;
        const int32_t fholes = f[ST_AFTER_HOLES];
        const LockRes lr = lock_score<false>(p.flags, f[ST_AFTER_LINES], orv, [fholes] { return fholes; }, old_holes,
                                             old_height, rew, score, lines, holes1, height1, deaths);
        dead1 = lr.died;
        if (wts1) {
            float w[NF];
#pragma unroll
            for (int r = 0; r < NF; ++r) {
                w[r] = wts1[(size_t)wrow * NF + r];
                asm volatile("" : "+v"(w[r]));  // in vector registers: the row is wave-uniform, and as scalars it spills
            }
            s1score = lin_score(w, f);
        }
        if (live) {
            sHoles[s1] = holes1;
            sHeight[s1] = height1;
        }
        const uint64_t lm = __ballot(cand && !dead1);
        if (lane == 0) {
            sLive[wave][0] = (uint32_t)lm;
            sLive[wave][1] = (uint32_t)(lm >> 32);
        }
    } else if (lane == 0) {
        sLive[wave][0] = sLive[wave][1] = 0u;
    }
    __syncthreads();

    // ---- second ply: the tasks (live s1, q), round-robin over the waves; lane = s2 ----
    {
        float w[NF];
#pragma unroll
        for (int r = 0; r < NF; ++r) {
            w[r] = wts2[(size_t)wrow * NF + r];
            asm volatile("" : "+v"(w[r]));  // (as in the first ply)
        }
        int k = 0;
        for (int qw = 0; qw < kLaWaves; ++qw) {
            uint64_t lm = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)sLive[qw][0]) |
                          (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)sLive[qw][1]) << 32;
            for (; lm; lm &= lm - 1) {
                const int s1 = qw * kWave + (int)__builtin_ctzll(lm);
                const uint32_t *C = B1 + s1 * pitch + kAfterP;
                for (int q = 0; q < 7; ++q) {
                    if ((k++ & (kLaWaves - 1)) != wave) continue;
                    const int32_t h1 = sHoles[s1], g1 = sHeight[s1];
                    int32_t bslot;
                    float bscore;
                    auto pass = [&](int s0, auto first) {
                        const int s = s0 + lane;
                        const bool live = s < S;
                        int32_t f[NF];
                        const bool valid = eval_slot_set<SET>(C, W, H, p.flags, q, live ? s : S - 1, h1, g1, f,
                                                              [](int, uint32_t, bool) {});
                        const float sc = lin_score(w, f);
                        if constexpr (decltype(first)::value) {  // (the score is read only where bslot >= 0)
                            bslot = live && valid ? s : -1;
                            bscore = sc;
                        } else if (live && valid && (bslot < 0 || sc > bscore)) {
                            bslot = s;
                            bscore = sc;
                        }
                    };
                    pass(0, PassTag<true>{});
                    for (int s0 = kWave; s0 < S; s0 += kWave) pass(s0, PassTag<false>{});
                    // k_policy_linear_set's reductions: the maximum, then the lowest slot that reaches it
                    const bool has = bslot >= 0;
                    const float top =
                        __int_as_float(wave_reduce(__float_as_int(has ? bscore : -__builtin_inff()), [](int a, int b) {
                            return __float_as_int(__builtin_fmaxf(__int_as_float(a), __int_as_float(b)));
                        }));
                    bool tied = has && bscore == top;
                    if (__ballot(tied) == 0) tied = has;
                    const int32_t win =
                        wave_reduce(tied ? bslot : INT32_MAX, [](int a, int b) { return a < b ? a : b; });
                    if (lane == 0) {
                        sT[q][s1] = top;
                        sSl2[q][s1] = win == INT32_MAX ? -1 : win;
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- choose ----
    if (active) {
        const bool live = t < S, open = cand && !dead1;
        const int ti = live ? t : 0;
        int32_t cnt[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) cnt[q] = p.stats[(ST_STAT_COUNT0 + q) * sd + e];
        uint32_t m[7], M = 0;
        next_odds(cnt, m);
#pragma unroll
        for (int q = 0; q < 7; ++q) M += m[q];
        float T[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            const int32_t sl2 = open ? sSl2[q][ti] : -1;
            T[q] = sl2 >= 0 ? sT[q][ti] : dead_value;
            if (live) {
                if (tails) tails[((size_t)e * 7 + q) * S + t] = cand ? T[q] : 0.0f;
                if (slots2_all) slots2_all[((size_t)e * 7 + q) * S + t] = cand ? sl2 : -1;
            }
        }
        const float tot = s1score + expect_chain(m, M, T);
        if (live && scores_all) scores_all[(size_t)e * S + t] = cand ? tot : 0.0f;
        const float top = __int_as_float(wave_reduce(__float_as_int(cand ? tot : -__builtin_inff()), [](int a, int b) {
            return __float_as_int(__builtin_fmaxf(__int_as_float(a), __int_as_float(b)));
        }));
        bool tied = cand && tot == top;
        if (__ballot(tied) == 0) tied = cand;
        const int32_t win = wave_reduce(tied ? t : INT32_MAX, [](int a, int b) { return a < b ? a : b; });
        if (win == INT32_MAX ? lane == 0 : tied && t == win) {
            sWin[wave] = win == INT32_MAX ? -1 : win;
            sTop[wave] = tot;
        }
    } else if (lane == 0) {
        sWin[wave] = -1;
    }
    __syncthreads();
    if (t == 0) {
        int32_t win = -1;
        float top = 0.0f;
        for (int q = 0; q < kLaWaves; ++q) {  // the first wave with the largest score: ties to the lowest s1
            if (sWin[q] >= 0 && (win < 0 || sTop[q] > top)) {
                win = sWin[q];
                top = sTop[q];
            }
        }
        const bool none = win < 0;
        const int trot = (win >= per) + (win >= 2 * per) + (win >= 3 * per), tx = win - trot * per - 3;
        if (slots) slots[e] = win;
        if (scores) scores[e] = none ? 0.0f : top;
        if (actions) {
            const int rot = (int)((pw >> 3) & 3u), ax = (int)((pw >> 5) & 63u);
            // k_placement_actions's rule
            actions[e] = (uint8_t)(none ? 2u : rot != trot ? 4u : (ax < tx ? 1u : (ax > tx ? 0u : 2u)));
        }
        if constexpr (COMMIT) {
            if (!none) p.piece[e] = placed_piece(id, trot, tx, p.lock_mod);
        }
    }
}

}  // namespace

hipError_t launch_next_weights(const KParams &p, int32_t *m, hipStream_t s) {
    hipLaunchKernelGGL(k_next_weights, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p, m);
    return hipGetLastError();
}

hipError_t launch_policy_expect(const KParams &p, int set, bool commit, const float *weights1, const float *weights2,
                                int64_t n_w, float dead_value, const int32_t *allowed, int32_t *slots,
                                uint8_t *actions, float *scores, float *scores_all, float *tails, int32_t *slots2_all,
                                hipStream_t s) {
    if (set != ST_FEATS_BASE && set != ST_FEATS_BCTS) return hipErrorInvalidValue;
    const dim3 grid((unsigned)p.n), block(kLaWaves * kWave);  // one workgroup per env
    const size_t lds = sizeof(uint32_t) * (size_t)(4 * (p.W + 6)) * (size_t)la_pitch(p.W);
#define ST_EX_ARGS p, weights1, weights2, n_w, dead_value, allowed, slots, actions, scores, scores_all, tails, slots2_all
    if (set == ST_FEATS_BCTS && commit)
        hipLaunchKernelGGL((k_policy_expect<ST_FEATS_BCTS, true>), grid, block, lds, s, ST_EX_ARGS);
    else if (set == ST_FEATS_BCTS)
        hipLaunchKernelGGL((k_policy_expect<ST_FEATS_BCTS, false>), grid, block, lds, s, ST_EX_ARGS);
    else if (commit)
        hipLaunchKernelGGL((k_policy_expect<ST_FEATS_BASE, true>), grid, block, lds, s, ST_EX_ARGS);
    else
        hipLaunchKernelGGL((k_policy_expect<ST_FEATS_BASE, false>), grid, block, lds, s, ST_EX_ARGS);
#undef ST_EX_ARGS
    return hipGetLastError();
}

}  // namespace st
