// st_lookahead.hip -- k_next_piece and k_policy_lookahead (st_next_piece,
// st_policy_lookahead, st_play_lookahead: the preview as an output, and the
// two-ply linear player) as a translation unit of their own.  Entry points:
// launch_next_piece, launch_policy_lookahead.  They use the evaluator
// (eval_slot_set, st_eval.h) and the core's draw (draw_shape, st_kernels.hip)
// and are compiled apart from every other kernel so that every other code
// object stays exactly as it was (st_kernels.hip, top).
#define ST_SIDE_TU 1
#include "st_kernels.hip"
#include "st_eval.h"

namespace st {
namespace {

// ---------------------------------------------------------------- next piece, two-ply player
// st_next_piece: the shape _choose_shape (tetris_env.py:183-191) would return
// for env e in its present state -- the piece its next _new_piece takes,
// behind a lock or a reset: shape_counts changes only at a spawn and clear()
// keeps it.  That is the preview (pv_id) where the MT word holds a valid one;
// an env without one (a lock of st_step's, a host-written or synced state)
// draws it here as st_step's prologue would -- k_reset's first draw: the counts
// of the moment, not counted -- and keeps it (pv_pack), so the next spawn does
// not draw again and st_mt_sync gives the words back.  One wave per 64 envs;
// next: uint8 [n] or null (the draw alone).
__global__ __launch_bounds__(kWave) void k_next_piece(KParams p, uint8_t *__restrict__ next) {
    __shared__ uint32_t S[kMtN];
    const int lane = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * kWave;
    const int64_t e = e0 + lane;
    const int64_t sd = p.stride;
    const bool real = e < p.n;
    int32_t *st = p.stats + e;  // (e < stride: the grid is stride / 64 waves)
    int32_t cnt[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) cnt[i] = st[(ST_STAT_COUNT0 + i) * sd];
    uint32_t mtst = (uint32_t)st[ST_STAT_MT_INDEX * sd];
    const uint32_t mt0 = mtst;
    int sid = pv_id(mt0);
    const bool need = real && !pv_ok(mt0);
    if (__ballot(need)) {
        const MtPre nopre{};
        const int pk = draw_shape<8, false>(need, cnt, mtst, p.mt + e0 * kMtPitch, S, lane, nopre, false);
        if (need) {
            sid = pk;
            st[ST_STAT_MT_INDEX * sd] = (int32_t)pv_pack(mtst, pk, mt_consumed(mt0, mtst));
        }
    }
    if (next && real) next[e] = (uint8_t)sid;
}

// st_policy_lookahead: the two-ply linear player (simpletetris.h, "Two-ply
// player").  One workgroup of kLaWaves waves per env.
//  1. stage: the env's column words (stage_env_columns), the piece, the
//     counters and the preview (k_next_piece ran before this kernel on the
//     stream: launch_policy_lookahead enqueues it).
//  2. first ply: thread t evaluates slot s1 = t (S <= 152 < 256: one pass over
//     the workgroup, waves past S idle) with eval_slot_set, whose col_out
//     writes the afterstate's columns into B1[s1][] -- W + 2 * kAfterP words,
//     floor bits, all-ones walls: the layout the evaluator reads -- at a row
//     pitch of (W + 16) | 1 words (odd: the lanes of a wave, one row each,
//     write one column to distinct banks).  It keeps S1, the candidate and dead
//     flags and X(s1)'s holes / piece_height: lock_score's outputs on the
//     slot's rows.
//  3. live list: each wave's ballot of (candidate, not dead) in LDS; barrier.
//  4. second ply: the waves walk the ballots in slot order and take the live
//     s1 round-robin (the k-th live slot goes to wave k % kLaWaves); lane = s2,
//     ceil(S / 64) passes of eval_slot_set on B1[s1] (broadcast reads) with the
//     next piece and X(s1)'s counters, lin_score with the second weight row,
//     k_policy_linear_set's two wave_reduces: M2 and its lowest s2 to LDS.
//  5. choose: after a barrier thread t adds T to S1 (one float32 add), writes
//     its table entries, and each wave reduces over its s1 the same way; after
//     a last barrier thread 0 takes the first wave with the largest score and
//     writes the env's outputs and, under COMMIT, the piece word (placed_piece).
template <int SET, bool COMMIT>
__global__ __launch_bounds__(kLaWaves *kWave) void k_policy_lookahead(
    KParams p, const float *__restrict__ wts1, const float *__restrict__ wts2, int64_t n_w, float dead_value,
    const int32_t *__restrict__ allowed, int32_t *__restrict__ slots, int32_t *__restrict__ slots2,
    uint8_t *__restrict__ actions, float *__restrict__ scores, float *__restrict__ scores_all,
    int32_t *__restrict__ slots2_all) {
    constexpr int NF = feat_rows(SET);
    // the output pointers wait in vector registers for the last phase: held as
    // scalars across both plies they pushed the kernel past the SGPR file
    asm volatile("" : "+v"(slots), "+v"(slots2), "+v"(actions), "+v"(scores), "+v"(scores_all), "+v"(slots2_all));
    extern __shared__ uint32_t B1[];  // [S][la_pitch(W)]
    __shared__ uint32_t L[kAfterCols];
    __shared__ int32_t sHoles[kLaSlots], sHeight[kLaSlots], sSl2[kLaSlots];
    __shared__ float sM2[kLaSlots];
    __shared__ uint32_t sLive[kLaWaves][2];
    __shared__ float sTop[kLaWaves];
    __shared__ int32_t sWin[kLaWaves], sWin2[kLaWaves];
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
    const int nraw = pv_id((uint32_t)p.stats[ST_STAT_MT_INDEX * sd + e]);
    const int nid = nraw < 7 ? nraw : 6;
    // e < 2^24 (st_create), so the row index is 32-bit arithmetic
    const uint32_t wrow = n_w > e ? (uint32_t)e : (uint32_t)e % (uint32_t)n_w;
    __syncthreads();

    // ---- first ply: s1 = t ----
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

    // ---- second ply: the live s1, round-robin over the waves; lane = s2 ----
    {
        float w[NF];
#pragma unroll
        for (int r = 0; r < NF; ++r) {
            w[r] = wts2[(size_t)wrow * NF + r];
            asm volatile("" : "+v"(w[r]));  // (as in the first ply)
        }
        int k = 0;
        for (int q = 0; q < kLaWaves; ++q) {
            uint64_t m = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)sLive[q][0]) |
                         (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)sLive[q][1]) << 32;
            for (; m; m &= m - 1) {
                if ((k++ & (kLaWaves - 1)) != wave) continue;
                const int s1 = q * kWave + (int)__builtin_ctzll(m);
                const uint32_t *C = B1 + s1 * pitch + kAfterP;
                const int32_t h1 = sHoles[s1], g1 = sHeight[s1];
                int32_t bslot;
                float bscore;
                auto pass = [&](int s0, auto first) {
                    const int s = s0 + lane;
                    const bool live = s < S;
                    int32_t f[NF];
                    const bool valid = eval_slot_set<SET>(C, W, H, p.flags, nid, live ? s : S - 1, h1, g1, f,
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
                const int32_t win = wave_reduce(tied ? bslot : INT32_MAX, [](int a, int b) { return a < b ? a : b; });
                if (lane == 0) {
                    sM2[s1] = top;
                    sSl2[s1] = win == INT32_MAX ? -1 : win;
                }
            }
        }
    }
    __syncthreads();

    // ---- choose ----
    if (active) {
        const bool live = t < S;
        const int32_t sl2 = cand && !dead1 ? sSl2[live ? t : 0] : -1;
        const float tail = sl2 >= 0 ? sM2[live ? t : 0] : dead_value;
        const float tot = s1score + tail;
        if (live) {
            if (scores_all) scores_all[(size_t)e * S + t] = cand ? tot : 0.0f;
            if (slots2_all) slots2_all[(size_t)e * S + t] = cand ? sl2 : -1;
        }
        const float top = __int_as_float(wave_reduce(__float_as_int(cand ? tot : -__builtin_inff()), [](int a, int b) {
            return __float_as_int(__builtin_fmaxf(__int_as_float(a), __int_as_float(b)));
        }));
        bool tied = cand && tot == top;
        if (__ballot(tied) == 0) tied = cand;
        const int32_t win = wave_reduce(tied ? t : INT32_MAX, [](int a, int b) { return a < b ? a : b; });
        if (win == INT32_MAX ? lane == 0 : tied && t == win) {
            sWin[wave] = win == INT32_MAX ? -1 : win;
            sWin2[wave] = sl2;
            sTop[wave] = tot;
        }
    } else if (lane == 0) {
        sWin[wave] = -1;
    }
    __syncthreads();
    if (t == 0) {
        int32_t win = -1, win2 = -1;
        float top = 0.0f;
        for (int q = 0; q < kLaWaves; ++q) {  // the first wave with the largest score: ties to the lowest s1
            if (sWin[q] >= 0 && (win < 0 || sTop[q] > top)) {
                win = sWin[q];
                win2 = sWin2[q];
                top = sTop[q];
            }
        }
        const bool none = win < 0;
        const int trot = (win >= per) + (win >= 2 * per) + (win >= 3 * per), tx = win - trot * per - 3;
        if (slots) slots[e] = win;
        if (slots2) slots2[e] = win2;
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

hipError_t launch_next_piece(const KParams &p, uint8_t *next, hipStream_t s) {
    hipLaunchKernelGGL(k_next_piece, dim3((unsigned)(p.stride / kWave)), dim3(kWave), 0, s, p, next);
    return hipGetLastError();
}

hipError_t launch_policy_lookahead(const KParams &p, int set, bool commit, const float *weights1,
                                   const float *weights2, int64_t n_w, float dead_value, const int32_t *allowed,
                                   int32_t *slots, int32_t *slots2, uint8_t *actions, float *scores,
                                   float *scores_all, int32_t *slots2_all, hipStream_t s) {
    if (set != ST_FEATS_BASE && set != ST_FEATS_BCTS) return hipErrorInvalidValue;
    // the preview the second ply places: drawn here where it is missing
    if (const hipError_t e = launch_next_piece(p, nullptr, s); e != hipSuccess) return e;
    const dim3 grid((unsigned)p.n), block(kLaWaves * kWave);  // one workgroup per env
    const size_t lds = sizeof(uint32_t) * (size_t)(4 * (p.W + 6)) * (size_t)la_pitch(p.W);
#define ST_LA_ARGS p, weights1, weights2, n_w, dead_value, allowed, slots, slots2, actions, scores, scores_all, slots2_all
    if (set == ST_FEATS_BCTS && commit)
        hipLaunchKernelGGL((k_policy_lookahead<ST_FEATS_BCTS, true>), grid, block, lds, s, ST_LA_ARGS);
    else if (set == ST_FEATS_BCTS)
        hipLaunchKernelGGL((k_policy_lookahead<ST_FEATS_BCTS, false>), grid, block, lds, s, ST_LA_ARGS);
    else if (commit)
        hipLaunchKernelGGL((k_policy_lookahead<ST_FEATS_BASE, true>), grid, block, lds, s, ST_LA_ARGS);
    else
        hipLaunchKernelGGL((k_policy_lookahead<ST_FEATS_BASE, false>), grid, block, lds, s, ST_LA_ARGS);
#undef ST_LA_ARGS
    return hipGetLastError();
}

}  // namespace st
