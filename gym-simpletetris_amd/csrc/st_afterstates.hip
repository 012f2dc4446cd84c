// st_afterstates.hip -- k_afterstates (st_afterstates), k_placement_actions
// (st_placement_actions), k_place (st_place, st_step_placements),
// k_policy_linear and k_play_sum (st_policy_linear, st_play_linear,
// st_play_linear_placements) as a translation unit of their own.  Entry
// points: launch_afterstates, launch_placement_actions, launch_place,
// launch_policy_linear, launch_policy_linear_commit, launch_play_sum.  They use
// the core's piece table and collision / drop / clear / scoring helpers
// (st_kernels.hip) and eval_slot (st_eval.h), and are compiled apart from the
// step kernels so that those code objects stay exactly as they were
// (st_kernels.hip, top).
#define ST_SIDE_TU 1
#include "st_kernels.hip"
#include "st_eval.h"

namespace st {
namespace {

// st_afterstates: the kernel st_eval.h ("afterstates") describes, over eval_slot.
__global__ __launch_bounds__(kWave) void k_afterstates(KParams p, int32_t *__restrict__ feat,
                                                       uint32_t *__restrict__ boards) {
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
    const size_t fbase = (size_t)e * ST_AFTER_NFEAT * S, bbase = (size_t)e * W * S;
    for (int s0 = 0; s0 < S; s0 += kWave) {
        const int s = s0 + lane;
        const bool live = s < S;
        const int sc = live ? s : S - 1;  // (lanes past the last slot compute it again, store nothing)
        int32_t f[ST_AFTER_NFEAT];
        const bool valid = eval_slot(L + kAfterP, W, H, p.flags, id, sc, old_holes, old_height, f,
                                     [&](int c, uint32_t w, bool ok) {
                                         if (boards && live) boards[bbase + (size_t)c * S + s] = ok ? w : 0u;
                                     });
        if (live) {
#pragma unroll
            for (int row = 0; row < ST_AFTER_NFEAT; ++row) feat[fbase + (size_t)row * S + s] = valid ? f[row] : 0;
        }
    }
}

// st_placement_actions: the primitive action that moves env e's live piece
// toward slot slots[e] -- k_policy_greedy's rule (gen_golden.greedy_action):
// rotate_left until the rotation matches, then move toward x, then hard-drop;
// a slot outside [0, S) hard-drops.  One lane per env.
__global__ __launch_bounds__(256) void k_placement_actions(KParams p, const int32_t *__restrict__ slots,
                                                           uint8_t *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.n) return;
    const int per = p.W + 6;
    const uint32_t pw = p.piece[e];
    const int rot = (int)((pw >> 3) & 3u), ax = (int)((pw >> 5) & 63u);
    const int32_t s = slots[e];
    uint32_t a = 2u;
    if (s >= 0 && s < 4 * per) {
        const int trot = s / per, tx = s - trot * per - 3;
        a = rot != trot ? 4u : (ax < tx ? 1u : (ax > tx ? 0u : 2u));
    }
    out[e] = (uint8_t)a;
}

// ---------------------------------------------------------------- placement step
// st_place: commit slot slots[e] of env e (simpletetris.h, "Placement step").
// A VALID slot -- in [0, S) and not is_occupied(cells, (x, 0), board), the
// validity of eval_slot on the env's current board and piece id -- makes the
// env's piece the slot's: rotation rot, anchor (x, 0) and a lock counter of
// lock_mod - 1 = max(lock_delay, 0), from which the next drop's
// (x + 1) % lock_mod is 0 (tetris_env.py:175): the hard drop behind it locks
// the piece whatever lock_delay is.  Any other slot leaves the piece word as
// it is, lock counter included.  Board, counters, MT and preview are not
// written.  Every shape holds cell (0, 0), so a valid slot has 0 <= x < W and
// x fits its six bits.
// One lane per env: the piece word, the slot and the slot's four box columns
// (floor bits, all-ones walls outside [0, W), as stage_env_columns gives them)
// are the lane's only loads; the piece word leaves with a plain vector store.
__global__ __launch_bounds__(256) void k_place(KParams p, const int32_t *__restrict__ slots,
                                               uint8_t *__restrict__ placed) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.n) return;
    const int W = p.W, per = W + 6;
    const uint32_t pid = p.piece[e] & 7u;
    const int id = (int)(pid < 7u ? pid : 6u);  // (a host-written id 7 stays inside the table)
    const int32_t s = slots[e];
    bool ok = false;
    if (s >= 0 && s < 4 * per) {
        const int r = (s >= per) + (s >= 2 * per) + (s >= 3 * per), x = s - r * per - 3;
        const uint32_t m = c_tab_m[id * 4 + r], g = c_tab_g[id * 4 + r];
        const int x0 = box_x0(g, x);  // in [-6, W + 2]
        const uint32_t floorb = ~((1u << p.H) - 1u);
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = x0 + j;
            v[j] = c >= 0 && c < W ? p.board[c * p.stride + e] | floorb : ~0u;
        }
        ok = !collides_v(m, 0, v);
        if (ok) p.piece[e] = placed_piece(id, r, x, p.lock_mod);
    }
    if (placed) placed[e] = ok ? 1 : 0;
}

// ---------------------------------------------------------------- linear feature player
// st_policy_linear: env e scores every slot of its current piece with weight
// row e % n_w and keeps the best one -- k_afterstates's evaluation (eval_slot)
// without its output stream: per env 4 + 1 + 4 + 44 bytes leave the kernel.
// The score is lin_score's float32 chain (st_eval.h, "score, reductions").
//
// One wave per env, lane = slot, ceil(S / 64) passes; ST_POLICY_WAVES envs per
// workgroup, each wave with its own W + 16 column words of LDS and no
// workgroup barrier (a wave past the last env leaves at once).  A lane keeps
// the first maximum of its own slots: the first pass sets it (10x20 has no
// other), a later pass replaces it only on a strictly larger score, since a
// lane's slots ascend.  Across lanes: the wave's maximum score over the lanes
// that hold a candidate, then the lowest slot among the lanes that reach it --
// two DPP reductions (wave_reduce), six VALU operations each, no LDS.  The lane
// whose candidate won -- lane 0 if no slot is valid -- writes the env's
// outputs with plain stores.
//
// st_play_linear's accumulators stay out of this kernel: its steps write
// their reward / done into rows of a ring the context owns, and k_play_sum adds
// a ring's worth at a time -- one lane per env, whole cache lines.  (Adding
// in this kernel, one lane per wave or one wave per 64 envs, measured 3.8 /
// 1.5 us per step at 65,536 envs.)
__global__ __launch_bounds__(256) void k_play_sum(const int32_t *__restrict__ reward, const uint8_t *__restrict__ done,
                                                  int rows, int64_t n, int64_t *__restrict__ ret,
                                                  int32_t *__restrict__ episodes, int32_t *__restrict__ out_reward,
                                                  uint8_t *__restrict__ out_done) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    int64_t r = 0;
    int32_t d = 0;
    for (int j = 0; j < rows; ++j) {
        r += (int64_t)reward[(int64_t)j * n + e];
        d += done[(int64_t)j * n + e] ? 1 : 0;
    }
    if (ret) ret[e] += r;
    if (episodes) episodes[e] += d;
    // the last row, i.e. the last step's outputs, for the caller
    if (out_reward) out_reward[e] = reward[(int64_t)(rows - 1) * n + e];
    if (out_done) out_done[e] = done[(int64_t)(rows - 1) * n + e];
}

// COMMIT (st_play_linear_placements): the lane that writes the env's outputs
// also stores the chosen slot's piece word (placed_piece: k_place's commit,
// without its launch); it stores nothing if no slot is valid.
template <int WAVES, bool COMMIT = false>
__global__ __launch_bounds__(WAVES *kWave) void k_policy_linear(KParams p, const float *__restrict__ wts, int64_t n_w,
                                                                int32_t *__restrict__ slots,
                                                                uint8_t *__restrict__ actions,
                                                                float *__restrict__ scores,
                                                                int32_t *__restrict__ best) {
    __shared__ uint32_t Lall[WAVES * kAfterCols];
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
    float w[ST_AFTER_NFEAT];
#pragma unroll
    for (int r = 0; r < ST_AFTER_NFEAT; ++r) w[r] = wts[(size_t)wrow * ST_AFTER_NFEAT + r];
    wave_sync();
    // the lane's candidate: its best slot so far (-1: none), that slot's score and rows
    int32_t bslot;
    float bscore;
    int32_t bf[ST_AFTER_NFEAT];
    auto pass = [&](int s0, auto first) {
        const int s = s0 + lane;
        const bool live = s < S;
        int32_t f[ST_AFTER_NFEAT];
        const bool valid = eval_slot(L + kAfterP, W, H, p.flags, id, live ? s : S - 1, old_holes, old_height, f,
                                     [](int, uint32_t, bool) {});
        const float sc = lin_score(w, f);
        if constexpr (decltype(first)::value) {  // (score and rows are read only where bslot >= 0)
            bslot = live && valid ? s : -1;
            bscore = sc;
#pragma unroll
            for (int r = 0; r < ST_AFTER_NFEAT; ++r) bf[r] = f[r];
        } else if (live && valid && (bslot < 0 || sc > bscore)) {
            bslot = s;
            bscore = sc;
#pragma unroll
            for (int r = 0; r < ST_AFTER_NFEAT; ++r) bf[r] = f[r];
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
            for (int r = 0; r < ST_AFTER_NFEAT; ++r) best[(size_t)r * p.n + e] = none ? 0 : bf[r];
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

hipError_t launch_afterstates(const KParams &p, int32_t *feat, uint32_t *boards, hipStream_t s) {
    hipLaunchKernelGGL(k_afterstates, dim3((unsigned)p.n), dim3(kWave), 0, s, p, feat, boards);  // one wave per env
    return hipGetLastError();
}

hipError_t launch_placement_actions(const KParams &p, const int32_t *slots, uint8_t *out, hipStream_t s) {
    hipLaunchKernelGGL(k_placement_actions, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p, slots, out);
    return hipGetLastError();
}

hipError_t launch_place(const KParams &p, const int32_t *slots, uint8_t *placed, hipStream_t s) {
    hipLaunchKernelGGL(k_place, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p, slots, placed);
    return hipGetLastError();
}

hipError_t launch_policy_linear_commit(const KParams &p, const float *weights, int64_t n_w, hipStream_t s) {
    constexpr int WV = ST_POLICY_WAVES;
    hipLaunchKernelGGL((k_policy_linear<WV, true>), dim3((unsigned)((p.n + WV - 1) / WV)), dim3(WV * kWave), 0, s, p,
                       weights, n_w, (int32_t *)nullptr, (uint8_t *)nullptr, (float *)nullptr, (int32_t *)nullptr);
    return hipGetLastError();
}

hipError_t launch_policy_linear(const KParams &p, const float *weights, int64_t n_w, int32_t *slots, uint8_t *actions,
                                float *scores, int32_t *best, hipStream_t s) {
    constexpr int WV = ST_POLICY_WAVES;
    hipLaunchKernelGGL((k_policy_linear<WV>), dim3((unsigned)((p.n + WV - 1) / WV)), dim3(WV * kWave), 0, s, p, weights,
                       n_w, slots, actions, scores, best);
    return hipGetLastError();
}

hipError_t launch_play_sum(const KParams &p, const int32_t *reward, const uint8_t *done, int rows, int64_t *acc_return,
                           int32_t *acc_episodes, int32_t *out_reward, uint8_t *out_done, hipStream_t s) {
    hipLaunchKernelGGL(k_play_sum, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, reward, done, rows, p.n,
                       acc_return, acc_episodes, out_reward, out_done);
    return hipGetLastError();
}

}  // namespace st
