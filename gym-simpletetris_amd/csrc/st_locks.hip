// st_locks.hip -- k_lock_set, k_afterstates_at and k_locks (st_lock_set,
// st_afterstates_at, st_routes_at, st_policy_locks, st_play_locks) as a
// translation unit of their own.  Entry points: launch_lock_set,
// launch_afterstates_at, launch_locks.  They use the core's piece table
// (st_kernels.hip), the column staging, evaluators and score (st_eval.h) and
// the search helpers (st_search.h); eval_at_set, the third evaluator, lives
// here.  Compiled apart from every other kernel so that every other code
// object stays exactly as it was (st_kernels.hip, top).
#define ST_SIDE_TU 1
#include "st_kernels.hip"
#include "st_eval.h"
#include "st_search.h"

namespace st {
namespace {

// ---------------------------------------------------------------- lock positions
// st_lock_set / st_afterstates_at / st_routes_at / st_policy_locks /
// st_play_locks: every (rot, x, y) the live piece can be locked at
// (simpletetris.h, "Lock positions"), a tuck under an overhang included -- the
// placements k_reachable's search walks through and then masks away with the
// landing bit.  One wave per env, a lane per slot, whole-row bit sets, as
// k_reachable / k_routes:
//  forward   k_reachable<false, false>'s layers; the last plane's grounded rows
//            that are free (grounded & F[s]: a start that collides and locks
//            where it stands is none) are ORed into the slot's lock word
//            K[s] on every layer.  The start's own layer needs nothing of its
//            own: the start state sits in the set of its plane, idle keeps it
//            there, and layer 1 grounds and locks it like any other.
//  choice    a lane walks the bits of its slots' lock words in ascending
//            pos = slot * 32 + y, evaluates each with eval_at_set (the rows of
//            eval_slot_set with the piece set at (x, y)), scores it with
//            lin_score and keeps its first maximum; the wave's choice is
//            k_routes's pair of wave_reduces on (score, lowest pos).
//  backward, walk   k_routes's (c) and (d) with "the target's landing" read
//            as bit y of slot s.
// LDS: k_routes's layout (route_lds_bytes), R holding the lock words;
// k_lock_set needs no D.

// eval_slot_set with the anchor row given: the piece at (x, y) is evaluable
// iff it is collision-free there and occupied a row lower (s in [0, S),
// 0 <= y < H: the caller checks).  It restates eval_slot_set for the reason
// eval_slot_set restates eval_slot (a row parameter on either moves the
// existing kernels' instructions) and must follow it change for change; the
// tests hold it to st_afterstates_set's rows bit for bit at every landing.
template <int SET, class ColOut>
__device__ __forceinline__ bool eval_at_set(const uint32_t *C, int W, int H, uint32_t flags, int id, int s, int y,
                                            int32_t old_holes, int32_t old_height, int32_t (&f)[feat_rows(SET)],
                                            ColOut col_out) {
    constexpr bool EXT = SET == ST_FEATS_BCTS;
    const uint32_t hmask = (1u << H) - 1u, floorb = ~hmask;
    const int per = W + 6;
    const int r = (s >= per) + (s >= 2 * per) + (s >= 3 * per), x = s - r * per - 3;
    const uint32_t m = c_tab_m[id * 4 + r], g = c_tab_g[id * 4 + r];
    const int x0 = box_x0(g, x);
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = C[x0 + j];
    const bool valid = !collides_v(m, y, v) && collides_v(m, y + 1, v);
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

// The env's piece word as k_reachable reads it.
struct LockStart {
    int id, rot, cx0, ay, lock0;
    bool ok;  // inside the lane grid and the row word (k_reachable: any other start reaches no slot)
};
__device__ __forceinline__ LockStart lock_start(uint32_t pw, int per, int NP) {
    LockStart st;
    const uint32_t pid = pw & 7u;
    st.id = (int)(pid < 7u ? pid : 6u);  // (a host-written id 7 stays inside the table)
    st.rot = (int)((pw >> 3) & 3u);
    st.cx0 = (int)((pw >> 5) & 63u) + 3;
    st.ay = (int)((pw >> 11) & 63u);
    st.lock0 = (int)(pw >> 17) < NP ? (int)(pw >> 17) : NP - 1;  // (as k_reachable reads it)
    st.ok = st.cx0 < per && st.ay < 32;
    return st;
}

// The forward layers: K[s] |= the rows the piece locks at in slot s.  F is
// filled, K and both copies of A are zero, and the wave has synchronised.
__device__ __forceinline__ void lock_forward(const uint32_t *F, uint32_t *K, uint32_t *A, int S, int per, int H, int NP,
                                             bool sreset, const LockStart &st, int lane) {
    const int setw = NP * S;
    if (st.ok && lane == 0) A[st.lock0 * S + st.rot * per + st.cx0] = 1u << st.ay;
    wave_sync();
    int cur = 0;
    const int max_fwd = st.ok ? 4 * per * H * NP : 0;
    for (int layer = 1; layer <= max_fwd; ++layer) {
        const uint32_t *const In = A + cur * setw;
        uint32_t *const Out = A + (cur ^ 1) * setw;
        bool grew = false;
        for (int s = lane; s < S; s += kWave) {
            const uint32_t f = F[s], fd = f >> 1;
            const int sl = s > 0 ? s - 1 : 0, sr = s < S - 1 ? s + 1 : s;
            const int su = s + per < S ? s + per : s + per - S, sd = s >= per ? s - per : s - per + S;
            uint32_t mvall = 0;
            for (int l = 0; l < NP; ++l) {
                const uint32_t *const I = In + l * S;
                const uint32_t a = I[s];
                const uint32_t nb = I[sl] | I[sr] | I[su] | I[sd];
                const uint32_t pos = a | ((nb | (a << 1)) & f) | (reach_fall(a, f) & ~fd);
                Out[l * S + s] = pos;
                mvall |= (pos << 1) & f;
            }
            uint32_t grounded = 0;
            for (int l = 0; l < NP; ++l) {
                const uint32_t pos = Out[l * S + s];
                const uint32_t moved = sreset ? (l == 0 ? mvall : 0u) : (pos << 1) & f;
                const uint32_t g = (pos & ~fd) | moved;
                const uint32_t old = In[l * S + s];
                const uint32_t nw = old | (g & fd) | grounded;
                Out[l * S + s] = nw;
                grew = grew || nw != old;
                grounded = g & ~fd;
            }
            K[s] |= grounded & f;  // the counter wraps: the piece locks, collision-free
        }
        wave_sync();
        cur ^= 1;
        if (!__ballot(grew)) break;
    }
}

__device__ __forceinline__ int wave_sum(int x) {  // over all 64 lanes, in every lane
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) x += __shfl_xor(x, d);
    return x;
}

// st_lock_set: rows uint32 [n][S], pos int32 [n][cap], count int32 [n], any null
__global__ __launch_bounds__(kWave) void k_lock_set(KParams p, uint32_t *__restrict__ rows, int32_t *__restrict__ pos,
                                                    int64_t cap, int32_t *__restrict__ count) {
    extern __shared__ uint32_t lock_lds[];
    const int lane = threadIdx.x;
    const int64_t e = blockIdx.x;  // the grid is p.n waves
    const int W = p.W, H = p.H, per = W + 6, S = 4 * per;
    const int NP = p.lock_mod;  // (the host checked L <= ST_REACH_MAX_LOCK)
    uint32_t *const C = lock_lds;        // column words
    uint32_t *const F = C + kAfterCols;  // [S] free rows
    uint32_t *const K = F + S;           // [S] lock rows
    uint32_t *const A = K + S;           // [2][NP][S]
    stage_env_columns(C, p, e, lane);
    const LockStart st = lock_start(p.piece[e], per, NP);
    wave_sync();
    for (int s = lane; s < S; s += kWave) {
        F[s] = reach_free(C + kAfterP, W, st.id, s);
        K[s] = 0u;
        for (int k = 0; k < 2 * NP; ++k) A[k * S + s] = 0u;
    }
    wave_sync();
    lock_forward(F, K, A, S, per, H, NP, (p.flags & ST_STEP_RESET) != 0u, st, lane);

    // the list: a lane's count, the wave's prefix sum, a walk over the lane's bits -- pass by pass, since
    // the slots of a pass all come before the next pass's
    int32_t base = 0;
    for (int s0 = 0; s0 < S; s0 += kWave) {
        const int s = s0 + lane;
        uint32_t w = s < S ? K[s] : 0u;
        if (rows && s < S) rows[(size_t)e * S + s] = w;
        const int c = __builtin_popcount(w);
        int x = c;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int t = __shfl_up(x, d);
            x += lane >= d ? t : 0;
        }
        int64_t i = base + x - c;
        if (pos) {
            while (w) {
                if (i < cap) pos[(size_t)e * (size_t)cap + (size_t)i] = s * 32 + __builtin_ctz(w);
                ++i;
                w &= w - 1u;
            }
        }
        base += __shfl(x, kWave - 1);
    }
    if (pos)
        for (int64_t i = base + lane; i < cap; i += kWave) pos[(size_t)e * (size_t)cap + (size_t)i] = -1;
    if (count && lane == 0) count[e] = base;
}

// st_afterstates_at: pos int32 [n][cap] (any values) -> feat int32 [n][rows][cap], boards uint32 [n][W][cap] or
// null; a lane per entry, ceil(cap / 64) passes; a non-evaluable entry stores zeros
template <int SET>
__global__ __launch_bounds__(kWave) void k_afterstates_at(KParams p, const int32_t *__restrict__ pos, int64_t cap,
                                                          int32_t *__restrict__ feat, uint32_t *__restrict__ boards) {
    constexpr int NF = feat_rows(SET);
    __shared__ uint32_t L[kAfterCols];
    const int lane = threadIdx.x;
    const int64_t e = blockIdx.x;  // the grid is p.n waves
    const int64_t sd = p.stride;
    const int W = p.W, H = p.H;
    const int S = 4 * (W + 6);
    stage_env_columns(L, p, e, lane);
    const uint32_t pid = p.piece[e] & 7u;
    const int id = (int)(pid < 7u ? pid : 6u);  // (a host-written id 7 stays inside the table)
    const int32_t old_holes = p.stats[ST_STAT_HOLES * sd + e];
    const int32_t old_height = p.stats[ST_STAT_PIECE_HEIGHT * sd + e];
    wave_sync();
    const size_t ucap = (size_t)cap;
    const size_t fbase = (size_t)e * NF * ucap, bbase = (size_t)e * W * ucap;
    for (int64_t i0 = 0; i0 < cap; i0 += kWave) {
        const int64_t i = i0 + lane;
        const bool live = i < cap;
        const int32_t q = live ? pos[(size_t)e * ucap + (size_t)i] : -1;
        const bool dec = q >= 0 && (q >> 5) < S && (q & 31) < H;  // decodes to a slot and a row of the board
        const int s = dec ? q >> 5 : S - 1, y = dec ? q & 31 : 0;  // (others compute something, store zeros)
        int32_t f[NF];
        const bool valid = eval_at_set<SET>(L + kAfterP, W, H, p.flags, id, s, y, old_holes, old_height, f,
                                            [&](int c, uint32_t w, bool ok) {
                                                if (boards && live)
                                                    boards[bbase + (size_t)c * ucap + (size_t)i] = ok && dec ? w : 0u;
                                            });
        if (live) {
#pragma unroll
            for (int row = 0; row < NF; ++row)
                feat[fbase + (size_t)row * ucap + (size_t)i] = valid && dec ? f[row] : 0;
        }
    }
}

struct LockIO {
    const int32_t *pos_in;  // st_routes_at: the targets int32 [n]
    const uint8_t *need;    // uint8 [n] or null: every env
    int32_t *rem;           // st_play_locks: an env is needed iff rem[e] == 0, and gets min(steps, ST_ROUTE_MAX)
    const float *wts;       // the planner: float [n_w][rows]
    int64_t n_w;
    int32_t *pos;           // the planner: the chosen position int32 [n]
    uint64_t *route;        // uint64 [ST_ROUTE_WORDS][n]; the planner: or null (no backward search, no walk)
    int32_t *steps;         // int32 [n] or null
    float *scores;          // the planner: float [n] or null
    int32_t *best;          // the planner: int32 [rows][n] or null
    int32_t *count;         // the planner: int32 [n] or null
};

// SET: a feature set -- the planner (st_policy_locks / st_play_locks); -1 -- st_routes_at for pos_in[e]
template <int SET>
__global__ __launch_bounds__(kWave) void k_locks(KParams p, LockIO io) {
    extern __shared__ uint32_t lock_lds[];
    const int lane = threadIdx.x;
    const int64_t e = blockIdx.x;  // the grid is p.n waves
    if (io.rem ? io.rem[e] != 0 : (io.need != nullptr && io.need[e] == 0)) return;  // (wave-uniform)
    const int W = p.W, H = p.H, per = W + 6, S = 4 * per;
    const int NP = p.lock_mod;  // (the host checked L <= ST_REACH_MAX_LOCK)
    const bool sreset = (p.flags & ST_STEP_RESET) != 0u;
    uint32_t *const C = lock_lds;        // column words
    uint32_t *const F = C + kAfterCols;  // [S] free rows
    uint32_t *const K = F + S;           // [S] lock rows
    uint32_t *const A = K + S;           // [2][NP][S]
    uint16_t *const D = reinterpret_cast<uint16_t *>(A + 2 * NP * S);  // [NP][S][32]
    const int setw = NP * S;

    stage_env_columns(C, p, e, lane);
    const LockStart st = lock_start(p.piece[e], per, NP);
    const int id = st.id, rot = st.rot, cx0 = st.cx0, ay = st.ay, lock0 = st.lock0;
    wave_sync();
    for (int s = lane; s < S; s += kWave) {
        F[s] = reach_free(C + kAfterP, W, id, s);
        K[s] = 0u;
        for (int k = 0; k < 2 * NP; ++k) A[k * S + s] = 0u;
    }
    wave_sync();
    auto is_free = [&](int r, int cx, int y) -> bool {
        return cx >= 0 && cx < per && y < 32 && ((F[r * per + cx] >> y) & 1u);
    };

    int tgt = -1, ty = 0;  // the target: slot and row
    if constexpr (SET >= 0) {
        lock_forward(F, K, A, S, per, H, NP, sreset, st, lane);

        constexpr int NF = feat_rows(SET);
        const int64_t sd_ = p.stride;
        const int32_t old_holes = p.stats[ST_STAT_HOLES * sd_ + e];
        const int32_t old_height = p.stats[ST_STAT_PIECE_HEIGHT * sd_ + e];
        const uint32_t wrow = io.n_w > e ? (uint32_t)e : (uint32_t)e % (uint32_t)io.n_w;
        float w[NF];
#pragma unroll
        for (int r = 0; r < NF; ++r) w[r] = io.wts[(size_t)wrow * NF + r];
        int32_t bpos = -1, nlock = 0;
        float bscore = 0.0f;
        int32_t bf[NF];
#pragma unroll
        for (int r = 0; r < NF; ++r) bf[r] = 0;
        for (int s = lane; s < S; s += kWave) {
            uint32_t k = K[s];
            nlock += __builtin_popcount(k);
            while (k) {  // (mostly one row, sometimes two or three)
                const int y = __builtin_ctz(k);
                k &= k - 1u;
                int32_t f[NF];
                const bool valid = eval_at_set<SET>(C + kAfterP, W, H, p.flags, id, s, y, old_holes, old_height, f,
                                                    [](int, uint32_t, bool) {});
                const float sc = lin_score(w, f);
                if (valid && (bpos < 0 || sc > bscore)) {  // (a lane's positions ascend: the first maximum stays)
                    bpos = s * 32 + y;
                    bscore = sc;
#pragma unroll
                    for (int r = 0; r < NF; ++r) bf[r] = f[r];
                }
            }
        }
        const bool has = bpos >= 0;
        const float top =
            __int_as_float(wave_reduce(__float_as_int(has ? bscore : -__builtin_inff()), [](int a, int b) {
                return __float_as_int(__builtin_fmaxf(__int_as_float(a), __int_as_float(b)));
            }));
        bool tied = has && bscore == top;
        if (__ballot(tied) == 0) tied = has;  // (a NaN score equals nothing: every candidate counts)
        const int32_t win = wave_reduce(tied ? bpos : INT32_MAX, [](int a, int b) { return a < b ? a : b; });
        const bool none = win == INT32_MAX;
        if (none ? lane == 0 : tied && bpos == win) {
            io.pos[e] = none ? -1 : win;
            if (io.scores) io.scores[e] = none ? 0.0f : bscore;
            if (io.best) {
#pragma unroll
                for (int r = 0; r < NF; ++r) io.best[(size_t)r * p.n + e] = none ? 0 : bf[r];
            }
        }
        if (io.count) {
            const int total = wave_sum(nlock);
            if (lane == 0) io.count[e] = total;
        }
        if (io.route == nullptr) return;  // (wave-uniform) the choice alone: steps is not written either
        tgt = none ? -1 : win >> 5;
        ty = none ? 0 : win & 31;
        wave_sync();
        for (int s = lane; s < S; s += kWave)
            for (int k = 0; k < NP; ++k) A[k * S + s] = 0u;  // B
        wave_sync();
    } else {
        const int32_t q = io.pos_in[e];
        if (q >= 0 && (q >> 5) < S && (q & 31) < H) {
            tgt = q >> 5;
            ty = q & 31;
        }
    }

    // the backward layers (k_routes (c)): the target is collision-free and grounded at row ty, or not served
    uint32_t *const B = A, *const Q = A + setw;
    const int s_start = rot * per + (cx0 < per ? cx0 : 0);
    const uint32_t ftgt = tgt >= 0 ? F[tgt] : 0u;
    const bool search = st.ok && ((ftgt >> ty) & 1u) && !((ftgt >> (ty + 1)) & 1u);  // (ty + 1 <= H <= 28)
    const uint32_t tland = search ? 1u << ty : 0u;
    const int max_layer = search ? 4 * per * H * NP : 0;
    int n = 0;  // steps: the layer at which the start state joined
    for (int layer = 1; layer <= max_layer; ++layer) {
        for (int s = lane; s < S; s += kWave) {
            const uint32_t fd = F[s] >> 1, tb = s == tgt ? tland : 0u;
            uint32_t E[kRoutePlanes];
#pragma unroll
            for (int l = 0; l < kRoutePlanes; ++l)
                if (l < NP) E[l] = (fd & B[l * S + s]) | (~fd & (l + 1 == NP ? tb : B[(l + 1 < NP ? l + 1 : l) * S + s]));
#pragma unroll
            for (int l = 0; l < kRoutePlanes; ++l)
                if (l < NP) Q[l * S + s] = (~fd & E[l]) | (fd & ((sreset ? E[0] : E[l]) >> 1));
        }
        wave_sync();
        bool grew = false;
        for (int s = lane; s < S; s += kWave) {
            const uint32_t fd = F[s] >> 1;
            const int sl = s > 0 ? s - 1 : 0, sr = s < S - 1 ? s + 1 : s;
            const int su = s + per < S ? s + per : s + per - S, sd = s >= per ? s - per : s - per + S;
            const uint32_t fl = F[sl], fr = F[sr], fu = F[su], fdn = F[sd];
            for (int l = 0; l < NP; ++l) {
                const uint32_t *const Ql = Q + l * S;
                const uint32_t q = Ql[s];
                const uint32_t pre = q | (fl & Ql[sl]) | (fr & Ql[sr]) | (fu & Ql[su]) | (fdn & Ql[sd]) |
                                     (fd & (q >> 1)) | route_rise(q & ~fd, fd);
                const uint32_t old = B[l * S + s];
                uint32_t nw = pre & ~old;
                if (nw) {
                    B[l * S + s] = old | nw;
                    grew = true;
                    do {
                        D[((l * S + s) << 5) + __builtin_ctz(nw)] = (uint16_t)layer;
                        nw &= nw - 1u;
                    } while (nw);
                }
            }
        }
        wave_sync();
        if ((B[lock0 * S + s_start] >> ay) & 1u) {  // (one address: wave-uniform)
            n = layer;
            break;
        }
        if (!__ballot(grew)) break;
    }

    // the walk (k_routes (d))
    uint64_t w0 = kRouteNone, w1 = kRouteNone;
    if (n > 0) {
        int r = rot, cx = cx0, y = ay, l = lock0;
        const int m = n < ST_ROUTE_MAX ? n : ST_ROUTE_MAX;
        for (int i = 0; i < m; ++i) {
            const int d = n - i;  // D(r, cx, y, l); below 2^16, the number of states
            int r2 = r, cx2 = cx, y2 = y, l2 = l;
            bool ok = false;
            if (lane < 7) {  // action `lane` on the state (:245-262)
                if (lane == 0) cx2 -= is_free(r2, cx2 - 1, y2) ? 1 : 0;
                else if (lane == 1) cx2 += is_free(r2, cx2 + 1, y2) ? 1 : 0;
                else if (lane == 2) y2 += __builtin_ctz(~(y2 < 31 ? F[r2 * per + cx2] >> (y2 + 1) : 0u));
                else if (lane == 3) y2 += is_free(r2, cx2, y2 + 1) ? 1 : 0;
                else if (lane == 4) r2 = is_free((r2 + 1) & 3, cx2, y2) ? (r2 + 1) & 3 : r2;
                else if (lane == 5) r2 = is_free((r2 + 3) & 3, cx2, y2) ? (r2 + 3) & 3 : r2;
                if (is_free(r2, cx2, y2 + 1)) {
                    ++y2;
                    l2 = sreset ? 0 : l2;
                }
                const int s1 = r2 * per + cx2;
                bool locked = false;
                if (!is_free(r2, cx2, y2 + 1)) {
                    l2 = l2 + 1 == NP ? 0 : l2 + 1;
                    locked = l2 == 0;
                }
                if (locked) ok = n - i == 1 && s1 == tgt && ((tland >> y2) & 1u);
                else
                    ok = n - i > 1 && ((B[l2 * S + s1] >> y2) & 1u) &&
                         D[((l2 * S + s1) << 5) + y2] == (uint16_t)(d - 1);
            }
            const uint64_t won = __ballot(ok);
            if (won == 0) break;  // (D(x) = d has a successor at d - 1: not taken)
            const int a = __builtin_ctzll(won);
            const int nx = __shfl(r2 | cx2 << 2 | y2 << 10 | l2 << 16, a);
            r = nx & 3;
            cx = (nx >> 2) & 255;
            y = (nx >> 10) & 63;
            l = nx >> 16;
            const uint64_t fld = (uint64_t)(7 - a) << (3 * (i % 21));  // 7 -> a: clear the bits a lacks
            if (i < 21) w0 ^= fld;
            else w1 ^= fld;
        }
    }
    if (lane == 0) {
        io.route[e] = w0;
        io.route[p.n + e] = w1;
        if (io.steps) io.steps[e] = n;
        if (io.rem) io.rem[e] = n < ST_ROUTE_MAX ? n : ST_ROUTE_MAX;
    }
}

}  // namespace

// k_locks: route_lds_bytes's layout (R holds the lock words); k_lock_set: the same without D
static size_t lock_lds_bytes(const KParams &p, bool dist) {
    const size_t S = 4 * (size_t)(p.W + 6), NP = (size_t)p.lock_mod;
    return sizeof(uint32_t) * (kAfterCols + 2 * S + 2 * NP * S) + (dist ? sizeof(uint16_t) * NP * S * 32 : 0);
}

hipError_t launch_lock_set(const KParams &p, uint32_t *rows, int32_t *pos, int64_t cap, int32_t *count, hipStream_t s) {
    hipLaunchKernelGGL(k_lock_set, dim3((unsigned)p.n), dim3(kWave), lock_lds_bytes(p, false), s, p, rows, pos, cap,
                       count);  // one wave per env
    return hipGetLastError();
}

hipError_t launch_afterstates_at(const KParams &p, int set, const int32_t *pos, int64_t cap, int32_t *feat,
                                 uint32_t *boards, hipStream_t s) {
    const dim3 grid((unsigned)p.n), block(kWave);  // one wave per env
    if (set == ST_FEATS_BCTS) hipLaunchKernelGGL((k_afterstates_at<ST_FEATS_BCTS>), grid, block, 0, s, p, pos, cap, feat, boards);
    else if (set == ST_FEATS_BASE) hipLaunchKernelGGL((k_afterstates_at<ST_FEATS_BASE>), grid, block, 0, s, p, pos, cap, feat, boards);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_locks(const KParams &p, int set, const float *weights, int64_t n_w, const int32_t *pos_in,
                        const uint8_t *need, int32_t *rem, int32_t *pos, uint64_t *route, int32_t *steps,
                        float *scores, int32_t *best, int32_t *count, hipStream_t s) {
    const dim3 grid((unsigned)p.n), block(kWave);  // one wave per env
    const size_t lds = lock_lds_bytes(p, true);
    const LockIO io{pos_in, need, rem, weights, n_w, pos, route, steps, scores, best, count};
    if (set == ST_FEATS_BCTS) hipLaunchKernelGGL((k_locks<ST_FEATS_BCTS>), grid, block, lds, s, p, io);
    else if (set == ST_FEATS_BASE) hipLaunchKernelGGL((k_locks<ST_FEATS_BASE>), grid, block, lds, s, p, io);
    else if (set == -1) hipLaunchKernelGGL((k_locks<-1>), grid, block, lds, s, p, io);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace st
