// st_routes.hip -- k_routes (st_routes, st_policy_routed, st_play_routed) and
// k_route_pop as a translation unit of their own.  Entry points:
// launch_routes, launch_route_pop.  They use the core's piece table
// (st_kernels.hip), the column staging, evaluator and score (st_eval.h) and
// the search helpers (st_search.h) and are compiled apart from every other
// kernel so that every other code object stays exactly as it was
// (st_kernels.hip, top).
#define ST_SIDE_TU 1
#include "st_kernels.hip"
#include "st_eval.h"
#include "st_search.h"

namespace st {
namespace {

// ---------------------------------------------------------------- routes
// st_routes / st_policy_routed / st_play_routed: the whole shortest route of
// the live piece into a slot (simpletetris.h, "Routes"), planned once a piece.
// One wave per env, a lane per slot, whole-row bit sets, as k_reachable; an
// env that is not needed leaves after one load, on a wave-uniform test.
//  (a) forward   k_reachable's untagged search: R[s] != kReachNone iff slot s
//                is reachable (the planner only).
//  (b) choice    k_policy_linear_set's pass over the slots -- eval_slot_set,
//                lin_score, the two wave_reduces -- with R as the mask (the
//                planner only; st_routes reads its target instead).
//  (c) backward  B[l][s]: the states with D <= layer, D(x) the length of the
//                shortest sequence from x that locks at the target's landing.
//                A layer evaluates the step rule on every state at once:
//                  E[l]  a piece that ARRIVES at (s, y) in plane l after
//                        gravity ends well: in the air it must be in B[l], on
//                        the ground in B[l + 1] -- or, from the last plane, at
//                        the target's landing (the lock);
//                  Q[l]  a piece that stands at (s, y) in plane l after the
//                        ACTION ends well: gravity moves it a row (to plane 0
//                        under step_reset) where the row below is free;
//                  P[l]  some action ends well: Q itself (idle and every
//                        refused action), a neighbour's Q where the neighbour
//                        is free (left / right / the two rotations), Q a row
//                        down (soft drop), and the upward occluded fill of the
//                        grounded rows of Q (hard drop: route_rise, the mirror
//                        of reach_fall).
//                A state that joins B at layer k gets D = k in a uint16 per
//                state (D[l][s][32]).  The search ends when the start state
//                joins (its layer is steps[s]) or when no set grew.
//  (d) walk      from the start state, at most ST_ROUTE_MAX times: lanes 0..6
//                apply one action each (k_reachable's layer-1 rule), a ballot
//                picks the lowest whose successor has D one lower (for D = 1:
//                that locks at the landing), its state is the next.
// LDS: column words, F and R, two copies of the forward sets -- reused as B and
// Q --, and D: 4 * (48 + 2 S + 2 (L + 1) S) + 64 (L + 1) S bytes.
struct RouteIO {
    const int32_t *slots_in;  // st_routes: the targets int32 [n]
    const uint8_t *need;      // uint8 [n] or null: every env
    int32_t *rem;             // st_play_routed: an env is needed iff rem[e] == 0, and gets min(steps, ST_ROUTE_MAX)
    const float *wts;         // the planner: float [n_w][rows]
    int64_t n_w;
    int32_t *slots;           // the planner: the chosen slot int32 [n]
    uint64_t *route;          // uint64 [ST_ROUTE_WORDS][n]
    int32_t *steps;           // int32 [n] or null
    float *scores;            // the planner: float [n] or null
};

// SET: a feature set -- the planner, (a) to (d); -1 -- st_routes, (c) and (d) for slots_in[e]
template <int SET>
__global__ __launch_bounds__(kWave) void k_routes(KParams p, RouteIO io) {
    extern __shared__ uint32_t route_lds[];
    const int lane = threadIdx.x;
    const int64_t e = blockIdx.x;  // the grid is p.n waves
    if (io.rem ? io.rem[e] != 0 : (io.need != nullptr && io.need[e] == 0)) return;  // (wave-uniform)
    const int W = p.W, H = p.H, per = W + 6, S = 4 * per;
    const int NP = p.lock_mod;  // planes: lock counter 0 .. L (the host checked L <= ST_REACH_MAX_LOCK)
    const bool sreset = (p.flags & ST_STEP_RESET) != 0u;
    uint32_t *const C = route_lds;       // column words
    uint32_t *const F = C + kAfterCols;  // [S] free rows
    uint32_t *const R = F + S;           // [S] the forward search's first lock layer
    uint32_t *const A = R + S;           // [2][NP][S]
    uint16_t *const D = reinterpret_cast<uint16_t *>(A + 2 * NP * S);  // [NP][S][32]
    const int setw = NP * S;

    stage_env_columns(C, p, e, lane);
    const uint32_t pw = p.piece[e];
    const uint32_t pid = pw & 7u;
    const int id = (int)(pid < 7u ? pid : 6u);  // (a host-written id 7 stays inside the table)
    const int rot = (int)((pw >> 3) & 3u), cx0 = (int)((pw >> 5) & 63u) + 3, ay = (int)((pw >> 11) & 63u);
    const int lock0 = (int)(pw >> 17) < NP ? (int)(pw >> 17) : NP - 1;  // (as k_reachable reads it)
    const bool start_ok = cx0 < per && ay < 32;  // (k_reachable: such a start reaches no slot)
    wave_sync();
    for (int s = lane; s < S; s += kWave) {
        F[s] = reach_free(C + kAfterP, W, id, s);
        R[s] = kReachNone;
        for (int k = 0; k < 2 * NP; ++k) A[k * S + s] = 0u;
    }
    wave_sync();
    auto is_free = [&](int r, int cx, int y) -> bool {
        return cx >= 0 && cx < per && y < 32 && ((F[r * per + cx] >> y) & 1u);
    };

    int tgt = -1;
    if constexpr (SET >= 0) {
        // (a) k_reachable<false, false>'s layers, its result words in R
        if (start_ok && lane == 0) A[lock0 * S + rot * per + cx0] = 1u << ay;
        wave_sync();
        int cur = 0;
        const int max_fwd = start_ok ? 4 * per * H * NP : 0;
        for (int layer = 1; layer <= max_fwd; ++layer) {
            const uint32_t *const In = A + cur * setw;
            uint32_t *const Out = A + (cur ^ 1) * setw;
            bool grew = false;
            for (int s = lane; s < S; s += kWave) {
                const uint32_t f = F[s], fd = f >> 1;
                const uint32_t tb = (f & 1u) ? 1u << (__builtin_ctz(~f) - 1) : 0u;  // a valid slot's landing
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
                if ((grounded & tb) && R[s] == kReachNone) R[s] = (uint32_t)layer << 3;
            }
            wave_sync();
            cur ^= 1;
            if (!__ballot(grew)) break;
        }

        // (b) k_policy_linear_set's choice, the mask being R
        constexpr int NF = feat_rows(SET);
        const int64_t sd_ = p.stride;
        const int32_t old_holes = p.stats[ST_STAT_HOLES * sd_ + e];
        const int32_t old_height = p.stats[ST_STAT_PIECE_HEIGHT * sd_ + e];
        const uint32_t wrow = io.n_w > e ? (uint32_t)e : (uint32_t)e % (uint32_t)io.n_w;
        float w[NF];
#pragma unroll
        for (int r = 0; r < NF; ++r) w[r] = io.wts[(size_t)wrow * NF + r];
        int32_t bslot = -1;
        float bscore = 0.0f;
        for (int s0 = 0; s0 < S; s0 += kWave) {
            const int s = s0 + lane;
            const bool live = s < S;
            int32_t f[NF];
            bool valid = eval_slot_set<SET>(C + kAfterP, W, H, p.flags, id, live ? s : S - 1, old_holes, old_height, f,
                                            [](int, uint32_t, bool) {});
            valid = valid && live && R[live ? s : 0] != kReachNone;
            const float sc = lin_score(w, f);
            if (valid && (bslot < 0 || sc > bscore)) {  // (a lane's slots ascend: the first maximum stays)
                bslot = s;
                bscore = sc;
            }
        }
        const bool has = bslot >= 0;
        const float top =
            __int_as_float(wave_reduce(__float_as_int(has ? bscore : -__builtin_inff()), [](int a, int b) {
                return __float_as_int(__builtin_fmaxf(__int_as_float(a), __int_as_float(b)));
            }));
        bool tied = has && bscore == top;
        if (__ballot(tied) == 0) tied = has;  // (a NaN score equals nothing: every candidate counts)
        const int32_t win = wave_reduce(tied ? bslot : INT32_MAX, [](int a, int b) { return a < b ? a : b; });
        const bool none = win == INT32_MAX;
        if (none ? lane == 0 : tied && bslot == win) {
            io.slots[e] = none ? -1 : win;
            if (io.scores) io.scores[e] = none ? 0.0f : bscore;
        }
        tgt = none ? -1 : win;
        wave_sync();
        for (int s = lane; s < S; s += kWave)
            for (int k = 0; k < NP; ++k) A[k * S + s] = 0u;  // B
        wave_sync();
    } else {
        tgt = io.slots_in[e];
        if (tgt < 0 || tgt >= S) tgt = -1;
    }

    // (c) the backward layers
    uint32_t *const B = A, *const Q = A + setw;
    const int s_start = rot * per + (cx0 < per ? cx0 : 0);
    const uint32_t ftgt = tgt >= 0 ? F[tgt] : 0u;
    const bool search = start_ok && (ftgt & 1u);
    const uint32_t tland = search ? 1u << (__builtin_ctz(~ftgt) - 1) : 0u;  // the target's landing row
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

    // (d) the walk
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

// st_play_routed's pop: one lane per env takes its route's next action (2
// without a route) and counts the piece with a route's last one.
__global__ __launch_bounds__(256) void k_route_pop(int64_t n, const uint64_t *__restrict__ route,
                                                   const int32_t *__restrict__ steps, int32_t *__restrict__ rem,
                                                   uint8_t *__restrict__ act, int32_t *__restrict__ pieces) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int32_t r = rem[e];
    uint32_t a = 2u;
    if (r > 0) {
        const int32_t st = steps[e];
        const int i = (st < ST_ROUTE_MAX ? st : ST_ROUTE_MAX) - r;
        a = (uint32_t)(route[(int64_t)(i / 21) * n + e] >> (3 * (i % 21))) & 7u;
        rem[e] = r - 1;
        if (pieces && r == 1 && st <= ST_ROUTE_MAX) pieces[e] += 1;
    }
    act[e] = (uint8_t)a;
}

}  // namespace

// column words, free / result words, two copies of the sets, one uint16 per piece state
static size_t route_lds_bytes(const KParams &p) {
    const size_t S = 4 * (size_t)(p.W + 6), NP = (size_t)p.lock_mod;
    return sizeof(uint32_t) * (kAfterCols + 2 * S + 2 * NP * S) + sizeof(uint16_t) * NP * S * 32;
}

hipError_t launch_routes(const KParams &p, int set, const float *weights, int64_t n_w, const int32_t *slots_in,
                         const uint8_t *need, int32_t *rem, int32_t *slots, uint64_t *route, int32_t *steps,
                         float *scores, hipStream_t s) {
    const dim3 grid((unsigned)p.n), block(kWave);  // one wave per env
    const size_t lds = route_lds_bytes(p);
    const RouteIO io{slots_in, need, rem, weights, n_w, slots, route, steps, scores};
    if (set == ST_FEATS_BCTS) hipLaunchKernelGGL((k_routes<ST_FEATS_BCTS>), grid, block, lds, s, p, io);
    else if (set == ST_FEATS_BASE) hipLaunchKernelGGL((k_routes<ST_FEATS_BASE>), grid, block, lds, s, p, io);
    else if (set == -1) hipLaunchKernelGGL((k_routes<-1>), grid, block, lds, s, p, io);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_route_pop(const KParams &p, const uint64_t *route, const int32_t *steps, int32_t *rem, uint8_t *act,
                            int32_t *pieces, hipStream_t s) {
    hipLaunchKernelGGL(k_route_pop, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p.n, route, steps, rem, act,
                       pieces);
    return hipGetLastError();
}

}  // namespace st
