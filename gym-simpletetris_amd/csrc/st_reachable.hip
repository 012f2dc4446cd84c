// st_reachable.hip -- k_reachable (st_reachable, st_route_actions) as a
// translation unit of its own.  Entry points: launch_reachable,
// launch_route_actions.  It uses the core's piece table (st_kernels.hip), the
// column staging (st_eval.h) and the set helpers (st_search.h) and is compiled
// apart from every other kernel so that the code objects of the step, rollout,
// export and afterstate kernels stay exactly as they were (st_kernels.hip,
// top).
#define ST_SIDE_TU 1
#include "st_kernels.hip"
#include "st_eval.h"
#include "st_search.h"

namespace st {
namespace {

// k_reachable: the search st_search.h ("reachability") describes.
template <bool TAGGED, bool ROUTE>
__global__ __launch_bounds__(kWave) void k_reachable(KParams p, const int32_t *__restrict__ slots,
                                                     int32_t *__restrict__ steps_out,
                                                     uint8_t *__restrict__ first_out) {
    extern __shared__ uint32_t reach_lds[];
    constexpr int NT = TAGGED ? 7 : 1;
    const int lane = threadIdx.x;
    const int64_t e = blockIdx.x;  // the grid is p.n waves
    const int W = p.W, per = W + 6, S = 4 * per;
    const int NP = p.lock_mod;  // planes: lock counter 0 .. L (the launcher checked L <= ST_REACH_MAX_LOCK)
    const bool sreset = (p.flags & ST_STEP_RESET) != 0u;
    uint32_t *const C = reach_lds;       // column words
    uint32_t *const F = C + kAfterCols;  // [S] free rows
    uint32_t *const T = F + S;           // [S] the landing bit of a valid (ROUTE: the target) slot, else 0
    uint32_t *const R = T + S;           // [S] layer << 3 | tag of the first lock there
    uint32_t *const A = R + S;           // [2][NT][NP][S]
    const int setw = NT * NP * S;

    stage_env_columns(C, p, e, lane);
    const uint32_t pw = p.piece[e];
    const uint32_t pid = pw & 7u;
    const int id = (int)(pid < 7u ? pid : 6u);  // (a host-written id 7 stays inside the table)
    const int rot = (int)((pw >> 3) & 3u), cx0 = (int)((pw >> 5) & 63u) + 3, ay = (int)((pw >> 11) & 63u);
    const int lock0 = (int)(pw >> 17) < NP ? (int)(pw >> 17) : NP - 1;  // (a host-written counter above L: unspecified)
    // a start outside the lane grid or the row word (host-written) can only lock where it is: no slot
    const bool start_ok = cx0 < per && ay < 32;
    int tgt = -1;
    if constexpr (ROUTE) {
        tgt = slots[e];
        if (tgt < 0 || tgt >= S) tgt = -1;
    }
    wave_sync();
    for (int s = lane; s < S; s += kWave) {
        const uint32_t f = reach_free(C + kAfterP, W, id, s);
        F[s] = f;
        // valid: free at row 0; the landing row: the last free row of the run from row 0
        T[s] = (f & 1u) && (!ROUTE || s == tgt) ? 1u << (__builtin_ctz(~f) - 1) : 0u;
        R[s] = kReachNone;
        for (int k = 0; k < NT * NP; ++k) A[k * S + s] = 0u;
    }
    wave_sync();
    bool search = start_ok;
    if constexpr (ROUTE) search = search && tgt >= 0 && T[tgt] != 0u;

    auto is_free = [&](int r, int cx, int y) -> bool {
        return cx >= 0 && cx < per && y < 32 && ((F[r * per + cx] >> y) & 1u);
    };
    if (search) {
        if constexpr (TAGGED) {
            if (lane < 7) {  // layer 1: action `lane` on the start state (:245-262)
                int r = rot, cx = cx0, y = ay, l = lock0;
                if (lane == 0) cx -= is_free(r, cx - 1, y) ? 1 : 0;
                else if (lane == 1) cx += is_free(r, cx + 1, y) ? 1 : 0;
                else if (lane == 2) y += __builtin_ctz(~(y < 31 ? F[r * per + cx] >> (y + 1) : 0u));
                else if (lane == 3) y += is_free(r, cx, y + 1) ? 1 : 0;
                else if (lane == 4) r = is_free((r + 1) & 3, cx, y) ? (r + 1) & 3 : r;
                else if (lane == 5) r = is_free((r + 3) & 3, cx, y) ? (r + 3) & 3 : r;
                if (is_free(r, cx, y + 1)) {
                    ++y;
                    l = sreset ? 0 : l;
                }
                const int s1 = r * per + cx;
                bool locked = false;
                if (!is_free(r, cx, y + 1)) {
                    l = l + 1 == NP ? 0 : l + 1;
                    locked = l == 0;
                }
                if (!locked) A[(lane * NP + l) * S + s1] = 1u << y;
                else if (T[s1] & (1u << y)) atomicMin(&R[s1], 1u << 3 | (uint32_t)lane);
            }
        } else {
            if (lane == 0) A[lock0 * S + rot * per + cx0] = 1u << ay;
        }
    }
    wave_sync();
    if constexpr (ROUTE) search = search && R[tgt < 0 ? 0 : tgt] == kReachNone;

    int cur = 0;
    const int max_layer = search ? 4 * per * p.H * NP : 0;
    for (int layer = TAGGED ? 2 : 1; layer <= max_layer; ++layer) {
        const uint32_t *const In = A + cur * setw;
        uint32_t *const Out = A + (cur ^ 1) * setw;
        bool grew = false, hit = false;
        for (int s = lane; s < S; s += kWave) {
            const uint32_t f = F[s], fd = f >> 1, tb = T[s];  // fd: the row below is free
            // (the first and the last slot are never free: what they read in is masked away)
            const int sl = s > 0 ? s - 1 : 0, sr = s < S - 1 ? s + 1 : s;
            const int su = s + per < S ? s + per : s + per - S, sd = s >= per ? s - per : s - per + S;
            for (int tag = 0; tag < NT; ++tag) {
                const uint32_t *const It = In + tag * NP * S;
                uint32_t *const Ot = Out + tag * NP * S;
                uint32_t mvall = 0;
                for (int l = 0; l < NP; ++l) {  // the action: every destination of plane l
                    const uint32_t *const I = It + l * S;
                    const uint32_t a = I[s];
                    const uint32_t nb = I[sl] | I[sr] | I[su] | I[sd];
                    const uint32_t pos = a | ((nb | (a << 1)) & f) | (reach_fall(a, f) & ~fd);
                    Ot[l * S + s] = pos;  // (the lane's own word: read back below)
                    mvall |= (pos << 1) & f;
                }
                uint32_t grounded = 0;  // of the plane below: its counter moves up to this one
                for (int l = 0; l < NP; ++l) {  // gravity, then _has_dropped and the counter
                    const uint32_t pos = Ot[l * S + s];
                    const uint32_t moved = sreset ? (l == 0 ? mvall : 0u) : (pos << 1) & f;
                    const uint32_t g = (pos & ~fd) | moved;
                    const uint32_t old = It[l * S + s];
                    const uint32_t nw = old | (g & fd) | grounded;
                    Ot[l * S + s] = nw;
                    grew = grew || nw != old;
                    grounded = g & ~fd;
                }
                // `grounded` of the last plane: the counter wraps to 0, the piece locks
                if ((grounded & tb) && R[s] == kReachNone) {
                    R[s] = (uint32_t)layer << 3 | (uint32_t)tag;
                    hit = true;
                }
            }
        }
        wave_sync();
        cur ^= 1;
        if (ROUTE && __ballot(hit)) break;
        if (!__ballot(grew)) break;
    }

    if constexpr (ROUTE) {
        if (lane == 0) {
            const uint32_t r = tgt < 0 ? kReachNone : R[tgt];
            first_out[e] = (uint8_t)(r == kReachNone ? 2u : r & 7u);
            if (steps_out) steps_out[e] = r == kReachNone ? 0 : (int32_t)(r >> 3);
        }
    } else {
        const size_t base = (size_t)e * S;
        for (int s = lane; s < S; s += kWave) {
            const uint32_t r = R[s];
            steps_out[base + s] = r == kReachNone ? 0 : (int32_t)(r >> 3);
            if constexpr (TAGGED) first_out[base + s] = (uint8_t)(r == kReachNone ? 2u : r & 7u);
        }
    }
}

}  // namespace

// column words, free / target / result words, two copies of the sets
static size_t reach_lds_bytes(const KParams &p, int tags) {
    const int S = 4 * (p.W + 6);
    return sizeof(uint32_t) * (size_t)(kAfterCols + 3 * S + 2 * tags * p.lock_mod * S);
}

hipError_t launch_reachable(const KParams &p, int32_t *steps, uint8_t *first, hipStream_t s) {
    const dim3 grid((unsigned)p.n), block(kWave);  // one wave per env
    if (first)
        hipLaunchKernelGGL((k_reachable<true, false>), grid, block, reach_lds_bytes(p, 7), s, p,
                           (const int32_t *)nullptr, steps, first);
    else
        hipLaunchKernelGGL((k_reachable<false, false>), grid, block, reach_lds_bytes(p, 1), s, p,
                           (const int32_t *)nullptr, steps, first);
    return hipGetLastError();
}

hipError_t launch_route_actions(const KParams &p, const int32_t *slots, uint8_t *actions, int32_t *steps,
                                hipStream_t s) {
    hipLaunchKernelGGL((k_reachable<true, true>), dim3((unsigned)p.n), dim3(kWave), reach_lds_bytes(p, 7), s, p, slots,
                       steps, actions);
    return hipGetLastError();
}

}  // namespace st
