// st_fork.hip -- k_fork (st_fork) as a translation unit of its own.  Entry
// point: launch_fork.  It uses the core's MT19937 layout and mt_sync_lanes
// (st_kernels.hip), which it shares with k_mt_sync, and is compiled apart from
// every other kernel so that every other code object stays exactly as it was
// (st_kernels.hip, top).
#define ST_SIDE_TU 1
#include "st_kernels.hip"

namespace st {
namespace {

// ---------------------------------------------------------------- fork
// st_fork: env e of p (dst) takes the state of env index[e] of f (src) --
// copy.deepcopy of the TetrisEngine with random.getstate(), or with KEEP
// (ST_FORK_KEEP_RNG) the engine alone while the env keeps its own stream.
// One workgroup of WAVES waves per 64 dst envs.  Every wave reads the 64
// indices and mask bytes (an env is WRITTEN iff it is real, masked in and its
// index lies in [0, f.n): nothing else is ever read or stored, so padding envs
// are neither sources nor targets).  Wave 0, lane = env, copies the W board
// rows and the counter rows: the stores into dst's SoA rows are coalesced, the
// loads gathers by index (one address for a broadcast).  Deep copy: the written
// lanes' MT rows -- kMtPitch words: both generation buffers and the pad, so the
// progress bits, a pending preview and its consumed-word count in the index
// word stay true of them -- are then copied one env at a time, 16 B per lane
// (kMtPitch * 4 = 316 * 16 B, every row base 16-B aligned), the written lanes
// dealt round robin to the waves, each wave loading its next row before it
// stores the present one.  (WAVES = 1 is the library's grid: four waves per
// 64 envs measured no faster, DESIGN.md "Fork".)  KEEP: no MT row moves; the written envs are put into
// CPython's form first (mt_sync_lanes: a preview they hold was drawn under the
// old shape counts, tetris_env.py:183-191, so its words go back), which wave 0
// does alone.
struct ForkSrc {
    const uint32_t *board;  // [W][stride]
    const int32_t *stats;   // [ST_NSTAT][stride]
    const uint32_t *mt;     // [stride][kMtPitch]
    int64_t n, stride;
    const int32_t *index;   // [p.n] or null: e
    const uint8_t *mask;    // [p.n] or null: every env
    int32_t same;           // f is p's own context: a deep copy of an env onto itself is skipped
};
constexpr int kMtRowQ = (int)(kMtPitch / 4);        // 16-B words of an MT row
constexpr int kForkQ = (kMtRowQ + kWave - 1) / kWave;  // per lane
static_assert(kMtPitch % 4 == 0, "MT rows are copied in 16-B accesses");

template <int WAVES, bool KEEP>
__global__ __launch_bounds__(WAVES *kWave) void k_fork(KParams p, ForkSrc f) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t e0 = (int64_t)blockIdx.x * kWave;
    const int64_t e = e0 + lane;
    const int64_t sd = p.stride, ss = f.stride;
    bool wr = e < p.n && (f.mask == nullptr || f.mask[e] != 0);
    int64_t s64 = e;
    if (e < p.n && f.index) s64 = f.index[e];
    wr = wr && s64 >= 0 && s64 < f.n;
    if (!KEEP && f.same && s64 == e) wr = false;
    const int s = wr ? (int)s64 : 0;  // (f.n <= 2^24)

    [[maybe_unused]] int idx = 0;
    if constexpr (KEEP) {
        const uint32_t r = wr ? (uint32_t)p.stats[(int64_t)ST_STAT_MT_INDEX * sd + e] : 0u;
        idx = mt_sync_lanes(p.mt, e0, r, wr, lane);
    }
    if (wave == 0 && wr) {
        int32_t t[ST_NSTAT];
#pragma unroll
        for (int r = 0; r < ST_NSTAT; ++r)
            t[r] = KEEP && r == ST_STAT_MT_INDEX ? idx : f.stats[(int64_t)r * ss + s];
        for (int x0 = 0; x0 < p.W; x0 += 8) {
            uint32_t b[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) b[j] = x0 + j < p.W ? f.board[(int64_t)(x0 + j) * ss + s] : 0u;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (x0 + j < p.W) p.board[(int64_t)(x0 + j) * sd + e] = b[j];
        }
#pragma unroll
        for (int r = 0; r < ST_NSTAT; ++r) p.stats[(int64_t)r * sd + e] = t[r];
    }
    if constexpr (!KEEP) {
        uint64_t m = __ballot(wr);
        int turn = 0;
        auto next = [&]() -> int {  // the wave's next written lane, or -1 (wave-uniform)
            while (m) {
                const int l = (int)__builtin_ctzll(m);
                m &= m - 1;
                if (turn++ % WAVES == wave) return l;
            }
            return -1;
        };
        auto load = [&](int l, u32x4(&v)[kForkQ]) {
            const u32x4 *g = reinterpret_cast<const u32x4 *>(f.mt + (int64_t)__builtin_amdgcn_readlane(s, l) * kMtPitch);
#pragma unroll
            for (int q = 0; q < kForkQ; ++q) {
                const int i = lane + kWave * q;
                if (i < kMtRowQ) v[q] = g[i];
            }
        };
        u32x4 a[kForkQ] = {}, b[kForkQ] = {};
        int l = next();
        if (l >= 0) load(l, a);
        while (l >= 0) {
            const int ln = next();
            if (ln >= 0) load(ln, b);
            u32x4 *g = reinterpret_cast<u32x4 *>(p.mt + (e0 + l) * kMtPitch);
#pragma unroll
            for (int q = 0; q < kForkQ; ++q) {
                const int i = lane + kWave * q;
                if (i < kMtRowQ) g[i] = a[q];
            }
#pragma unroll
            for (int q = 0; q < kForkQ; ++q) a[q] = b[q];
            l = ln;
        }
    }
}

}  // namespace

hipError_t launch_fork(const KParams &dst, const KParams &src, const int32_t *index, const uint8_t *mask, bool keep_rng,
                       int waves, hipStream_t s) {
    const ForkSrc f{src.board, src.stats, src.mt, src.n, src.stride, index, mask, dst.stats == src.stats};
    const dim3 grid((unsigned)(dst.stride / kWave));
    if (keep_rng) hipLaunchKernelGGL((k_fork<1, true>), grid, dim3(kWave), 0, s, dst, f);
    else if (waves == 1) hipLaunchKernelGGL((k_fork<1, false>), grid, dim3(kWave), 0, s, dst, f);
    else if (waves == 4) hipLaunchKernelGGL((k_fork<4, false>), grid, dim3(4 * kWave), 0, s, dst, f);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace st
