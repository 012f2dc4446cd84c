// st_step_export.hip -- k_step_export (st_step + st_export_env in one launch),
// entry point launch_step_export, as a translation unit of its own: it shares
// the step waves and export_record with the core (st_kernels.hip) and is
// compiled here, apart from k_step, so that the code objects of k_step /
// k_rollout / k_rollout2 stay exactly as they were (st_kernels.hip, top).
#define ST_SIDE_TU 1
#include "st_kernels.hip"

namespace st {
namespace {

// st_step_export: k_step (packed outputs, no stamps, not gated) with the
// export record of one env written by the workgroup that stepped it -- the
// single-env surface's step and read-back in ONE launch.  Both waves run
// step_logic / step_draw_once unchanged and meet at one more workgroup barrier
// (each has passed B0 once: neither role returns early without VEC);
// behind it the workgroup's 128 threads write the record from what the two
// waves stored to global memory moments before: obs / reward / done and the
// hot counter rows (logic wave), the count rows, the MT index word, the MT
// words and the next-generation chunk (draw wave).
// What orders the tail's loads behind those stores ("The fused
// tail"): (1) each wave waits for its own stores before it arrives -- an
// explicit s_waitcnt vmcnt(0), because a workgroup-scope release fence on
// gfx950 waits for LDS traffic only and s_barrier waits for no counter; a
// store counted out of vmcnt has been acknowledged by L2, `nt` or not;
// (2) the workgroup barrier; (3) the tail's loads are issued behind it (the
// acquire fence keeps the compiler from moving them up), are vector loads
// (memory the kernel itself stored to is never read through the scalar
// cache) and non-temporal, i.e. served by L2, where the stores are.  Were
// they served by the CU's L1 instead, the LLVM AMDGPU memory model's rule for
// gfx942 / gfx950 would hold: the waves of a workgroup share one
// write-through L1 (no threadgroup-split mode here), which their stores
// went through.  Other workgroups skip the wait, the barrier and the tail
// (the branch is workgroup-uniform): for them this is k_step.
template <int WT, int HT, bool SC0>
__global__ __launch_bounds__(2 * kWave) void k_step_export(uint32_t *board, int32_t *stats, const uint8_t *actions,
                                                           uint32_t *mt, int64_t stride, int64_t n, KParams p0,
                                                           int64_t env, uint32_t *obs, int32_t *rew, uint8_t *done,
                                                           uint32_t parts, uint32_t *out) {
    KParams p = p0;
    p.board = board;
    p.stats = stats;
    p.actions = actions;
    p.mt = mt;
    p.stride = stride;
    p.n = n;
    p.obs = obs;
    p.reward = rew;
    p.done = done;
    __shared__ StepLds<WT, false, 1> sm;
    if (threadIdx.x < kWave) step_logic<WT, HT, false, false, 1, SC0, false>(p, sm);
    else step_draw_once<WT, HT, false, false, SC0, false>(p, sm);
    if ((int64_t)blockIdx.x != env / kWave) return;
    __builtin_amdgcn_s_setprio(0);  // the tail is nobody's critical chain
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores have reached L2
    wg_barrier();
    export_record(p, env, obs, rew, done, parts, out, (int)threadIdx.x, 2 * kWave);
}

}  // namespace

hipError_t launch_step_export(const KParams &p, int64_t env, uint32_t parts, uint32_t *out, hipStream_t s) {
    const dim3 grid((unsigned)(p.stride / kWave)), block(2 * kWave);  // logic + draw wave
#define ST_STEP_EXPORT_ARGS ST_STEP_ARGS(p), env, p.obs, p.reward, p.done, parts, out
    if (p.W == 10 && p.H == 20) {
        if (!(p.flags & kScoringFlags)) hipLaunchKernelGGL((k_step_export<10, 20, true>), grid, block, 0, s, ST_STEP_EXPORT_ARGS);
        else hipLaunchKernelGGL((k_step_export<10, 20, false>), grid, block, 0, s, ST_STEP_EXPORT_ARGS);
    } else {
        hipLaunchKernelGGL((k_step_export<0, 0, false>), grid, block, 0, s, ST_STEP_EXPORT_ARGS);
    }
#undef ST_STEP_EXPORT_ARGS
    return hipGetLastError();
}

}  // namespace st
