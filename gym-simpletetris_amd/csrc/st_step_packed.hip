// st_step_packed.hip -- st_step's packed-obs kernels (k_step<.., F32 = false,
// ..>: the prologue-draw schedule, step_draw_once), entry point
// launch_step_packed, as a translation unit of their own.  k_step itself is
// core text (st_kernels.hip); it is instantiated here, apart from the float32
// step: instantiated in the library's own module, step_draw_once changed the
// code the compiler emits for the float32 k_step, whose source it does not
// touch (st_kernels.hip, top).
#define ST_SIDE_TU 1
#include "st_kernels.hip"

namespace st {

// st_step's packed-obs launches (every k_step<.., F32 = false, ..>: the
// prologue-draw schedule, step_draw_once); launch_step keeps the float32 ones
hipError_t launch_step_packed(const KParams &p, hipStream_t s) {
    const dim3 grid((unsigned)(p.stride / kWave)), block(2 * kWave);  // logic + draw wave
    const bool sc0 = !(p.flags & kScoringFlags);
    if (p.final_obs || p.info || p.gate) {  // st_step_vec: the vector env's outputs (VEC); gated launches
        if (p.W == 10 && p.H == 20) {
            if (sc0) hipLaunchKernelGGL((k_step<10, 20, false, false, true, true>), grid, block, 0, s, ST_STEP_ARGS(p));
            else hipLaunchKernelGGL((k_step<10, 20, false, false, false, true>), grid, block, 0, s, ST_STEP_ARGS(p));
        } else {
            hipLaunchKernelGGL((k_step<0, 0, false, false, false, true>), grid, block, 0, s, ST_STEP_ARGS(p));
        }
    } else if (p.stamps && p.W == 10 && p.H == 20) {
        if (sc0) hipLaunchKernelGGL((k_step<10, 20, false, true, true>), grid, block, 0, s, ST_STEP_ARGS(p));
        else hipLaunchKernelGGL((k_step<10, 20, false, true>), grid, block, 0, s, ST_STEP_ARGS(p));
    } else if (p.W == 10 && p.H == 20) {
        if (sc0) hipLaunchKernelGGL((k_step<10, 20, false, false, true>), grid, block, 0, s, ST_STEP_ARGS(p));
        else hipLaunchKernelGGL((k_step<10, 20, false>), grid, block, 0, s, ST_STEP_ARGS(p));
    } else {
        hipLaunchKernelGGL((k_step<0, 0, false>), grid, block, 0, s, ST_STEP_ARGS(p));
    }
    return hipGetLastError();
}

}  // namespace st
