// st_step_packed.hip -- st_step's packed-obs kernels (k_step<.., F32 = false,
// ..>: the prologue-draw schedule, step_draw_once) and their launcher as a
// translation unit of their own.  The kernels live in st_kernels.hip beside
// the step waves they share with the float32 step and k_rollout2, and are
// compiled here, apart from them: instantiated in the library's own module,
// step_draw_once changed the code the compiler emits for the float32 k_step,
// whose source it does not touch (st_kernels.hip, top).
#define ST_STEP_PACKED_TU 1
#include "st_kernels.hip"
