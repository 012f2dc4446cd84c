// st_step_export.hip -- k_step_export (st_step + st_export_env in one launch)
// as a translation unit of its own: the kernel and its launcher live in
// st_kernels.hip beside the step waves they share with k_step, and are
// compiled here, apart from it, so that adding them leaves the code objects
// of k_step / k_rollout / k_rollout2 exactly as they were (st_kernels.hip,
// top).
#define ST_STEP_EXPORT_TU 1
#include "st_kernels.hip"
