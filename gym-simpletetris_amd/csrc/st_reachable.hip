// st_reachable.hip -- k_reachable (st_reachable, st_route_actions) as a
// translation unit of its own: the kernel and its launchers live in
// st_kernels.hip beside the piece table and the column staging they share with
// k_afterstates, and are compiled here, apart from every other kernel, so that
// adding them leaves the code objects of the step, rollout, export and
// afterstate kernels exactly as they were (st_kernels.hip, top).
#define ST_REACHABLE_TU 1
#include "st_kernels.hip"
