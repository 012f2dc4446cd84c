// st_afterstates.hip -- k_afterstates (st_afterstates), k_placement_actions
// (st_placement_actions), k_place (st_place, st_step_placements),
// k_policy_linear and k_play_sum (st_policy_linear, st_play_linear,
// st_play_linear_placements) as a translation unit of their own: the kernels and
// their launchers live in st_kernels.hip beside the piece table and the
// collision / drop / clear / scoring helpers they share with the step
// kernels, and are compiled here, apart from them, so that adding them leaves
// the code objects of k_step / k_rollout / k_rollout2 / k_step_export exactly
// as they were (st_kernels.hip, top).
#define ST_AFTERSTATES_TU 1
#include "st_kernels.hip"
