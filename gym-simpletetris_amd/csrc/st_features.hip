// st_features.hip -- k_afterstates_set and k_policy_linear_set (st_afterstates_set,
// st_policy_linear_set, st_play_linear_set: the ST_FEATS_BCTS rows, and the
// slot mask) as a translation unit of their own: the kernels, their evaluator
// eval_slot_set and their launchers live in st_kernels.hip beside the helpers
// they share with the afterstates module, and are compiled here, apart from
// it, so that adding them leaves the code objects of k_afterstates and
// k_policy_linear exactly as they were (st_kernels.hip, top).
#define ST_FEATURES_TU 1
#include "st_kernels.hip"
