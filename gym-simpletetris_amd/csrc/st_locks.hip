// st_locks.hip -- k_lock_set, k_afterstates_at and k_locks (st_lock_set,
// st_afterstates_at, st_routes_at, st_policy_locks, st_play_locks) as a
// translation unit of their own: the kernels and their launchers live in
// st_kernels.hip beside the piece table, the column staging, the slot
// evaluators and the search helpers they share with k_reachable and k_routes,
// and are compiled here, apart from every other kernel, so that adding them
// leaves every other code object exactly as it was (st_kernels.hip, top).
#define ST_LOCKS_TU 1
#include "st_kernels.hip"
