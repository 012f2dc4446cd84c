// st_routes.hip -- k_routes (st_routes, st_policy_routed, st_play_routed) and
// k_route_pop as a translation unit of their own: the kernels and their
// launchers live in st_kernels.hip beside the piece table, the column staging,
// the slot evaluators and the search helpers they share with k_reachable and
// k_policy_linear_set, and are compiled here, apart from every other kernel, so
// that adding them leaves every other code object exactly as it was
// (st_kernels.hip, top).
#define ST_ROUTES_TU 1
#include "st_kernels.hip"
