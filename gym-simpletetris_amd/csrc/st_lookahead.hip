// st_lookahead.hip -- k_next_piece and k_policy_lookahead (st_next_piece,
// st_policy_lookahead, st_play_lookahead: the preview as an output, and the
// two-ply linear player) as a translation unit of their own: the kernels and
// their launchers live in st_kernels.hip beside the evaluator (eval_slot_set)
// and the draw (draw_shape) they share with the other modules, and are
// compiled here, apart from them, so that adding them leaves the code objects
// of every other kernel exactly as they were (st_kernels.hip, top).
#define ST_LOOKAHEAD_TU 1
#include "st_kernels.hip"
