// st_expect.hip -- k_next_weights and k_policy_expect (st_next_weights,
// st_policy_expect, st_play_expect: the odds of the next piece as an output,
// and the expectimax player over them) as a translation unit of their own: the
// kernels and their launchers live in st_kernels.hip beside the evaluator
// (eval_slot_set), the chain (lin_score) and the reductions they share with the
// other modules, and are compiled here, apart from them, so that adding them
// leaves the code objects of every other kernel exactly as they were
// (st_kernels.hip, top).
#define ST_EXPECT_TU 1
#include "st_kernels.hip"
