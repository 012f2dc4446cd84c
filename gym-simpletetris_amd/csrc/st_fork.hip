// st_fork.hip -- k_fork (st_fork) as a translation unit of its own: the kernel
// and its launcher live in st_kernels.hip beside the MT19937 layout and
// mt_sync_lanes, which it shares with k_mt_sync, and are compiled here, apart
// from every other kernel, so that adding them leaves every other code object
// exactly as it was (st_kernels.hip, top).
#define ST_FORK_TU 1
#include "st_kernels.hip"
