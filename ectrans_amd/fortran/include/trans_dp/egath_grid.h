! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(egath_grid)
#undef egath_grid
#endif
#if defined(EGATH_GRID)
#undef EGATH_GRID
#endif
#include "../egath_grid_dp.h"
#define egath_grid EGATH_GRID_DP
#define EGATH_GRID EGATH_GRID_DP
