! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(edist_grid)
#undef edist_grid
#endif
#if defined(EDIST_GRID)
#undef EDIST_GRID
#endif
#include "../edist_grid_dp.h"
#define edist_grid EDIST_GRID_DP
#define EDIST_GRID EDIST_GRID_DP
