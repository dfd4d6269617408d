! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(egath_grid)
#undef egath_grid
#endif
#if defined(EGATH_GRID)
#undef EGATH_GRID
#endif
#include "../egath_grid_sp.h"
#define egath_grid EGATH_GRID_SP
#define EGATH_GRID EGATH_GRID_SP
