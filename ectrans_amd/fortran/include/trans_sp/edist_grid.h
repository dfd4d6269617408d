! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(edist_grid)
#undef edist_grid
#endif
#if defined(EDIST_GRID)
#undef EDIST_GRID
#endif
#include "../edist_grid_sp.h"
#define edist_grid EDIST_GRID_SP
#define EDIST_GRID EDIST_GRID_SP
