! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(horiz_field)
#undef horiz_field
#endif
#if defined(HORIZ_FIELD)
#undef HORIZ_FIELD
#endif
#include "../horiz_field_dp.h"
#define horiz_field HORIZ_FIELD_DP
#define HORIZ_FIELD HORIZ_FIELD_DP
