! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(einv_transad)
#undef einv_transad
#endif
#if defined(EINV_TRANSAD)
#undef EINV_TRANSAD
#endif
#include "../einv_transad_dp.h"
#define einv_transad EINV_TRANSAD_DP
#define EINV_TRANSAD EINV_TRANSAD_DP
