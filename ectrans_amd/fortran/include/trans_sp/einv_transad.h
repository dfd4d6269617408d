! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(einv_transad)
#undef einv_transad
#endif
#if defined(EINV_TRANSAD)
#undef EINV_TRANSAD
#endif
#include "../einv_transad_sp.h"
#define einv_transad EINV_TRANSAD_SP
#define EINV_TRANSAD EINV_TRANSAD_SP
