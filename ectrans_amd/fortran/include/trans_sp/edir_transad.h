! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(edir_transad)
#undef edir_transad
#endif
#if defined(EDIR_TRANSAD)
#undef EDIR_TRANSAD
#endif
#include "../edir_transad_sp.h"
#define edir_transad EDIR_TRANSAD_SP
#define EDIR_TRANSAD EDIR_TRANSAD_SP
