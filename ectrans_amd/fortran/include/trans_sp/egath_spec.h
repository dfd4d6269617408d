! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(egath_spec)
#undef egath_spec
#endif
#if defined(EGATH_SPEC)
#undef EGATH_SPEC
#endif
#include "../egath_spec_sp.h"
#define egath_spec EGATH_SPEC_SP
#define EGATH_SPEC EGATH_SPEC_SP
