! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(edist_spec)
#undef edist_spec
#endif
#if defined(EDIST_SPEC)
#undef EDIST_SPEC
#endif
#include "../edist_spec_sp.h"
#define edist_spec EDIST_SPEC_SP
#define EDIST_SPEC EDIST_SPEC_SP
