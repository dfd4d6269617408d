! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(etrans_release)
#undef etrans_release
#endif
#if defined(ETRANS_RELEASE)
#undef ETRANS_RELEASE
#endif
#include "../etrans_release_sp.h"
#define etrans_release ETRANS_RELEASE_SP
#define ETRANS_RELEASE ETRANS_RELEASE_SP
