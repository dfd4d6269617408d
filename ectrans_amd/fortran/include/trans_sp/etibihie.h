! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(etibihie)
#undef etibihie
#endif
#if defined(ETIBIHIE)
#undef ETIBIHIE
#endif
#include "../etibihie_sp.h"
#define etibihie ETIBIHIE_SP
#define ETIBIHIE ETIBIHIE_SP
