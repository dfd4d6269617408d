! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(etibihie)
#undef etibihie
#endif
#if defined(ETIBIHIE)
#undef ETIBIHIE
#endif
#include "../etibihie_dp.h"
#define etibihie ETIBIHIE_DP
#define ETIBIHIE ETIBIHIE_DP
