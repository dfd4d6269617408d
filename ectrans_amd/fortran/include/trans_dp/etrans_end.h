! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(etrans_end)
#undef etrans_end
#endif
#if defined(ETRANS_END)
#undef ETRANS_END
#endif
#include "../etrans_end_dp.h"
#define etrans_end ETRANS_END_DP
#define ETRANS_END ETRANS_END_DP
