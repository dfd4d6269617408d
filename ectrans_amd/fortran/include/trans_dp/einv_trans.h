! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(einv_trans)
#undef einv_trans
#endif
#if defined(EINV_TRANS)
#undef EINV_TRANS
#endif
#include "../einv_trans_dp.h"
#define einv_trans EINV_TRANS_DP
#define EINV_TRANS EINV_TRANS_DP
