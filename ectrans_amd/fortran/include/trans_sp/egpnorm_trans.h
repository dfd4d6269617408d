! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(egpnorm_trans)
#undef egpnorm_trans
#endif
#if defined(EGPNORM_TRANS)
#undef EGPNORM_TRANS
#endif
#include "../egpnorm_trans_sp.h"
#define egpnorm_trans EGPNORM_TRANS_SP
#define EGPNORM_TRANS EGPNORM_TRANS_SP
