! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(esetup_trans)
#undef esetup_trans
#endif
#if defined(ESETUP_TRANS)
#undef ESETUP_TRANS
#endif
#include "../esetup_trans_sp.h"
#define esetup_trans ESETUP_TRANS_SP
#define ESETUP_TRANS ESETUP_TRANS_SP
