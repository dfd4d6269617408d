! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(edir_trans)
#undef edir_trans
#endif
#if defined(EDIR_TRANS)
#undef EDIR_TRANS
#endif
#include "../edir_trans_sp.h"
#define edir_trans EDIR_TRANS_SP
#define EDIR_TRANS EDIR_TRANS_SP
