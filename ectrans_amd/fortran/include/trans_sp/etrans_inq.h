! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(etrans_inq)
#undef etrans_inq
#endif
#if defined(ETRANS_INQ)
#undef ETRANS_INQ
#endif
#include "../etrans_inq_sp.h"
#define etrans_inq ETRANS_INQ_SP
#define ETRANS_INQ ETRANS_INQ_SP
