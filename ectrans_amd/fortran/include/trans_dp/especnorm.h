! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(especnorm)
#undef especnorm
#endif
#if defined(ESPECNORM)
#undef ESPECNORM
#endif
#include "../especnorm_dp.h"
#define especnorm ESPECNORM_DP
#define ESPECNORM ESPECNORM_DP
