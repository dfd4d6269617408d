! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(especnorm)
#undef especnorm
#endif
#if defined(ESPECNORM)
#undef ESPECNORM
#endif
#include "../especnorm_sp.h"
#define especnorm ESPECNORM_SP
#define ESPECNORM ESPECNORM_SP
