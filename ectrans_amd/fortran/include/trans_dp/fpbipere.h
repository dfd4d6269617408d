! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(fpbipere)
#undef fpbipere
#endif
#if defined(FPBIPERE)
#undef FPBIPERE
#endif
#include "../fpbipere_dp.h"
#define fpbipere FPBIPERE_DP
#define FPBIPERE FPBIPERE_DP
