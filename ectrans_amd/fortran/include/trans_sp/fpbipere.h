! Automatically generated interface header for backward compatibility of generic symbols !
#if defined(fpbipere)
#undef fpbipere
#endif
#if defined(FPBIPERE)
#undef FPBIPERE
#endif
#include "../fpbipere_sp.h"
#define fpbipere FPBIPERE_SP
#define FPBIPERE FPBIPERE_SP
