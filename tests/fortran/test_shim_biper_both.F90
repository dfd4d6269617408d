! FPBIPERE, ETIBIHIE and HORIZ_FIELD of BOTH precision libraries in one executable, under their suffixed names (include/*_dp.h and
! *_sp.h).  C+I (21 x 17) of two fields is HORIZ_FIELD and its mirror image, the domain is 30 x 24.  Checked: the test field stays within
! 280 (1 +- 0.1); E comes out finite and C+I unchanged; ETIBIHIE on the PGPBI(KDLON, KNUBI, KDGL) layout gives FPBIPERE's values exactly (the
! same arithmetic on another layout); the two precisions agree to single precision.  Exit code 0 = pass.
PROGRAM TEST_SHIM_BIPER_BOTH
USE, INTRINSIC :: ISO_C_BINDING, ONLY : C_INT32_T, C_FLOAT, C_DOUBLE
IMPLICIT NONE
#include "setup_trans0.h"
#include "fpbipere_dp.h"
#include "fpbipere_sp.h"
#include "etibihie_dp.h"
#include "etibihie_sp.h"
#include "horiz_field_dp.h"
#include "horiz_field_sp.h"
INTEGER(C_INT32_T), PARAMETER :: X = 30, Y = 24, UX = 21, UY = 17, NF = 2
REAL(C_DOUBLE) :: ZH(UX,UY), ZA(X*Y,NF), ZE(X,NF,Y), ZNAN
REAL(C_FLOAT) :: ZHS(UX,UY), ZAS(X*Y,NF), ZES(X,NF,Y)
INTEGER(C_INT32_T) :: JX, JY, JF

CALL SETUP_TRANS0(KPRINTLEV=0, LDMPOFF=.TRUE., KMAX_RESOL=1)
CALL HORIZ_FIELD_DP(UX, UY, ZH)
CALL HORIZ_FIELD_SP(UX, UY, ZHS)
IF (MINVAL(ZH) < 251._C_DOUBLE .OR. MAXVAL(ZH) > 309._C_DOUBLE .OR. MAXVAL(ABS(ZH - REAL(ZHS,C_DOUBLE))) > 1E-3_C_DOUBLE) ERROR STOP 2
ZNAN = 0
ZNAN = ZNAN/ZNAN
ZA = ZNAN
ZE = ZNAN
DO JY = 1, UY
  DO JX = 1, UX
    ZA((JY-1)*X + JX, 1) = ZH(JX,JY)
    ZA((JY-1)*X + JX, 2) = ZH(UX+1-JX,UY+1-JY)
    ZE(JX,1,JY) = ZH(JX,JY)
    ZE(JX,2,JY) = ZH(UX+1-JX,UY+1-JY)
  ENDDO
ENDDO
ZAS = REAL(ZA, C_FLOAT)
ZES = REAL(ZE, C_FLOAT)
CALL FPBIPERE_DP(UX, UY, X, Y, NF, X*Y, ZA, 0, LDZON=.TRUE.)
CALL FPBIPERE_SP(UX, UY, X, Y, NF, X*Y, ZAS, 0, LDZON=.TRUE.)
CALL ETIBIHIE_DP(X, Y, NF, UX, UY, 1, X, ZE, .TRUE., .TRUE., 0)
CALL ETIBIHIE_SP(X, Y, NF, UX, UY, 1, X, ZES, .TRUE., .TRUE., 0)
DO JF = 1, NF
  DO JY = 1, Y
    DO JX = 1, X
      IF (.NOT. (ABS(ZA((JY-1)*X + JX, JF)) < 1000._C_DOUBLE)) ERROR STOP 3
      IF (ZA((JY-1)*X + JX, JF) /= ZE(JX,JF,JY)) ERROR STOP 4
      IF (ZAS((JY-1)*X + JX, JF) /= ZES(JX,JF,JY)) ERROR STOP 5
      IF (ABS(ZA((JY-1)*X + JX, JF) - REAL(ZAS((JY-1)*X + JX, JF), C_DOUBLE)) > 2E-2_C_DOUBLE) ERROR STOP 6
    ENDDO
  ENDDO
ENDDO
DO JY = 1, UY
  DO JX = 1, UX
    IF (ZA((JY-1)*X + JX, 1) /= ZH(JX,JY) .OR. ZAS((JY-1)*X + JX, 1) /= REAL(ZH(JX,JY), C_FLOAT)) ERROR STOP 7
  ENDDO
ENDDO
PRINT '(A)', 'FORTRAN SHIM BIPER OK (dp and sp)'
END PROGRAM TEST_SHIM_BIPER_BOTH
