! FPBIPERE, ETIBIHIE and HORIZ_FIELD through the Fortran drop-in under their generic names: compiled against ONE precision through the
! back-compat headers (-Iinclude/trans_dp, or -DEMI_SP -Iinclude/trans_sp).  The program reads a list of calls from <dir>/cases.txt,
! the input arrays as raw files of the library's real kind, and writes each result as a raw file; tests/test_biper_fortran_emu.py
! prepares the inputs from tests/golden/biper and compares the outputs with the goldens byte for byte.  Lines of cases.txt:
!   fpbipere X Y UX UY NF KD1 MODE in out   MODE 1: LDZON=.TRUE., 0: LDZON=.FALSE., -1: no optional argument at all
!   boyd     X Y UX UY NF KD1 BW PL in out  LDBOYD=.TRUE., KDBOYD(3) = KDBOYD(6) = BW, PLBOYD = PL (MODE 2: without PLBOYD -- refused)
!   etibihie X Y UX UY NF KSTART KDLSM LDBIX LDBIY KDADD in out
!   horiz    KX KY out
! A refused call must abort with the ABORT_TRANS text, so the program never gets to print NOT REFUSED behind one.  Exit code 0 = pass.
PROGRAM TEST_SHIM_BIPER
USE, INTRINSIC :: ISO_C_BINDING, ONLY : C_INT32_T, C_FLOAT, C_DOUBLE
IMPLICIT NONE
#ifdef EMI_SP
INTEGER, PARAMETER :: RK = C_FLOAT
#else
INTEGER, PARAMETER :: RK = C_DOUBLE
#endif
#include "setup_trans0.h"
#include "fpbipere.h"
#include "etibihie.h"
#include "horiz_field.h"
CHARACTER(LEN=512) :: CLDIR, CLIN, CLOUT
CHARACTER(LEN=16) :: CLR
INTEGER(C_INT32_T) :: X, Y, UX, UY, NF, KD1, MODE, KS, KE, IBX, IBY, BW, KADD, IOS
INTEGER(C_INT32_T) :: KB(6)
REAL(RK) :: PL
REAL(RK), ALLOCATABLE :: P(:)

CALL GET_COMMAND_ARGUMENT(1, CLDIR)
CALL SETUP_TRANS0(KPRINTLEV=0, LDMPOFF=.TRUE., KMAX_RESOL=1)
OPEN(10, FILE=TRIM(CLDIR)//'/cases.txt', STATUS='OLD')
DO
  READ(10, *, IOSTAT=IOS) CLR
  IF (IOS /= 0) EXIT
  BACKSPACE(10)
  SELECT CASE (TRIM(CLR))
  CASE ('fpbipere')
    READ(10, *) CLR, X, Y, UX, UY, NF, KD1, MODE, CLIN, CLOUT
    CALL LOAD(KD1*NF)
    IF (MODE == 1) THEN
      CALL FPBIPERE(UX, UY, X, Y, NF, KD1, P, 0, LDZON=.TRUE.)
    ELSEIF (MODE == 0) THEN
      CALL FPBIPERE(UX, UY, X, Y, NF, KD1, P, 0, LDZON=.FALSE.)
    ELSEIF (MODE == -1) THEN
      CALL FPBIPERE(UX, UY, X, Y, NF, KD1, P, 0)
    ELSE
      CALL FPBIPERE(UX, UY, X, Y, NF, KD1, P, 1)
      PRINT *, 'NOT REFUSED'
    ENDIF
    CALL DUMP()
  CASE ('boyd')
    READ(10, *) CLR, X, Y, UX, UY, NF, KD1, BW, PL, MODE, CLIN, CLOUT
    KB = 0; KB(3) = BW; KB(6) = BW
    CALL LOAD(KD1*NF)
    IF (MODE == 2) THEN
      CALL FPBIPERE(UX, UY, X, Y, NF, KD1, P, 0, LDZON=.TRUE., LDBOYD=.TRUE., KDBOYD=KB)
      PRINT *, 'NOT REFUSED'
    ELSE
      CALL FPBIPERE(UX, UY, X, Y, NF, KD1, P, 0, LDZON=.TRUE., LDBOYD=.TRUE., KDBOYD=KB, PLBOYD=PL)
    ENDIF
    CALL DUMP()
  CASE ('etibihie')
    READ(10, *) CLR, X, Y, UX, UY, NF, KS, KE, IBX, IBY, KADD, CLIN, CLOUT
    CALL LOAD((KE - KS + 1)*NF*Y)
    CALL ETIBIHIE(X, Y, NF, UX, UY, KS, KE, P, IBX == 1, IBY == 1, KADD)
    IF (KADD /= 0) PRINT *, 'NOT REFUSED'
    CALL DUMP()
  CASE ('horiz')
    READ(10, *) CLR, X, Y, CLOUT
    IF (ALLOCATED(P)) DEALLOCATE(P)
    ALLOCATE(P(X*Y))
    CALL HORIZ_FIELD(X, Y, P)
    CALL DUMP()
  CASE DEFAULT
    ERROR STOP 2
  END SELECT
ENDDO
CLOSE(10)
PRINT '(A)', 'FORTRAN SHIM BIPER DONE'
CONTAINS
SUBROUTINE LOAD(N)
  INTEGER(C_INT32_T), INTENT(IN) :: N
  IF (ALLOCATED(P)) DEALLOCATE(P)
  ALLOCATE(P(N))
  OPEN(11, FILE=TRIM(CLDIR)//'/'//TRIM(CLIN), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='OLD')
  READ(11) P
  CLOSE(11)
END SUBROUTINE
SUBROUTINE DUMP()
  OPEN(12, FILE=TRIM(CLDIR)//'/'//TRIM(CLOUT), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='REPLACE')
  WRITE(12) P
  CLOSE(12)
END SUBROUTINE
END PROGRAM TEST_SHIM_BIPER
