/* trans_set_resol_lonlat: spectral fields onto regular lat-lon grids through the transi-style API, nlat odd (poles and equator) and
 * even (shifted by half a cell), global arrays (lglobal) in host and in device memory.  Checked against closed forms in the
 * normalisation of ecTrans: a constant, P_1^0 = sqrt(3) sin(lat), and the sectoral harmonic m = n = 3,
 * 2 P_3^3 (re cos 3 lon - im sin 3 lon) with P_3^3 = sqrt(3/2 5/4 7/6) cos^3(lat), whose longitude phase shows the half-cell shift.
 * trans_dirtrans and the adjoints are refused on such a handle.  Exit code 0 = pass. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "../../ectrans_amd/transi/transi_mi.h"

#define CHECK(x)                                                    \
  do {                                                              \
    int rc_ = (x);                                                  \
    if (rc_ != TRANS_SUCCESS) {                                     \
      fprintf(stderr, "%s failed: %s\n", #x, trans_error_msg(rc_)); \
      return 1;                                                     \
    }                                                               \
  } while (0)
#define HIPOK(x)                                                     \
  do {                                                               \
    hipError_t e_ = (x);                                             \
    if (e_ != hipSuccess) {                                          \
      fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_)); \
      return 1;                                                      \
    }                                                                \
  } while (0)

static const double C0 = 1.25, A10 = -0.75, RE33 = 0.5, IM33 = -0.3;

static double closed_form(int f, double lat, double lon) {
  if (f == 0) return C0;
  if (f == 1) return A10 * sqrt(3.0) * sin(lat);
  const double c = cos(lat), p33 = sqrt(1.5 * 1.25 * 7.0 / 6.0) * c * c * c;
  return 2.0 * p33 * (RE33 * cos(3.0 * lon) - IM33 * sin(3.0 * lon));
}

static int run(int nlon, int nlat) {
  const int nsmax = 21, shifted = nlat % 2 == 0, nfld = 3;
  const double pi = 3.14159265358979323846;
  struct Trans_t trans;
  CHECK(trans_new(&trans));
  CHECK(trans_set_resol_lonlat(&trans, nlon, nlat));
  CHECK(trans_set_trunc(&trans, nsmax));
  CHECK(trans_setup(&trans));
  if (trans.llatlon != (shifted ? 2 : 1) || trans.ngptotg != nlat * nlon || trans.ngptot != trans.ngptotg + (shifted ? 0 : nlon)) {
    fprintf(stderr, "%dx%d: llatlon %d ngptotg %d ngptot %d\n", nlat, nlon, trans.llatlon, trans.ngptotg, trans.ngptot);
    return 2;
  }
  CHECK(trans_inquire(&trans, "nasm0"));
  const size_t ns = (size_t)trans.nspec2, ng = (size_t)trans.ngptotg;
  const size_t bsp = sizeof(double) * nfld * ns, bgp = sizeof(double) * nfld * ng;
  double *hsp = calloc(1, bsp), *hgp = calloc(1, bgp), *cgp = calloc(1, bgp);
  hsp[(size_t)(trans.nasm0[0] - 1) * nfld + 0] = C0;
  hsp[(size_t)(trans.nasm0[0] - 1 + 2) * nfld + 1] = A10;
  hsp[(size_t)(trans.nasm0[3] - 1) * nfld + 2] = RE33;
  hsp[(size_t)(trans.nasm0[3] - 1 + 1) * nfld + 2] = IM33;
  double *dsp, *dgp;
  HIPOK(hipMalloc((void **)&dsp, bsp));
  HIPOK(hipMalloc((void **)&dgp, bgp));
  HIPOK(hipMemcpy(dsp, hsp, bsp, hipMemcpyHostToDevice));
  HIPOK(hipMemset(dgp, 0, bgp));
  struct InvTrans_t vh = new_invtrans(&trans);
  vh.nscalar = nfld, vh.rspscalar = hsp, vh.rgp = hgp, vh.lglobal = 1;
  CHECK(trans_invtrans(&vh));
  struct InvTrans_t vd = new_invtrans(&trans);
  vd.nscalar = nfld, vd.rspscalar = dsp, vd.rgp = dgp, vd.lglobal = 1;
  CHECK(trans_invtrans(&vd));
  HIPOK(hipMemcpy(cgp, dgp, bgp, hipMemcpyDeviceToHost));
  if (memcmp(cgp, hgp, bgp)) {
    fprintf(stderr, "%dx%d: device-resident and host arrays differ\n", nlat, nlon);
    return 3;
  }
  double worst = 0.0;
  for (int f = 0; f < nfld; f++)
    for (int j = 0; j < nlat; j++) {
      const double lat = shifted ? pi / 2 - (j + 0.5) * pi / nlat : pi / 2 - j * pi / (nlat - 1);
      for (int i = 0; i < nlon; i++) {
        const double lon = (i + (shifted ? 0.5 : 0.0)) * 2.0 * pi / nlon;
        const double e = fabs(hgp[(size_t)f * ng + (size_t)j * nlon + i] - closed_form(f, lat, lon));
        if (e > worst) worst = e;
      }
    }
  printf("lonlat %dx%d: max error against the closed forms %.2e\n", nlat, nlon, worst);
  if (!(worst < 1e-12)) return 4;
  /* without lglobal the array has ngptot points per field: on the unshifted grid nlat + 1 rows, the equator twice */
  const size_t ngl = (size_t)trans.ngptot;
  double *lgp = calloc(nfld * ngl, sizeof(double));
  struct InvTrans_t vl = new_invtrans(&trans);
  vl.nscalar = nfld, vl.rspscalar = hsp, vl.rgp = lgp;
  CHECK(trans_invtrans(&vl));
  const size_t north = (size_t)((nlat + 1) / 2) * nlon;
  for (int f = 0; f < nfld; f++) {
    if (memcmp(lgp + f * ngl, hgp + f * ng, north * 8) || memcmp(lgp + f * ngl + north + (shifted ? 0 : nlon), hgp + f * ng + north, (ng - north) * 8) ||
        (!shifted && memcmp(lgp + f * ngl + north - nlon, lgp + f * ngl + north, nlon * 8))) {
      fprintf(stderr, "%dx%d: the local array is not the global one plus the second equator row (field %d)\n", nlat, nlon, f);
      return 5;
    }
  }
  /* the handle serves the inverse transform only */
  struct DirTrans_t d = new_dirtrans(&trans);
  d.nscalar = nfld, d.rspscalar = hsp, d.rgp = lgp;
  struct DirTransAdj_t da = new_dirtrans_adj(&trans);
  da.nscalar = nfld, da.rspscalar = hsp, da.rgp = lgp;
  struct InvTransAdj_t va = new_invtrans_adj(&trans);
  va.nscalar = nfld, va.rspscalar = hsp, va.rgp = lgp;
  if (trans_dirtrans(&d) == TRANS_SUCCESS || trans_dirtrans_adj(&da) == TRANS_SUCCESS || trans_invtrans_adj(&va) == TRANS_SUCCESS) {
    fprintf(stderr, "%dx%d: a direct or adjoint transform on a lonlat handle was not refused\n", nlat, nlon);
    return 6;
  }
  HIPOK(hipFree(dsp));
  HIPOK(hipFree(dgp));
  free(hsp), free(hgp), free(cgp), free(lgp);
  CHECK(trans_delete(&trans));
  return 0;
}

int main(void) {
  CHECK(trans_use_mpi(0));
  int rc = run(72, 37);
  if (!rc) rc = run(72, 36);
  if (!rc) rc = run(90, 45); /* row length with an odd half */
  if (rc) return rc;
  CHECK(trans_finalize());
  printf("TRANSI LONLAT OK\n");
  return 0;
}
