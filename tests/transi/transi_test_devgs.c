/* C caller of the transi-style API whose rgp / rspec live in DEVICE memory (hipMalloc) in trans_distgrid, trans_gathgrid,
 * trans_distspec and trans_gathspec: the layer passes EMI_MEM_AUTO for both arrays, the library finds the local array on the device
 * and lays the fields out there, in place; the global arrays stay on the host.  Each call is made twice, on host arrays and on
 * hipMalloc'ed ones, with the same data: the results are the same bytes.  NPROMA cuts the rows and leaves a partly filled last
 * block.  Exit code 0 = pass. */
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
#define SAME(a, b, bytes, what)                                   \
  do {                                                            \
    if (memcmp((a), (b), (bytes)) != 0) {                         \
      fprintf(stderr, "%s: device and host arrays differ\n", what); \
      return 1;                                                   \
    }                                                             \
  } while (0)

static double rnd(unsigned long long *s) {
  *s = *s * 6364136223846793005ULL + 1442695040888963407ULL;
  return (double)(*s >> 11) / 9007199254740992.0 - 0.5;
}

int main(void) {
  const int nsmax = 21, ndgl = 2 * (nsmax + 1), nfld = 5, nproma = 37;
  int *nloen = malloc(sizeof(int) * ndgl);
  for (int i = 0; i <= nsmax; i++) nloen[i] = nloen[ndgl - 1 - i] = 20 + 4 * i;
  CHECK(trans_use_mpi(0));
  struct Trans_t trans;
  CHECK(trans_new(&trans));
  CHECK(trans_set_resol(&trans, ndgl, nloen));
  CHECK(trans_set_trunc(&trans, nsmax));
  CHECK(trans_setup(&trans));
  const size_t ns = (size_t)trans.nspec2, nsg = (size_t)trans.nspec2g, ng = (size_t)trans.ngptot, ngg = (size_t)trans.ngptotg;
  const int nblk = (int)((ng - 1) / nproma + 1);
  const size_t bgp = sizeof(double) * nblk * nfld * nproma, bgpg = sizeof(double) * nfld * ngg, bsp = sizeof(double) * ns * nfld, bspg = sizeof(double) * nsg * nfld;
  int task[5] = {1, 1, 1, 1, 1};
  unsigned long long seed = 7;
  double *gpg = malloc(bgpg), *spg = malloc(bspg), *gp_h = malloc(bgp), *gp_d2h = malloc(bgp), *sp_h = malloc(bsp), *sp_d2h = malloc(bsp);
  double *gpg_h = malloc(bgpg), *gpg_d = malloc(bgpg), *spg_h = malloc(bspg), *spg_d = malloc(bspg);
  for (size_t i = 0; i < nfld * ngg; i++) gpg[i] = rnd(&seed);
  for (size_t i = 0; i < nsg * nfld; i++) spg[i] = rnd(&seed);
  double *gp_d, *sp_d;
  HIPOK(hipMalloc((void **)&gp_d, bgp));
  HIPOK(hipMalloc((void **)&sp_d, bsp));
  memset(gp_h, 0xff, bgp);
  HIPOK(hipMemset(gp_d, 0xff, bgp));

  /* trans_distgrid: the padding of the last block comes back zero in both memories */
  struct DistGrid_t dg = new_distgrid(&trans);
  dg.rgpg = gpg, dg.rgp = gp_h, dg.nfrom = task, dg.nfld = nfld, dg.nproma = nproma, dg.ngpblks = nblk;
  CHECK(trans_distgrid(&dg));
  dg = new_distgrid(&trans);
  dg.rgpg = gpg, dg.rgp = gp_d, dg.nfrom = task, dg.nfld = nfld, dg.nproma = nproma, dg.ngpblks = nblk;
  CHECK(trans_distgrid(&dg));
  HIPOK(hipMemcpy(gp_d2h, gp_d, bgp, hipMemcpyDeviceToHost));
  SAME(gp_d2h, gp_h, bgp, "trans_distgrid");

  /* trans_gathgrid */
  struct GathGrid_t gg = new_gathgrid(&trans);
  gg.rgpg = gpg_h, gg.rgp = gp_h, gg.nto = task, gg.nfld = nfld, gg.nproma = nproma, gg.ngpblks = nblk;
  CHECK(trans_gathgrid(&gg));
  gg = new_gathgrid(&trans);
  gg.rgpg = gpg_d, gg.rgp = gp_d, gg.nto = task, gg.nfld = nfld, gg.nproma = nproma, gg.ngpblks = nblk;
  CHECK(trans_gathgrid(&gg));
  SAME(gpg_d, gpg_h, bgpg, "trans_gathgrid");
  SAME(gpg_h, gpg, bgpg, "trans_gathgrid after trans_distgrid");

  /* trans_distspec */
  struct DistSpec_t ds = new_distspec(&trans);
  ds.rspecg = spg, ds.rspec = sp_h, ds.nfrom = task, ds.nfld = nfld;
  CHECK(trans_distspec(&ds));
  HIPOK(hipMemset(sp_d, 0xff, bsp));
  ds = new_distspec(&trans);
  ds.rspecg = spg, ds.rspec = sp_d, ds.nfrom = task, ds.nfld = nfld;
  CHECK(trans_distspec(&ds));
  HIPOK(hipMemcpy(sp_d2h, sp_d, bsp, hipMemcpyDeviceToHost));
  SAME(sp_d2h, sp_h, bsp, "trans_distspec");

  /* trans_gathspec */
  struct GathSpec_t gs = new_gathspec(&trans);
  gs.rspecg = spg_h, gs.rspec = sp_h, gs.nto = task, gs.nfld = nfld;
  CHECK(trans_gathspec(&gs));
  gs = new_gathspec(&trans);
  gs.rspecg = spg_d, gs.rspec = sp_d, gs.nto = task, gs.nfld = nfld;
  CHECK(trans_gathspec(&gs));
  SAME(spg_d, spg_h, bspg, "trans_gathspec");
  SAME(spg_h, spg, bspg, "trans_gathspec after trans_distspec");

  HIPOK(hipFree(gp_d));
  HIPOK(hipFree(sp_d));
  CHECK(trans_delete(&trans));
  CHECK(trans_finalize());
  printf("TRANSI DEVGS OK\n");
  return 0;
}
