/* An MPI host of the C-ABI for DIST_x / GATH_x on device arrays (emi_dist_spec_m ...): every rank is one task of the W-set (the ranks
 * may share a GPU) and the all-to-all-v between them is ectrans_amd/mpi/emi_mpi_hook.c.  Octahedral T21 in fp64 and in fp32, three
 * fields whose sources / targets alternate between task 1 and the last task: the blocks of the exchange are odd numbers of reals, in
 * fp32 no multiples of 8 bytes.  On every task the device path gives the bytes of the host path (the host collectives of the same
 * transport), and GATH after DIST returns the global fields. */
#include <mpi.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "../../ectrans_amd/mpi/emi_mpi_hook.h"
#include "../../include/ectrans_mi.h"

#define NF 3
#define CHECK(x)                                                              \
  do {                                                                        \
    if ((x) != 0) {                                                           \
      fprintf(stderr, "rank %d: %s failed: %s\n", rank, #x, emi_last_error()); \
      MPI_Abort(MPI_COMM_WORLD, 1);                                           \
    }                                                                         \
  } while (0)
#define SAME(a, b, n, what)                                            \
  do {                                                                 \
    if (memcmp((a), (b), (n)) != 0) {                                  \
      fprintf(stderr, "rank %d, fp%d: %s differs\n", rank, 8 * esz, what); \
      MPI_Abort(MPI_COMM_WORLD, 3);                                    \
    }                                                                  \
  } while (0)

int main(int argc, char **argv) {
  int rank, size;
  MPI_Init(&argc, &argv);
  MPI_Comm_rank(MPI_COMM_WORLD, &rank);
  MPI_Comm_size(MPI_COMM_WORLD, &size);
  const int N = 21, ndgl = 2 * (N + 1), nproma = 37;
  CHECK(emi_mpi_attach(MPI_COMM_WORLD, 2, 0, 0.0, -1));
  int nloen[2 * (21 + 1)];
  for (int i = 0; i <= N; i++) nloen[i] = nloen[ndgl - 1 - i] = 20 + 4 * i;
  int task[NF], nmine = 0;
  for (int f = 0; f < NF; f++) task[f] = f % 2 ? size : 1, nmine += task[f] == rank + 1;
  for (int esz = 8; esz >= 4; esz -= 4) {
    emi_setup_t cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.ksmax = N, cfg.kdgl = ndgl, cfg.kloen = nloen, cfg.precision = esz;
    int r = 0, ns, ng, nsg, ngg;
    CHECK(emi_setup(&cfg, &r));
    CHECK(emi_inq_int(r, "nspec2", &ns));
    CHECK(emi_inq_int(r, "ngptot", &ng));
    CHECK(emi_inq_int(r, "nspec2g", &nsg));
    CHECK(emi_inq_int(r, "ngptotg", &ngg));
    const int nblk = (ng - 1) / nproma + 1;
    const size_t bsp = (size_t)ns * NF * esz, bgp = (size_t)nblk * NF * nproma * esz, bspg = (size_t)nmine * nsg * esz, bgpg = (size_t)nmine * ngg * esz;
    /* the global fields of this task: the same values whatever the task count */
    char *spg = malloc(bspg + 1), *gpg = malloc(bgpg + 1), *spg_h = malloc(bspg + 1), *gpg_h = malloc(bgpg + 1), *spg_d = malloc(bspg + 1), *gpg_d = malloc(bgpg + 1);
    for (int k = 0, f = 0; f < NF; f++) {
      if (task[f] != rank + 1) continue;
      for (int i = 0; i < nsg; i++) {
        const double v = 1000.0 * f + i;
        if (esz == 8) ((double *)spg)[(size_t)k * nsg + i] = v;
        else ((float *)spg)[(size_t)k * nsg + i] = (float)v;
      }
      for (int i = 0; i < ngg; i++) {
        const double v = -1000.0 * f - i;
        if (esz == 8) ((double *)gpg)[(size_t)k * ngg + i] = v;
        else ((float *)gpg)[(size_t)k * ngg + i] = (float)v;
      }
      k++;
    }
    char *sp_h = calloc(1, bsp + 1), *gp_h = calloc(1, bgp + 1), *sp_c = malloc(bsp + 1), *gp_c = malloc(bgp + 1);
    void *sp_d, *gp_d;
    if (hipMalloc(&sp_d, bsp + 16) != hipSuccess || hipMalloc(&gp_d, bgp + 16) != hipSuccess || hipMemset(sp_d, 0, bsp + 16) != hipSuccess ||
        hipMemset(gp_d, 0, bgp + 16) != hipSuccess)
      MPI_Abort(MPI_COMM_WORLD, 2);
    /* host path, then device path with the global image on the host */
    CHECK(emi_dist_spec(r, nmine ? spg : NULL, NF, task, NULL, sp_h));
    CHECK(emi_dist_grid(r, nmine ? gpg : NULL, NF, task, NULL, nproma, gp_h));
    CHECK(emi_dist_spec_m(r, EMI_MEM_AUTO, nmine ? spg : NULL, NF, task, NULL, EMI_MEM_AUTO, sp_d));
    CHECK(emi_dist_grid_m(r, EMI_MEM_AUTO, nmine ? gpg : NULL, NF, task, NULL, nproma, EMI_MEM_AUTO, gp_d));
    if (hipMemcpy(sp_c, sp_d, bsp, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(gp_c, gp_d, bgp, hipMemcpyDeviceToHost) != hipSuccess)
      MPI_Abort(MPI_COMM_WORLD, 2);
    SAME(sp_c, sp_h, bsp, "DIST_SPEC on a device array");
    SAME(gp_c, gp_h, bgp, "DIST_GRID on a device array");
    CHECK(emi_gath_spec(r, nmine ? spg_h : NULL, NF, task, sp_h));
    CHECK(emi_gath_grid(r, nmine ? gpg_h : NULL, NF, task, nproma, gp_h));
    CHECK(emi_gath_spec_m(r, EMI_MEM_AUTO, nmine ? spg_d : NULL, NF, task, EMI_MEM_AUTO, sp_d));
    CHECK(emi_gath_grid_m(r, EMI_MEM_AUTO, nmine ? gpg_d : NULL, NF, task, nproma, EMI_MEM_AUTO, gp_d));
    SAME(spg_d, spg_h, bspg, "GATH_SPEC on a device array");
    SAME(gpg_d, gpg_h, bgpg, "GATH_GRID on a device array");
    SAME(spg_d, spg, bspg, "GATH_SPEC after DIST_SPEC");
    SAME(gpg_d, gpg, bgpg, "GATH_GRID after DIST_GRID");
    (void)hipFree(sp_d);
    (void)hipFree(gp_d);
    CHECK(emi_release(r));
  }
  CHECK(emi_finalize());
  emi_mpi_detach();
  printf("MPI DEVGS OK rank %d of %d\n", rank, size);
  MPI_Finalize();
  return 0;
}
