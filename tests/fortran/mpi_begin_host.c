/* C helper of tests/fortran/test_shim_vsets_gs.F90 on the CPU functional emulator: the entry points of mpi_begin.c with a transport
 * for HOST memory -- the emulator's "device" buffers are host arrays and its streams run at once, so the exchange hook is a plain
 * MPI_Alltoallv on bytes and nothing of the HIP runtime is touched (the MPI transport of ectrans_amd/mpi stages through it). */
#include <mpi.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/ectrans_mi.h"

static MPI_Comm g_comm = MPI_COMM_NULL;

static int hook(void *user, const void *sb, const long long *sc, const long long *sd, void *rb, const long long *rc, const long long *rd, int n,
                void *stream) {
  (void)user, (void)stream;
  int *v = (int *)malloc(4 * (size_t)n * sizeof(int));
  if (!v) return -1;
  for (int r = 0; r < n; r++) v[r] = (int)sc[r], v[n + r] = (int)sd[r], v[2 * n + r] = (int)rc[r], v[3 * n + r] = (int)rd[r];
  const int bad = MPI_Alltoallv(sb, v, v + n, MPI_BYTE, rb, v + 2 * n, v + 3 * n, MPI_BYTE, g_comm) != MPI_SUCCESS;
  free(v);
  return bad ? -1 : 0;
}
static int hc_bcast(void *user, void *buf, long long bytes, int root) {
  (void)user;
  return MPI_Bcast(buf, (int)bytes, MPI_BYTE, root, g_comm) != MPI_SUCCESS ? -1 : 0;
}
static int hc_allgatherv(void *user, const void *sendbuf, long long sendbytes, void *recvbuf, const long long *recvbytes, const long long *displs, int nproc) {
  (void)user;
  int me = 0;
  MPI_Comm_rank(g_comm, &me);
  for (int r = 0; r < nproc; r++) {
    if (r == me) memcpy((char *)recvbuf + displs[r], sendbuf, (size_t)sendbytes);
    if (hc_bcast(NULL, (char *)recvbuf + displs[r], recvbytes[r], r)) return -1;
  }
  return 0;
}
int emi_test_mpi_begin_v(int nprtrv, int *nproc, int *myproc) {
  int rank, size;
  MPI_Init(0, 0);
  MPI_Comm_dup(MPI_COMM_WORLD, &g_comm);
  MPI_Comm_rank(g_comm, &rank);
  MPI_Comm_size(g_comm, &size);
  *nproc = size;
  *myproc = rank + 1;
  emi_init_t cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.kmax_resol = 2, cfg.nproc = size, cfg.myproc = rank + 1, cfg.device = -1, cfg.nprtrv = nprtrv;
  if (emi_set_alltoallv(size > 1 ? hook : NULL, NULL) || emi_set_host_collectives(hc_bcast, hc_allgatherv, NULL)) return -1;
  return emi_init(&cfg);
}
void emi_test_mpi_end(void) {
  if (g_comm != MPI_COMM_NULL) MPI_Comm_free(&g_comm);
  MPI_Finalize();
}
