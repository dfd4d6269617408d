/* The limited-area part of the transi-style C layer on one domain, for any number of tasks: trans_set_resol_lam / trans_set_trunc_lam,
 * trans_setup, trans_inquire, trans_distspec / trans_distgrid, trans_invtrans with several flag sets, trans_dirtrans, both adjoints
 * (rmeanu / rmeanv included), lglobal, trans_gathgrid / trans_gathspec and trans_specnorm with and without rmet.
 *
 *   transi_test_lam <dir> <nx> <ny> <dx> <dy> <trunc_x> <trunc_y> <nvordiv> <nscalar> <nproma> host|device
 *
 * <dir> holds the GLOBAL inputs as raw doubles, written by the Python test (tests/transi_lam_common.py): vor / div [nspec2g][nvordiv],
 * sc [nspec2g][nscalar], mu / mv [nvordiv], gp [2 nvordiv + nscalar][ngptotg], gpad_<mask> [nfld(mask)][ngptotg] for the masks of the
 * adjoint, rmet [nspec2g / 4 + 1].  Every task distributes them from task 1, transforms its share in NPROMA blocks whose padding
 * holds NaN, and the results are gathered on task 1, which writes them back as global arrays: the files do not depend on the number
 * of tasks.  "device": the arrays of the transforms and of trans_specnorm come from hipMalloc (the means stay in host memory).
 * With MPI (-DTRANSI_LAM_MPI) the program attaches the MPI transport first.  The last line of a passing run is "TRANSI LAM OK". */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>
#ifdef TRANSI_LAM_MPI
#include <mpi.h>

#include "../../ectrans_amd/mpi/emi_mpi_hook.h"
#endif
#include "../../ectrans_amd/transi/transi_mi.h"

static const char *g_dir;
static int g_dev = 0, g_rank = 0;

#define FAIL(...)                                                  \
  do {                                                             \
    fprintf(stderr, "transi_test_lam: rank %d, line %d: ", g_rank, __LINE__); \
    fprintf(stderr, __VA_ARGS__);                                  \
    fprintf(stderr, "\n");                                         \
    exit(1);                                                       \
  } while (0)
#define OK(call)                                                                       \
  do {                                                                                 \
    const int rc_ = (call);                                                            \
    if (rc_ != TRANS_SUCCESS) FAIL("%s returned %d (%s)", #call, rc_, trans_error_msg(rc_)); \
  } while (0)
#define WANT(call, code)                                                     \
  do {                                                                       \
    const int rc_ = (call);                                                  \
    if (rc_ != (code)) FAIL("%s returned %d, expected %d", #call, rc_, (code)); \
  } while (0)

static double *alloc(size_t n, double fill) {
  double *p = (double *)malloc(sizeof(double) * (n ? n : 1));
  if (!p) FAIL("out of memory");
  for (size_t i = 0; i < n; i++) p[i] = fill;
  return p;
}
static double *rd(const char *name, size_t n) {
  char path[1024];
  snprintf(path, sizeof(path), "%s/%s", g_dir, name);
  FILE *f = fopen(path, "rb");
  if (!f) FAIL("cannot open %s", path);
  double *p = alloc(n, 0.0);
  if (fread(p, sizeof(double), n, f) != n || fgetc(f) != EOF) FAIL("%s does not hold %zu doubles", path, n);
  fclose(f);
  return p;
}
static void wr(const char *name, const void *p, size_t bytes) {
  char path[1024];
  if (g_rank != 1) return;
  snprintf(path, sizeof(path), "%s/%s", g_dir, name);
  FILE *f = fopen(path, "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes) FAIL("cannot write %s", path);
  fclose(f);
}
/* the array a call works on: host memory, or a copy in device memory */
static double *arr(const double *h, size_t n) {
  double *a;
  if (!g_dev) {
    a = alloc(n, 0.0);
    memcpy(a, h, sizeof(double) * n);
  } else if (hipMalloc((void **)&a, sizeof(double) * (n ? n : 1)) != hipSuccess || hipMemcpy(a, h, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess) {
    FAIL("hipMalloc / hipMemcpy of %zu doubles", n);
  }
  return a;
}
static void back(double *h, double *a, size_t n) { /* ... and back, released */
  if (!g_dev) {
    memcpy(h, a, sizeof(double) * n);
    free(a);
  } else if (hipMemcpy(h, a, sizeof(double) * n, hipMemcpyDeviceToHost) != hipSuccess || hipFree(a) != hipSuccess) {
    FAIL("hipMemcpy / hipFree");
  }
}

static struct Trans_t T;
static int nuv, nsc, nproma, nb;
static int *ones;

static int nfld_of(int mask) { return 2 * nuv + nsc + (mask & 1 ? 2 * nsc : 0) + (mask & 2 ? 2 * nuv : 0) + (mask & 4 ? 2 * nuv : 0); }
static size_t blocked(int nf) { return (size_t)nb * nf * nproma; }

/* global [nf][ngptotg] on task 1 -> this task's NPROMA blocks, the padding of the last block NaN */
static double *dist_grid(const double *g, int nf) {
  double *loc = alloc(blocked(nf), 0.0);
  struct DistGrid_t a = new_distgrid(&T);
  a.rgpg = T.myproc == 1 ? g : NULL, a.rgp = loc, a.nfrom = ones, a.nfld = nf, a.nproma = nproma, a.ngpblks = nb;
  OK(trans_distgrid(&a));
  for (int f = 0; f < nf; f++)
    for (long p = T.ngptot; p < (long)nb * nproma; p++) {
      double *e = &loc[((size_t)(p / nproma) * nf + f) * nproma + p % nproma];
      if (*e != 0.0) FAIL("trans_distgrid left %g in the padding", *e);
      *e = NAN;
    }
  return loc;
}
/* ... and back: [nf][ngptotg] on task 1; the padding must still hold NaN */
static void gath_grid(const char *name, const double *loc, int nf) {
  for (int f = 0; f < nf; f++)
    for (long p = T.ngptot; p < (long)nb * nproma; p++)
      if (!isnan(loc[((size_t)(p / nproma) * nf + f) * nproma + p % nproma])) FAIL("%s: the padding of the last block was written", name);
  double *g = alloc((size_t)nf * T.ngptotg, -777.0);
  struct GathGrid_t a = new_gathgrid(&T);
  a.rgpg = T.myproc == 1 ? g : NULL, a.rgp = loc, a.nto = ones, a.nfld = nf, a.nproma = nproma, a.ngpblks = nb;
  OK(trans_gathgrid(&a));
  wr(name, g, sizeof(double) * nf * T.ngptotg);
  free(g);
}
static double *dist_spec(const double *g, int nf) {
  double *loc = alloc((size_t)T.nspec2 * nf, -777.0);
  struct DistSpec_t a = new_distspec(&T);
  a.rspecg = T.myproc == 1 ? g : NULL, a.rspec = loc, a.nfrom = ones, a.nfld = nf;
  OK(trans_distspec(&a));
  return loc;
}
static double *gath_spec(const char *name, const double *loc, int nf) {
  double *g = alloc((size_t)T.nspec2g * nf, -777.0);
  struct GathSpec_t a = new_gathspec(&T);
  a.rspecg = T.myproc == 1 ? g : NULL, a.rspec = loc, a.nto = ones, a.nfld = nf;
  OK(trans_gathspec(&a));
  if (name) wr(name, g, sizeof(double) * nf * T.nspec2g);
  return g;
}
static void name_of(char *buf, const char *stem, int mask, const char *what) { snprintf(buf, 64, "%s_%d%s.f64", stem, mask, what); }

/* return codes that must stay as they are: a Gaussian handle, a lat-lon handle, and the LAM-specific refusals */
static void refusals(int nx, int ny, double dx, double dy, int mx, int my) {
  struct Trans_t g, l;
  int nloen[8] = {16, 16, 16, 16, 16, 16, 16, 16};
  double spec[42][1], norm[1], met[6] = {1, 1, 1, 4, 1, 1}, mean[1] = {0.0}, gp[3 * 128];
  /* nmsmax < 0; readfp on a LAM handle */
  OK(trans_new(&l));
  OK(trans_set_resol_lam(&l, nx, ny, dx, dy));
  if (!l.llam || l.ndgl != ny || l.nlon != nx || l.nmsmax != -1 || l.ndgux != -1) FAIL("trans_set_resol_lam");
  WANT(trans_setup(&l), TRANS_ERROR);
  OK(trans_set_trunc_lam(&l, mx, my));
  OK(trans_set_read(&l, "/nonexistent/legpol"));
  WANT(trans_setup(&l), TRANS_NOTIMPL);
  OK(trans_delete(&l));
  /* a truncation at half the row length: ESETUP_TRANS refuses, transi says TRANS_ERROR */
  OK(trans_new(&l));
  OK(trans_set_resol_lam(&l, nx, ny, dx, dy));
  OK(trans_set_trunc_lam(&l, nx / 2, my));
  WANT(trans_setup(&l), TRANS_ERROR);
  OK(trans_delete(&l));
  /* the Gaussian quantities of a LAM handle; a missing mean; a stale struct */
  WANT(trans_inquire(&T, "rgw"), TRANS_NOTIMPL);
  WANT(trans_inquire(&T, "nasm0"), TRANS_NOTIMPL);
  WANT(trans_inquire(&T, "nonsense"), TRANS_UNRECOGNIZED_ARG);
  if (nuv > 0) {
    double *v = alloc((size_t)T.nspec2 * nuv, 0.0), *o = alloc(blocked(nfld_of(0)), 0.0);
    struct InvTrans_t iv = new_invtrans(&T);
    iv.nvordiv = nuv, iv.rspvor = v, iv.rspdiv = v, iv.rgp = o, iv.rmeanv = mean;
    WANT(trans_invtrans(&iv), TRANS_MISSING_ARG); /* Array RMEANU was not allocated */
    WANT(trans_invtrans(&iv), TRANS_STALE_ARG);
    struct DirTrans_t d = new_dirtrans(&T);
    d.nvordiv = nuv, d.rspvor = v, d.rspdiv = v, d.rgp = o, d.rmeanu = mean;
    WANT(trans_dirtrans(&d), TRANS_MISSING_ARG);
    free(v), free(o);
  }
  /* a Gaussian handle: mvalue, rmeanu; rmet is SPECNORM's PMET(0:NSMAX) */
  OK(trans_new(&g));
  if (g.llam != 0 || g.nmsmax != -1 || g.ndgux != -1 || g.pexwn != 1.0 || g.peywn != 1.0 || g.mvalue) FAIL("trans_new defaults");
  OK(trans_set_resol(&g, 8, nloen));
  OK(trans_set_trunc(&g, 5));
  OK(trans_setup(&g));
  WANT(trans_inquire(&g, "mvalue"), TRANS_NOTIMPL);
  /* nvalue has nspec2 entries, those of THIS task's wavenumbers: n = m .. nsmax twice from NASM0(m), for every m of nmyms */
  OK(trans_inquire(&g, "nvalue,nmyms,nasm0"));
  {
    int k = 0, seen = 0;
    for (int jm = 0; jm < g.nump; jm++) {
      const int m = g.nmyms[jm];
      if (m < 0 || m > 5 || g.nasm0[m] - 1 != k) FAIL("Gaussian handle: NASM0(%d) = %d, %d entries before it", m, m >= 0 && m <= 5 ? g.nasm0[m] : 0, k);
      for (int n = m; n <= 5; n++, k += 2)
        if (k + 2 > g.nspec2 || g.nvalue[k] != n || g.nvalue[k + 1] != n) FAIL("Gaussian handle: nvalue of (m = %d, n = %d) at %d", m, n, k);
      seen++;
    }
    if (k != g.nspec2 || seen != g.nump || (g.nproc > 1 && g.nspec2 >= g.nspec2g)) FAIL("Gaussian handle: nvalue covers %d of %d entries", k, g.nspec2);
  }
  if (g.nproc == 1) {
    if (g.nspec2 != 42 || g.ngptot != 128) FAIL("Gaussian handle: nspec2 %d ngptot %d", g.nspec2, g.ngptot);
    memset(spec, 0, sizeof(spec));
    memset(gp, 0, sizeof(gp));
    struct InvTrans_t iv = new_invtrans(&g);
    iv.nscalar = 1, iv.rspscalar = &spec[0][0], iv.rgp = gp, iv.rmeanu = mean;
    WANT(trans_invtrans(&iv), TRANS_NOTIMPL);
    struct DirTrans_t d = new_dirtrans(&g);
    d.nscalar = 1, d.rspscalar = &spec[0][0], d.rgp = gp, d.rmeanv = mean;
    WANT(trans_dirtrans(&d), TRANS_NOTIMPL);
    /* Re(m = 2, n = 3) = 3 under rmet[3] = 4: sqrt(2 x 4 x 9); Re(0, 0) = 2 under rmet[0] = 1 in the other call */
    spec[12 + 10 + 2][0] = 3.0; /* NASM0(2) = 12 + 10, n - m = 1 */
    struct SpecNorm_t s = new_specnorm(&g);
    s.rspec = &spec[0][0], s.rnorm = norm, s.nfld = 1, s.rmet = met;
    OK(trans_specnorm(&s));
    if (norm[0] != sqrt(72.0)) FAIL("trans_specnorm with rmet on the sphere: %.17g", norm[0]);
    s = new_specnorm(&g);
    s.rspec = &spec[0][0], s.rnorm = norm, s.nfld = 1;
    OK(trans_specnorm(&s));
    if (norm[0] != sqrt(18.0)) FAIL("trans_specnorm on the sphere: %.17g", norm[0]);
  }
  OK(trans_delete(&g));
  /* a lat-lon handle: rmet stays refused */
  if (T.nproc == 1) {
    OK(trans_new(&g));
    OK(trans_set_resol_lonlat(&g, 16, 8));
    OK(trans_set_trunc(&g, 5));
    OK(trans_setup(&g));
    memset(spec, 0, sizeof(spec));
    struct SpecNorm_t s = new_specnorm(&g);
    s.rspec = &spec[0][0], s.rnorm = norm, s.nfld = 1, s.rmet = met;
    WANT(trans_specnorm(&s), TRANS_NOTIMPL);
    OK(trans_delete(&g));
  }
  if (g_rank == 1) printf("TRANSI LAM REFUSALS OK\n");
}

int main(int argc, char **argv) {
#ifdef TRANSI_LAM_MPI
  int size;
  MPI_Init(&argc, &argv);
  MPI_Comm_rank(MPI_COMM_WORLD, &g_rank);
  MPI_Comm_size(MPI_COMM_WORLD, &size);
  g_rank += 1;
  if (emi_mpi_attach(MPI_COMM_WORLD, 8, 0, 6371.22e3, -1) != 0) FAIL("emi_mpi_attach");
  OK(trans_use_mpi(1));
#else
  g_rank = 1;
#endif
  if (argc != 12) FAIL("usage: transi_test_lam <dir> <nx> <ny> <dx> <dy> <trunc_x> <trunc_y> <nvordiv> <nscalar> <nproma> host|device");
  g_dir = argv[1];
  const int nx = atoi(argv[2]), ny = atoi(argv[3]), mx = atoi(argv[6]), my = atoi(argv[7]);
  const double dx = atof(argv[4]), dy = atof(argv[5]);
  nuv = atoi(argv[8]), nsc = atoi(argv[9]), nproma = atoi(argv[10]);
  g_dev = !strcmp(argv[11], "device");
  if (nuv <= 0 || nsc <= 0) FAIL("wind and scalar fields are both needed");
  OK(trans_set_handles_limit(8));
  OK(trans_new(&T));
  OK(trans_set_resol_lam(&T, nx, ny, dx, dy));
  OK(trans_set_trunc_lam(&T, mx, my));
  OK(trans_setup(&T));
  if (T.myproc != g_rank) FAIL("myproc %d", T.myproc);
  if (nproma <= 0) nproma = T.ngptot;
  nb = (T.ngptot - 1) / nproma + 1;
  const int nfmax = nfld_of(7) > nuv + nsc ? nfld_of(7) : nuv + nsc;
  ones = (int *)malloc(sizeof(int) * (size_t)nfmax);
  for (int f = 0; f < nfmax; f++) ones[f] = 1;
  /* ---- (a) sizes and inquiries */
  OK(trans_inquire(&T, "nvalue,mvalue,nmyms,nloen"));
  const int sizes[12] = {T.nspec2, T.nspec2g, T.nspec2mx, T.nump, T.ngptot, T.ngptotg, T.ngptotmx, T.nproc, T.myproc, T.ndgux, T.nspec, T.llam};
  wr("sizes.i32", sizes, sizeof(sizes));
  wr("nvalue.i32", T.nvalue, sizeof(int) * (size_t)T.nspec2);
  wr("mvalue.i32", T.mvalue, sizeof(int) * (size_t)T.nspec2);
  wr("nmyms.i32", T.nmyms, sizeof(int) * (size_t)T.nump);
  wr("nloen.i32", T.nloen, sizeof(int) * (size_t)T.ndgl);
  if (g_rank == 1 && (T.nump < 1 || T.nmyms[0] != 0)) FAIL("task 1 does not hold m = 0: the means are written elsewhere");
  /* ---- the global inputs, and this task's share */
  const size_t ns2 = (size_t)T.nspec2, ns2g = (size_t)T.nspec2g, ngg = (size_t)T.ngptotg;
  double *vorg = rd("vor.f64", ns2g * nuv), *divg = rd("div.f64", ns2g * nuv), *scg = rd("sc.f64", ns2g * nsc);
  double *mu = rd("mu.f64", nuv), *mv = rd("mv.f64", nuv), *gpg = rd("gp.f64", ngg * nfld_of(0)), *rmet = rd("rmet.f64", ns2g / 4 + 1);
  double *vor = dist_spec(vorg, nuv), *div = dist_spec(divg, nuv), *sc = dist_spec(scg, nsc);
  /* (f) the round trip of the gather: the global array again, byte for byte */
  double *again = gath_spec(NULL, sc, nsc);
  if (g_rank == 1 && memcmp(again, scg, sizeof(double) * ns2g * nsc)) FAIL("trans_distspec -> trans_gathspec is not the identity");
  free(again);
  char fn[64];
  /* ---- (b) trans_invtrans: no flag, all flags, lscalarders alone, luvder_EW + lvordivgp */
  const int masks[4] = {0, 7, 1, 6};
  for (int k = 0; k < 4; k++) {
    const int mask = masks[k], nf = nfld_of(mask);
    double *out = alloc(blocked(nf), NAN), *a_v = arr(vor, ns2 * nuv), *a_d = arr(div, ns2 * nuv), *a_s = arr(sc, ns2 * nsc), *a_o = arr(out, blocked(nf));
    struct InvTrans_t iv = new_invtrans(&T);
    iv.nvordiv = nuv, iv.nscalar = nsc, iv.rspvor = a_v, iv.rspdiv = a_d, iv.rspscalar = a_s, iv.rmeanu = mu, iv.rmeanv = mv;
    iv.rgp = a_o, iv.nproma = nproma, iv.ngpblks = nb;
    iv.lscalarders = mask & 1, iv.luvder_EW = (mask & 2) != 0, iv.lvordivgp = (mask & 4) != 0;
    OK(trans_invtrans(&iv));
    back(out, a_o, blocked(nf));
    name_of(fn, "inv", mask, "");
    gath_grid(fn, out, nf);
    if (T.nproc == 1 && mask == 7) { /* (e) lglobal: [nfld][ngptotg] in one block, whatever nproma says */
      double *gl = alloc((size_t)nf * ngg, NAN), *a_g = arr(gl, (size_t)nf * ngg);
      struct InvTrans_t ig = new_invtrans(&T);
      ig.nvordiv = nuv, ig.nscalar = nsc, ig.rspvor = a_v, ig.rspdiv = a_d, ig.rspscalar = a_s, ig.rmeanu = mu, ig.rmeanv = mv;
      ig.rgp = a_g, ig.nproma = 13, ig.lglobal = 1, ig.lscalarders = ig.luvder_EW = ig.lvordivgp = 1;
      OK(trans_invtrans(&ig));
      back(gl, a_g, (size_t)nf * ngg);
      wr("invg_7.f64", gl, sizeof(double) * nf * ngg);
      free(gl);
    }
    back(vor, a_v, ns2 * nuv), back(div, a_d, ns2 * nuv), back(sc, a_s, ns2 * nsc);
    free(out);
  }
  /* ---- trans_dirtrans of the global grid fields: u, v, scalars; the means are outputs */
  {
    const int nf = nfld_of(0);
    double *in = dist_grid(gpg, nf), *again_g = alloc(ngg * nf, -777.0);
    struct GathGrid_t gg = new_gathgrid(&T); /* (f) the round trip of the grid */
    gg.rgpg = T.myproc == 1 ? again_g : NULL, gg.rgp = in, gg.nto = ones, gg.nfld = nf, gg.nproma = nproma, gg.ngpblks = nb;
    OK(trans_gathgrid(&gg));
    if (g_rank == 1 && memcmp(again_g, gpg, sizeof(double) * ngg * nf)) FAIL("trans_distgrid -> trans_gathgrid is not the identity");
    free(again_g);
    double *o_v = alloc(ns2 * nuv, NAN), *o_d = alloc(ns2 * nuv, NAN), *o_s = alloc(ns2 * nsc, NAN), *o_mu = alloc(nuv, -777.0), *o_mv = alloc(nuv, -777.0);
    double *a_in = arr(in, blocked(nf)), *a_v = arr(o_v, ns2 * nuv), *a_d = arr(o_d, ns2 * nuv), *a_s = arr(o_s, ns2 * nsc);
    struct DirTrans_t d = new_dirtrans(&T);
    d.nvordiv = nuv, d.nscalar = nsc, d.rspvor = a_v, d.rspdiv = a_d, d.rspscalar = a_s, d.rmeanu = o_mu, d.rmeanv = o_mv;
    d.rgp = a_in, d.nproma = nproma, d.ngpblks = nb;
    OK(trans_dirtrans(&d));
    back(o_v, a_v, ns2 * nuv), back(o_d, a_d, ns2 * nuv), back(o_s, a_s, ns2 * nsc), back(in, a_in, blocked(nf));
    free(gath_spec("dir_vor.f64", o_v, nuv)), free(gath_spec("dir_div.f64", o_d, nuv)), free(gath_spec("dir_sc.f64", o_s, nsc));
    wr("dir_mu.f64", o_mu, sizeof(double) * nuv), wr("dir_mv.f64", o_mv, sizeof(double) * nuv);
    free(in), free(o_v), free(o_d), free(o_s), free(o_mu), free(o_mv);
  }
  /* ---- trans_invtrans_adj: grid inputs (with the extra fields of the flags) -> spectral fields and means */
  for (int k = 0; k < 2; k++) {
    const int mask = masks[k], nf = nfld_of(mask);
    name_of(fn, "gpad", mask, "");
    double *g = rd(fn, ngg * nf), *in = dist_grid(g, nf);
    double *o_v = alloc(ns2 * nuv, NAN), *o_d = alloc(ns2 * nuv, NAN), *o_s = alloc(ns2 * nsc, NAN), *o_mu = alloc(nuv, -777.0), *o_mv = alloc(nuv, -777.0);
    double *a_in = arr(in, blocked(nf)), *a_v = arr(o_v, ns2 * nuv), *a_d = arr(o_d, ns2 * nuv), *a_s = arr(o_s, ns2 * nsc);
    struct InvTransAdj_t ia = new_invtrans_adj(&T);
    ia.nvordiv = nuv, ia.nscalar = nsc, ia.rspvor = a_v, ia.rspdiv = a_d, ia.rspscalar = a_s, ia.rmeanu = o_mu, ia.rmeanv = o_mv;
    ia.rgp = a_in, ia.nproma = nproma, ia.ngpblks = nb;
    ia.lscalarders = mask & 1, ia.luvder_EW = (mask & 2) != 0, ia.lvordivgp = (mask & 4) != 0;
    OK(trans_invtrans_adj(&ia));
    back(o_v, a_v, ns2 * nuv), back(o_d, a_d, ns2 * nuv), back(o_s, a_s, ns2 * nsc), back(in, a_in, blocked(nf));
    name_of(fn, "invad", mask, "_vor");
    free(gath_spec(fn, o_v, nuv));
    name_of(fn, "invad", mask, "_div");
    free(gath_spec(fn, o_d, nuv));
    name_of(fn, "invad", mask, "_sc");
    free(gath_spec(fn, o_s, nsc));
    name_of(fn, "invad", mask, "_mu");
    wr(fn, o_mu, sizeof(double) * nuv);
    name_of(fn, "invad", mask, "_mv");
    wr(fn, o_mv, sizeof(double) * nuv);
    free(g), free(in), free(o_v), free(o_d), free(o_s), free(o_mu), free(o_mv);
  }
  /* ---- trans_dirtrans_adj: spectral fields and means -> u, v, scalars */
  {
    const int nf = nfld_of(0);
    double *out = alloc(blocked(nf), NAN), *a_v = arr(vor, ns2 * nuv), *a_d = arr(div, ns2 * nuv), *a_s = arr(sc, ns2 * nsc), *a_o = arr(out, blocked(nf));
    struct DirTransAdj_t da = new_dirtrans_adj(&T);
    da.nvordiv = nuv, da.nscalar = nsc, da.rspvor = a_v, da.rspdiv = a_d, da.rspscalar = a_s, da.rmeanu = mu, da.rmeanv = mv;
    da.rgp = a_o, da.nproma = nproma, da.ngpblks = nb;
    OK(trans_dirtrans_adj(&da));
    back(out, a_o, blocked(nf)), back(vor, a_v, ns2 * nuv), back(div, a_d, ns2 * nuv), back(sc, a_s, ns2 * nsc);
    gath_grid("dirad.f64", out, nf);
    free(out);
  }
  /* ---- (f) trans_specnorm without and with rmet (ESPECNORM's zero-based metric of nspec2g / 4 + 1 elements) */
  {
    double *norm = alloc(nsc, -777.0), *a_s = arr(sc, ns2 * nsc);
    struct SpecNorm_t s = new_specnorm(&T);
    s.rspec = a_s, s.rnorm = norm, s.nfld = nsc;
    OK(trans_specnorm(&s));
    wr("norm.f64", norm, sizeof(double) * nsc);
    s = new_specnorm(&T);
    s.rspec = a_s, s.rnorm = norm, s.nfld = nsc, s.rmet = rmet;
    OK(trans_specnorm(&s));
    WANT(trans_specnorm(&s), TRANS_STALE_ARG);
    wr("norm_met.f64", norm, sizeof(double) * nsc);
    back(sc, a_s, ns2 * nsc);
    free(norm);
  }
  refusals(nx, ny, dx, dy, mx, my);
  free(vorg), free(divg), free(scg), free(mu), free(mv), free(gpg), free(rmet), free(vor), free(div), free(sc), free(ones);
  OK(trans_delete(&T));
  if (T.mvalue || T.nvalue || T.handle) FAIL("trans_delete");
  OK(trans_finalize());
#ifdef TRANSI_LAM_MPI
  emi_mpi_detach();
  MPI_Finalize();
#endif
  printf("TRANSI LAM OK rank %d\n", g_rank);
  return 0;
}
