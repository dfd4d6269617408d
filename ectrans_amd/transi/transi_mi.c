/* transi_mi.c -- see transi_mi.h.  Thin marshalling onto include/ectrans_mi.h. */
#include "transi_mi.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h> /* device copies of a lat-lon rgp with lglobal (trans_invtrans) */

#include "../../include/ectrans_mi.h"

static int g_limit = 100, g_limit_set = 0;
static double g_radius = 6371.22e3;
static int g_radius_set = 0;
static int g_init = 0;
static char g_msg[1200];

const char *trans_error_msg(int errcode) {
  switch (errcode) {
    case TRANS_SUCCESS: return "Trans: No error";
    case TRANS_NOTIMPL: return "Trans: Not (yet) implemented";
    case TRANS_MISSING_ARG: return "Trans: Required member of the argument structure is missing or not allocated";
    case TRANS_UNRECOGNIZED_ARG: return "Trans: Unrecognized argument";
    case TRANS_STALE_ARG: return "Trans: Passed argument was already used in a previous call";
    default:
      strcpy(g_msg, "Trans: ");
      strncat(g_msg, emi_last_error(), sizeof(g_msg) - 16);
      return g_msg;
  }
}

/* Several tasks: the host attaches a transport first (emi_mpi_attach of ectrans_amd/mpi, emi_rccl_attach of
 * ectrans_amd/rccl: they call emi_init with the task count and number and register the exchange and the host
 * collectives); trans_init then adopts what it finds, as the Fortran shim's SETUP_TRANS0 does.  trans_use_mpi(true) is
 * therefore only accepted once such a transport is attached (the reference: transi.h:177, MPL_INIT inside trans_init). */
int trans_use_mpi(_bool b) {
  int np = 0, me = 0;
  if (!b) return TRANS_SUCCESS;
  return emi_inq_tasks(&np, &me) == 0 ? TRANS_SUCCESS : TRANS_NOTIMPL;
}
/* NPRTRV / NPRGPEW (transi.h:144,156): the decomposition of this library is NPRTRW x 1; LEQ_REGIONS (transi.h:167)
 * has no effect on it (the grid-point distribution equals the latitude bands). */
int trans_set_nprtrv(int n) { return n == 1 ? TRANS_SUCCESS : TRANS_NOTIMPL; }
int trans_set_nprgpew(int n) { return n == 1 ? TRANS_SUCCESS : TRANS_NOTIMPL; }
int trans_set_leq_regions(_bool b) {
  (void)b;
  return TRANS_SUCCESS;
}
int trans_set_handles_limit(int n) {
  if (g_init) return TRANS_ERROR;
  g_limit = n;
  g_limit_set = 1;
  return TRANS_SUCCESS;
}
int trans_set_radius(double r) {
  if (g_init) return TRANS_ERROR;
  g_radius = r;
  g_radius_set = 1;
  return TRANS_SUCCESS;
}

int trans_init(void) {
  if (g_init) return TRANS_SUCCESS;
  int np = 0, me = 0;
  if (emi_inq_tasks(&np, &me) == 0) { /* a transport (or the host) has initialised the library: adopt its tasks */
    /* ... but not silently its handle limit and planet radius: trans_set_handles_limit / trans_set_radius of this host must
     * agree with what the transport passed to emi_init (transi's own default radius is 6371.22e3, transi_module.F90:129-136) */
    int lim = 0;
    double rad = 0.0;
    if (emi_inq_init(&lim, &rad) != 0) return TRANS_ERROR;
    if ((g_limit_set && g_limit > lim) || (g_radius_set && g_radius != rad)) {
      fprintf(stderr, "trans_init: the attached transport initialised the library with kmax_resol %d, radius %.17g; this host asks for %d, %.17g\n",
              lim, rad, g_limit, g_radius);
      return TRANS_ERROR;
    }
    g_init = 1;
    return TRANS_SUCCESS;
  }
  emi_init_t cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.kmax_resol = g_limit;
  cfg.prad = g_radius;
  cfg.nproc = 1;
  cfg.myproc = 1;
  cfg.device = -1;
  if (emi_init(&cfg) != 0) return TRANS_ERROR;
  g_init = 1;
  return TRANS_SUCCESS;
}

int trans_new(struct Trans_t *t) {
  memset(t, 0, sizeof(*t));
  t->nsmax = -1;
  t->lsplit = 1;
  t->flt = -1;
  t->llam = 0;
  t->nmsmax = -1;
  t->ndgux = -1;
  t->pexwn = t->peywn = 1.0;
  return TRANS_SUCCESS;
}

/* transi.c:116-142: a plane grid of ny rows of nx points with cells of dx x dy; the truncation in x and in y */
int trans_set_resol_lam(struct Trans_t *t, int nx, int ny, double dx, double dy) {
  const double two_pi = 6.283185307179586476925286766559;
  if (nx <= 0 || ny <= 0 || !(dx > 0.0) || !(dy > 0.0)) return TRANS_ERROR;
  free(t->nloen);
  t->nloen = NULL;
  t->ndgl = ny;
  t->nlon = nx;
  t->pexwn = two_pi / ((double)nx * dx);
  t->peywn = two_pi / ((double)ny * dy);
  t->llam = 1;
  return TRANS_SUCCESS;
}
int trans_set_trunc_lam(struct Trans_t *t, int trunc_x, int trunc_y) {
  t->llam = 1;
  t->nmsmax = trunc_x;
  t->nsmax = trunc_y;
  return TRANS_SUCCESS;
}

int trans_set_resol(struct Trans_t *t, int ndgl, const int *nloen) {
  t->ndgl = ndgl;
  free(t->nloen);
  t->nloen = (int *)malloc(sizeof(int) * (size_t)ndgl);
  if (!t->nloen) return TRANS_ERROR;
  memcpy(t->nloen, nloen, sizeof(int) * (size_t)ndgl);
  return TRANS_SUCCESS;
}

/* transi.c:94-114: nlat even = the shifted grid (no poles, no equator); nlat odd = poles and equator, set up with ndgl = nlat - 1
 * (SETUP_TRANS works with ndgl + 2 rows, the equator twice) */
int trans_set_resol_lonlat(struct Trans_t *t, int nlon, int nlat) {
  if (nlon <= 0 || nlat < 2) return TRANS_ERROR;
  free(t->nloen);
  t->nloen = NULL;
  t->nlon = nlon;
  t->ndgl = nlat % 2 == 0 ? nlat : nlat - 1;
  t->llatlon = nlat % 2 == 0 ? 2 : 1;
  return TRANS_SUCCESS;
}

int trans_set_trunc(struct Trans_t *t, int nsmax) {
  t->nsmax = nsmax;
  return TRANS_SUCCESS;
}

static int set_path(char **dst, const char *path) {
  free(*dst);
  *dst = NULL;
  if (!path) return TRANS_MISSING_ARG;
  *dst = (char *)malloc(strlen(path) + 1);
  if (!*dst) return TRANS_ERROR;
  strcpy(*dst, path);
  return TRANS_SUCCESS;
}

int trans_set_read(struct Trans_t *t, const char *filepath) { return set_path(&t->readfp, filepath); }

int trans_set_write(struct Trans_t *t, const char *filepath) { return set_path(&t->writefp, filepath); }

int trans_set_cache(struct Trans_t *t, const void *cache, size_t cachesize) {
  t->cache = cache;
  t->cachesize = cachesize;
  return TRANS_SUCCESS;
}

static void fill_sizes(struct Trans_t *t) {
  t->myproc = t->nproc = 1;
  emi_inq_tasks(&t->nproc, &t->myproc);
  emi_inq_int(t->handle, "nspec2", &t->nspec2);
  t->nspec = t->nspec2 / 2;
  emi_inq_int(t->handle, "nspec2g", &t->nspec2g);
  emi_inq_int(t->handle, "nspec2mx", &t->nspec2mx);
  emi_inq_int(t->handle, "nump", &t->nump);
  emi_inq_int(t->handle, "ngptot", &t->ngptot);
  emi_inq_int(t->handle, "ngptotg", &t->ngptotg);
  emi_inq_int(t->handle, "ngptotmx", &t->ngptotmx);
}

/* a limited-area handle: ESETUP_TRANS with one row length (transi_module.F90:1050-1100) */
static int setup_lam(struct Trans_t *t) {
  if (t->ndgl <= 0 || t->nlon <= 0) return TRANS_MISSING_ARG;
  if (t->nmsmax < 0) {
    fprintf(stderr, "trans_setup: ERROR: nmsmax < 0\n");
    return TRANS_ERROR;
  }
  if (t->llatlon) {
    fprintf(stderr, "trans_setup: ERROR: a limited-area handle cannot be a lonlat handle\n");
    return TRANS_ERROR;
  }
  if (t->readfp || t->writefp || t->cachesize > 0 || t->flt > 0) {
    fprintf(stderr, "trans_setup: ERROR: %s is not available on a limited-area handle (there are no Legendre polynomials)\n",
            t->readfp ? "readfp" : t->writefp ? "writefp" : t->cachesize > 0 ? "cache" : "flt");
    return TRANS_NOTIMPL;
  }
  if (t->nsmax < 0) {
    fprintf(stderr, "trans_setup: ERROR: nsmax < 0\n");
    return TRANS_ERROR;
  }
  if (t->ndgux < 0) t->ndgux = t->ndgl;
  free(t->nloen); /* nloen is constant on a limited-area handle */
  t->nloen = (int *)malloc(sizeof(int) * (size_t)t->ndgl);
  if (!t->nloen) return TRANS_ERROR;
  for (int j = 0; j < t->ndgl; j++) t->nloen[j] = t->nlon;
  emi_esetup_t cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.kmsmax = t->nmsmax;
  cfg.ksmax = t->nsmax;
  cfg.kdgl = t->ndgl;
  cfg.kdlon = t->nlon;
  cfg.kdgux = t->ndgux;
  cfg.pexwn = t->pexwn;
  cfg.peywn = t->peywn;
  cfg.precision = 8;
  if (emi_esetup(&cfg, &t->handle) != 0) {
    fprintf(stderr, "trans_setup: ERROR: %s\n", emi_last_error());
    return TRANS_ERROR;
  }
  fill_sizes(t);
  return TRANS_SUCCESS;
}

int trans_setup(struct Trans_t *t) {
  int rc = trans_init();
  if (rc) return rc;
  if (t->llam) return setup_lam(t);
  if (t->ndgl <= 0 || (!t->nloen && t->nlon <= 0)) return TRANS_MISSING_ARG;
  if (t->flt > 0) return TRANS_NOTIMPL;
  if (t->llatlon && (t->nlon <= 0 || t->readfp || t->writefp || t->cachesize > 0)) return TRANS_NOTIMPL; /* no Legendre file of lat-lon rows */
  if (t->nsmax < 0) t->nsmax = t->ndgl - 1; /* default: linear truncation on the given latitudes */
  emi_setup_t cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.ksmax = t->nsmax;
  cfg.kdgl = t->ndgl;
  cfg.kloen = t->nloen;
  cfg.kdlon = t->nlon;
  cfg.precision = 8;
  cfg.ldll = t->llatlon != 0;
  cfg.ldshiftll = t->llatlon == 2;
  emi_legpol_io_t io;
  memset(&io, 0, sizeof(io));
  if (t->cachesize > 0 && !t->cache) { /* transi_module.F90:737-741 */
    fprintf(stderr, "Cache memory was not allocated\n");
    return TRANS_MISSING_ARG;
  }
  if (t->readfp && t->readfp[0]) {
    io.io = "readf";
    io.fname = t->readfp;
  } else if (t->writefp && t->writefp[0]) {
    io.io = "writef";
    io.fname = t->writefp;
  } else if (t->cachesize > 0) {
    io.io = "membuf";
    io.ptr = t->cache;
    io.len = t->cachesize;
  }
  if (emi_setup_legpol(&cfg, io.io ? &io : NULL, &t->handle) != 0) return TRANS_ERROR;
  fill_sizes(t);
  if (t->llatlon == 1) t->ngptotg -= t->nlon; /* the user's global field has nlat rows: the equator once (transi_module.F90:1140) */
  return TRANS_SUCCESS;
}

/* a limited-area handle: nmyms, and n / m of every local coefficient (four reals per (m, n), x-wavenumbers in MYMS order) */
static int inq_one_lam(struct Trans_t *t, const char *v) {
  static const char *gauss[] = {"rmu", "rgw", "ndglu", "nnmeng", "nmeng", "nasm0"};
  for (size_t i = 0; i < sizeof(gauss) / sizeof(gauss[0]); i++)
    if (!strcmp(v, gauss[i])) {
      fprintf(stderr, "trans_inquire: ERROR: %s is a quantity of the Gaussian grid: not available on a limited-area handle\n", v);
      return TRANS_NOTIMPL;
    }
  if (!strcmp(v, "nloen")) return TRANS_SUCCESS; /* filled by trans_setup */
  if (strcmp(v, "nmyms") && strcmp(v, "nvalue") && strcmp(v, "mvalue")) return TRANS_UNRECOGNIZED_ARG;
  if (!t->nmyms) {
    t->nmyms = (int *)malloc(sizeof(int) * (size_t)(t->nump > 0 ? t->nump : 1));
    if (!t->nmyms) return TRANS_ERROR;
    if (emi_inq_int_array(t->handle, "myms", t->nmyms, t->nump)) return TRANS_ERROR;
  }
  if (!strcmp(v, "nmyms")) return TRANS_SUCCESS;
  int *kntmp = (int *)malloc(sizeof(int) * (size_t)(t->nmsmax + 1));
  int **dst = !strcmp(v, "nvalue") ? &t->nvalue : &t->mvalue;
  if (!*dst) *dst = (int *)malloc(sizeof(int) * (size_t)(t->nspec2 > 0 ? t->nspec2 : 1));
  if (!kntmp || !*dst || emi_inq_int_array(t->handle, "kntmp", kntmp, t->nmsmax + 1)) {
    free(kntmp);
    return TRANS_ERROR;
  }
  int k = 0;
  for (int jm = 0; jm < t->nump; jm++) {
    const int m = t->nmyms[jm];
    for (int n = 0; n <= kntmp[m] && k + 4 <= t->nspec2; n++)
      for (int j = 0; j < 4; j++) (*dst)[k++] = dst == &t->nvalue ? n : m;
  }
  free(kntmp);
  return k == t->nspec2 ? TRANS_SUCCESS : TRANS_ERROR;
}

static int inq_one(struct Trans_t *t, const char *v) {
  if (t->llam) return inq_one_lam(t, v);
  if (!strcmp(v, "mvalue")) {
    fprintf(stderr, "trans_inquire: ERROR: mvalue is a quantity of a limited-area handle\n");
    return TRANS_NOTIMPL;
  }
  const int ns = t->nsmax + 1;
  if (!strcmp(v, "rmu") || !strcmp(v, "rgw")) {
    double **dst = !strcmp(v, "rmu") ? &t->rmu : &t->rgw;
    const int nrows = t->llatlon == 1 ? t->ndgl + 2 : t->ndgl; /* the rows of the handle (a lat-lon one has no rgw: the library refuses) */
    if (!*dst) *dst = (double *)malloc(sizeof(double) * (size_t)nrows);
    return emi_inq_real_array(t->handle, v, *dst, nrows) ? TRANS_ERROR : TRANS_SUCCESS;
  }
  struct {
    const char *name, *emi;
    int **dst;
    int len;
  } ints[] = {{"nasm0", "nasm0", &t->nasm0, ns}, {"nmyms", "myms", &t->nmyms, ns}, {"ndglu", "ndglu", &t->ndglu, ns},
              {"nnmeng", "nmen", &t->nnmeng, t->llatlon == 1 ? t->ndgl + 2 : t->ndgl},
              {"nmeng", "nmen", &t->nnmeng, t->llatlon == 1 ? t->ndgl + 2 : t->ndgl}};
  for (size_t i = 0; i < sizeof(ints) / sizeof(ints[0]); i++)
    if (!strcmp(v, ints[i].name)) {
      if (!*ints[i].dst) *ints[i].dst = (int *)malloc(sizeof(int) * (size_t)ints[i].len);
      return emi_inq_int_array(t->handle, ints[i].emi, *ints[i].dst, ints[i].len) ? TRANS_ERROR : TRANS_SUCCESS;
    }
  if (!strcmp(v, "nvalue")) {
    /* [nspec2]: the zonal wavenumbers of THIS task, in MYMS order (with several tasks nspec2 < nspec2g) */
    int *ms = (int *)malloc(sizeof(int) * (size_t)ns);
    if (!t->nvalue) t->nvalue = (int *)malloc(sizeof(int) * (size_t)(t->nspec2 > 0 ? t->nspec2 : 1));
    if (!ms || !t->nvalue || emi_inq_int_array(t->handle, "myms", ms, ns)) {
      free(ms);
      return TRANS_ERROR;
    }
    int k = 0;
    for (int jm = 0; jm < t->nump; jm++)
      for (int n = ms[jm]; n <= t->nsmax && k + 2 <= t->nspec2; n++) {
        t->nvalue[k++] = n;
        t->nvalue[k++] = n;
      }
    free(ms);
    return k == t->nspec2 ? TRANS_SUCCESS : TRANS_ERROR;
  }
  if (!strcmp(v, "nloen")) return TRANS_SUCCESS; /* input, already there */
  return TRANS_UNRECOGNIZED_ARG;
}

int trans_inquire(struct Trans_t *t, const char *varlist) {
  if (!t || !t->handle) return TRANS_MISSING_ARG;
  char buf[512];
  strncpy(buf, varlist, sizeof(buf) - 1);
  buf[sizeof(buf) - 1] = 0;
  for (char *tok = strtok(buf, ", "); tok; tok = strtok(NULL, ", ")) {
    int rc = inq_one(t, tok);
    if (rc) return rc;
  }
  return TRANS_SUCCESS;
}

/* lglobal: rgp is the global field [nfld][ngptotg]; valid with one task only (transi_module.F90:1514-1527) */
static int check_global(const struct Trans_t *t, int lglobal) {
  if (lglobal && t->nproc != 1) {
    fprintf(stderr, "assert_global: ERROR: Configuration only valid for nproc == 1\n");
    return TRANS_ERROR;
  }
  return TRANS_SUCCESS;
}

/* A transi call returns when its results are there (transi has no stream argument): calls on device-resident arrays are queued
 * asynchronously by the library, so wait for the resolution's last call here.  Host-array calls have already synchronised. */
static int run_and_wait(int rc, int handle) {
  if (rc) return TRANS_ERROR;
  return emi_wait(handle) ? TRANS_ERROR : TRANS_SUCCESS;
}

/* a handle set up with trans_set_resol_lonlat serves trans_invtrans only (the library keeps no Gaussian grid beside the lat-lon one) */
static int lonlat_refused(const struct Trans_t *t, const char *who) {
  if (!t->llatlon) return 0;
  fprintf(stderr, "%s: ERROR: not available on a lonlat handle (LDLL): it serves trans_invtrans only\n", who);
  return 1;
}

/* rmeanu / rmeanv: [nvordiv] doubles of a limited-area handle, both required with wind fields (transi_module.F90:1694-1697); a
 * Gaussian handle has none */
static int check_means(const struct Trans_t *t, const char *who, int nvordiv, const double *rmeanu, const double *rmeanv) {
  if (!t->llam) return (rmeanu || rmeanv) ? TRANS_NOTIMPL : TRANS_SUCCESS; /* LAM only */
  if (nvordiv > 0 && (!rmeanu || !rmeanv)) {
    fprintf(stderr, "%s: ERROR: Array %s was not allocated\n", who, !rmeanu ? "RMEANU" : "RMEANV");
    return TRANS_MISSING_ARG;
  }
  return TRANS_SUCCESS;
}

struct DirTrans_t new_dirtrans(struct Trans_t *t) {
  struct DirTrans_t d;
  memset(&d, 0, sizeof(d));
  d.trans = t;
  return d;
}

int trans_dirtrans(struct DirTrans_t *d) {
  if (d->count++ > 0) return TRANS_STALE_ARG;
  if (!d->trans || !d->rgp) return TRANS_MISSING_ARG;
  if (d->nscalar > 0 && !d->rspscalar) return TRANS_MISSING_ARG;
  if (d->nvordiv > 0 && (!d->rspvor || !d->rspdiv)) return TRANS_MISSING_ARG;
  const int rcm = check_means(d->trans, "trans_dirtrans", d->nvordiv, d->rmeanu, d->rmeanv);
  if (rcm) return rcm;
  if (lonlat_refused(d->trans, "trans_dirtrans")) return TRANS_NOTIMPL;
  emi_dirtrans_t a;
  memset(&a, 0, sizeof(a));
  a.mem_space = EMI_MEM_AUTO; /* rgp / rsp* in device memory are used in place, host arrays are staged (emi_ptr_space) */
  if (d->nvordiv > 0) {
    a.spvor = d->rspvor;
    a.spdiv = d->rspdiv;
    a.nf_uv = d->nvordiv;
  }
  if (d->nscalar > 0) {
    a.spscalar = d->rspscalar;
    a.nf_scalar = d->nscalar;
  }
  /* lglobal: rgp is the global field [nfld][ngptotg] (transi_module.F90:1721-1728): one task, so global == local and
   * the call is the unblocked one */
  if (check_global(d->trans, d->lglobal)) return TRANS_ERROR;
  a.kproma = (d->nproma > 0 && !d->lglobal) ? d->nproma : d->trans->ngptot;
  a.gp = d->rgp;
  a.gp_nfld = 2 * d->nvordiv + d->nscalar;
  if (d->trans->llam) /* the means are outputs here (the struct declares them const, as the reference's does) */
    return run_and_wait(emi_edir_trans(d->trans->handle, &a, (void *)d->rmeanu, (void *)d->rmeanv), d->trans->handle);
  return run_and_wait(emi_dir_trans(d->trans->handle, &a), d->trans->handle);
}

struct InvTrans_t new_invtrans(struct Trans_t *t) {
  struct InvTrans_t v;
  memset(&v, 0, sizeof(v));
  v.trans = t;
  return v;
}

/* llatlon == 1 with lglobal: rgp is [nfld][ngptotg] = nlat rows per field, the library computes NDGL = nlat + 1 rows (the equator
 * twice, rows NDGL/2 and NDGL/2 + 1).  The transform runs into a scratch array in the memory rgp lives in and every field is
 * copied across without the second equator row (transi_module.F90:1577-1597) -- device to device when rgp is in device memory. */
static int invtrans_lonlat_global(struct InvTrans_t *v, emi_invtrans_t *a) {
  const struct Trans_t *t = v->trans;
  const size_t nlon = (size_t)t->nlon, ng = (size_t)t->ngptot, ngg = (size_t)t->ngptotg, nf = (size_t)a->gp_nfld;
  const size_t north = (size_t)(t->ndgl + 2) / 2 * nlon, south = ngg - north; /* points up to and including the equator; the rest */
  const int dev = emi_ptr_space(v->rgp) == EMI_MEM_DEVICE;
  double *tmp = NULL;
  if (dev) {
    if (hipMalloc((void **)&tmp, sizeof(double) * ng * nf) != hipSuccess) return TRANS_ERROR;
  } else if (!(tmp = (double *)malloc(sizeof(double) * ng * nf))) {
    return TRANS_ERROR;
  }
  a->gp = tmp;
  int rc = run_and_wait(emi_inv_trans(t->handle, a), t->handle);
  if (!rc && dev) {
    if (hipMemcpy2D(v->rgp, ngg * 8, tmp, ng * 8, north * 8, nf, hipMemcpyDeviceToDevice) != hipSuccess ||
        hipMemcpy2D(v->rgp + north, ngg * 8, tmp + north + nlon, ng * 8, south * 8, nf, hipMemcpyDeviceToDevice) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess)
      rc = TRANS_ERROR;
  } else if (!rc) {
    for (size_t f = 0; f < nf; f++) {
      memcpy(v->rgp + f * ngg, tmp + f * ng, north * 8);
      memcpy(v->rgp + f * ngg + north, tmp + f * ng + north + nlon, south * 8);
    }
  }
  if (dev)
    (void)hipFree(tmp);
  else
    free(tmp);
  return rc;
}

int trans_invtrans(struct InvTrans_t *v) {
  if (v->count++ > 0) return TRANS_STALE_ARG;
  if (!v->trans || !v->rgp) return TRANS_MISSING_ARG;
  if (v->nscalar > 0 && !v->rspscalar) return TRANS_MISSING_ARG;
  if (v->nvordiv > 0 && (!v->rspvor || !v->rspdiv)) return TRANS_MISSING_ARG;
  const int rcm = check_means(v->trans, "trans_invtrans", v->nvordiv, v->rmeanu, v->rmeanv);
  if (rcm) return rcm;
  emi_invtrans_t a;
  memset(&a, 0, sizeof(a));
  a.mem_space = EMI_MEM_AUTO; /* rgp / rsp* in device memory are used in place, host arrays are staged (emi_ptr_space) */
  if (v->nvordiv > 0) {
    a.spvor = v->rspvor;
    a.spdiv = v->rspdiv;
    a.nf_uv = v->nvordiv;
  }
  if (v->nscalar > 0) {
    a.spscalar = v->rspscalar;
    a.nf_scalar = v->nscalar;
  }
  a.ldscders = v->lscalarders;
  a.lduvder = v->luvder_EW;
  a.ldvorgp = a.lddivgp = v->lvordivgp;
  if (check_global(v->trans, v->lglobal)) return TRANS_ERROR;
  a.kproma = (v->nproma > 0 && !v->lglobal) ? v->nproma : v->trans->ngptot; /* lglobal: as trans_dirtrans */
  a.gp = v->rgp;
  a.gp_nfld = 2 * v->nvordiv + v->nscalar + (v->lscalarders ? 2 * v->nscalar : 0) + (v->lvordivgp ? 2 * v->nvordiv : 0) +
              (v->luvder_EW ? 2 * v->nvordiv : 0);
  a.ldlatlon = v->trans->llatlon != 0;
  if (v->trans->llatlon == 1 && v->lglobal) return invtrans_lonlat_global(v, &a);
  if (v->trans->llam) return run_and_wait(emi_einv_trans(v->trans->handle, &a, v->rmeanu, v->rmeanv), v->trans->handle);
  return run_and_wait(emi_inv_trans(v->trans->handle, &a), v->trans->handle);
}

/* ---- adjoints ---- */
struct DirTransAdj_t new_dirtrans_adj(struct Trans_t *t) {
  struct DirTransAdj_t d;
  memset(&d, 0, sizeof(d));
  d.trans = t;
  return d;
}
int trans_dirtrans_adj(struct DirTransAdj_t *d) {
  if (d->count++ > 0) return TRANS_STALE_ARG;
  if (!d->trans || !d->rgp) return TRANS_MISSING_ARG;
  if (d->nscalar > 0 && !d->rspscalar) return TRANS_MISSING_ARG;
  if (d->nvordiv > 0 && (!d->rspvor || !d->rspdiv)) return TRANS_MISSING_ARG;
  const int rcm = check_means(d->trans, "trans_dirtrans_adj", d->nvordiv, d->rmeanu, d->rmeanv);
  if (rcm) return rcm;
  if (lonlat_refused(d->trans, "trans_dirtrans_adj")) return TRANS_NOTIMPL;
  emi_dirtrans_t a;
  memset(&a, 0, sizeof(a));
  a.mem_space = EMI_MEM_AUTO; /* rgp / rsp* in device memory are used in place, host arrays are staged (emi_ptr_space) */
  if (d->nvordiv > 0) a.spvor = d->rspvor, a.spdiv = d->rspdiv, a.nf_uv = d->nvordiv;
  if (d->nscalar > 0) a.spscalar = d->rspscalar, a.nf_scalar = d->nscalar;
  if (check_global(d->trans, d->lglobal)) return TRANS_ERROR;
  a.kproma = (d->nproma > 0 && !d->lglobal) ? d->nproma : d->trans->ngptot;
  a.gp = d->rgp; /* written */
  a.gp_nfld = 2 * d->nvordiv + d->nscalar;
  if (d->trans->llam) return run_and_wait(emi_edir_transad(d->trans->handle, &a, d->rmeanu, d->rmeanv), d->trans->handle);
  return run_and_wait(emi_dir_transad(d->trans->handle, &a), d->trans->handle);
}
struct InvTransAdj_t new_invtrans_adj(struct Trans_t *t) {
  struct InvTransAdj_t v;
  memset(&v, 0, sizeof(v));
  v.trans = t;
  return v;
}
int trans_invtrans_adj(struct InvTransAdj_t *v) {
  if (v->count++ > 0) return TRANS_STALE_ARG;
  if (!v->trans || !v->rgp) return TRANS_MISSING_ARG;
  if (v->nscalar > 0 && !v->rspscalar) return TRANS_MISSING_ARG;
  if (v->nvordiv > 0 && (!v->rspvor || !v->rspdiv)) return TRANS_MISSING_ARG;
  const int rcm = check_means(v->trans, "trans_invtrans_adj", v->nvordiv, v->rmeanu, v->rmeanv);
  if (rcm) return rcm;
  if (lonlat_refused(v->trans, "trans_invtrans_adj")) return TRANS_NOTIMPL;
  if (check_global(v->trans, v->lglobal)) return TRANS_ERROR;
  emi_invtrans_t a;
  memset(&a, 0, sizeof(a));
  a.mem_space = EMI_MEM_AUTO; /* rgp / rsp* in device memory are used in place, host arrays are staged (emi_ptr_space) */
  if (v->nvordiv > 0) a.spvor = v->rspvor, a.spdiv = v->rspdiv, a.nf_uv = v->nvordiv; /* written */
  if (v->nscalar > 0) a.spscalar = v->rspscalar, a.nf_scalar = v->nscalar;
  a.ldscders = v->lscalarders; /* the extra grid fields are further inputs (inv_transad.h) */
  a.lduvder = v->luvder_EW;
  a.ldvorgp = a.lddivgp = v->lvordivgp;
  a.kproma = (v->nproma > 0 && !v->lglobal) ? v->nproma : v->trans->ngptot;
  a.gp = v->rgp;
  a.gp_nfld = 2 * v->nvordiv + v->nscalar + (v->lscalarders ? 2 * v->nscalar : 0) + (v->lvordivgp ? 2 * v->nvordiv : 0) +
              (v->luvder_EW ? 2 * v->nvordiv : 0);
  if (v->trans->llam) /* the means are outputs here */
    return run_and_wait(emi_einv_transad(v->trans->handle, &a, (void *)v->rmeanu, (void *)v->rmeanv), v->trans->handle);
  return run_and_wait(emi_inv_transad(v->trans->handle, &a), v->trans->handle);
}

/* ---- global <-> distributed arrays: DIST_GRID / GATH_GRID / DIST_SPEC / GATH_SPEC of the C-ABI, any task count
 * (transi.h:499-616; nfrom / nto: the task of every field, 1-based; rgpg / rspecg hold the fields of THIS task) ---- */
struct DistGrid_t new_distgrid(struct Trans_t *t) {
  struct DistGrid_t a;
  memset(&a, 0, sizeof(a));
  a.trans = t;
  a.nproma = t->ngptot;
  a.ngpblks = 1;
  return a;
}
struct GathGrid_t new_gathgrid(struct Trans_t *t) {
  struct GathGrid_t a;
  memset(&a, 0, sizeof(a));
  a.trans = t;
  a.nproma = t->ngptot;
  a.ngpblks = 1;
  return a;
}
struct DistSpec_t new_distspec(struct Trans_t *t) {
  struct DistSpec_t a;
  memset(&a, 0, sizeof(a));
  a.trans = t;
  return a;
}
struct GathSpec_t new_gathspec(struct Trans_t *t) {
  struct GathSpec_t a;
  memset(&a, 0, sizeof(a));
  a.trans = t;
  return a;
}
int trans_distgrid(struct DistGrid_t *a) {
  if (a->count++ > 0) return TRANS_STALE_ARG;
  if (!a->trans || !a->rgp || !a->nfrom || a->nfld <= 0 || a->nproma <= 0) return TRANS_MISSING_ARG;
  const long ng = a->trans->ngptot, np = a->nproma, nb = (ng - 1) / np + 1;
  if (a->ngpblks < nb) return TRANS_ERROR;
  /* each array where it lives (EMI_MEM_AUTO): a hipMalloc'ed rgp takes the device path of the library, in place */
  if ((a->trans->llam ? emi_edist_grid_m : emi_dist_grid_m)(a->trans->handle, EMI_MEM_AUTO, a->rgpg, a->nfld, a->nfrom, NULL, a->nproma, EMI_MEM_AUTO, a->rgp))
    return TRANS_ERROR;
  /* the padding of the last NPROMA block (and any further block): zero, as the Fortran DIST_GRID of the shim leaves it -- a
   * malloc'ed rgp must not carry NaNs into a later trans_dirtrans or a checksum */
  const int dev = emi_ptr_space(a->rgp) == EMI_MEM_DEVICE;
  for (long b = nb - 1; b < a->ngpblks; b++) {
    const long first = b == nb - 1 ? ng - (nb - 1) * np : 0;
    for (int f = 0; f < a->nfld; f++) {
      double *pad = a->rgp + ((size_t)b * a->nfld + f) * np + first;
      if (!dev) memset(pad, 0, sizeof(double) * (size_t)(np - first));
      else if (np > first && hipMemset(pad, 0, sizeof(double) * (size_t)(np - first)) != hipSuccess) return TRANS_ERROR;
    }
  }
  return TRANS_SUCCESS;
}
int trans_gathgrid(struct GathGrid_t *a) {
  if (a->count++ > 0) return TRANS_STALE_ARG;
  if (!a->trans || !a->rgp || !a->nto || a->nfld <= 0 || a->nproma <= 0) return TRANS_MISSING_ARG;
  return (a->trans->llam ? emi_egath_grid_m : emi_gath_grid_m)(a->trans->handle, EMI_MEM_AUTO, a->rgpg, a->nfld, a->nto, a->nproma, EMI_MEM_AUTO, a->rgp) ? TRANS_ERROR
                                                                                                                                                        : TRANS_SUCCESS;
}
/* rspecg is [nspec2g][nfldg] here (Fortran PSPECG(nfldg, nspec2g), transi.h:1140-1186), [nfldg][nspec2g] in the C-ABI: it goes through a
 * transposed host copy, so rspecg itself must be a host array; rspec is used where it lives (EMI_MEM_AUTO) */
static int count_mine(const struct Trans_t *t, const int *task, int nfld) {
  int n = 0;
  for (int f = 0; f < nfld; f++) n += task[f] == t->myproc;
  return n;
}
int trans_distspec(struct DistSpec_t *a) {
  if (a->count++ > 0) return TRANS_STALE_ARG;
  if (!a->trans || !a->rspec || !a->nfrom || a->nfld <= 0) return TRANS_MISSING_ARG;
  const int nm = count_mine(a->trans, a->nfrom, a->nfld);
  const size_t ng = (size_t)a->trans->nspec2g;
  double *tmp = NULL;
  if (nm > 0) {
    if (!a->rspecg) return TRANS_MISSING_ARG;
    if (emi_ptr_space(a->rspecg) == EMI_MEM_DEVICE) return TRANS_ERROR;
    tmp = (double *)malloc(sizeof(double) * ng * (size_t)nm);
    if (!tmp) return TRANS_ERROR;
    for (size_t i = 0; i < ng; i++)
      for (int f = 0; f < nm; f++) tmp[(size_t)f * ng + i] = a->rspecg[i * (size_t)nm + f];
  }
  const int rc = (a->trans->llam ? emi_edist_spec_m : emi_dist_spec_m)(a->trans->handle, EMI_MEM_AUTO, tmp, a->nfld, a->nfrom, NULL, EMI_MEM_AUTO, a->rspec);
  free(tmp);
  return rc ? TRANS_ERROR : TRANS_SUCCESS;
}
int trans_gathspec(struct GathSpec_t *a) {
  if (a->count++ > 0) return TRANS_STALE_ARG;
  if (!a->trans || !a->rspec || !a->nto || a->nfld <= 0) return TRANS_MISSING_ARG;
  const int nm = count_mine(a->trans, a->nto, a->nfld);
  const size_t ng = (size_t)a->trans->nspec2g;
  double *tmp = NULL;
  if (nm > 0) {
    if (!a->rspecg) return TRANS_MISSING_ARG;
    if (emi_ptr_space(a->rspecg) == EMI_MEM_DEVICE) return TRANS_ERROR;
    tmp = (double *)malloc(sizeof(double) * ng * (size_t)nm);
    if (!tmp) return TRANS_ERROR;
  }
  const int rc = (a->trans->llam ? emi_egath_spec_m : emi_gath_spec_m)(a->trans->handle, EMI_MEM_AUTO, tmp, a->nfld, a->nto, EMI_MEM_AUTO, a->rspec);
  if (!rc)
    for (size_t i = 0; i < ng; i++)
      for (int f = 0; f < nm; f++) a->rspecg[i * (size_t)nm + f] = tmp[(size_t)f * ng + i];
  free(tmp);
  return rc ? TRANS_ERROR : TRANS_SUCCESS;
}

struct SpecNorm_t new_specnorm(struct Trans_t *t) {
  struct SpecNorm_t s;
  memset(&s, 0, sizeof(s));
  s.trans = t;
  s.nmaster = 1;
  return s;
}

int trans_specnorm(struct SpecNorm_t *s) {
  if (s->count++ > 0) return TRANS_STALE_ARG;
  if (!s->trans || !s->rspec || !s->rnorm || s->nfld <= 0) return TRANS_MISSING_ARG;
  const struct Trans_t *t = s->trans;
  if (t->llam) /* rmet: ESPECNORM's zero-based metric of nspec2g / 4 + 1 elements (transi_mi.h) */
    return emi_especnorm(t->handle, EMI_MEM_AUTO, s->rspec, s->nfld, s->rmet, s->rmet ? t->nspec2g / 4 + 1 : 0, s->rnorm) ? TRANS_ERROR : TRANS_SUCCESS;
  if (s->rmet && t->llatlon) return TRANS_NOTIMPL;
  if (s->rmet) /* SPECNORM's PMET(0:NSMAX) */
    return emi_specnorm_met(t->handle, EMI_MEM_AUTO, s->rspec, s->nfld, s->rmet, t->nsmax + 1, NULL, 0, s->rnorm) ? TRANS_ERROR : TRANS_SUCCESS;
  return emi_specnorm(t->handle, EMI_MEM_AUTO, s->rspec, s->nfld, s->rnorm) ? TRANS_ERROR : TRANS_SUCCESS;
}

struct VorDivToUV_t new_vordiv_to_UV(void) {
  struct VorDivToUV_t v;
  memset(&v, 0, sizeof(v));
  return v;
}
/* transi_module.F90:2663-2740: the same argument checks, then VORDIV_TO_UV(RSPVOR, RSPDIV, RSPU, RSPV, NSMAX) */
int trans_vordiv_to_UV(struct VorDivToUV_t *v) {
  if (v->count++ > 0) return TRANS_STALE_ARG;
  if (v->ncoeff == 0 || v->nsmax == 0) return TRANS_MISSING_ARG;
  if (!v->rspvor || !v->rspdiv || !v->rspu || !v->rspv) return TRANS_MISSING_ARG;
  if (!g_init) {
    const int rc = trans_init();
    if (rc) return rc;
  }
  return emi_vordiv_to_uv(v->nsmax, 8, EMI_MEM_AUTO, v->rspvor, v->rspdiv, v->rspu, v->rspv, v->nfld, v->ncoeff) ? TRANS_ERROR : TRANS_SUCCESS;
}

int trans_delete(struct Trans_t *t) {
  int rc = TRANS_SUCCESS;
  if (t->handle) rc = emi_release(t->handle) ? TRANS_ERROR : TRANS_SUCCESS;
  free(t->readfp), free(t->writefp);
  free(t->nloen), free(t->nmyms), free(t->nasm0), free(t->nvalue), free(t->ndglu), free(t->nnmeng), free(t->rmu), free(t->rgw), free(t->mvalue);
  memset(t, 0, sizeof(*t));
  return rc;
}

int trans_finalize(void) {
  g_init = 0;
  return emi_finalize() ? TRANS_ERROR : TRANS_SUCCESS;
}
