// ectrans_mi.hip -- host orchestration + C-ABI (include/ectrans_mi.h) of libectrans_mi.so.
// Built with hipcc --offload-arch=gfx950 (product) or g++ -x c++ -DEMI_CPU_EMU (test emulator).
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/ectrans_mi.h"
#include "emi_kernels.h"
#include "emi_setup.h"
#include <dlfcn.h>

// ---- roctx ranges named after the reference's GSTATS phases (gpu/internal/tpm_stats.F90:33-55 turns GSTATS into NVTX ranges;
// labels of ectrans-benchmark.F90:1681-1697), so that a rocprofv3 --marker-trace of a Fortran or C host shows INV_TRANS /
// LTINV_CTL / FTINV_CTL ... around the kernel launches.  librocprofiler-sdk-roctx is opened at run time (no link dependency:
// absent library or EMI_ROCTX=0 = no ranges); a range covers the host-side enqueue of its phase.
struct EmiRoctx {
  int (*push)(const char *) = nullptr;
  int (*pop)() = nullptr;
  bool tried = false;
  void load() {
    tried = true;
#ifndef EMI_CPU_EMU
    const char *e = getenv("EMI_ROCTX");
    if (e && atoi(e) == 0) return;
    void *h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return;
    push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
    pop = (int (*)())dlsym(h, "roctxRangePop");
    if (!push || !pop) push = nullptr, pop = nullptr;
#endif
  }
};
static EmiRoctx g_roctx;
struct EmiRange {  // RAII: one nested range
  bool on;
  explicit EmiRange(const char *label) {
    if (!g_roctx.tried) g_roctx.load();
    on = g_roctx.push != nullptr;
    if (on) g_roctx.push(label);
  }
  ~EmiRange() {
    if (on) g_roctx.pop();
  }
};
extern "C" int emi_roctx_active(void) {
  if (!g_roctx.tried) g_roctx.load();
  return g_roctx.push != nullptr;
}
static const char *const EMI_LBL_SETUP = "SETUP_TRANS    - Setup ecTrans handle", *const EMI_LBL_SULEG = "SULEG          - Comp. of Leg. poly.",
                         *const EMI_LBL_INV = "INV_TRANS      - Inverse transform", *const EMI_LBL_DIR = "DIR_TRANS      - Direct transform",
                         *const EMI_LBL_LTINV = "LTINV_CTL      - Inv. Legendre transform", *const EMI_LBL_LTDIR = "LTDIR_CTL      - Dir. Legendre transform",
                         *const EMI_LBL_FTDIR = "FTDIR_CTL      - Dir. Fourier transform", *const EMI_LBL_FTINV = "FTINV_CTL      - Inv. Fourier transform",
                         *const EMI_LBL_TRMTOL = "LTINV_CTL      - M to L transposition", *const EMI_LBL_TRLTOM = "LTDIR_CTL      - L to M transposition";

#ifdef EMI_CPU_EMU
thread_local EmuCtx *emu_ctx = nullptr;
#endif

// ------------------------------------------------------------------------------------------
// errors + runtime helpers
// ------------------------------------------------------------------------------------------
static char g_err[1024] = "";
void emi_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char *emi_last_error(void) { return g_err; }

#define EMI_FAIL(code, ...)     \
  do {                          \
    emi_set_error(__VA_ARGS__); \
    return (code);              \
  } while (0)

#ifndef EMI_CPU_EMU
static void (*g_oom_hook)() = nullptr;  // frees what the library holds only as a cache (emi_stage.h: idle staging buffers)
int emi_dev_malloc(void **p, size_t bytes) {
  if (hipMalloc(p, bytes ? bytes : 16) == hipSuccess) return 0;
  (void)hipGetLastError();
  if (g_oom_hook) g_oom_hook();
  EMI_CHECK(hipMalloc(p, bytes ? bytes : 16));
  return 0;
}
int emi_dev_free(void *p) {
  if (p) EMI_CHECK(hipFree(p));
  return 0;
}
int emi_dev_memset(void *p, int v, size_t bytes, emi_stream_t s) {
  EMI_CHECK(hipMemsetAsync(p, v, bytes, s));
  return 0;
}
int emi_h2d(void *d, const void *s, size_t b, emi_stream_t st) {
  EMI_CHECK(hipMemcpyAsync(d, s, b, hipMemcpyHostToDevice, st));
  return 0;
}
int emi_d2h(void *d, const void *s, size_t b, emi_stream_t st) {
  EMI_CHECK(hipMemcpyAsync(d, s, b, hipMemcpyDeviceToHost, st));
  return 0;
}
int emi_d2d(void *d, const void *s, size_t b, emi_stream_t st) {
  EMI_CHECK(hipMemcpyAsync(d, s, b, hipMemcpyDeviceToDevice, st));
  return 0;
}
int emi_stream_sync(emi_stream_t s) {
  EMI_CHECK(hipStreamSynchronize(s));
  return 0;
}
int emi_mem_info(size_t *f, size_t *t) {
  EMI_CHECK(hipMemGetInfo(f, t));
  return 0;
}
#else
int emi_dev_malloc(void **p, size_t bytes) {
  *p = aligned_alloc(64, ((bytes ? bytes : 16) + 63) / 64 * 64);
  return *p ? 0 : -1;
}
int emi_dev_free(void *p) {
  free(p);
  return 0;
}
int emi_dev_memset(void *p, int v, size_t bytes, emi_stream_t) {
  memset(p, v, bytes);
  return 0;
}
int emi_h2d(void *d, const void *s, size_t b, emi_stream_t) {
  memcpy(d, s, b);
  return 0;
}
int emi_d2h(void *d, const void *s, size_t b, emi_stream_t) {
  memcpy(d, s, b);
  return 0;
}
int emi_d2d(void *d, const void *s, size_t b, emi_stream_t) {
  memmove(d, s, b);
  return 0;
}
int emi_stream_sync(emi_stream_t) { return 0; }
int emi_mem_info(size_t *f, size_t *t) {
  *f = (size_t)8 << 30;
  *t = (size_t)8 << 30;
  return 0;
}
#endif

#include "emi_stage.h"
#ifndef EMI_CPU_EMU
static const bool g_oom_hook_set = (g_oom_hook = emi_stage::trim, true);
#endif

// ---- EMI_MEM_AUTO: where do the caller's arrays live?  The reference GPU back-end treats its caller's arrays as present-or-copyin
// (gpu/internal/trltog_mod.F90:501-523, trgtol_mod.F90:444-448, ltinv_mod.F90:334-338, updsp_mod.F90:96-97): arrays already on the
// device are used in place, host arrays are copied.  Device and managed allocations of any visible GPU count as device memory;
// pageable, pinned and registered host memory is staged (kernels reading rows over PCIe piece by piece would be far slower).
extern "C" int emi_ptr_space(const void *p) {
#ifdef EMI_CPU_EMU
  (void)p;
  return EMI_MEM_HOST;  // the emulator's "device" memory is host memory: staging is a memcpy
#else
  if (!p) return EMI_MEM_HOST;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {  // older runtimes: "invalid value" for memory HIP has never seen
    (void)hipGetLastError();
    return EMI_MEM_HOST;
  }
  return (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged || at.type == hipMemoryTypeArray) ? EMI_MEM_DEVICE : EMI_MEM_HOST;
#endif
}
// mem_space of a call -> EMI_MEM_HOST or EMI_MEM_DEVICE; AUTO classifies every array that is present
static int agree_on_mixed_arrays(const char *who, int ndev, int nhost);
// `collective`: the routine is called by every task together (the transforms): with several tasks a task whose arrays are in both memories must
// not fail alone -- its peers, whose arrays are all in one place, would go on into the exchange and wait for it forever -- so the outcome of
// the classification is agreed over the host collectives (one word per task) before anybody starts.
static int resolve_space(const char *who, int mem_space, std::initializer_list<const void *> arrays, int *out, bool collective = false) {
  if (mem_space == EMI_MEM_HOST || mem_space == EMI_MEM_DEVICE) {
    *out = mem_space;
    return 0;
  }
  if (mem_space != EMI_MEM_AUTO) EMI_FAIL(EMI_ERR_ARG, "%s: mem_space = %d (EMI_MEM_HOST, EMI_MEM_DEVICE or EMI_MEM_AUTO)", who, mem_space);
  int ndev = 0, nhost = 0;
  for (const void *q : arrays)
    if (q) (emi_ptr_space(q) == EMI_MEM_DEVICE ? ndev : nhost)++;
  if (collective) {
    if (agree_on_mixed_arrays(who, ndev, nhost)) return EMI_ERR_ARG;
  } else if (ndev && nhost) {
    EMI_FAIL(EMI_ERR_ARG, "%s: %d ARRAYS OF THE CALL ARE IN DEVICE MEMORY AND %d IN HOST MEMORY (all of them must live in one place)", who, ndev, nhost);
  }
  *out = ndev ? EMI_MEM_DEVICE : EMI_MEM_HOST;
  return 0;
}

template <class T>
static int upload(const std::vector<T> &h, T **d) {
  void *p = nullptr;
  if (emi_dev_malloc(&p, h.size() * sizeof(T))) return -1;
  if ((!h.empty() && emi_h2d(p, h.data(), h.size() * sizeof(T), 0)) || emi_stream_sync(0)) {  // (the wait: the host vector may die right after this call)
    emi_dev_free(p);
    return -1;
  }
  *d = (T *)p;
  return 0;
}
// Device allocations with one owner that frees them: a plan, for its tables, or a stage of SETUP_TRANS, for its temporaries.
struct DevAllocs {
  std::vector<void *> list;
  DevAllocs() = default;
  DevAllocs(const DevAllocs &) = delete;
  DevAllocs &operator=(const DevAllocs &) = delete;
  ~DevAllocs() {
    for (void *p : list) emi_dev_free(p);
  }
  int alloc(void **p, size_t bytes) {
    if (emi_dev_malloc(p, bytes)) return -1;
    list.push_back(*p);
    return 0;
  }
};
// a host table to the device, entered with its owner and assigned to the field that names it
template <class T, class F>
static int upload(DevAllocs &owner, const std::vector<T> &h, F *field) {
  T *d = nullptr;
  if (upload(h, &d)) return -1;
  owner.list.push_back(d);
  *field = d;
  return 0;
}

// launch the fp64 or the fp32 instantiation of a kernel; RT names the real type inside the argument list
#define EMI_LAUNCH_P(esz, kern, grid, block, lds, st, ...)                     \
  do {                                                                         \
    if ((esz) == 8) {                                                          \
      typedef double RT;                                                       \
      EMI_LAUNCH(emi_f64::kern, grid, block, lds, st, __VA_ARGS__);            \
    } else {                                                                   \
      typedef float RT;                                                        \
      EMI_LAUNCH(emi_f32::kern, grid, block, lds, st, __VA_ARGS__);            \
    }                                                                          \
  } while (0)

// ------------------------------------------------------------------------------------------
// per-resolution plan
// ------------------------------------------------------------------------------------------
struct FftClass {  // one launch group of the FFT kernels: latitudes sharing a workgroup size, fields per workgroup and kernel
  int nthr = 0, fbk = 0;
  int hot = 0;  // > 0: specialised kernel k_fft_*_hot<hot> (EMI_HOT_PLAN_LIST)
  int r16 = 0;  // > 0: register-resident kernel k_fft_*_r16<r16> (EMI_R16_LIST)
  int split = 0;  // 2: k_fft_*_r16p<r16> (EMI_R16S_LIST): the row as two convolutions of half its half-length
  int mr = 0;   // 1: direct mixed-radix kernels k_fft_*_mr (EMI_MR_RADICES)
  int gmem = 0;  // 1: the work array does not fit the LDS; k_fft_*_gm on a global scratch buffer (elems: complex numbers per workgroup)
  long long gm_elems = 0;
  std::vector<int> lats;
  int *d_lats = nullptr;
  FftRowDev *d_rows = nullptr;  // one record per latitude of `lats`
  size_t lds = 0;
};
// Legendre tile maps for one column-tile count: block id -> (ml, row tile, column tile).
// Workgroups are dealt round-robin over the 8 XCDs (block b runs on XCD b % 8).  Each XCD gets, for
// every wavenumber, a fixed range of column tiles (and, when there are fewer column tiles than XCDs,
// a residue class of row tiles): the ~64 tiles an XCD has in flight then share a few operand column
// blocks and the Legendre-panel row blocks of one m in its 4 MiB L2, instead of streaming 26 different
// column blocks per row tile (measured: 13x the algorithmic HBM bytes).  Tiles stay m-ascending
// (longest K first) within every XCD, so all XCDs progress through m together.
struct LegMaps {  // (the maps are the plan's allocations, like every table)
  int2 *d_inv = nullptr, *d_dir = nullptr, *d_inv_wide = nullptr, *d_dir_wide = nullptr;  // *_wide: fp32 library, the tiles of zonal wavenumber 0 (k_leg_*_wide)
  long long n_inv = 0, n_dir = 0, n_inv_wide = 0, n_dir_wide = 0;
};

struct Plan {  // owns its device memory; whoever drops a plan that has run something waits for the device first (emi_release)
  Plan() = default;
  Plan(const Plan &) = delete;
  Plan &operator=(const Plan &) = delete;
  ~Plan();
  int nsmax = 0, ndgl = 0, ndgnh = 0;
  bool reduced = false;
  // LDLL: a regular lat-lon grid (rmu = the sines of its rows, no Gaussian weights, no PT panels: INV_TRANS(LDLATLON) only);
  // shiftll: LDSHIFTLL, rows and longitudes offset by half a cell (the longitude half by g.llphase in k_prepack_inv)
  bool ldll = false, shiftll = false;
  // ESETUP_TRANS: a limited-area (bi-Fourier) handle.  nsmax holds KMSMAX, the truncation in x (the wavenumbers that are distributed and
  // that the x-direction kernels cut at); lam_n = KSMAX, the truncation in y.  Full grid of NDGL rows of NDLON points, NMEN = KMSMAX on
  // every row; no Legendre panels, no Gaussian latitudes: rw holds 1 / NDGL and racthe EXWN on every row, which makes the x-direction
  // kernels' per-row weight the normalisation and their GM_EWDER factor i m EXWN.
  bool lam = false;
  int lam_n = 0, kdgux = 0;
  double exwn = 0.0, eywn = 0.0;
  std::vector<int> kntmp;           // [KMSMAX + 1] the ellipse (ellips.F90:71-97)
  std::vector<int> l_kntmp, nesm0;  // [nump] of the local wavenumbers; nesm0 0-based
  std::vector<int> l_npme;          // [nump] NPME of the local wavenumbers: zero-based position of (m, n = 0) in PMET (ESPECNORM)
  const int *d_npme = nullptr;
  LamDev lamdev{};
  int lam_nthr = 0;
  size_t lam_lds = 0;
  double ra = 6371229.0;
  // ---- global geometry (identical on every task)
  std::vector<int> nloen, nmen, ndglu, procm;  // procm[m]: owning task (0-based) of wavenumber m
  std::vector<int> latlo;                      // [nproc+1] latitude band of every task
  std::vector<double> rmu, rw, racthe, cos2;
  int ngptotg = 0, nspec2g = 0;
  // ---- this task's share
  int nproc = 1, me = 0;  // W-set decomposition (NPRTRW, MYSETW - 1)
  // V-sets: the band of W-set w (latitudes latlo[w] .. latlo[w+1]) is cut into NPRTRV sub-bands of whole latitudes, the grid
  // shares of its tasks; vlat[w * nprv + v]: first latitude (0-based, global) of task (w, v), vlat[nproc * nprv] = NDGL
  int nprv = 1, mev = 0;
  std::vector<int> vlat;
  int vfirst(int w, int v) const { return nprv > 1 ? vlat[(size_t)w * nprv + v] : latlo[w]; }        // first latitude of task (w, v)
  int vlast(int w, int v) const { return nprv > 1 ? vlat[(size_t)w * nprv + v + 1] : latlo[w + 1]; }  // one past its last latitude
  long long vpoints(int w, int v) const {  // grid points of task (w, v)
    long long c = 0;
    for (int j = vfirst(w, v); j < vlast(w, v); j++) c += nloen[j];
    return c;
  }
  long long voffset(int v) const {  // first point of sub-band v inside this task's band
    long long c = 0;
    for (int j = latlo[me]; j < vfirst(me, v); j++) c += nloen[j];
    return c;
  }
  int nump = 0, nlat = 0, lat0 = 0;
  int ngptot = 0, nspec2 = 0;
  std::vector<int> mval, nasm0;            // [nump]
  std::vector<int> l_nmen, l_gpoff, l_fbase;  // [nlat]
  std::vector<int> wbase, wrows, ldp, ldk, lattile_pref, ktile_pref, lbase;
  std::vector<long long> offS, offA, offTS, offTA;
  long long frows = 0, lrows = 0, wrows_total = 0, p_elems = 0, pt_elems = 0;
  // exchange (rows of the Fourier buffers per peer); inverse sends Legendre-side -> FFT-side
  std::vector<long long> leg_rows, leg_disp, fft_rows, fft_disp;  // [nproc]
  // device
  EmiGeomDev g{};
  DevAllocs dev_allocs;  // the panels and every table, the Legendre tile maps included
  int esz = 8;  // bytes per real: 8 (fp64 library, the reference's _dp build) or 4 (fp32, _sp)
  char *d_P = nullptr, *d_PT = nullptr;  // esz-sized reals
  // fft
  std::vector<FftPlanDev> fplans;
  std::vector<int> planid;  // [nlat]
  FftTabDev ftab{};
  std::vector<FftClass> fclass;
  std::map<int, LegMaps> legmaps;  // by column-tile count
  // work buffers (grown on demand): W, Legendre-side Fourier buffer, FFT-side Fourier buffer
  // (the same allocation when nproc == 1)
  char *d_W = nullptr, *d_FBL = nullptr, *d_FBF = nullptr;  // esz-sized reals; capacities in reals
  size_t cap_W = 0, cap_FBL = 0, cap_FBF = 0;
  void *d_desc = nullptr;
  size_t cap_desc = 0;
  char *d_fftscr = nullptr;  // work arrays of the rows that exceed the LDS (k_fft_*_gm)
  size_t cap_fftscr = 0;
  void *d_normws = nullptr;  // SPECNORM with PMET: the per-wavenumber sums and the metric of one call (calls end synchronised)
  size_t cap_normws = 0;
  // Calls on one resolution share d_desc, W and the Fourier buffers, whatever stream each call names: every call
  // starts by making its stream wait for the event the previous call of this resolution recorded at its end.
#ifndef EMI_CPU_EMU
  hipEvent_t ev_done = nullptr;
#endif
  bool ev_valid = false;
};

Plan::~Plan() {
#ifndef EMI_CPU_EMU
  if (ev_done) (void)hipEventDestroy(ev_done);
#endif
  emi_dev_free(d_W);
  emi_dev_free(d_FBL);
  if (d_FBF != d_FBL) emi_dev_free(d_FBF);
  emi_dev_free(d_desc);
  emi_dev_free(d_fftscr);
  emi_dev_free(d_normws);
}

static int roundup(int a, int b) { return (a + b - 1) / b * b; }
// EMI_TEST_PATHS (tests only; read at every SETUP_TRANS / call, so a test can flip it): bit 0 = exchange-order row tables on ONE task
// (g.fftrow / legN / legS as with several tasks), bit 1 = the 4-batch three-stream pipeline on one task, bit 2 = the scalar fields of
// DIR_TRANS through k_postpack_dir instead of k_leg_dir's epilogue.  Each is the code several tasks (or the adjoint options) run; the
// switch keeps it under the one-GPU test tier.  Results are identical with and without.
static int test_paths() {
  const char *e = getenv("EMI_TEST_PATHS");
  return e ? atoi(e) : 0;
}
// dynamic LDS of k_leg_dir: the operand stage of its two-parity tile (panel and Fourier rows of 16 latitudes: 56 KiB in fp64, 28 in fp32) and the
// staged destinations of the tile's 64 fields (1 KiB).  A constant per precision since round 5 (no row-number tables, nothing depends on
// NDGNH), so the check is a compile-time one: two workgroups per CU need it below 64 KiB each.
static_assert(LG_LDS_BYTES_DIR + 1024 + 64 <= 65536, "k_leg_dir: stage image + epilogue table above 64 KiB, two workgroups per CU no longer fit");
static size_t leg_dir_lds_bytes(const Plan &P) {
  return (size_t)LG_LDS_BYTES_DIR * P.esz / 8 + 1024 + 64;
}

// order a call on `st` behind the previous call of the same resolution (device-side wait, nothing blocks the host)
static int plan_begin(Plan &P, emi_stream_t st) {
#ifndef EMI_CPU_EMU
  if (P.ev_valid) EMI_CHECK(hipStreamWaitEvent(st, P.ev_done, 0));
#else
  (void)P;
  (void)st;
#endif
  return 0;
}
static int plan_end(Plan &P, emi_stream_t st) {
#ifndef EMI_CPU_EMU
  if (!P.ev_done) EMI_CHECK(hipEventCreateWithFlags(&P.ev_done, hipEventDisableTiming));
  EMI_CHECK(hipEventRecord(P.ev_done, st));
  P.ev_valid = true;
#else
  (void)P;
  (void)st;
#endif
  return 0;
}
// host waits until the last call of the resolution has finished (before its buffers are freed or regrown)
static const char *emi_rt_errstr(int rc) {
#ifndef EMI_CPU_EMU
  return hipGetErrorString((hipError_t)rc);
#else
  (void)rc;
  return "";
#endif
}
// Returns the status of the wait (0 = the stream reached the event): a kernel fault or a lost device surfaces here, and emi_wait -- the
// only completion point of the Fortran shim and transi for device-resident arrays -- turns it into EMI_ERR_RUNTIME.
static int plan_quiesce(Plan &P) {
#ifndef EMI_CPU_EMU
  if (P.ev_valid) return (int)hipEventSynchronize(P.ev_done);
#else
  (void)P;
#endif
  return 0;
}

static struct {
  bool init = false;
  int max_resol = 1;
  double ra = 6371229.0;
  int nproc = 1, myproc = 1;  // the W-set decomposition the plans are built on: NPRTRW tasks, this one is MYSETW
  // NPRTRV > 1 (sump_trans0_mod.F90:49, pe2set_mod.F90:111-112): nproc_all = NPRTRW x NPRTRV tasks; task myproc_all is
  // (MYSETW, MYSETV) = ((myproc_all - 1) / NPRTRV + 1, mod(myproc_all - 1, NPRTRV) + 1); the tasks of a W-set are neighbours
  int nproc_all = 1, myproc_all = 1, nprtrv = 1, mysetv = 1, nprtrv_preset = 0;
  std::vector<std::unique_ptr<Plan>> plans;  // [max_resol] a slot holds a plan from the end of its SETUP_TRANS to its TRANS_RELEASE
  int max_batch = 0;
  int profile = 0;  // 1: phase timers per call; 2: accumulated over the calls since emi_set_profile(2)
  emi_alltoallv_fn a2a = nullptr;
  void *a2a_user = nullptr;
  emi_bcast_fn hc_bcast = nullptr;  // host collectives for DIST_x / GATH_x with several tasks
  emi_allgatherv_fn hc_gather = nullptr;
  void *hc_user = nullptr;
} G;

static Plan *get_plan(int kresol) {
  if (!G.init || kresol < 1 || kresol > (int)G.plans.size()) return nullptr;
  return G.plans[kresol - 1].get();
}

extern "C" int emi_set_nprtrv(int nprtrv) {
  if (G.init) EMI_FAIL(EMI_ERR_STATE, "emi_set_nprtrv: after SETUP_TRANS0");
  if (nprtrv < 1) EMI_FAIL(EMI_ERR_ARG, "emi_set_nprtrv: NPRTRV = %d", nprtrv);
  G.nprtrv_preset = nprtrv;
  return EMI_SUCCESS;
}
extern "C" int emi_init(const emi_init_t *cfg) {
  // SETUP_TRANS0 is idempotent (setup_trans0.F90:108-111)
  if (G.init) return EMI_SUCCESS;
  emi_init_t c{};
  if (cfg) c = *cfg;
  G.max_resol = c.kmax_resol > 0 ? c.kmax_resol : 1;
  G.ra = c.prad > 0 ? c.prad : 6371229.0;
  G.nproc_all = c.nproc > 0 ? c.nproc : 1;
  G.myproc_all = c.myproc > 0 ? c.myproc : 1;
  if (G.myproc_all > G.nproc_all) EMI_FAIL(EMI_ERR_ARG, "emi_init: myproc %d > nproc %d", G.myproc_all, G.nproc_all);
  G.nprtrv = c.nprtrv > 0 ? c.nprtrv : (G.nprtrv_preset > 0 ? G.nprtrv_preset : 1);
  if (G.nproc_all % G.nprtrv != 0)
    EMI_FAIL(EMI_ERR_ARG, "SUMP_TRANS0: NPROC INCONSISTENT WITH NPRTRW (NPROC = %d is not a multiple of NPRTRV = %d)", G.nproc_all, G.nprtrv);
  G.nproc = G.nproc_all / G.nprtrv;                 // NPRTRW
  G.myproc = (G.myproc_all - 1) / G.nprtrv + 1;     // MYSETW
  G.mysetv = (G.myproc_all - 1) % G.nprtrv + 1;     // MYSETV
#ifndef EMI_CPU_EMU
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    EMI_FAIL(EMI_ERR_RUNTIME, "emi_init: no HIP device visible -- libectrans_mi has no CPU path");
  if (c.device >= 0) EMI_CHECK(hipSetDevice(c.device));
#endif
  G.plans.clear();
  G.plans.resize(G.max_resol);
  const char *pe = getenv("EMI_PROFILE");
  G.profile = pe ? atoi(pe) : 0;
  const char *mb = getenv("EMI_MAX_BATCH");
  if (mb) G.max_batch = atoi(mb);
  G.init = true;
  return EMI_SUCCESS;
}

// ------------------------------------------------------------------------------------------
// SETUP_TRANS
// ------------------------------------------------------------------------------------------

// Direct mixed-radix plan of k_fft_*_mr for a complex length sz: radices A, B, C (B, C may be 1) from EMI_MR_RADICES and the
// workgroup threads for `nf` fields per workgroup, by a lane-time model: a pass of radix R costs ops(R) / R + 15 lane
// operations per point (butterfly; LDS round trip, twiddle, addressing), times the idle share of its last sweep.
static double mr_radix_ops(int R) {
  switch (R) {
    case 2: return 4; case 3: return 14; case 4: return 16; case 5: return 36; case 7: return 66; case 11: return 150;
    case 13: return 204; case 17: return 336; case 19: return 414; case 23: return 594;
    case 6: return 3 * 4 + 2 * 14 + 12; case 8: return 4 * 4 + 2 * 16 + 18; case 9: return 6 * 14 + 24; case 10: return 5 * 4 + 2 * 36 + 24;
    case 12: return 4 * 14 + 3 * 16 + 36; case 14: return 7 * 4 + 2 * 66 + 36; case 15: return 5 * 14 + 3 * 36 + 48; case 16: return 8 * 16 + 54;
    case 18: return 9 * 4 + 2 * 108 + 48; case 20: return 5 * 16 + 4 * 36 + 72; case 21: return 7 * 14 + 3 * 66 + 72;
    default: return -1;
  }
}
static bool mr_choose(int sz, int esz, int fac[3], int &fbk, int &nthr) {
  std::vector<int> rs = {
#define EMI_MR_ROW(r_) r_,
      EMI_MR_RADICES(EMI_MR_ROW)
  };
#ifdef EMI_MR_RADICES_F32
  if (esz == 4)
    for (int r : {EMI_MR_RADICES_F32(EMI_MR_ROW)}) rs.push_back(r);
#endif
#undef EMI_MR_ROW
  double best = 1e300;
  bool found = false;
  auto consider = [&](int A, int B, int C) {
    const int P1 = (B * C) | 1;
    const size_t per_field = (size_t)A * P1 * 2 * esz;
    if (per_field > 160 * 1024 || A * P1 > 65535) return;
    int fb = 16;
    while (fb > 1 && fb * per_field > 40960) fb >>= 1;  // (80 / 160 KiB of fields per workgroup were measured: slower)
    const int R[3] = {A, B, C};
    for (int nt = 128; nt <= 256; nt += 64) {
      double cost = 0;
      for (int ip = 0; ip < 3; ip++) {
        if (R[ip] == 1) continue;
        const long long nb = (long long)fb * (sz / R[ip]);
        const long long sweeps = (nb + nt - 1) / nt;
        cost += (double)(sweeps * nt) / (double)nb * (mr_radix_ops(R[ip]) / R[ip] + 15.0);  // (the 15: 0 ... 60 change the phase by < 1 %)
      }
      // The LDS footprint fixes the workgroups per CU, so a smaller workgroup means fewer waves to hide latencies behind, and the
      // Fourier-space stages run over all threads of the workgroup whatever the passes use.  Measured at TCo1279 (per pair, the
      // rows these kernels carry): one size for all rows 64 threads 66 ms, 128: 51.2, 192: 42.1, 256: 38.8 (first version); final
      // kernels with a premium of 0 / 0.12 / 0.25 / 0.5 per wave less: 28.5 / 26.9 / 25.9 / 25.3 ms (0.5 = 256 threads for every
      // row); 320 / 384 / 512 threads: 35.7 / 35.2 / 31.1 ms.
      cost *= 1.0 + 0.5 * (256 - nt) / 64.0;
      if (cost < best * (1.0 - 1e-9) || (cost <= best * (1.0 + 1e-9) && nt > nthr)) {
        best = cost, found = true;
        fac[0] = A, fac[1] = B, fac[2] = C, fbk = fb, nthr = nt;
      }
    }
  };
  for (int A : rs) {
    if (sz % A) continue;
    const int m1 = sz / A;
    if (m1 == 1) consider(A, 1, 1);
    for (int B : rs) {
      if (m1 % B) continue;
      const int C = m1 / B;
      if (C == 1) consider(A, B, 1);
      for (int Cc : rs)
        if (Cc == C) consider(A, B, C);
    }
  }
  return found;
}

// ---- the FFT policy: which kernel family runs a row of length n, and how.  fft_choose decides; build_fft_plans keeps the books.
struct FftSwitches {  // read once per SETUP_TRANS (tests flip them between setups)
  bool mr, r16, r16s, hot;
  static bool off(const char *name) { return getenv(name) && atoi(getenv(name)) == 0; }
  FftSwitches() : mr(!off("EMI_FFT_MR")), r16(!off("EMI_FFT_R16")), r16s(!off("EMI_FFT_R16S")), hot(!getenv("EMI_FFT_NO_HOT")) {}
};
struct HotPlan {  // one row of EMI_HOT_PLAN_LIST: kernel id, work length, factor list, fields per workgroup (of the fp64 library)
  int pc, S, nfac, fac[5], nfl;
};
static const HotPlan g_hot_plans[] = {
#define EMI_HOT_ROW(pc_, S_, nf_, a_, b_, c_, d_, e_, nfl_) {pc_, S_, nf_, {a_, b_, c_, d_, e_}, nfl_},
    EMI_HOT_PLAN_LIST(EMI_HOT_ROW)
#undef EMI_HOT_ROW
};
#define EMI_LIST_ROW(r_) r_,
static const int g_r16_list[] = {EMI_R16_LIST(EMI_LIST_ROW)}, g_r16s_list[] = {EMI_R16S_LIST(EMI_LIST_ROW)};
#undef EMI_LIST_ROW

// fields per workgroup of the in-place LDS kernels: as many as fit ~40 KiB of LDS (power of two, <= 16); longer rows get one
// field per workgroup and more threads
static int fft_fields_40k(size_t per_field) {
  int fbk = 16;
  while (fbk > 1 && fbk * per_field > 40960) fbk >>= 1;
  return fbk;
}
// Threads per workgroup follow the LDS footprint: 256 up to
// 40 KiB, 512 up to 80 KiB, else 1024 -- i.e. always 16 waves per CU at 128 VGPRs.  (One thread per
// radix-8 butterfly, S/8, removes the idle lanes of the second sweep at S = 2560/3072/4608/5120
// but makes workgroups of 5, 9 and 10 waves, of which only one fits the 16-wave budget: measured
// 25 % slower.)
static int fft_threads(size_t lds_bytes) { return lds_bytes <= 40960 ? 256 : (lds_bytes <= 81920 ? 512 : 1024); }

struct FftChoice {
  FftPlanDev pl{};  // n, cmode, sz, blue, mr, r16, split, S, nfac, fac, fbk decided; offsets and launch class are the caller's
  int nthr = 0;     // threads per workgroup (fields per workgroup: pl.fbk)
  int hot = 0;      // > 0: k_fft_*_hot<hot>
  bool gmem = false;  // the work array does not fit the LDS: k_fft_*_gm on a global scratch buffer
};
static int fft_choose(int n, int esz, const FftSwitches &sw, FftChoice &c) {
  FftPlanDev &pl = c.pl;
  pl.n = n;
  pl.cmode = (n % 2 != 0);
  pl.sz = pl.cmode ? n : n / 2;
  std::vector<int> fac;
  pl.blue = !emi::factorize_smooth(pl.sz, fac);
  pl.S = pl.sz;
  // Register-resident kernels (k_fft_*_r16<R1>, round 3): rows of even length whose Bluestein work length fits 256 R1, R1 from
  // EMI_R16_LIST and at least 8 -- at TCo1279 every row of 1540 to 4098 points.  EMI_FFT_R16=0 keeps the in-place LDS kernels (the
  // tests run the same rows through both families).
  // Rows of that range with a 7-smooth half-length take them too: per
  // point the generic kernels cost 8.7 ps and row, the convolution 5.5 - 6 ps per work point (profiles/r3c_pmc_fft.txt), although it
  // does four times the arithmetic -- every one of those 100-odd row lengths has its own factor list, which the generic kernels
  // walk at run time.
  // Direct mixed-radix kernels (k_fft_*_mr, round 3): even rows whose half-length is a product of at most three radices of
  // EMI_MR_RADICES -- no convolution.  EMI_FFT_MR=0: off (tests: the same rows through the convolution kernels).
  int mr_fbk = 0, mr_nthr = 0, mr_fac[3] = {1, 1, 1};
  if (!pl.cmode && pl.sz >= 2 && sw.mr) pl.mr = mr_choose(pl.sz, esz, mr_fac, mr_fbk, mr_nthr) ? 1 : 0;
  if (pl.mr) {
    pl.blue = 0;
    fac.assign(mr_fac, mr_fac + 3);
  }
  if (!pl.mr && !pl.cmode && sw.r16) {
    const int need = 2 * pl.sz - 1;
    if (need > 1536)  // shorter rows: in-place kernels with several fields per workgroup
      for (int r : g_r16_list)
        if (!pl.r16 && 256 * r >= need) pl.r16 = r;
    // Split kernels (k_fft_*_r16p<R1>, round 6): a row too long for one register-resident convolution whose half-length is even runs as
    // two convolutions of length sz / 2, one after the other, joined by one decimation step (emi_kernels_body.h).  TCo1279 fp64: 44.6
    // against 48.2 ms per pair for the rows of k_fft_*_hot<23 | 24>; TCo2559 fp32: the rows of 4100 .. 8192 points 192 against 249 ms per
    // pair (profiles/r6_fft_experiments.txt).  EMI_FFT_R16S=0: off (tests and A/B runs: the same rows through the in-place LDS kernels).
    if (!pl.r16 && need > 4096 && pl.sz % 2 == 0 && sw.r16s)
      for (int r : g_r16s_list)
        if (!pl.r16 && 256 * r >= pl.sz - 1) pl.r16 = r, pl.split = 2;
    if (pl.r16) pl.blue = 1;
  }
  if (pl.r16) {
    pl.S = 256 * pl.r16;
    fac.assign(1, pl.r16);  // bookkeeping only: the factor list of these kernels is R1, 16, 16 at compile time
  } else if (pl.blue) {
    pl.S = emi::next_235(2 * pl.sz - 1);
    emi::factorize_smooth(pl.S, fac);
    // Specialised kernels (EMI_HOT_PLAN_LIST): the work length and factor list of the cheapest one that is long
    // enough -- cost model S x (passes + 1), as next_235 -- replace the generic choice when they cost no more: that
    // covers the merged tails (8, 8, 8, 6 | 9 | 10: one LDS round trip fewer than 8, 8, 8, 2, 3 ...) and any work length of the
    // list that is not of the form 2^a {1,3,5,9,15} (there are none at present, see emi_types.h).
    // Even NLOEN only: odd rows run the generic kernels, which have no composite butterflies.  The plan must be the
    // one for the fields-per-workgroup this work length gets (the 40-KiB rule).
    if (!pl.cmode && sw.hot) {
      long long best = (long long)pl.S * (long long)(fac.size() + 1);
      const HotPlan *pick = nullptr;
      for (const HotPlan &r : g_hot_plans) {
        if (r.S < 2 * pl.sz - 1) continue;
        if (fft_fields_40k((size_t)FFT_LDS_ELEMS(r.S) * 2 * esz) < r.nfl) continue;  // (the fp32 library has room for twice the fields: it runs the plan with the list's count, below)
        const long long cost = (long long)r.S * (r.nfac + 1);
        if (cost <= best) {  // list order: a merged tail (ids 22-27) comes after the plain list of its length
          best = cost;
          pick = &r;
        }
      }
      if (pick) {
        pl.S = pick->S;
        fac.assign(pick->fac, pick->fac + pick->nfac);
      }
    }
  }
  if (pl.S > 65535 || fac.size() > 14) EMI_FAIL(EMI_ERR_UNSUPPORTED, "FFT length %d not supported (work size %d)", n, pl.S);
  pl.nfac = (int)fac.size();
  for (int i = 0; i < pl.nfac; i++) pl.fac[i] = fac[i];
  const size_t per_field = (size_t)FFT_LDS_ELEMS(pl.S) * 2 * esz;
  pl.fbk = fft_fields_40k(per_field);
  // a row whose work array exceeds the 160 KiB of LDS (fp64: more than 10240 complex points -- the four longest rows of
  // TCo2559, or any caller grid: the reference takes any KLOEN, ftdir_mod.F90:67-84) runs the same passes on a slice
  // of a global scratch buffer (k_fft_*_gm): slow per row, but such rows are few
  c.gmem = pl.fbk * per_field > 160 * 1024 && !pl.mr;
  c.nthr = fft_threads(pl.fbk * per_field);
  if (pl.r16) {  // one field per workgroup, 256 or 320 threads, one plane + the 240 small twiddles of LDS
    pl.fbk = 1;
    c.nthr = 16 * pl.r16 > 256 ? roundup(16 * pl.r16, 64) : 256;
  } else if (pl.mr) {
    pl.fbk = mr_fbk;
    c.nthr = mr_nthr;
  } else if (pl.blue && !pl.cmode && !c.gmem && sw.hot) {
    // specialised kernel for this work length and factor list?
    // The list's fields-per-workgroup are those of the fp64 library.  The fp32 library could hold twice as many in its 40 KiB, for which no
    // kernel is compiled: until round 6 its short rows (work lengths <= 1536) therefore fell through to the generic kernels -- 14.7 of the
    // 117 ms of FFT per pair at TCo1279 (profiles/r6_pmc_fft_fp32.txt: k_fft_dir 8.35 + k_fft_inv 6.32 ms).  They take the list's plan with
    // the list's field count now (half the LDS per workgroup; the wave budget of the CU is what limits both).
    int hot_fbk = 0;
    for (const HotPlan &r : g_hot_plans)
      if (r.S == pl.S && r.nfac == pl.nfac && r.nfl <= pl.fbk && std::equal(r.fac, r.fac + r.nfac, pl.fac)) c.hot = r.pc, hot_fbk = r.nfl;
    if (c.hot) {
      pl.fbk = hot_fbk;
      c.nthr = fft_threads(pl.fbk * per_field);  // = hot_threads(pc): what the specialised kernels are compiled for
    }
  }
  for (int i = 0; i < pl.nfac; i++)
    if (!c.hot && !pl.r16 && !pl.mr && (pl.fac[i] == 6 || pl.fac[i] > 8)) EMI_FAIL(EMI_ERR_RUNTIME, "internal: composite FFT radix %d without a specialised kernel (length %d)", pl.fac[i], n);
  return 0;
}

// Work sizes share their tables: the twiddle tables and
// the digit-reversal table depend only on the work size S and its factor list, so all plans with the
// same S share one copy (TCo1279: ~20 work sizes for 1280 row lengths -- 2 MB of twiddles that stay in
// L2 instead of 130 MB); the real-pack twiddles, the chirp and the filter spectrum are per length.
struct FftShared {
  int S, tw_off, perm_off, ptw_off[14];
  std::vector<int> fac;
  int r16 = 0, mr = 0;
};
struct FftTabSizes { size_t tw = 0, ptw = 0, perm = 0, rtw = 0, chirp = 0, bhat = 0; };

// the tables of one work size: tw, ptw, perm at the offsets of `sh`
static void fft_fill_shared(const FftShared &sh, std::vector<d2> &tw, std::vector<d2> &ptw, std::vector<uint16_t> &perm) {
  const int S = sh.S;
  if (sh.mr) {
    const int A = sh.fac[0], B = sh.fac[1], C = sh.fac[2], P1 = (B * C) | 1;
    auto w = [&](long long e) {
      long double a = 2.0L * (long double)M_PIl * (long double)(e % S) / (long double)S;
      return d2{(double)cosl(a), (double)-sinl(a)};
    };
    d2 *t1 = ptw.data() + sh.ptw_off[0], *t2 = ptw.data() + sh.ptw_off[1];
    for (int k1 = 0; k1 < A; k1++) t1[k1] = w((long long)C * k1);
    for (int q = 0; q < A * B; q++) t2[q] = w((long long)q);
    for (int k = 0; k < S; k++) perm[sh.perm_off + k] = (uint16_t)((k % A) * P1 + ((k / A) % B) * C + k / (A * B));
    return;
  }
  if (sh.r16) {
    d2 *dst = ptw.data() + sh.ptw_off[0];
    for (int row = 0; row < 7; row++) {
      const int mult = row < 3 ? row + 1 : 4 * (row - 2);
      for (int t = 0; t < 256; t++) {
        long double a = 2.0L * (long double)M_PIl * (long double)(((long long)t * mult) % S) / (long double)S;
        *dst++ = d2{(double)cosl(a), (double)-sinl(a)};
      }
    }
    return;
  }
  for (int k = 0; k < S; k++) {
    long double a = 2.0L * (long double)M_PIl * (long double)k / (long double)S;
    tw[sh.tw_off + k] = d2{(double)cosl(a), (double)-sinl(a)};
  }
  // per-pass twiddle tables, [t-1][j] with j fastest (coalesced reads)
  long long lenp = 1;
  for (size_t ip = 0; ip < sh.fac.size(); ip++) {
    const int R = sh.fac[ip];
    d2 *dst = ptw.data() + sh.ptw_off[ip];
    if (lenp > 1)
      for (int t = 1; t < R; t++)
        for (long long j = 0; j < lenp; j++) {
          long double a = 2.0L * (long double)M_PIl * (long double)((j * t) % (lenp * R)) / (long double)(lenp * R);
          *dst++ = d2{(double)cosl(a), (double)-sinl(a)};
        }
    lenp *= R;
  }
  std::vector<uint16_t> pm;
  emi::dit_positions(S, sh.fac, pm);
  std::copy(pm.begin(), pm.end(), perm.begin() + sh.perm_off);
}

// the tables of one row length: rtw, chirp, bhat at the offsets of `pl` (perm: filled before)
static void fft_fill_length(const FftPlanDev &pl, const std::vector<uint16_t> &perm, std::vector<d2> &rtw, std::vector<d2> &chirp, std::vector<d2> &bhat) {
  const int n = pl.n;
  const double tpi = 2.0 * M_PI;
  for (int k = 0; k <= pl.sz; k++) {
    double a = tpi * (double)k / (double)n;
    rtw[pl.rtw_off + k] = d2{std::cos(a), -std::sin(a)};
  }
  if (!pl.blue) return;
  d2 *c = chirp.data() + pl.chirp_off;
  const int csz = pl.split ? pl.sz / 2 : pl.sz;  // length of the chirp-z transform(s) of the row: the split kernels run two of sz / 2
  for (int k = 0; k < csz; k++) {
    long long k2 = ((long long)k * k) % (2LL * csz);
    double a = M_PI * (double)k2 / (double)csz;
    c[k] = d2{std::cos(a), -std::sin(a)};  // exp(-i pi k^2/csz)
  }
  // filter b_j = conj(c_|j|) wrapped to length L; Bhat = DFT_L(b) (direct O(L*sz) sum in
  // long double: setup only, keeps the table accurate to ~1e-17), stored at the DIT positions
  const int L = pl.S, r0 = pl.fac[0];
  const uint16_t *pm = pl.r16 ? nullptr : perm.data() + pl.perm_off;
  std::vector<long double> cr(L);
  for (int k = 0; k < L; k++) cr[k] = cosl(2.0L * (long double)M_PIl * (long double)k / (long double)L);
  d2 *bh = bhat.data() + pl.bhat_off;
  for (int k = 0; k < L; k++) {
    long double sr = c[0].x, si = -c[0].y;
    long long jk = 0;
    for (int jj = 1; jj < csz; jj++) {
      // b_j + b_{L-j} term: conj(c_j) * (w^{jk} + w^{-jk}) = conj(c_j) * 2 cos(2 pi j k/L)
      jk += k;
      if (jk >= L) jk -= L;
      long double cs = 2.0L * cr[jk];
      sr += (long double)c[jj].x * cs;
      si += -(long double)c[jj].y * cs;
    }
    // position p = pm[k] of the DIT-ordered spectrum belongs to the middle butterfly q = p / R0 as its
    // element t = p % R0; stored [t][q] so that a wave reads its filter values coalesced
    if (pl.r16) {
      // k = k0 + R1 (k1 + 16 k2) sits in register k2 of thread 16 k0 + k1 of the fused middle pass: table [k2][16 k0 + k1]
      const int k0 = k % pl.r16, kk = k / pl.r16, k1 = kk % 16, k2 = kk / 16;
      bh[(size_t)k2 * (16 * pl.r16) + 16 * k0 + k1] = d2{(double)(sr / (long double)L), (double)(si / (long double)L)};  // the 1/S of the convolution folded in
      continue;
    }
    const int p = pm[k];
    bh[(size_t)(p % r0) * (L / r0) + p / r0] = d2{(double)sr, (double)si};
  }
}

// the shared tables of a new plan: found, or entered with their offsets
static const FftShared &fft_share_tables(const FftPlanDev &pl, std::map<int, int> &sidx, std::vector<FftShared> &shared, FftTabSizes &n) {
  const int skey = pl.S * 16 + (pl.r16 ? 15 : (pl.mr ? 14 : pl.nfac));  // the tables depend on the factor list: merged and plain lists differ in length
  auto si = sidx.find(skey);
  if (si != sidx.end()) return shared[si->second];
  FftShared sh{};
  sh.S = pl.S;
  sh.fac.assign(pl.fac, pl.fac + pl.nfac);
  sh.r16 = pl.r16;
  sh.mr = pl.mr;
  sh.tw_off = (int)n.tw;
  sh.perm_off = (int)n.perm;
  if (pl.mr) {
    // twiddle bases of pass 2, [k1]: w^(C k1), and of pass 3, [k1 + A k2]: w^(k1 + A k2) (input r of a butterfly times base^r);
    // perm[k] = LDS position of coefficient k
    const int A = pl.fac[0], B = pl.fac[1];
    sh.ptw_off[0] = (int)n.ptw;
    n.ptw += (size_t)A;
    sh.ptw_off[1] = (int)n.ptw;
    n.ptw += (size_t)A * B;
    sh.ptw_off[2] = (int)n.ptw;
    n.perm += pl.S;
  } else if (pl.r16) {
    // the digit twiddles of A1 / B1: rows 0..2 = w^(t qa), qa = 1..3; rows 3..6 = w^(4 t qb), qb = 1..4; w = exp(-2 pi i / S), t < 256
    sh.ptw_off[0] = (int)n.ptw;
    n.ptw += 7 * 256;
  } else {
    n.tw += pl.S;
    n.perm += pl.S;
    long long lenp = 1;
    for (int ip = 0; ip < pl.nfac; ip++) {
      sh.ptw_off[ip] = (int)n.ptw;
      if (lenp > 1) n.ptw += (size_t)(pl.fac[ip] - 1) * lenp;
      lenp *= pl.fac[ip];
    }
  }
  sidx.emplace(skey, (int)shared.size());
  shared.push_back(sh);
  return shared.back();
}

static int build_fft_plans(Plan &P) {
  // Pass 1 (serial, cheap): one plan per distinct row length (fft_choose); table offsets; launch classes.
  // Pass 2 fills the tables on the host threads, one task per table.
  const FftSwitches sw;
  std::map<int, int> idx;            // row length -> plan
  std::map<int, int> sidx;           // work size -> shared tables
  std::vector<FftShared> shared;
  FftTabSizes nt;
  P.planid.assign(P.nlat, 0);
  for (int j = 0; j < P.nlat; j++) {  // local latitudes
    const int n = P.nloen[P.lat0 + j];
    auto it = idx.find(n);
    if (it != idx.end()) {
      P.planid[j] = it->second;
      continue;
    }
    FftChoice c;
    if (int rc = fft_choose(n, P.esz, sw, c)) return rc;
    FftPlanDev &pl = c.pl;
    const FftShared &sh = fft_share_tables(pl, sidx, shared, nt);
    pl.tw_off = sh.tw_off;
    pl.perm_off = sh.perm_off;
    for (int ip = 0; ip < pl.nfac; ip++) pl.ptw_off[ip] = sh.ptw_off[ip];
    pl.rtw_off = (int)nt.rtw;
    nt.rtw += pl.sz + 1;
    if (pl.blue) {
      pl.chirp_off = (int)nt.chirp;
      nt.chirp += pl.split ? pl.sz / 2 : pl.sz;
      pl.bhat_off = (int)nt.bhat;
      nt.bhat += pl.S;
    }
    if (nt.tw > 0x7fffffffULL || nt.ptw > 0x7fffffffULL || nt.bhat > 0x7fffffffULL) EMI_FAIL(EMI_ERR_UNSUPPORTED, "FFT tables too large");
    int cls = -1;
    for (size_t k = 0; k < P.fclass.size(); k++) {
      const FftClass &fc = P.fclass[k];
      if (fc.nthr == c.nthr && fc.fbk == pl.fbk && fc.hot == c.hot && fc.r16 == pl.r16 && fc.split == pl.split && fc.mr == pl.mr && fc.gmem == (int)c.gmem) cls = (int)k;
    }
    if (cls < 0) {
      cls = (int)P.fclass.size();
      P.fclass.emplace_back();
      FftClass &fc = P.fclass[cls];
      fc.nthr = c.nthr, fc.fbk = pl.fbk, fc.hot = c.hot, fc.r16 = pl.r16, fc.split = pl.split, fc.mr = pl.mr, fc.gmem = c.gmem;
    }
    pl.lds_class = cls;
    idx[n] = P.planid[j] = (int)P.fplans.size();
    P.fplans.push_back(pl);
  }
  if (P.lam) {
    // The y-direction of a limited-area handle: ONE complex plan of length NDGL for the generic in-LDS passes (k_lam_inv, k_lam_dir) --
    // mixed radix where NDGL is a product of 2, 3, 4, 5, 7, 8, Bluestein otherwise -- with the tables every plan has.  No launch class:
    // the kernels take it by number (LamDev::yplan).
    FftPlanDev pl{};
    pl.n = pl.sz = pl.S = P.ndgl;
    pl.cmode = 1;
    std::vector<int> fac;
    pl.blue = !emi::factorize_smooth(pl.sz, fac);
    if (pl.blue) {
      pl.S = emi::next_235(2 * pl.sz - 1);
      emi::factorize_smooth(pl.S, fac);
    }
    // [field][point] work array of an even number of fields (u and v of a wind pair share a workgroup in k_lam_dir), an odd number of
    // complex elements from field to field; up to 80 KiB per workgroup (two per CU) where that holds two fields, the whole LDS otherwise
    const int fs = FFT_LDS_ELEMS(pl.S) + 1, fs_max = 160 * 1024 / (4 * P.esz);
    if (fs > fs_max || pl.S > 65535 || fac.size() > 14)
      EMI_FAIL(EMI_ERR_UNSUPPORTED,
               "ESETUP_TRANS: KDGL = %d NEEDS A WORK ARRAY OF %d COMPLEX NUMBERS PER FIELD (KDGL WHERE IT FACTORISES IN 2, 3, 5, 7, ELSE THE CONVOLUTION LENGTH ABOVE 2 KDGL); THE "
               "Y-DIRECTION KERNELS HOLD TWO FIELDS IN THE 160 KIB OF LDS: AT MOST %d",
               P.ndgl, fs, fs_max);
    pl.nfac = (int)fac.size();
    for (int i = 0; i < pl.nfac; i++) pl.fac[i] = fac[i];
    const size_t per_field = (size_t)fs * 2 * P.esz;
    pl.fbk = std::max(2, std::min(16, (int)(80 * 1024 / per_field) / 2 * 2));
    const FftShared &sh = fft_share_tables(pl, sidx, shared, nt);
    pl.tw_off = sh.tw_off;
    pl.perm_off = sh.perm_off;
    for (int ip = 0; ip < pl.nfac; ip++) pl.ptw_off[ip] = sh.ptw_off[ip];
    pl.rtw_off = (int)nt.rtw;
    nt.rtw += pl.sz + 1;
    if (pl.blue) {
      pl.chirp_off = (int)nt.chirp;
      nt.chirp += pl.sz;
      pl.bhat_off = (int)nt.bhat;
      nt.bhat += pl.S;
    }
    pl.lds_class = -1;
    P.lamdev.yplan = (int)P.fplans.size();
    P.lamdev.fbk = pl.fbk;
    P.lamdev.fs = fs;
    P.lam_lds = (size_t)pl.fbk * per_field;
    P.lam_nthr = std::min(512, fft_threads(P.lam_lds));  // (EMI_KERNEL_LAM: at most 512 threads)
    P.fplans.push_back(pl);
  }
  // ---- pass 2: fill the tables
  std::vector<d2> tw(nt.tw), rtw(nt.rtw), chirp(nt.chirp), bhat(nt.bhat), ptw(nt.ptw);
  std::vector<uint16_t> perm(nt.perm);
  emi::parallel_for((int)shared.size(), [&](int is) { fft_fill_shared(shared[is], tw, ptw, perm); });
  // longest rows first: their O(L * sz) filter sums dominate
  std::vector<int> order(P.fplans.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = (int)i;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return P.fplans[a].n > P.fplans[b].n; });
  emi::parallel_for((int)order.size(), [&](int io) { fft_fill_length(P.fplans[order[io]], perm, rtw, chirp, bhat); });
  for (int j = 0; j < P.nlat; j++) {
    const FftPlanDev &pl = P.fplans[P.planid[j]];
    FftClass &fc = P.fclass[pl.lds_class];
    fc.lats.push_back(j);
    if (fc.gmem)
      fc.gm_elems = std::max(fc.gm_elems, (long long)pl.fbk * FFT_LDS_ELEMS(pl.S));
    else if (fc.mr)
      fc.lds = std::max(fc.lds, (size_t)pl.fbk * pl.fac[0] * ((pl.fac[1] * pl.fac[2]) | 1) * 2 * P.esz);
    else if (fc.r16)
      fc.lds = (size_t)fc.r16 * 272 * 8 + (size_t)((fc.split ? 128 * fc.r16 : 0) + 240) * 2 * P.esz;  // plane (+ the parked half of k_fft_*_r16p) + small twiddles
    else
      fc.lds = std::max(fc.lds, (size_t)pl.fbk * FFT_LDS_ELEMS(pl.S) * 2 * P.esz);
  }
  // exp(-2 pi i c k1 / 256), [k1 - 1][c]: the small twiddles of k_fft_*_r16
  std::vector<d2> tw256(15 * 16);
  for (int k1 = 1; k1 < 16; k1++)
    for (int c = 0; c < 16; c++) {
      long double a = 2.0L * (long double)M_PIl * (long double)(c * k1) / 256.0L;
      tw256[(k1 - 1) * 16 + c] = d2{(double)cosl(a), (double)-sinl(a)};
    }
  // the tables are computed in (long) double and rounded once for the fp32 library
  auto upload_c = [&](const std::vector<d2> &v, const void **d) {
    if (P.esz == 8) return upload(P.dev_allocs, v, d);
    std::vector<f2> w(v.size());
    for (size_t i = 0; i < v.size(); i++) w[i] = f2{(float)v[i].x, (float)v[i].y};
    return upload(P.dev_allocs, w, d);
  };
  FftTabDev &ft = P.ftab;
  if (upload_c(tw, &ft.tw) || upload_c(ptw, &ft.ptw) || upload_c(rtw, &ft.rtw) || upload_c(chirp, &ft.chirp) || upload_c(bhat, &ft.bhat) || upload_c(tw256, &ft.tw256) ||
      upload(P.dev_allocs, perm, &ft.perm) || upload(P.dev_allocs, P.fplans, &ft.plans) || upload(P.dev_allocs, P.planid, &ft.planid))
    return EMI_ERR_RUNTIME;
  for (FftClass &fc : P.fclass) {
    if (upload(P.dev_allocs, fc.lats, &fc.d_lats)) return EMI_ERR_RUNTIME;
    std::vector<FftRowDev> rows(fc.lats.size());
    for (size_t i = 0; i < fc.lats.size(); i++) {
      const int j = fc.lats[i];
      const FftPlanDev &pl = P.fplans[P.planid[j]];
      FftRowDev &r = rows[i];
      r.lat = j, r.planid = P.planid[j], r.n = pl.n, r.sz = pl.sz;
      r.nmen = P.l_nmen[j], r.fb0 = P.l_fbase[j], r.gpoff = P.l_gpoff[j], r.chirp_off = pl.chirp_off;
      r.rtw_off = pl.rtw_off, r.bhat_off = pl.bhat_off, r.ptw_off0 = pl.ptw_off[0];
      r.mr_abc = pl.mr ? (pl.fac[0] | (pl.fac[1] << 8) | (pl.fac[2] << 16) | (pl.fbk << 24)) : 0;
      r.racthe = P.racthe[P.lat0 + j], r.rw = P.rw[P.lat0 + j];
    }
    if (upload(P.dev_allocs, rows, &fc.d_rows)) return EMI_ERR_RUNTIME;
  }
  return 0;
}


// ------------------------------------------------------------------------------------------
// CDIO_LEGPOL: the reference's Legendre-polynomial file / memory segment (NPROC = 1 only,
// setup_trans.F90:360-384).  Byte format of write_legpol_mod.F90:66-158 / read_legpol_mod.F90:78-215:
//   4 x int32   'LEGP' 'OL  ' NSMAX NDGNH
//   2*NDGNH x int32   (NLOEN(jgl), NMEN(jgl)), jgl = 1..NDGNH
//   per wavenumber in MYMS order:  RPNMA(IDGLU, ILA) then RPNMS(IDGLU, ILS), 8-byte reals, column-major,
//   IDGLU = MIN(NDGNH, NDGLU(m)), ILA = (NSMAX-m+2)/2, ILS = (NSMAX-m+3)/2, columns with n descending
// ('LEGPOLBF' files carry butterfly-compressed matrices of the FLT option, which this library refuses.)
// ------------------------------------------------------------------------------------------
struct LegpolSource {
  const char *base = nullptr;
  size_t len = 0;
  void *map = nullptr;
  size_t maplen = 0;
  std::vector<size_t> offA, offS;  // byte offsets of RPNMA / RPNMS per wavenumber
  ~LegpolSource() {
    if (map) munmap(map, maplen);
  }
};

static int legpol_open(LegpolSource &src, const emi_legpol_io_t *io, bool membuf) {
  if (membuf) {
    if (!io->ptr) EMI_FAIL(EMI_ERR_ARG, "SETUP_TRANS: KLEGPOLPTR NULL POINTER");
    if (!io->len) EMI_FAIL(EMI_ERR_ARG, "SETUP_TRANS: KLEGPOLPTR_LEN ARGUMENT MISSING");
    src.base = (const char *)io->ptr;
    src.len = io->len;
    return 0;
  }
  if (!io->fname || !io->fname[0]) EMI_FAIL(EMI_ERR_ARG, "SETUP_TRANS: CDLEGPOLFNAME ARGUMENT MISSING");
  int fd = open(io->fname, O_RDONLY);
  struct stat st;
  if (fd < 0 || fstat(fd, &st) != 0) {
    if (fd >= 0) close(fd);
    EMI_FAIL(EMI_ERR_ARG, "READ_LEGPOL: BYTES_IO_OPEN FAILED (%s)", io->fname);
  }
  src.maplen = (size_t)st.st_size;
  src.map = src.maplen ? mmap(nullptr, src.maplen, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
  close(fd);
  if (src.map == MAP_FAILED || !src.map) {
    src.map = nullptr;
    EMI_FAIL(EMI_ERR_ARG, "READ_LEGPOL:BYTES_IO_READ FAILED (%s)", io->fname);
  }
  src.base = (const char *)src.map;
  src.len = src.maplen;
  return 0;
}

// header checks of read_legpol_mod.F90:78-118 and the per-wavenumber offsets
static int legpol_index(LegpolSource &src, int nsmax, int ndgnh, const std::vector<int> &nloen, const std::vector<int> &nmen,
                        const std::vector<int> &ndglu) {
  const size_t head = 16 + (size_t)8 * ndgnh;
  if (src.len < 16) EMI_FAIL(EMI_ERR_ARG, "READ_LEGPOL:BYTES_IO_READ FAILED (segment shorter than its header)");
  int ib[4];
  memcpy(ib, src.base, 16);
  if (memcmp(src.base, "LEGPOL  ", 8) != 0) EMI_FAIL(EMI_ERR_ARG, "READ_LEGPOL:WRONG LABEL");
  if (ib[2] != nsmax) EMI_FAIL(EMI_ERR_ARG, "READ_LEGPOL:WRONG SPECTRAL TRUNCATION");
  if (ib[3] != ndgnh) EMI_FAIL(EMI_ERR_ARG, "READ_LEGPOL:WRONG NO OF GAUSSIAN LATITUDES");
  if (src.len < head) EMI_FAIL(EMI_ERR_ARG, "READ_LEGPOL:BYTES_IO_READ FAILED (segment shorter than its latitude table)");
  for (int j = 0; j < ndgnh; j++) {
    int v[2];
    memcpy(v, src.base + 16 + (size_t)8 * j, 8);
    if (v[0] != nloen[j]) EMI_FAIL(EMI_ERR_ARG, "READ_LEGPOL:WRONG NLOEN (latitude %d: %d, file %d)", j + 1, nloen[j], v[0]);
    if (v[1] != nmen[j]) EMI_FAIL(EMI_ERR_ARG, "READ_LEGPOL:WRONG NMEN (latitude %d: %d, file %d)", j + 1, nmen[j], v[1]);
  }
  size_t off = head;
  src.offA.assign(nsmax + 1, 0);
  src.offS.assign(nsmax + 1, 0);
  for (int m = 0; m <= nsmax; m++) {
    const size_t nd = (size_t)std::min(ndgnh, ndglu[m]);
    src.offA[m] = off;
    off += nd * (size_t)((nsmax - m + 2) / 2) * 8;
    src.offS[m] = off;
    off += nd * (size_t)((nsmax - m + 3) / 2) * 8;
  }
  if (off > src.len) EMI_FAIL(EMI_ERR_ARG, "READ_LEGPOL:BYTES_IO_READ FAILED (%zu bytes needed, %zu present)", off, src.len);
  return 0;
}

static int legpol_write(int kresol, const char *fname);

// ---- SETUP_TRANS in stages.  emi_setup_legpol (the driver, at the end) calls them in this order; each takes what it reads and fills as its
// arguments.  What describes the plan lives in Plan; SetupTables carries the host images of the device tables the plan does not keep.
enum LegpolMode { LP_NONE, LP_READF, LP_WRITEF, LP_MEMBUF };
struct SetupTables {
  std::vector<int> ebase, rowm;                      // local index tables
  std::vector<double> eps, specw, lapin, l_rw, l_racthe;
  std::vector<int> legN, legS, fftrow;               // Fourier-buffer row tables
  bool rowtable = false;                             // several tasks (or EMI_TEST_PATHS bit 0): the FFT side looks its rows up in fftrow
};
struct SetupClock {  // EMI_SETUP_TIMING=1 prints where SETUP_TRANS spends its wall time
  const bool on = getenv("EMI_SETUP_TIMING") && atoi(getenv("EMI_SETUP_TIMING"));
  double t = now();
  static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  void phase(const char *what) {
    if (on) fprintf(stderr, "[emi_setup] %-28s %8.3f s\n", what, now() - t);
    t = now();
  }
};

// stage 1: the arguments and the CDIO_LEGPOL mode (setup_trans.F90:360-384)
static int setup_arguments(const emi_setup_t *cfg, const emi_legpol_io_t *io, LegpolMode *lp_mode) {
  if (!G.init) EMI_FAIL(EMI_ERR_STATE, "SETUP_TRANS: SETUP_TRANS0 HAS TO BE CALLED BEFORE SETUP_TRANS");
  if (!cfg) EMI_FAIL(EMI_ERR_ARG, "emi_setup: null config");
  if (cfg->kdgl <= 0 || cfg->kdgl % 2 != 0) EMI_FAIL(EMI_ERR_ARG, "SETUP_TRANS: KDGL IS NOT A POSITIVE, EVEN NUMBER");
  if (cfg->lduseflt) EMI_FAIL(EMI_ERR_UNSUPPORTED, "SETUP_TRANS: LDUSEFLT not supported (as gpu/external/setup_trans.F90:442)");
  if (cfg->ldshiftll && !cfg->ldll) EMI_FAIL(EMI_ERR_ARG, "SETUP_TRANS: LDSHIFTLL WITHOUT LDLL");
  if (cfg->ldll) {  // one row length: KDLON, or a KLOEN whose entries are all equal
    if (!cfg->kloen && cfg->kdlon <= 0) EMI_FAIL(EMI_ERR_ARG, "SETUP_TRANS: LDLL NEEDS KDLON (OR A UNIFORM KLOEN)");
    for (int j = 1; cfg->kloen && j < cfg->kdgl; j++)
      if (cfg->kloen[j] != cfg->kloen[0]) EMI_FAIL(EMI_ERR_ARG, "SETUP_TRANS: LDLL NEEDS ONE ROW LENGTH (KLOEN(%d) = %d, KLOEN(1) = %d)", j + 1, cfg->kloen[j], cfg->kloen[0]);
  }
  if (cfg->ldstretch) EMI_FAIL(EMI_ERR_UNSUPPORTED, "SETUP_TRANS: PSTRET stretching not supported");
  if (cfg->precision != 0 && cfg->precision != 8 && cfg->precision != 4)
    EMI_FAIL(EMI_ERR_ARG, "emi_setup: precision must be 8 (fp64, the _dp library) or 4 (fp32, _sp), got %d", cfg->precision);
  if (cfg->ksmax < 0) EMI_FAIL(EMI_ERR_ARG, "SETUP_TRANS: KSMAX < 0");
  *lp_mode = LP_NONE;
  if (io && io->io && io->io[0]) {
    std::string mode(io->io);
    while (!mode.empty() && mode.back() == ' ') mode.pop_back();
    if (G.nproc_all > 1) EMI_FAIL(EMI_ERR_UNSUPPORTED, "SETUP_TRANS:CDIO_LEGPOL OPTIONS ONLY FOR NPROC=1 ");
    if (cfg->ldll) EMI_FAIL(EMI_ERR_UNSUPPORTED, "SETUP_TRANS: CDIO_LEGPOL is not available with LDLL (the file format describes Gaussian latitudes)");
    if (mode == "readf" || mode == "READF")
      *lp_mode = LP_READF;
    else if (mode == "writef" || mode == "WRITEF")
      *lp_mode = LP_WRITEF;
    else if (mode == "membuf" || mode == "MEMBUF")
      *lp_mode = LP_MEMBUF;
    else
      EMI_FAIL(EMI_ERR_ARG, "SETUP_TRANS:CDIO_LEGPOL UNKNOWN METHOD (%s)", mode.c_str());
    if (*lp_mode != LP_MEMBUF && (!io->fname || !io->fname[0])) EMI_FAIL(EMI_ERR_ARG, "SETUP_TRANS: CDLEGPOLFNAME ARGUMENT MISSING");
  }
  return 0;
}

// stage 2: the global geometry of P.nsmax / P.ndgl -- NLOEN and the point offsets cum[0 .. NDGL], the Gaussian latitudes and weights,
// cos^2 and 1 / (a cos) (suleg_mod.F90:264-293, 386-394), the wavenumber cut-offs NMEN / NDGLU
static int setup_geometry(const emi_setup_t *cfg, Plan &P, std::vector<long long> &cum) {
  const int L = P.ndgl;
  int ndlon = cfg->kdlon > 0 ? cfg->kdlon : 2 * L;
  P.nloen.assign(L, ndlon);
  if (P.ldll) {
    if (cfg->kloen) P.nloen.assign(L, cfg->kloen[0]);  // uniform (setup_arguments); NDGL may be KDGL + 2
    if (P.nloen[0] <= 0) EMI_FAIL(EMI_ERR_ARG, "SETUP_TRANS: KLOEN INVALID (ONE or MORE POINTS <= 0)");
  } else if (cfg->kloen) {
    ndlon = 0;
    for (int j = 0; j < L; j++) {
      if (cfg->kloen[j] <= 0) EMI_FAIL(EMI_ERR_ARG, "SETUP_TRANS: KLOEN INVALID (ONE or MORE POINTS <= 0)");
      ndlon = std::max(ndlon, cfg->kloen[j]);
    }
    for (int j = 0; j < L; j++) {
      P.nloen[j] = cfg->kloen[j];
      if (cfg->kloen[j] != ndlon) P.reduced = true;
    }
  }
  P.nspec2g = (P.nsmax + 1) * (P.nsmax + 2);
  cum.assign(L + 1, 0);
  for (int j = 0; j < L; j++) cum[j + 1] = cum[j] + P.nloen[j];
  if (cum[L] > 2000000000LL) EMI_FAIL(EMI_ERR_UNSUPPORTED, "grid too large for 32-bit point offsets");
  P.ngptotg = (int)cum[L];
  P.cos2.assign(L, 0.0);
  P.racthe.assign(L, 0.0);
  if (P.ldll) {
    // The rows of the lat-lon grid (setup_trans.F90:258-271), north to south, row L-1-j the mirror of row j.  Unshifted: colatitude
    // j pi / (L - 2), j = 0 .. L/2 - 1 -- the pole (mu = 1) down to the equator (mu = 0, held twice); shifted: (j + 1/2) pi / L.
    // mu = cos(colatitude) exactly on the row (the reference moves the pole and equator rows, suleg_mod.F90:314-332).
    const double pi = 2.0 * std::asin(1.0), eps = 1000.0 * 2.220446049250313e-16;
    P.rmu.assign(L, 0.0);
    P.rw.assign(L, 0.0);  // no Gaussian weights
    for (int j = 0; j < L / 2; j++) {
      const double th = P.shiftll ? ((double)j + 0.5) * pi / (double)L : (double)j * pi / (double)(L - 2);
      double mu = std::cos(th), c = std::sin(th);
      if (!P.shiftll && j == 0) mu = 1.0, c = 0.0;
      if (!P.shiftll && j == L / 2 - 1) mu = 0.0, c = 1.0;
      // 1 / (a cos(latitude)); on a pole row the reference's regularised 1 / ((cos + eps) a) (suleg_mod.F90:179,352), which keeps u, v and
      // the derivatives finite there.  Off the poles eps would cost eps / cos -- 2.5e-11 on the row next to the pole of a 0.5 degree grid,
      // more than the parity bounds of this library -- so it is left out where it is not needed.
      const double ract = c > 0.0 ? 1.0 / c / P.ra : 1.0 / eps / P.ra;
      P.rmu[j] = mu, P.rmu[L - 1 - j] = -mu;
      P.cos2[j] = P.cos2[L - 1 - j] = c * c;
      P.racthe[j] = P.racthe[L - 1 - j] = ract;
    }
  } else {
    emi::gauss_latitudes(L, P.rmu, P.rw);
    for (int j = 0; j < L; j++) {
      double th = std::asin(P.rmu[j]), c = std::cos(th);
      P.cos2[j] = c * c;
      P.racthe[j] = 1.0 / c / P.ra;
    }
  }
  emi::wavenumber_cutoffs(P.nsmax, L, P.nloen, P.reduced, P.cos2, P.nmen, P.ndglu);
  return 0;
}

// stage 3: the distribution over NPRTRW x NPRTRV tasks, identical on every task: the W-set of every wavenumber, the latitude
// band of every W-set and its cut into the grid shares of the V-sets
static int setup_distribution(int N, int L, const std::vector<int> &nloen, const std::vector<long long> &cum, int nprw, int nprv,
                              std::vector<int> &procm, std::vector<int> &latlo, std::vector<int> &vlat) {
  // wavenumbers: the reference's zig-zag W-set assignment (suwavedi_mod.F90:118-137)
  procm.assign(N + 1, 0);
  int ik = 0, ind = 1;
  for (int m = 0; m <= N; m++) {
    ik += ind;
    if (ik > nprw) {
      ik = nprw;
      ind = -1;
    } else if (ik < 1) {
      ik = 1;
      ind = 1;
    }
    procm[m] = ik - 1;
  }
  // latitudes: contiguous bands of whole latitudes (the Fourier-space distribution of sumplatb_mod.F90 with
  // LDSPLIT=.FALSE., which weighs a latitude by NLOEN); the grid-point distribution is chosen identical, so
  // TRGTOL/TRLTOG stay local copies.  The weight here is the measured cost of a row in the FFT kernels (ps per
  // field, both directions, TCo1279 kernel statistics by work length): 20 ps per point up to NLOEN = 1500, falling
  // linearly to 16.9 ps at 4900, plus 1.75 ns per row -- with equal numbers of points the polar tasks of an 8-task
  // TCo1279 job spent 18 % longer in the FFT phase than the equatorial ones (26.8 against 22.6 ms) and set the
  // job's pace (the reference's weight is NLOEN).
  std::vector<long long> wcum(L + 1, 0);
  for (int j = 0; j < L; j++) {
    const double n = (double)nloen[j];
    const double w = n * (n <= 1500.0 ? 20.0 : std::max(15.0, 20.0 - (n - 1500.0) * 0.00091)) + 1750.0;
    wcum[j + 1] = wcum[j] + (long long)(w + 0.5);
  }
  latlo.assign(nprw + 1, 0);
  for (int r = 1; r < nprw; r++) {
    long long target = wcum[L] * r / nprw;
    int j = (int)(std::lower_bound(wcum.begin(), wcum.end(), target) - wcum.begin());
    j = std::max(j, latlo[r - 1] + 1);
    j = std::min(j, L - (nprw - r));
    latlo[r] = j;
  }
  latlo[nprw] = L;
  // V-sets: every band in NPRTRV sub-bands of whole latitudes with (nearly) equal numbers of points -- the grid-point
  // distribution over all NPROC tasks (the reference: sumplat with NPRGPNS = NPROC bands; whole latitudes here as for the bands)
  if (nprv > 1) {
    vlat.assign((size_t)nprw * nprv + 1, L);
    for (int w = 0; w < nprw; w++) {
      const int a0 = latlo[w], a1 = latlo[w + 1];
      if (a1 - a0 < nprv) EMI_FAIL(EMI_ERR_ARG, "SETUP_TRANS: too many tasks: band %d has %d latitudes for %d V-sets", w + 1, a1 - a0, nprv);
      vlat[(size_t)w * nprv] = a0;
      for (int v = 1; v < nprv; v++) {
        const long long target = cum[a0] + (cum[a1] - cum[a0]) * v / nprv;
        int j = (int)(std::lower_bound(cum.begin() + a0, cum.begin() + a1, target) - cum.begin());
        j = std::max(j, vlat[(size_t)w * nprv + v - 1] + 1);
        j = std::min(j, a1 - (nprv - v));
        vlat[(size_t)w * nprv + v] = j;
      }
    }
  }
  return 0;
}

// stage 4: this task's share (W-set P.me of the distribution) and its local index tables
static void setup_local_tables(Plan &P, const std::vector<long long> &cum, SetupTables &T) {
  const int N = P.nsmax;
  P.lat0 = P.latlo[P.me];
  P.nlat = P.latlo[P.me + 1] - P.lat0;
  P.ngptot = (int)(cum[P.latlo[P.me + 1]] - cum[P.lat0]);
  for (int m = 0; m <= N; m++)
    if (P.procm[m] == P.me) P.mval.push_back(m);
  P.nump = (int)P.mval.size();
  const int NU = P.nump, NL = P.nlat;
  for (auto *v : {&P.nasm0, &P.wrows, &P.ldp, &P.ldk, &T.ebase}) v->assign(NU, 0);
  for (auto *v : {&P.wbase, &P.lbase, &P.lattile_pref, &P.ktile_pref}) v->assign(NU + 1, 0);
  for (auto *v : {&P.offS, &P.offA, &P.offTS, &P.offTA}) v->assign(NU, 0);
  int ipos = 0;
  long long poff = 0, ptoff = 0;
  for (int ml = 0; ml < NU; ml++) {
    const int m = P.mval[ml];
    P.nasm0[ml] = ipos;  // 0-based (D%NASM0 - 1, suwavedi_mod.F90:128-133)
    ipos += (N - m + 1) * 2;
    for (int n = m; n <= N; n++) {  // SPNORMD weights (spnormd_mod.F90:40-57)
      T.specw.push_back(m == 0 ? 1.0 : 2.0);
      T.specw.push_back(m == 0 ? 0.0 : 2.0);
    }
    P.wrows[ml] = roundup(N + 2 - m, P.esz == 4 ? 32 : 16);  // whole stages of k_leg_inv: 8 (fp64) | 16 (fp32) rows per parity (LG_KR)
    P.wbase[ml + 1] = P.wbase[ml] + P.wrows[ml];
    int nd = std::min(P.ndgnh, P.ndglu[m]);
    P.lbase[ml + 1] = P.lbase[ml] + nd;
    P.ldp[ml] = roundup(std::max(nd, 1), 64);
    long long pan = (long long)(P.wrows[ml] / 2) * P.ldp[ml];
    P.offS[ml] = poff;
    P.offA[ml] = poff + pan;
    poff += 2 * pan;
    P.ldk[ml] = roundup(P.wrows[ml] / 2, 128);  // whole 128-k tiles of k_leg_dir (zero padded)
    long long pant = (long long)roundup(std::max(nd, 1), 16) * P.ldk[ml];  // k_leg_dir reads stages of 16 latitudes in both precisions (LG_LS)
    P.offTS[ml] = ptoff;
    P.offTA[ml] = ptoff + pant;
    ptoff += 2 * pant;
    P.lattile_pref[ml + 1] = P.lattile_pref[ml] + (nd + 63) / 64;
    {  // k_leg_dir's row tiles.  fp64: 2 per 128 n-pairs (one parity each), and for the rest none | one two-parity tile (<= 64 n-pairs) | two;
       // fp32: two-parity tiles of 64 n-pairs
      const int nk = P.wrows[ml] / 2, r = nk % 128;
      P.ktile_pref[ml + 1] = P.ktile_pref[ml] + (P.esz == 4 ? (nk + 63) / 64 : 2 * (nk / 128) + (r == 0 ? 0 : r <= 64 ? 1 : 2));
    }
    T.ebase[ml] = (int)T.eps.size();
    for (int n = m; n <= N + 2; n++)  // REPSNM (pre_suleg_mod.F90:55-63)
      T.eps.push_back(std::sqrt((double)(n * n - m * m) / (double)(4 * n * n - 1)));
  }
  P.nspec2 = ipos;
  P.p_elems = poff;
  P.pt_elems = P.ldll ? 0 : ptoff;  // LDLL: no direct transform, no transposed panels
  P.wrows_total = P.wbase[NU];
  T.rowm.resize(P.wrows_total);
  for (int ml = 0; ml < NU; ml++)
    for (int r = 0; r < P.wrows[ml]; r++) T.rowm[P.wbase[ml] + r] = ml;
  P.l_nmen.assign(NL, 0);
  P.l_gpoff.assign(NL, 0);
  P.l_fbase.assign(NL + 1, 0);
  T.l_rw.resize(NL);
  T.l_racthe.resize(NL);
  for (int jl = 0; jl < NL; jl++) {
    const int j = P.lat0 + jl;
    P.l_nmen[jl] = P.nmen[j];
    P.l_gpoff[jl] = (int)(cum[j] - cum[P.lat0]);
    P.l_fbase[jl + 1] = P.l_fbase[jl] + P.nmen[j] + 1;
    T.l_rw[jl] = P.rw[j];
    T.l_racthe[jl] = P.racthe[j];
  }
  P.frows = P.l_fbase[NL];
  P.lrows = 2LL * P.lbase[NU];
  T.lapin.assign(N + 4, 0.0);  // RLAPIN(-1:N+2) (pre_suleg_mod.F90:64-69)
  for (int n = 1; n <= N + 2; n++) T.lapin[n + 1] = -(P.ra * P.ra / (double)(n * (n + 1)));
}

// stage 5: the Fourier-buffer row tables.  One task: both sides share one latitude-major buffer
// (row = fbase[lat] + m).  Several tasks: the Legendre-side buffer is cut into one block per
// destination task, the FFT-side buffer into one block per source task with exactly the same row
// order, so the all-to-all-v moves whole blocks.  Inside a block the rows are latitude-major, then
// wavenumber -- the order of the one-task buffer restricted to the block: an FFT workgroup then finds the
// wavenumbers of its latitude in NPROC short contiguous runs.  (The other order, wavenumber-major, makes
// every Fourier row of a latitude a separate far-apart line: measured on one task, EMI_FB_ORDER=m with
// EMI_FB_TABLE=1, the FFT kernels are 13-20 % slower and the Legendre kernels 1 % faster; the row table
// itself costs the FFT kernels 1.5 %.)
// `exchange_order`: the tables of several tasks (also on one task: EMI_TEST_PATHS bit 0); else plain affine rows, no table on the FFT side.
static int setup_row_tables(Plan &P, bool exchange_order, SetupTables &T) {
  const int N = P.nsmax, L = P.ndgl, NP = P.nproc, NU = P.nump, NL = P.nlat;
  std::vector<int> &legN = T.legN, &legS = T.legS, &fftrow = T.fftrow;
  legN.assign(std::max(P.lbase[NU], 1), 0);  // never empty: k_leg_dir clamps its look-ups to an entry that exists
  legS.assign(std::max(P.lbase[NU], 1), 0);
  fftrow.assign(P.frows, 0);
  T.rowtable = exchange_order;
  for (auto *v : {&P.leg_rows, &P.leg_disp, &P.fft_rows, &P.fft_disp}) v->assign(NP, 0);
  if (!exchange_order) {
    for (int ml = 0; ml < NU; ml++) {
      const int m = P.mval[ml], nd = P.lbase[ml + 1] - P.lbase[ml], isl0 = P.ndgnh - nd;
      for (int j = 0; j < nd; j++) {
        legN[P.lbase[ml] + j] = P.l_fbase[isl0 + j] + m;
        legS[P.lbase[ml] + j] = P.l_fbase[L - 1 - isl0 - j] + m;
      }
    }
    for (long long i = 0; i < P.frows; i++) fftrow[i] = (int)i;
    P.leg_rows[0] = P.fft_rows[0] = P.frows;
    return 0;
  }
  auto band_of = [&](int lat) { return (int)(std::upper_bound(P.latlo.begin(), P.latlo.end(), lat) - P.latlo.begin()) - 1; };
  for (int ml = 1; ml < NU; ml++)
    if (P.mval[ml] <= P.mval[ml - 1]) EMI_FAIL(EMI_ERR_RUNTIME, "internal: local wavenumbers not ascending");
  // Legendre side: block d holds the rows (lat in band d, local wavenumber ml with m <= NMEN(lat))
  for (int ml = 0; ml < NU; ml++) {
    const int m = P.mval[ml];
    for (int lat = 0; lat < L; lat++)
      if (P.nmen[lat] >= m) P.leg_rows[band_of(lat)]++;
  }
  for (int d = 1; d < NP; d++) P.leg_disp[d] = P.leg_disp[d - 1] + P.leg_rows[d - 1];
  {
    // the local wavenumbers are ascending, so those present at a latitude are ml = 0 .. cnt-1 and the
    // row of (lat, ml) is the first row of the latitude + ml
    std::vector<long long> pos(P.leg_disp), latbase(L);
    for (int lat = 0; lat < L; lat++) {
      const int cnt = (int)(std::upper_bound(P.mval.begin(), P.mval.end(), P.nmen[lat]) - P.mval.begin());
      latbase[lat] = pos[band_of(lat)];
      pos[band_of(lat)] += cnt;
    }
    for (int ml = 0; ml < NU; ml++) {
      const int nd = P.lbase[ml + 1] - P.lbase[ml], isl0 = P.ndgnh - nd;
      for (int j = 0; j < nd; j++) {
        legN[P.lbase[ml] + j] = (int)(latbase[isl0 + j] + ml);
        legS[P.lbase[ml] + j] = (int)(latbase[L - 1 - isl0 - j] + ml);
      }
    }
  }
  // FFT side: block s holds the rows (local lat, wavenumber m of task s with m <= NMEN(lat)), same order
  for (int m = 0; m <= N; m++)
    for (int jl = 0; jl < NL; jl++)
      if (P.l_nmen[jl] >= m) P.fft_rows[P.procm[m]]++;
  for (int sr = 1; sr < NP; sr++) P.fft_disp[sr] = P.fft_disp[sr - 1] + P.fft_rows[sr - 1];
  {
    std::vector<long long> pos(P.fft_disp);
    for (int jl = 0; jl < NL; jl++)
      for (int m = 0; m <= P.l_nmen[jl]; m++) fftrow[P.l_fbase[jl] + m] = (int)pos[P.procm[m]]++;
  }
  long long tl = 0, tf = 0;
  for (int r = 0; r < NP; r++) tl += P.leg_rows[r], tf += P.fft_rows[r];
  if (tl != P.lrows || tf != P.frows) EMI_FAIL(EMI_ERR_RUNTIME, "internal: exchange tables inconsistent (%lld/%lld, %lld/%lld)", tl, P.lrows, tf, P.frows);
  return 0;
}

// ---- stage 6: the Legendre panels of the local wavenumbers, host part: PS[k][j] = P_{m+2k}^m(mu_{isl0+j}),
// PA[k][j] = P_{m+2k+1}^m, zero padded; plus the [j][k] transposed copy for the direct transform.
// A panel of wavenumber ml on the host is [par][k][j], k < wrows / 2, j < ldp; three ways to fill one:
// CDIO_LEGPOL = readf / membuf: from the file or segment (read_legpol_mod.F90:120-215)
static void panel_from_source(const Plan &P, const LegpolSource &src, int ml, std::vector<double> &pan) {
  const int N = P.nsmax, m = P.mval[ml], nd = P.lbase[ml + 1] - P.lbase[ml], ld = P.ldp[ml], nk = P.wrows[ml] / 2;
  // reference column c holds n descending: row k of the panel (n = m + 2k + par) is column nc-1-k
  for (int par = 0; par < 2; par++) {
    const int nc = par ? (N - m + 2) / 2 : (N - m + 3) / 2;
    const char *mat = src.base + (par ? src.offA[m] : src.offS[m]);
    double *dst = pan.data() + (size_t)par * nk * ld;
    for (int k = 0; k < nc; k++) memcpy(dst + (size_t)k * ld, mat + ((size_t)(nc - 1 - k) * nd) * 8, (size_t)nd * 8);
  }
}
// LDUSERPNM: SUPOL per latitude on the host threads, every panel [ml] filled latitude by latitude
static void panels_belousov(const Plan &P, std::vector<std::vector<double>> &pans) {
  const int N = P.nsmax, NU = P.nump;
  const int nmaxb = N + 1;  // INSMAX = NTMAX + 1 (suleg_mod.F90:402-410)
  const emi::BelousovTables BT = emi::belousov_tables(nmaxb);
  pans.resize(NU);
  for (int ml = 0; ml < NU; ml++) pans[ml].assign((size_t)2 * (P.wrows[ml] / 2) * P.ldp[ml], 0.0);
  emi::parallel_for(P.ndgnh, [&](int j) {
    std::vector<double> pol((size_t)(nmaxb + 1) * (nmaxb + 1), 0.0);
    emi::belousov_latitude(BT, P.rmu[j], pol.data());
    for (int ml = 0; ml < NU; ml++) {
      const int m = P.mval[ml], nd = P.lbase[ml + 1] - P.lbase[ml], isl0 = P.ndgnh - nd;
      if (j < isl0) continue;
      const int ld = P.ldp[ml], nk = P.wrows[ml] / 2;
      double *pan = pans[ml].data();
      for (int par = 0; par < 2; par++)
        for (int k = 0; m + 2 * k + par <= N + 1; k++)
          pan[((size_t)par * nk + k) * ld + (j - isl0)] = pol[(size_t)m * (nmaxb + 1) + (m + 2 * k + par)];
    }
  });
}
// the ordinary Legendre recurrence (supolf_mod.F90:124-142), what k_legpol computes on the device
static void panel_by_recurrence(const Plan &P, int ml, std::vector<double> &pan) {
  const int N = P.nsmax, m = P.mval[ml], nd = P.lbase[ml + 1] - P.lbase[ml], isl0 = P.ndgnh - nd, ld = P.ldp[ml], nk = P.wrows[ml] / 2;
  const int nmax = N + 2;
  std::vector<double> col(nmax + 1);
  std::vector<int> corr(nmax + 1);
  emi::LegCoef lc = emi::legendre_coefficients(m, nmax);
  for (int j = 0; j < nd; j++) {
    double mu = P.rmu[isl0 + j];
    for (int par = 0; par < 2; par++) {
      emi::legendre_column(lc, mu, par, col.data(), corr.data(), P.ldll);
      double *dst = pan.data() + (size_t)par * nk * ld;
      for (int k = 0; m + 2 * k + par <= N + 1; k++) dst[(size_t)k * ld + j] = col[m + 2 * k + par];
    }
  }
}
// Allocates the two panel arrays and fills what the host fills: m = 0, 1 by the recurrence, m >= 2 left to k_legpol (stage 8, once
// the device tables exist) unless `all_m`: every panel from `src` when there is one, else by SUPOL when `belousov`, else by the
// recurrence (EMI_LEGPOL_HOST=1; the host and the device recurrence agree bit for bit, tests/test_gpu_parity.py).
static int setup_panels_host(Plan &P, const LegpolSource *src, bool belousov, bool all_m) {
  const size_t esz = P.esz;
  if (P.dev_allocs.alloc((void **)&P.d_P, (size_t)P.p_elems * esz) || (P.pt_elems && P.dev_allocs.alloc((void **)&P.d_PT, (size_t)P.pt_elems * esz)))
    EMI_FAIL(EMI_ERR_RUNTIME, "cannot allocate %.2f GiB for the Legendre panels", (P.p_elems + P.pt_elems) * (double)esz / (1 << 30));
  std::vector<std::vector<double>> belpan;
  if (belousov) panels_belousov(P, belpan);
  if (emi_dev_memset(P.d_P, 0, (size_t)P.p_elems * esz, 0) || (P.d_PT && emi_dev_memset(P.d_PT, 0, (size_t)P.pt_elems * esz, 0))) return EMI_ERR_RUNTIME;
  emi_stream_sync(0);
  std::atomic<int> bad{0};
  emi::parallel_for(P.nump, [&](int ml) {
    if (P.mval[ml] >= 2 && !all_m) return;
    const int nd = P.lbase[ml + 1] - P.lbase[ml], ld = P.ldp[ml], nk = P.wrows[ml] / 2;
    std::vector<double> pan((size_t)2 * nk * ld, 0.0);
    if (belousov)
      pan.swap(belpan[ml]);
    else if (src)
      panel_from_source(P, *src, ml, pan);
    else
      panel_by_recurrence(P, ml, pan);
    // unshifted LDLL: the odd functions vanish on the equator row; Belousov's series leaves rounding there (cos(k acos(0)) is not 0
    // for odd k), which would make the two copies of the equator differ in their last bits
    if (P.ldll && !P.shiftll && nd == P.ndgnh)
      for (int k = 0; k < nk; k++) pan[((size_t)nk + k) * ld + (nd - 1)] = 0.0;
    // the recurrences always run in double (as the reference's _sp build does: the JPRD work arrays of suleg_mod.F90:130-162);
    // the fp32 library rounds the finished panel once
    std::vector<float> cvt;
    auto put = [&](char *dst, const std::vector<double> &v) {
      if (esz == 8) return emi_h2d(dst, v.data(), v.size() * 8, 0);
      cvt.resize(v.size());
      for (size_t i = 0; i < v.size(); i++) cvt[i] = (float)v[i];
      int rc = emi_h2d(dst, cvt.data(), cvt.size() * 4, 0);
      emi_stream_sync(0);  // cvt is reused
      return rc;
    };
    if (put(P.d_P + P.offS[ml] * esz, pan)) bad = 1;
    if (!P.d_PT) {
      emi_stream_sync(0);
      return;
    }
    const int ldk = P.ldk[ml], ndp = roundup(std::max(nd, 1), 16);  // = the panel extent behind offTA (pant)
    std::vector<double> pt((size_t)2 * ndp * ldk, 0.0);
    for (int par = 0; par < 2; par++)
      for (int k = 0; k < nk; k++)
        for (int j = 0; j < nd; j++) pt[((size_t)par * ndp + j) * ldk + k] = pan[((size_t)par * nk + k) * ld + j];
    if (put(P.d_PT + P.offTS[ml] * esz, pt)) bad = 1;
    emi_stream_sync(0);
  });
  return bad ? EMI_ERR_RUNTIME : 0;
}

// stage 7: the device tables of P.g
static int setup_device_tables(Plan &P, const SetupTables &T) {
  EmiGeomDev &g = P.g;
  g.nsmax = P.nsmax;
  g.nump = P.nump;
  g.nlat = P.nlat;
  g.ngptot = P.ngptot;
  g.m0_wide = P.esz == 4 ? 1 : 0;  // the fp32 library computes zonal wavenumber 0 in double (ledir_mod.F90:133-171)
  g.P = P.d_P;
  g.PT = P.d_PT;
  if (upload(P.dev_allocs, P.mval, &g.mval) || upload(P.dev_allocs, P.l_nmen, &g.nmen) || upload(P.dev_allocs, P.l_gpoff, &g.gpoff) || upload(P.dev_allocs, P.nasm0, &g.nasm0) ||
      upload(P.dev_allocs, P.l_fbase, &g.fbase) || upload(P.dev_allocs, T.fftrow, &g.fftrow) || upload(P.dev_allocs, P.lbase, &g.lbase) || upload(P.dev_allocs, T.legN, &g.legN) ||
      upload(P.dev_allocs, T.legS, &g.legS) || upload(P.dev_allocs, P.wbase, &g.wbase) || upload(P.dev_allocs, P.wrows, &g.wrows) || upload(P.dev_allocs, T.rowm, &g.rowm) ||
      upload(P.dev_allocs, T.ebase, &g.ebase) || upload(P.dev_allocs, P.ldp, &g.ldp) || upload(P.dev_allocs, P.ldk, &g.ldk) || upload(P.dev_allocs, P.lattile_pref, &g.lattile_pref) ||
      upload(P.dev_allocs, P.ktile_pref, &g.ktile_pref) || upload(P.dev_allocs, T.eps, &g.eps) || upload(P.dev_allocs, T.lapin, &g.lapin) || upload(P.dev_allocs, T.l_rw, &g.rw) ||
      upload(P.dev_allocs, T.l_racthe, &g.racthe) || upload(P.dev_allocs, T.specw, &g.specw) || upload(P.dev_allocs, P.offS, &g.offS) || upload(P.dev_allocs, P.offA, &g.offA) ||
      upload(P.dev_allocs, P.offTS, &g.offTS) || upload(P.dev_allocs, P.offTA, &g.offTA))
    return EMI_ERR_RUNTIME;
  if (!T.rowtable) g.fftrow = nullptr;  // one task: rows are fbase[lat] + m, no table (the upload stays the plan's)
  g.llphase = nullptr;
  if (P.shiftll) {
    // LDSHIFTLL: longitudes (i + 1/2) 2 pi / nlon = a rotation of the Fourier coefficient of wavenumber m by e^{i m pi / nlon}
    // (fsc_mod.F90:86-127 does it per row); one row length, so one factor per wavenumber, applied by k_prepack_inv
    const double pi = 2.0 * std::asin(1.0);
    std::vector<double> ph(2 * (size_t)std::max(P.nump, 1), 0.0);
    for (int ml = 0; ml < P.nump; ml++) {
      const double a = (double)P.mval[ml] * pi / (double)P.nloen[0];
      ph[2 * ml] = P.mval[ml] == 0 ? 1.0 : std::cos(a);
      ph[2 * ml + 1] = P.mval[ml] == 0 ? 0.0 : std::sin(a);
    }
    if (upload(P.dev_allocs, ph, &g.llphase)) return EMI_ERR_RUNTIME;
  }
  return 0;
}

// stage 8: the Legendre panels of m >= 2 on the device: one thread per (wavenumber, parity, latitude)
static int setup_panels_device(Plan &P) {
  const int NU = P.nump, nmax = P.nsmax + 2;
  std::vector<double> dcl((size_t)NU * (nmax + 1), 0.0), ddl((size_t)NU * (nmax + 1), 0.0), zf(NU, 0.0), mu(P.rmu.begin(), P.rmu.begin() + P.ndgnh);
  std::vector<int> blk;
  emi::parallel_for(NU, [&](int ml) {
    if (P.mval[ml] < 2) return;
    emi::LegCoef lc = emi::legendre_coefficients(P.mval[ml], nmax);
    std::copy(lc.dcl.begin(), lc.dcl.end(), dcl.begin() + (size_t)ml * (nmax + 1));
    std::copy(lc.ddl.begin(), lc.ddl.end(), ddl.begin() + (size_t)ml * (nmax + 1));
    zf[ml] = lc.zfac_m;
  });
  for (int ml = 0; ml < NU; ml++) {  // m ascending = longest recurrences first
    if (P.mval[ml] < 2) continue;
    const int nd = P.lbase[ml + 1] - P.lbase[ml];
    for (int par = 0; par < 2; par++)
      for (int jt = 0; jt * 64 < nd; jt++) {
        blk.push_back(ml);
        blk.push_back(par << 16 | jt);
      }
  }
  if (blk.empty()) return 0;
  DevAllocs tmp;  // the kernel's inputs live for this stage only
  LegPolDev la{};
  la.ndgnh = P.ndgnh;
  la.nmax = nmax;
  la.nofloor = P.ldll ? 1 : 0;
  if (upload(tmp, dcl, &la.dcl) || upload(tmp, ddl, &la.ddl) || upload(tmp, zf, &la.zfac) || upload(tmp, mu, &la.mu) || upload(tmp, blk, &la.blk)) return EMI_ERR_RUNTIME;
  EmiRange rg_suleg(EMI_LBL_SULEG);  // GSTATS 140
  EMI_LAUNCH_P(P.esz, k_legpol, blk.size() / 2, 64, 0, (emi_stream_t)0, P.g, la);
  emi_stream_sync(0);
  return 0;
}

static int first_free_slot() {
  for (int i = 0; i < G.max_resol; i++)
    if (!G.plans[i]) return i;
  return -1;
}

extern "C" int emi_setup_legpol(const emi_setup_t *cfg, const emi_legpol_io_t *io, int *kresol) {
  EmiRange rg_setup(EMI_LBL_SETUP);  // GSTATS 2
  LegpolMode lp_mode;
  if (int rc = setup_arguments(cfg, io, &lp_mode)) return rc;
  LegpolSource lp_src;
  if ((lp_mode == LP_READF || lp_mode == LP_MEMBUF) && legpol_open(lp_src, io, lp_mode == LP_MEMBUF)) return EMI_ERR_ARG;
  const bool lp_read = lp_src.base != nullptr;
  const int slot = first_free_slot();
  if (slot < 0) EMI_FAIL(EMI_ERR_STATE, "SETUP_TRANS:IDEF_RESOL > NMAX_RESOL");
  std::unique_ptr<Plan> pp(new Plan());  // whatever exit is taken from here on, the plan frees what it has allocated
  Plan &P = *pp;
  P.nsmax = cfg->ksmax;
  P.ldll = cfg->ldll != 0;
  P.shiftll = P.ldll && cfg->ldshiftll != 0;
  P.ndgl = cfg->kdgl + (P.ldll && !P.shiftll ? 2 : 0);  // unshifted LDLL: both poles, and the equator twice (setup_trans.F90:258-271)
  P.ndgnh = (P.ndgl + 1) / 2;
  P.ra = G.ra;
  P.esz = cfg->precision == 4 ? 4 : 8;
  P.nproc = G.nproc;
  P.me = G.myproc - 1;
  P.nprv = G.nprtrv;
  P.mev = G.mysetv - 1;
  if (G.nproc_all > 1 && !G.a2a) EMI_FAIL(EMI_ERR_STATE, "SETUP_TRANS: %d tasks but no all-to-all-v hook registered (emi_set_alltoallv)", G.nproc_all);
  if (P.nproc > P.ndgl / 2 || P.nproc > P.nsmax + 1) EMI_FAIL(EMI_ERR_ARG, "SETUP_TRANS: too many tasks (%d) for NDGL=%d, NSMAX=%d", P.nproc, P.ndgl, P.nsmax);
  int rc;
  std::vector<long long> cum;  // [NDGL + 1] grid points before every latitude
  SetupTables T;
  SetupClock clock;
  if ((rc = setup_geometry(cfg, P, cum))) return rc;
  clock.phase("gaussian latitudes");
  if (lp_read && legpol_index(lp_src, P.nsmax, P.ndgnh, P.nloen, P.nmen, P.ndglu)) return EMI_ERR_ARG;
  if ((rc = setup_distribution(P.nsmax, P.ndgl, P.nloen, cum, P.nproc, P.nprv, P.procm, P.latlo, P.vlat))) return rc;
  setup_local_tables(P, cum, T);
  if ((rc = setup_row_tables(P, P.nproc > 1 || (test_paths() & 1), T))) return rc;
  clock.phase("distribution + index tables");
  const bool belousov = cfg->lduserpnm != 0 && !lp_read;
  const bool legpol_host = lp_read || belousov || (getenv("EMI_LEGPOL_HOST") && atoi(getenv("EMI_LEGPOL_HOST")));
  if ((rc = setup_panels_host(P, lp_read ? &lp_src : nullptr, belousov, legpol_host))) return rc;
  clock.phase("legendre panels (host part)");
  if ((rc = setup_device_tables(P, T))) return rc;
  clock.phase("device tables");
  if (!legpol_host) {
    if ((rc = setup_panels_device(P))) return rc;
    clock.phase("legendre panels (device)");
  }
  rc = build_fft_plans(P);
  clock.phase("fft plans + tables");
  if (rc) return rc;
  emi_stream_sync(0);
  G.plans[slot] = std::move(pp);
  if (kresol) *kresol = slot + 1;
  if (lp_mode == LP_WRITEF) {  // suleg_mod.F90:1186
    rc = legpol_write(slot + 1, io->fname);
    clock.phase("legendre file written");
    if (rc) {
      emi_release(slot + 1);
      return rc;
    }
  }
  return EMI_SUCCESS;
}

extern "C" int emi_setup(const emi_setup_t *cfg, int *kresol) { return emi_setup_legpol(cfg, nullptr, kresol); }

// ------------------------------------------------------------------------------------------
// ESETUP_TRANS (etrans/include/etrans/esetup_trans.h): a limited-area, bi-Fourier handle.  Same stages as SETUP_TRANS without the
// Legendre ones: arguments, geometry (a full grid, NMEN = KMSMAX), distribution (the zig-zag of SUWAVEDI over the x-wavenumbers, as
// suemp_trans_preleg_mod.F90:106-132; whole-row bands), local tables (the ellipse), row tables, device tables, FFT plans of both directions.
// ------------------------------------------------------------------------------------------
static void lam_ellipse(int M, int N, std::vector<int> &kntmp) {  // ellips.F90:71-97, in double
  kntmp.assign(M + 1, 0);
  for (int m = 1; m < M; m++) kntmp[m] = (int)((double)N / (double)M * std::sqrt(std::max(0.0, (double)(M * M - m * m))) + 1.0e-10);
  kntmp[0] = N;
  if (M > 0) kntmp[M] = 0;
}

extern "C" int emi_esetup(const emi_esetup_t *cfg, int *kresol) {
  EmiRange rg_setup(EMI_LBL_SETUP);
  if (!G.init) EMI_FAIL(EMI_ERR_STATE, "ESETUP_TRANS: SETUP_TRANS0 HAS TO BE CALLED BEFORE ESETUP_TRANS");
  if (!cfg) EMI_FAIL(EMI_ERR_ARG, "emi_esetup: null config");
  if (cfg->kdgl < 2) EMI_FAIL(EMI_ERR_ARG, "ESETUP_TRANS: KDGL = %d, AT LEAST 2 ROWS ARE NEEDED", cfg->kdgl);
  for (int j = 1; cfg->kloen && j < cfg->kdgl; j++)
    if (cfg->kloen[j] != cfg->kloen[0])
      EMI_FAIL(EMI_ERR_ARG, "ESETUP_TRANS: KLOEN MUST HOLD ONE ROW LENGTH (KLOEN(%d) = %d, KLOEN(1) = %d)", j + 1, cfg->kloen[j], cfg->kloen[0]);
  const int ndlon = cfg->kloen ? cfg->kloen[0] : cfg->kdlon;
  if (ndlon < 2) EMI_FAIL(EMI_ERR_ARG, "ESETUP_TRANS: KLOEN INVALID (ROW LENGTH %d)", ndlon);
  if (cfg->kmsmax < 0 || cfg->ksmax < 0) EMI_FAIL(EMI_ERR_ARG, "ESETUP_TRANS: KMSMAX = %d, KSMAX = %d", cfg->kmsmax, cfg->ksmax);
  // the spectrum of a row (of a column) ends below its Nyquist wavenumber: C(n) and C(NDGL - n) are different entries
  if (2 * cfg->kmsmax >= ndlon) EMI_FAIL(EMI_ERR_ARG, "ESETUP_TRANS: KMSMAX = %d MUST BE BELOW HALF THE ROW LENGTH %d", cfg->kmsmax, ndlon);
  if (2 * cfg->ksmax >= cfg->kdgl) EMI_FAIL(EMI_ERR_ARG, "ESETUP_TRANS: KSMAX = %d MUST BE BELOW HALF OF KDGL = %d", cfg->ksmax, cfg->kdgl);
  if (cfg->precision != 0 && cfg->precision != 8 && cfg->precision != 4)
    EMI_FAIL(EMI_ERR_ARG, "emi_esetup: precision must be 8 (fp64, the _dp library) or 4 (fp32, _sp), got %d", cfg->precision);
  if (G.nprtrv > 1) EMI_FAIL(EMI_ERR_UNSUPPORTED, "ESETUP_TRANS: NPRTRV = %d: V-SETS ARE NOT AVAILABLE ON A LIMITED-AREA HANDLE", G.nprtrv);
  if (G.nproc > 1 && !G.a2a) EMI_FAIL(EMI_ERR_STATE, "ESETUP_TRANS: %d tasks but no all-to-all-v hook registered (emi_set_alltoallv)", G.nproc);
  const int slot = first_free_slot();
  if (slot < 0) EMI_FAIL(EMI_ERR_STATE, "ESETUP_TRANS:IDEF_RESOL > NMAX_RESOL");
  std::unique_ptr<Plan> pp(new Plan());
  Plan &P = *pp;
  const int M = cfg->kmsmax, N = cfg->ksmax, L = cfg->kdgl, NP = G.nproc;
  P.lam = true;
  P.nsmax = M, P.lam_n = N, P.ndgl = L, P.ndgnh = (L + 1) / 2, P.kdgux = cfg->kdgux;
  P.exwn = cfg->pexwn, P.eywn = cfg->peywn;
  P.ra = G.ra;
  P.esz = cfg->precision == 4 ? 4 : 8;
  P.nproc = NP, P.me = G.myproc - 1, P.nprv = 1, P.mev = 0;
  if (NP > L || NP > M + 1) EMI_FAIL(EMI_ERR_ARG, "ESETUP_TRANS: too many tasks (%d) for KDGL=%d, KMSMAX=%d", NP, L, M);
  // ---- geometry
  P.nloen.assign(L, ndlon);
  P.nmen.assign(L, M);
  P.ndglu.assign(M + 1, L);
  P.rw.assign(L, 1.0 / (double)L);  // with the x-kernels' 1 / NLOEN: forward transforms scaled by 1 / (NDLON NDGL)
  P.racthe.assign(L, P.exwn);       // GM_EWDER of the x-kernels: i m EXWN (efsc_mod.F90)
  P.cos2.assign(L, 1.0);
  std::vector<long long> cum(L + 1, 0);
  for (int j = 0; j < L; j++) cum[j + 1] = cum[j] + ndlon;
  if (cum[L] > 2000000000LL) EMI_FAIL(EMI_ERR_UNSUPPORTED, "grid too large for 32-bit point offsets");
  P.ngptotg = (int)cum[L];
  lam_ellipse(M, N, P.kntmp);
  P.nspec2g = 0;
  for (int m = 0; m <= M; m++) P.nspec2g += 4 * (P.kntmp[m] + 1);
  // ---- distribution: the zig-zag over m; bands of whole rows, the first mod(NDGL, NPRTRW) of them one row longer (what
  // suemp_trans_preleg_mod.F90:187-197 sets out to do)
  int rc;
  if ((rc = setup_distribution(M, L, P.nloen, cum, NP, 1, P.procm, P.latlo, P.vlat))) return rc;
  for (int r = 0; r <= NP; r++) P.latlo[r] = r * (L / NP) + std::min(r, L % NP);
  // ---- this task's share
  SetupTables T;
  P.lat0 = P.latlo[P.me];
  P.nlat = P.latlo[P.me + 1] - P.lat0;
  P.ngptot = (int)(cum[P.latlo[P.me + 1]] - cum[P.lat0]);
  for (int m = 0; m <= M; m++)
    if (P.procm[m] == P.me) P.mval.push_back(m);
  P.nump = (int)P.mval.size();
  const int NU = P.nump, NL = P.nlat;
  int ipos = 0;
  for (int ml = 0; ml < NU; ml++) {
    P.l_kntmp.push_back(P.kntmp[P.mval[ml]]);
    P.nesm0.push_back(ipos);
    ipos += 4 * (P.kntmp[P.mval[ml]] + 1);
  }
  P.nspec2 = ipos;
  {  // NPME(0) = 1, NPME(m) = NPME(m - 1) + KNTMP(m - 1) + 1 (suemp_trans_preleg_mod.F90:75-86)
    std::vector<int> npme(M + 1, 1);
    for (int m = 1; m <= M; m++) npme[m] = npme[m - 1] + P.kntmp[m - 1] + 1;
    for (int ml = 0; ml < NU; ml++) P.l_npme.push_back(npme[P.mval[ml]]);
  }
  P.lbase.assign(NU + 1, 0);  // no hemispheres: the row tables of the y-side are lamdev.rowbase
  P.l_nmen.assign(NL, M);
  P.l_gpoff.assign(NL, 0);
  P.l_fbase.assign(NL + 1, 0);
  T.l_rw.assign(NL, 1.0 / (double)L);
  T.l_racthe.assign(NL, P.exwn);
  for (int jl = 0; jl < NL; jl++) {
    P.l_gpoff[jl] = jl * ndlon;
    P.l_fbase[jl + 1] = P.l_fbase[jl] + M + 1;
  }
  P.frows = P.l_fbase[NL];
  P.lrows = (long long)NU * L;
  P.wrows_total = 0;
  const bool exchange_order = NP > 1 || (test_paths() & 1);
  if ((rc = setup_row_tables(P, exchange_order, T))) return rc;
  std::vector<int> rowbase(L, 0);
  if (exchange_order) {  // block d of the y-side buffer: the rows (row of band d, local wavenumber), row-major -- the order of setup_row_tables
    for (int d = 0; d < NP; d++)
      for (int j = P.latlo[d]; j < P.latlo[d + 1]; j++) rowbase[j] = (int)P.leg_disp[d] + (j - P.latlo[d]) * NU;
  } else {
    for (int j = 0; j < L; j++) rowbase[j] = j * (M + 1);
  }
  // ---- device tables
  EmiGeomDev &g = P.g;
  g.nsmax = M, g.nump = NU, g.nlat = NL, g.ngptot = P.ngptot;
  LamDev &ld = P.lamdev;
  ld.ndgl = L, ld.exwn = P.exwn, ld.eywn = P.eywn;
  if (upload(P.dev_allocs, P.mval, &g.mval) || upload(P.dev_allocs, P.l_nmen, &g.nmen) || upload(P.dev_allocs, P.l_gpoff, &g.gpoff) ||
      upload(P.dev_allocs, P.l_fbase, &g.fbase) || upload(P.dev_allocs, T.fftrow, &g.fftrow) || upload(P.dev_allocs, T.l_rw, &g.rw) ||
      upload(P.dev_allocs, T.l_racthe, &g.racthe) || upload(P.dev_allocs, P.l_kntmp, &ld.kntmp) || upload(P.dev_allocs, P.nesm0, &ld.nesm0) ||
      upload(P.dev_allocs, rowbase, &ld.rowbase) || upload(P.dev_allocs, P.l_npme, &P.d_npme))
    return EMI_ERR_RUNTIME;
  if (!T.rowtable) g.fftrow = nullptr;
  if ((rc = build_fft_plans(P))) return rc;
  emi_stream_sync(0);
  G.plans[slot] = std::move(pp);
  if (kresol) *kresol = slot + 1;
  return EMI_SUCCESS;
}

extern "C" int emi_set_alltoallv(emi_alltoallv_fn fn, void *user) {
  G.a2a = fn;
  G.a2a_user = user;
  return EMI_SUCCESS;
}

extern "C" int emi_release(int kresol) {
  Plan *P = get_plan(kresol);
  if (!P) EMI_FAIL(EMI_ERR_STATE, "TRANS_RELEASE: unknown resolution %d", kresol);
  plan_quiesce(*P);
  emi_stream_sync(0);
  G.plans[kresol - 1].reset();
  emi_stage::trim();  // the idle staging buffers of host-array calls were sized for this resolution
  return EMI_SUCCESS;
}

// Frees the idle device staging buffers kept between host-array calls (several GiB after a large call; other allocators of
// the process -- torch, the host model -- cannot see or reclaim them).  Waits for the work queued on the null stream first:
// a buffer is idle once its call has returned, but that call's last copies may still be in flight.
extern "C" int emi_trim_cache(void) {
  emi_stream_sync(0);
  emi_stage::trim();
  return EMI_SUCCESS;
}

extern "C" int emi_finalize(void) {
  if (!G.init) return EMI_SUCCESS;
  for (int i = 0; i < (int)G.plans.size(); i++)
    if (G.plans[i]) emi_release(i + 1);
  G.plans.clear();
  emi_stage::trim();
  G.init = false;
  return EMI_SUCCESS;
}

// ------------------------------------------------------------------------------------------
// TRANS_INQ
// ------------------------------------------------------------------------------------------
extern "C" int emi_inq_int(int kresol, const char *name, int *value) {
  Plan *P = get_plan(kresol);
  if (!P) EMI_FAIL(EMI_ERR_STATE, "TRANS_INQ: unknown resolution %d", kresol);
  std::string s(name ? name : "");
  if (s == "nspec2")
    *value = P->nspec2;
  else if (s == "nspec2g")
    *value = P->nspec2g;
  else if (s == "nspec2mx") {
    int mx = 0;
    std::vector<int> cnt(P->nproc, 0);
    for (int m = 0; m <= P->nsmax; m++) cnt[P->procm[m]] += P->lam ? 4 * (P->kntmp[m] + 1) : 2 * (P->nsmax - m + 1);
    for (int c : cnt) mx = std::max(mx, c);
    *value = mx;
  } else if (s == "nspec")  // (D%NSPEC = D%NSPEC2 on a limited-area handle, suemp_trans_preleg_mod.F90:146)
    *value = P->lam ? P->nspec2 : P->nspec2 / 2;
  else if (s == "nspecg")
    *value = P->lam ? P->nspec2g : P->nspec2g / 2;
  else if (s == "ngptot")  // this task's grid points: its sub-band with V-sets, else its band
    *value = P->nprv > 1 ? (int)P->vpoints(P->me, P->mev) : P->ngptot;
  else if (s == "ngptot_band")  // grid points of the whole band of this task's W-set (the FFT work of its V-set)
    *value = P->ngptot;
  else if (s == "ngptotg")
    *value = P->ngptotg;
  else if (s == "ngptotmx") {
    long long mx = 0;
    for (int r = 0; r < P->nproc; r++)
      for (int v = 0; v < P->nprv; v++) mx = std::max(mx, P->vpoints(r, v));
    *value = (int)mx;
  } else if (s == "nump")
    *value = P->nump;
  else if (s == "ndgl")
    *value = P->ndgl;
  else if (s == "nsmax")  // KSMAX: on a limited-area handle the truncation in y ("nmsmax": in x)
    *value = P->lam ? P->lam_n : P->nsmax;
  else if (s == "nmsmax")
    *value = P->nsmax;
  else if (s == "ldlam")
    *value = P->lam ? 1 : 0;
  else if (s == "ndgux") {
    if (!P->lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "ETRANS_INQ: %s: resolution %d is not a limited-area handle (ESETUP_TRANS)", s.c_str(), kresol);
    *value = P->kdgux;
  } else if (s == "ldll")
    *value = P->ldll ? 1 : 0;
  else if (s == "lshiftll" || s == "ldshiftll")
    *value = P->shiftll ? 1 : 0;
  else if (s == "ndlon")
    *value = *std::max_element(P->nloen.begin(), P->nloen.end());
  else if (s == "nproc")
    *value = P->nproc * P->nprv;
  else if (s == "nprtrw")
    *value = P->nproc;
  else if (s == "nprtrv")
    *value = P->nprv;
  else if (s == "myproc")
    *value = P->me * P->nprv + P->mev + 1;
  else if (s == "mysetw")
    *value = P->me + 1;
  else if (s == "mysetv")
    *value = P->mev + 1;
  else if (s == "nfrstlat")  // first (1-based, global) latitude of this task's grid share (its band; its sub-band with V-sets)
    *value = P->vfirst(P->me, P->mev) + 1;
  else if (s == "nlstlat")
    *value = P->vlast(P->me, P->mev);
  else
    EMI_FAIL(EMI_ERR_ARG, "emi_inq_int: unknown name '%s'", s.c_str());
  return EMI_SUCCESS;
}

extern "C" int emi_inq_int_array(int kresol, const char *name, int *out, int len) {
  Plan *P = get_plan(kresol);
  if (!P) EMI_FAIL(EMI_ERR_STATE, "TRANS_INQ: unknown resolution %d", kresol);
  std::string s(name ? name : "");
  const std::vector<int> *v = nullptr;
  std::vector<int> tmp;
  const bool lam_name = s == "kntmp" || s == "nesm0" || s == "ncpl2m" || s == "ncpl4m" || s == "npme" || s == "numpp" || s == "npossp" || s == "nallms" ||
                        s == "nptrms" || s == "ndim0g";
  if (lam_name && !P->lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "ETRANS_INQ: %s: resolution %d is not a limited-area handle (ESETUP_TRANS)", s.c_str(), kresol);
  if (P->lam && (s == "ndglu" || s == "nasm0"))
    EMI_FAIL(EMI_ERR_UNSUPPORTED, "TRANS_INQ: %s: resolution %d is a limited-area handle (ESETUP_TRANS): it has no Legendre transform", s.c_str(), kresol);
  if (lam_name) {
    // the tables of suemp_trans_preleg_mod.F90:76-177 over the x-wavenumbers 0 .. KMSMAX; positions 1-based as there
    const int M = P->nsmax, NP = P->nproc;
    std::vector<int> numpp(NP, 0), ispec(NP, 0), nptrms(NP, 1);
    for (int m = 0; m <= M; m++) numpp[P->procm[m]]++, ispec[P->procm[m]] += P->kntmp[m] + 1;
    for (int a = 1; a < NP; a++) nptrms[a] = nptrms[a - 1] + numpp[a - 1];
    std::vector<int> nallms(M + 1, 0), ic(NP, 0);
    for (int m = 0; m <= M; m++) nallms[ic[P->procm[m]]++ + nptrms[P->procm[m]] - 1] = m;
    if (s == "kntmp")
      tmp = P->kntmp;
    else if (s == "ncpl2m" || s == "ncpl4m") {
      tmp.resize(M + 1);
      for (int m = 0; m <= M; m++) tmp[m] = (s == "ncpl2m" ? 2 : 4) * (P->kntmp[m] + 1);
    } else if (s == "npme") {
      tmp.assign(M + 1, 1);
      for (int m = 1; m <= M; m++) tmp[m] = tmp[m - 1] + P->kntmp[m - 1] + 1;
    } else if (s == "nesm0") {  // -99 for the wavenumbers of other tasks
      tmp.assign(M + 1, -99);
      for (int ml = 0; ml < P->nump; ml++) tmp[P->mval[ml]] = P->nesm0[ml] + 1;
    } else if (s == "numpp")
      tmp = numpp;
    else if (s == "npossp") {
      tmp.assign(NP + 1, 1);
      for (int a = 1; a <= NP; a++) tmp[a] = tmp[a - 1] + 4 * ispec[a - 1];
    } else if (s == "nallms")
      tmp = nallms;
    else if (s == "nptrms")
      tmp = nptrms;
    else {  // ndim0g
      tmp.assign(M + 1, 0);
      int ipos = 1;
      for (int m : nallms) tmp[m] = ipos, ipos += 4 * (P->kntmp[m] + 1);
    }
    v = &tmp;
  } else if (s == "nloen")
    v = &P->nloen;
  else if (s == "nmen" || s == "nmeng")
    v = &P->nmen;
  else if (s == "ndglu")
    v = &P->ndglu;
  else if (s == "nasm0") {  // D%NASM0(0:NSMAX): 1-based address of (m, n=m), -99 for foreign m
    tmp.assign(P->nsmax + 1, -99);
    for (int ml = 0; ml < P->nump; ml++) tmp[P->mval[ml]] = P->nasm0[ml] + 1;
    v = &tmp;
  } else if (s == "myms")
    v = &P->mval;
  else if (s == "procm") {  // D%NPROCM: owning W-set (1-based) of every wavenumber
    tmp = P->procm;
    for (auto &x : tmp) x += 1;
    v = &tmp;
  } else if (s == "latlo") {  // [nproc+1] 0-based first latitude of every task's grid share, task order
    if (P->nprv > 1)
      v = &P->vlat;
    else
      v = &P->latlo;
  } else if (s == "fftwork") {  // [ndgl] work length of the FFT of every latitude of this task (0 elsewhere): NLOEN/2 or NLOEN,
    // or the Bluestein length; diagnostic (tests check which specialised kernel a row length selects)
    tmp.assign(P->ndgl, 0);
    for (int j = 0; j < P->nlat; j++) tmp[P->lat0 + j] = P->fplans[P->planid[j]].S;
    v = &tmp;
  } else if (s == "fftplan") {  // [ndgl][5] what runs the FFT of every latitude of this task (0 elsewhere); diagnostic (tests check
    // which plan a row length selects): kernel family -- 0 generic in-LDS, 1 specialised in-LDS (k_fft_*_hot), 2 register-resident
    // (k_fft_*_r16), 3 split (k_fft_*_r16p), 4 direct mixed radix (k_fft_*_mr), 5 generic on global scratch (k_fft_*_gm) --, the
    // mixed-radix factors A, B, C (1 where absent; 0 for the other families), fields per workgroup
    tmp.assign((size_t)P->ndgl * 5, 0);
    for (int j = 0; j < P->nlat; j++) {
      const FftPlanDev &pl = P->fplans[P->planid[j]];
      const FftClass &fc = P->fclass[pl.lds_class];
      int *o = &tmp[(size_t)(P->lat0 + j) * 5];
      o[0] = fc.mr ? 4 : fc.split ? 3 : fc.r16 ? 2 : fc.gmem ? 5 : fc.hot ? 1 : 0;
      if (fc.mr) o[1] = pl.fac[0], o[2] = pl.fac[1], o[3] = pl.fac[2];
      o[4] = pl.fbk;
    }
    v = &tmp;
  } else if (s == "fftfac") {  // [ndgl][15] the factor list of the FFT of every latitude of this task (0 elsewhere): the pass count, then
    // the factors in pass order (the register-resident and split kernels: R1 alone, their 16, 16 are compile-time); diagnostic (tests
    // check which radix lands in which pass of the generic kernels, which walk this list at run time)
    tmp.assign((size_t)P->ndgl * 15, 0);
    for (int j = 0; j < P->nlat; j++) {
      const FftPlanDev &pl = P->fplans[P->planid[j]];
      int *o = &tmp[(size_t)(P->lat0 + j) * 15];
      o[0] = pl.nfac;
      for (int i = 0; i < pl.nfac; i++) o[1 + i] = pl.fac[i];
    }
    v = &tmp;
  } else
    EMI_FAIL(EMI_ERR_ARG, "emi_inq_int_array: unknown name '%s'", s.c_str());
  if (len < (int)v->size()) EMI_FAIL(EMI_ERR_ARG, "TRANS_INQ: %s TOO SMALL (%d < %zu)", s.c_str(), len, v->size());
  std::copy(v->begin(), v->end(), out);
  return EMI_SUCCESS;
}

extern "C" int emi_inq_real_array(int kresol, const char *name, double *out, int len) {
  Plan *P = get_plan(kresol);
  if (!P) EMI_FAIL(EMI_ERR_STATE, "TRANS_INQ: unknown resolution %d", kresol);
  std::string s(name ? name : "");
  const std::vector<double> *v = nullptr;
  std::vector<double> tmp;
  if (P->lam && s != "rlepinm" && s != "plepinm")
    EMI_FAIL(EMI_ERR_UNSUPPORTED, "TRANS_INQ: %s: resolution %d is a limited-area handle (ESETUP_TRANS): it has no Gaussian latitudes, weights or Laplacian table", s.c_str(), kresol);
  if (s == "rlepinm" || s == "plepinm") {
    // FALD%RLEPINM (suemp_trans_preleg_mod.F90:86-100): 1 / -((m EXWN)^2 + (n EYWN)^2) at NPME(m) + n, 0 for (0, 0)
    if (!P->lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "ETRANS_INQ: %s: resolution %d is not a limited-area handle (ESETUP_TRANS)", s.c_str(), kresol);
    for (int m = 0; m <= P->nsmax; m++)
      for (int n = 0; n <= P->kntmp[m]; n++) {
        const double l = -((double)m * m * P->exwn * P->exwn + (double)n * n * P->eywn * P->eywn);
        tmp.push_back(l != 0.0 ? 1.0 / l : 0.0);
      }
    v = &tmp;
  } else if (s == "rmu" || s == "pmu")
    v = &P->rmu;
  else if (s == "rgw" || s == "pgw" || s == "rw") {
    if (P->ldll) EMI_FAIL(EMI_ERR_UNSUPPORTED, "TRANS_INQ: %s: a handle set up with LDLL keeps no Gaussian weights", s.c_str());
    v = &P->rw;
  }
  else if (s == "racthe")
    v = &P->racthe;
  else if (s == "rlapin" || s == "plapin") {
    // RLAPIN(-1:NSMAX+2) (pre_suleg_mod.F90:64-69): eigenvalues of the inverse Laplacian, -a^2/(n(n+1)); 0 for n <= 0
    if (len < P->nsmax + 4) EMI_FAIL(EMI_ERR_ARG, "TRANS_INQ: PLAPIN TOO SMALL");
    out[0] = out[1] = 0.0;
    for (int n = 1; n <= P->nsmax + 2; n++) out[n + 1] = -(P->ra * P->ra / (double)(n * (n + 1)));
    return EMI_SUCCESS;
  } else
    EMI_FAIL(EMI_ERR_ARG, "emi_inq_real_array: unknown name '%s'", s.c_str());
  if (len < (int)v->size()) EMI_FAIL(EMI_ERR_ARG, "TRANS_INQ: %s TOO SMALL", s.c_str());
  std::copy(v->begin(), v->end(), out);
  return EMI_SUCCESS;
}

extern "C" int emi_inq_legendre(int kresol, int m, int symmetric, double *out, int *nrows, int *ncols) {
  Plan *P = get_plan(kresol);
  if (!P) EMI_FAIL(EMI_ERR_STATE, "TRANS_INQ: unknown resolution %d", kresol);
  if (P->lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "TRANS_INQ: emi_inq_legendre: resolution %d is a limited-area handle (ESETUP_TRANS): it has no Legendre polynomials", kresol);
  if (m < 0 || m > P->nsmax) EMI_FAIL(EMI_ERR_ARG, "emi_inq_legendre: m out of range");
  if (P->procm[m] != P->me) EMI_FAIL(EMI_ERR_ARG, "emi_inq_legendre: wavenumber %d belongs to task %d", m, P->procm[m] + 1);
  const int ml = (int)(std::lower_bound(P->mval.begin(), P->mval.end(), m) - P->mval.begin());
  const int N = P->nsmax, nd = std::min(P->ndgnh, P->ndglu[m]);
  const int nc = symmetric ? (N - m + 3) / 2 : (N - m + 2) / 2;
  if (nrows) *nrows = nd;
  if (ncols) *ncols = nc;
  if (!out) return EMI_SUCCESS;
  const int ld = P->ldp[ml], nk = P->wrows[ml] / 2;
  std::vector<double> pan((size_t)nk * ld);
  const char *src = P->d_P + (symmetric ? P->offS[ml] : P->offA[ml]) * P->esz;
  if (P->esz == 8) {
    if (emi_d2h(pan.data(), src, pan.size() * 8, 0)) return EMI_ERR_RUNTIME;
    emi_stream_sync(0);
  } else {
    std::vector<float> pf(pan.size());
    if (emi_d2h(pf.data(), src, pf.size() * 4, 0)) return EMI_ERR_RUNTIME;
    emi_stream_sync(0);
    for (size_t i = 0; i < pf.size(); i++) pan[i] = pf[i];
  }
  // reference column c (0-based) holds n descending: k = nc-1-c
  for (int c = 0; c < nc; c++)
    for (int j = 0; j < nd; j++) out[(size_t)c * nd + j] = pan[(size_t)(nc - 1 - c) * ld + j];
  return EMI_SUCCESS;
}

// WRITE_LEGPOL (write_legpol_mod.F90:66-158): the panels as emi_inq_legendre returns them, in MYMS order
static int legpol_write(int kresol, const char *fname) {
  Plan *P = get_plan(kresol);
  if (!P) EMI_FAIL(EMI_ERR_STATE, "WRITE_LEGPOL: unknown resolution %d", kresol);
  if (P->lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "WRITE_LEGPOL: resolution %d is a limited-area handle (ESETUP_TRANS): it has no Legendre polynomials", kresol);
  FILE *f = fopen(fname, "wb");
  if (!f) EMI_FAIL(EMI_ERR_ARG, "WRITE_LEGPOL: BYTES_IO_OPEN FAILED (%s)", fname);
  int head[4];
  memcpy(head, "LEGPOL  ", 8);
  head[2] = P->nsmax;
  head[3] = P->ndgnh;
  bool ok = fwrite(head, 4, 4, f) == 4;
  std::vector<int> lat(2 * (size_t)P->ndgnh);
  for (int j = 0; j < P->ndgnh; j++) {
    lat[2 * j] = P->nloen[j];
    lat[2 * j + 1] = P->nmen[j];
  }
  ok = ok && fwrite(lat.data(), 4, lat.size(), f) == lat.size();
  std::vector<double> buf;
  for (int m = 0; ok && m <= P->nsmax; m++)
    for (int sym = 0; ok && sym < 2; sym++) {  // anti-symmetric first
      int nr = 0, nc = 0;
      if (emi_inq_legendre(kresol, m, sym, nullptr, &nr, &nc)) {
        fclose(f);
        return EMI_ERR_RUNTIME;
      }
      buf.resize((size_t)nr * nc);
      if (emi_inq_legendre(kresol, m, sym, buf.data(), &nr, &nc)) {
        fclose(f);
        return EMI_ERR_RUNTIME;
      }
      ok = fwrite(buf.data(), 8, buf.size(), f) == buf.size();
    }
  ok = (fclose(f) == 0) && ok;
  if (!ok) EMI_FAIL(EMI_ERR_RUNTIME, "WRITE_LEGPOL:BYTES_IO_WRITE FAILED (%s)", fname);
  return EMI_SUCCESS;
}

// ------------------------------------------------------------------------------------------
// transforms
// ------------------------------------------------------------------------------------------
struct HostStage {  // staging of host arrays through device memory (mem_space == HOST): emi_stage.h
  size_t esz;
  explicit HostStage(int e) : esz((size_t)e) {}
  std::vector<void *> dev;
  bool failed = false;  // a staging buffer could not be allocated or filled: the call must not launch anything
  std::vector<std::pair<void *, std::pair<void *, size_t>>> outs;  // dev -> (host, bytes)
  ~HostStage() {
    for (void *p : dev) emi_stage::release(p);
  }
  const void *in(const void *h, size_t elems, bool host, emi_stream_t s) {
    if (!h || !host) return h;
    void *d = emi_stage::acquire(elems * esz);
    if (!d) {
      failed = true;
      return nullptr;
    }
    dev.push_back(d);
    if (emi_h2d(d, h, elems * esz, s)) failed = true;
    return d;
  }
  // preload: the call does not write every element of the array (padding of the last NPROMA block, more
  // fields in the array than the call produces) -- start from the caller's contents so that the copy back
  // leaves those elements as they were, as the reference does
  void *out(void *h, size_t elems, bool host, bool preload = false, emi_stream_t s = 0) {
    if (!h || !host) return h;
    void *d = emi_stage::acquire(elems * esz);
    if (!d) {
      failed = true;
      return nullptr;
    }
    dev.push_back(d);
    if (preload && emi_h2d(d, h, elems * esz, s)) failed = true;
    outs.push_back({d, {h, elems * esz}});
    return d;
  }
  void flush(emi_stream_t s) {
    for (auto &o : outs) emi_d2h(o.second.first, o.first, o.second.second, s);
    emi_stream_sync(s);
  }
};

static int grow(Plan &P, char **p, size_t *cap, size_t need, const char *what, emi_stream_t st) {
  if (need <= *cap) return 0;
  plan_quiesce(P);  // kernels of the previous call (on whatever stream it named) may still use the old buffer
  emi_stream_sync(0);
  emi_dev_free(*p);
  *p = nullptr;
  *cap = 0;
  void *q;
  if (emi_dev_malloc(&q, need)) EMI_FAIL(EMI_ERR_RUNTIME, "cannot allocate %.2f GiB %s", need / 1073741824.0, what);
  *p = (char *)q;
  *cap = need;
  emi_dev_memset(q, 0, need, st);  // on the caller's stream: ordered ahead of this call's kernels
  return 0;
}

static int ensure_work(Plan &P, int bfpad, int nfb, emi_stream_t st) {
  const size_t rowb = (size_t)2 * bfpad * P.esz;
  if (grow(P, &P.d_W, &P.cap_W, (size_t)P.wrows_total * rowb, "packed-spectral work buffer", st)) return -1;
  if (P.nproc == 1) {
    // + 1 per buffer: a row of zeros behind the Fourier rows (k_leg_dir reads it for latitudes past the last one of a stage)
    if (grow(P, &P.d_FBL, &P.cap_FBL, (size_t)nfb * (P.frows + 1) * rowb, "Fourier work buffer", st)) return -1;
    P.d_FBF = P.d_FBL;
    P.cap_FBF = P.cap_FBL;
  } else {
    if (grow(P, &P.d_FBL, &P.cap_FBL, (size_t)nfb * (P.lrows + 1) * rowb, "Fourier (Legendre-side) exchange buffer", st)) return -1;
    if (grow(P, &P.d_FBF, &P.cap_FBF, (size_t)nfb * P.frows * rowb, "Fourier (FFT-side) exchange buffer", st)) return -1;
  }
  return 0;
}

// Per-phase device timing with HIP event pairs recorded on the stream each kernel runs on.
// Nothing is synchronised inside a transform call; emi_last_phase_ms() resolves the events lazily.
struct PhaseTimer {
  static const int MAXIV = 4096;
  int n = 0, ncreated = 0;
  bool on = false;
  int kinds[MAXIV];        // 0 spectral pack / unpack, 1 Legendre, 2 FFT, 3 exchange (the all-to-all-v hook, on the stream it is queued on)
  double xbytes = 0;       // bytes this task handed to the exchange hook since the measurement started (send side, peers only)
  long long fft_kernels = 0;  // kernel launches of the FFT phases since the measurement started (launch_fft)
#ifndef EMI_CPU_EMU
  hipEvent_t e0[MAXIV], e1[MAXIV];
  // keep: the intervals of earlier calls stay (accumulating mode, emi_set_profile(2)): nothing has to be resolved --
  // i.e. no host synchronisation -- between the calls of a timed loop
  void begin(bool on_, bool keep = false) {
    on = on_;
    if (!keep) n = 0, xbytes = 0, fft_kernels = 0;
  }
  int start(int kind, emi_stream_t s) {
    if (!on || n >= MAXIV) return -1;
    if (n >= ncreated) {  // events are created as the intervals are first used
      (void)hipEventCreate(&e0[n]);
      (void)hipEventCreate(&e1[n]);
      ncreated = n + 1;
    }
    kinds[n] = kind;
    (void)hipEventRecord(e0[n], s);
    return n++;
  }
  void stop(int iv, emi_stream_t s) {
    if (iv >= 0) (void)hipEventRecord(e1[iv], s);
  }
  void resolve(double *ms3, int *launches) {  // four entries each
    for (int i = 0; i < 4; i++) ms3[i] = 0, launches[i] = 0;
    if (!on) return;
    for (int i = 0; i < n; i++) {
      (void)hipEventSynchronize(e1[i]);
      float ms = 0;
      (void)hipEventElapsedTime(&ms, e0[i], e1[i]);
      ms3[kinds[i]] += ms;
      launches[kinds[i]]++;
    }
  }
#else
  void begin(bool on_, bool keep = false) {  // (no events: the bytes handed to the exchange hook are still counted)
    on = on_;
    if (!keep) xbytes = 0, fft_kernels = 0;
  }
  int start(int, emi_stream_t) { return -1; }
  void stop(int, emi_stream_t) {}
  void resolve(double *ms3, int *launches) {
    for (int i = 0; i < 4; i++) ms3[i] = 0, launches[i] = 0;
  }
#endif
};
static PhaseTimer g_pt;

// TRLTOM / TRMTOL (trltom_mod.F90:96-136, trmtol_mod.F90:101-141): one all-to-all-v of whole
// row blocks of the Fourier buffers.  to_fft: Legendre-side -> FFT-side (inverse transform).
// The hook always sees ALL tasks of the job (one entry per task, zero bytes for tasks that are not peers of this exchange): with
// V-sets TRMTOL / TRLTOM run among the NPRTRW tasks that share this task's V-set (task w * NPRTRV + mysetv), TRLTOG / TRGTOL
// among the NPRTRV tasks of its W-set -- no sub-communicators, any transport that handles empty blocks works unchanged.
// Displacements of the empty blocks continue the dense order (the Python transport checks it).
static int hook_alltoallv(const void *sb, const std::vector<long long> &psc, void *rb, const std::vector<long long> &prc, int npeers, int stride, int first,
                          emi_stream_t st) {
  const int NA = G.nproc_all;
  std::vector<long long> sc(NA, 0), sd(NA, 0), rc(NA, 0), rd(NA, 0);
  for (int k = 0; k < npeers; k++) sc[first + k * stride] = psc[k], rc[first + k * stride] = prc[k];
  for (int r = 1; r < NA; r++) sd[r] = sd[r - 1] + sc[r - 1], rd[r] = rd[r - 1] + rc[r - 1];
  const int iv = g_pt.start(3, st);
  for (int r = 0; r < NA; r++)
    if (g_pt.on && r != G.myproc_all - 1) g_pt.xbytes += (double)sc[r];
  const int rc_hook = G.a2a(G.a2a_user, sb, sc.data(), sd.data(), rb, rc.data(), rd.data(), NA, (void *)st);
  g_pt.stop(iv, st);
  if (rc_hook != 0) EMI_FAIL(EMI_ERR_RUNTIME, "all-to-all-v hook failed");
  return 0;
}
static int exchange(Plan &P, bool to_fft, int ldf, emi_stream_t st, char *FBl, char *FBf) {
  if (P.nproc == 1) return 0;
  const int NP = P.nproc;
  std::vector<long long> sc(NP), rc(NP);
  const long long rowb = (long long)ldf * P.esz;
  for (int r = 0; r < NP; r++) {
    // the blocks of both buffers are dense and in task order (leg_disp / fft_disp are the running sums of the rows)
    const long long lr = P.leg_rows[r] * rowb, fr = P.fft_rows[r] * rowb;
    sc[r] = to_fft ? lr : fr;
    rc[r] = to_fft ? fr : lr;
  }
  const void *sb = to_fft ? FBl : FBf;
  void *rb = to_fft ? FBf : FBl;
  return hook_alltoallv(sb, sc, rb, rc, NP, P.nprv, P.mev, st);
}

static int ensure_desc(Plan &P, size_t bytes);
// The field descriptors of a call go to the device through a small ring of pinned host buffers, so that the copy is
// asynchronous and the call never waits for the stream: the host prepares and queues the next call while the
// kernels of this one run (0.6 ms of host work per pair, otherwise exposed between any two calls).  A ring slot is
// reused four calls later, after the event behind its copy.  The device buffer is one per resolution: the copy of
// the next call is ordered behind this call's kernels on the caller's stream.
static int upload_desc(Plan &P, const std::vector<char> &hd, emi_stream_t st) {
  if (ensure_desc(P, hd.size())) return EMI_ERR_RUNTIME;
#ifdef EMI_CPU_EMU
  emi_h2d(P.d_desc, hd.data(), hd.size(), st);
  return 0;
#else
  static struct {
    void *h[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t cap[4] = {0, 0, 0, 0};
    hipEvent_t ev[4];
    bool init[4] = {false, false, false, false};
    unsigned next = 0;
  } ring;
  const int k = (int)(ring.next++ & 3u);
  if (ring.init[k]) {
    EMI_CHECK(hipEventSynchronize(ring.ev[k]));
  } else {
    EMI_CHECK(hipEventCreateWithFlags(&ring.ev[k], hipEventDisableTiming));
    ring.init[k] = true;
  }
  if (ring.cap[k] < hd.size()) {
    if (ring.h[k]) (void)hipHostFree(ring.h[k]);
    ring.h[k] = nullptr;
    ring.cap[k] = 0;
    const size_t cap = std::max(hd.size(), (size_t)1 << 16);
    EMI_CHECK(hipHostMalloc(&ring.h[k], cap, hipHostMallocDefault));
    ring.cap[k] = cap;
  }
  memcpy(ring.h[k], hd.data(), hd.size());
  EMI_CHECK(hipMemcpyAsync(P.d_desc, ring.h[k], hd.size(), hipMemcpyHostToDevice, (hipStream_t)st));
  EMI_CHECK(hipEventRecord(ring.ev[k], (hipStream_t)st));
  return 0;
#endif
}

static int ensure_desc(Plan &P, size_t bytes) {
  if (bytes <= P.cap_desc) return 0;
  plan_quiesce(P);
  emi_stream_sync(0);
  emi_dev_free(P.d_desc);
  P.d_desc = nullptr;
  size_t cap = std::max(bytes, (size_t)1 << 16);
  if (emi_dev_malloc(&P.d_desc, cap)) return EMI_ERR_RUNTIME;
  P.cap_desc = cap;
  return 0;
}

// All eight XCDs share every wavenumber: an XCD takes a range of column tiles (and a residue class of row tiles when there are fewer
// column tiles than XCDs), column tiles innermost, so that consecutive tiles of an XCD share the panel rows.  (Measured and rejected,
// wavenumber groups of 4 / 2 / 1 XCDs -- fetched bytes go up, time never down; row tiles innermost -- 10 % fewer
// bytes for k_leg_dir and 1.4 % more time.)
// which: 0 every wavenumber, 1 all but the wide one (fp32 library: m = 0 accumulates in double and has a kernel of its own), 2 only that one
static int build_tilemap(Plan &P, const std::vector<int> &pref, int nct, int2 **d_map, long long *nblocks, int which = 0) {
  const int nx = 8;  // XCDs
  int gx = 1;
  while (gx * 2 <= std::min(nct, nx)) gx *= 2;
  const int gy = nx / gx;
  std::vector<std::vector<int2>> per(8);
  for (int ml = 0; ml < P.nump; ml++) {
    const bool wide = P.esz == 4 && P.mval[ml] == 0;
    if ((which == 1 && wide) || (which == 2 && !wide)) continue;
    const int nrt = pref[ml + 1] - pref[ml];
    for (int x = 0; x < nx; x++) {
      // rotate the column ranges and row residues with the wavenumber: the ranges differ by one tile, rotation
      // evens the per-XCD totals out (a fixed assignment leaves XCDs with 4 of 26 column tiles 23 %
      // more work than those with 3)
      const int xc = (x + ml) % gx, xl = (x / gx + ml) % gy;
      const int c0 = (int)((long long)xc * nct / gx), c1 = (int)((long long)(xc + 1) * nct / gx);
      for (int rt = xl; rt < nrt; rt += gy)
        for (int ct = c0; ct < c1; ct++) per[x].push_back(int2{ml, (rt << 16) | ct});
    }
  }
  size_t mx = 0;
  for (auto &v : per) mx = std::max(mx, v.size());
  std::vector<int2> map(mx * 8, int2{-1, 0});
  for (int x = 0; x < 8; x++)
    for (size_t k = 0; k < per[x].size(); k++) map[k * 8 + x] = per[x][k];
  *nblocks = (long long)map.size();
  if (map.empty()) {  // (which == 2 on a task that does not own m = 0)
    *d_map = nullptr;
    return 0;
  }
  return upload(P.dev_allocs, map, d_map);
}

static int leg_tilemaps(Plan &P, int nct, LegMaps **out) {
  auto it = P.legmaps.find(nct);
  if (it == P.legmaps.end()) {
    LegMaps lm;
    const bool split = P.esz == 4;  // fp32 library: k_leg_inv / k_leg_dir without the double-precision tiles, which go to k_leg_*_wide
    if (build_tilemap(P, P.lattile_pref, nct, &lm.d_inv, &lm.n_inv, split ? 1 : 0) || build_tilemap(P, P.ktile_pref, nct, &lm.d_dir, &lm.n_dir, split ? 1 : 0) ||
        (split && (build_tilemap(P, P.lattile_pref, nct, &lm.d_inv_wide, &lm.n_inv_wide, 2) || build_tilemap(P, P.ktile_pref, nct, &lm.d_dir_wide, &lm.n_dir_wide, 2))))
      return EMI_ERR_RUNTIME;
    it = P.legmaps.emplace(nct, lm).first;
  }
  *out = &it->second;
  return 0;
}

static int pick_batch(Plan &P, int nfields, int depth) {
  // fields per batch: bounded by free HBM (W + FB rows x 16 B per field; FB twice when batches are
  // pipelined) and EMI_MAX_BATCH; multiples of 64 fields so the 128-column tiles are full
  size_t fr = 0, tot = 0;
  emi_mem_info(&fr, &tot);
  size_t have = fr + P.cap_W + P.cap_FBL + (P.nproc > 1 ? P.cap_FBF : 0) + emi_stage::idle_bytes();
  const int nfb = depth > 1 ? 2 : 1;
  double per_field = (double)(P.wrows_total + nfb * P.frows + (P.nproc > 1 ? nfb * P.lrows : 0)) * 2.0 * P.esz;
  long long cap = (long long)((double)have * 0.85 / per_field);
  cap = cap / 64 * 64;
  if (cap < 64) cap = 64;
  if (G.max_batch > 0) cap = std::min<long long>(cap, std::max(64, roundup(G.max_batch, 64)));
  long long want = roundup((nfields + depth - 1) / depth, 64);
  return (int)std::min(cap, std::max(64LL, want));
}


static int launch_fft(Plan &P, bool inverse, bool adj, const GridFld *d_flds, int nfld, char *FB, int ldf, int nproma,
                       emi_stream_t st) {
  for (size_t c = 0; c < P.fclass.size(); c++) {
    FftClass &fc = P.fclass[c];
    if (fc.lats.empty() || nfld <= 0) continue;
    const int nchunk = (nfld + fc.fbk - 1) / fc.fbk;
    const long long nblocks = (long long)fc.lats.size() * nchunk;
    FftLaunchDev lc{fc.d_lats, (int)fc.lats.size(), nchunk, nblocks, adj ? 1 : 0, fc.d_rows};
    const int nthr = fc.nthr;
    if (g_pt.on) g_pt.fft_kernels++;  // every class that reaches this point launches exactly one kernel
    if (fc.gmem) {  // work arrays in global memory, one slice per workgroup
      const size_t needb = (size_t)nblocks * fc.gm_elems * 2 * P.esz;
      if (needb > P.cap_fftscr) {
        plan_quiesce(P);
        emi_stream_sync(0);
        emi_dev_free(P.d_fftscr);
        P.d_fftscr = nullptr;
        P.cap_fftscr = 0;
        void *q = nullptr;
        if (emi_dev_malloc(&q, needb)) EMI_FAIL(EMI_ERR_RUNTIME, "cannot allocate %.2f GiB of FFT scratch for the rows that exceed the LDS", needb / 1073741824.0);
        P.d_fftscr = (char *)q;
        P.cap_fftscr = needb;
      }
      if (inverse) {
        if (P.esz == 8)
          EMI_LAUNCH(emi_f64::k_fft_inv_gm, nblocks, nthr, 0, st, P.g, P.ftab, lc, d_flds, nfld, (const double *)FB, ldf, nproma, (d2 *)P.d_fftscr, fc.gm_elems);
        else
          EMI_LAUNCH(emi_f32::k_fft_inv_gm, nblocks, nthr, 0, st, P.g, P.ftab, lc, d_flds, nfld, (const float *)FB, ldf, nproma, (f2 *)P.d_fftscr, fc.gm_elems);
      } else {
        if (P.esz == 8)
          EMI_LAUNCH(emi_f64::k_fft_dir_gm, nblocks, nthr, 0, st, P.g, P.ftab, lc, d_flds, nfld, (double *)FB, ldf, nproma, (d2 *)P.d_fftscr, fc.gm_elems);
        else
          EMI_LAUNCH(emi_f32::k_fft_dir_gm, nblocks, nthr, 0, st, P.g, P.ftab, lc, d_flds, nfld, (float *)FB, ldf, nproma, (f2 *)P.d_fftscr, fc.gm_elems);
      }
      continue;
    }
    if (fc.mr) {
      if (inverse)
        EMI_LAUNCH_P(P.esz, k_fft_inv_mr, nblocks, nthr, fc.lds, st, P.g, P.ftab, lc, d_flds, nfld, (const RT *)FB, ldf, nproma);
      else
        EMI_LAUNCH_P(P.esz, k_fft_dir_mr, nblocks, nthr, fc.lds, st, P.g, P.ftab, lc, d_flds, nfld, (RT *)FB, ldf, nproma);
      continue;
    }
    if (fc.r16 && fc.split) {
      switch (fc.r16) {
#define EMI_R16P_LAUNCH(r_)                                                                                                                 \
  case r_:                                                                                                                                  \
    if (inverse)                                                                                                                            \
      EMI_LAUNCH_P(P.esz, k_fft_inv_r16p<r_>, nblocks, nthr, fc.lds, st, P.g, P.ftab, lc, d_flds, nfld, (const RT *)FB, ldf, nproma);      \
    else                                                                                                                                    \
      EMI_LAUNCH_P(P.esz, k_fft_dir_r16p<r_>, nblocks, nthr, fc.lds, st, P.g, P.ftab, lc, d_flds, nfld, (RT *)FB, ldf, nproma);            \
    break;
        EMI_R16S_LIST(EMI_R16P_LAUNCH)
#undef EMI_R16P_LAUNCH
        default: EMI_FAIL(EMI_ERR_RUNTIME, "internal: no k_fft_*_r16p kernel for R1 = %d", fc.r16);
      }
      continue;
    }
    if (fc.r16) {
      switch (fc.r16) {
#define EMI_R16_LAUNCH(r_)                                                                                                                  \
  case r_:                                                                                                                                  \
    if (inverse)                                                                                                                            \
      EMI_LAUNCH_P(P.esz, k_fft_inv_r16<r_>, nblocks, nthr, fc.lds, st, P.g, P.ftab, lc, d_flds, nfld, (const RT *)FB, ldf, nproma);       \
    else                                                                                                                                    \
      EMI_LAUNCH_P(P.esz, k_fft_dir_r16<r_>, nblocks, nthr, fc.lds, st, P.g, P.ftab, lc, d_flds, nfld, (RT *)FB, ldf, nproma);             \
    break;
        EMI_R16_LIST(EMI_R16_LAUNCH)
#undef EMI_R16_LAUNCH
        default: EMI_FAIL(EMI_ERR_RUNTIME, "internal: no k_fft_*_r16 kernel for R1 = %d", fc.r16);
      }
      continue;
    }
    switch (fc.hot) {
#define EMI_HOT_LAUNCH(pc_, S_, nf_, a_, b_, c_, d_, e_, nfl_)                                                                                       \
  case pc_:                                                                                                                                    \
    if (inverse)                                                                                                                               \
      EMI_LAUNCH_P(P.esz, k_fft_inv_hot<pc_>, nblocks, nthr, fc.lds, st, P.g, P.ftab, lc, d_flds, nfld, (const RT *)FB, ldf, nproma);         \
    else                                                                                                                                       \
      EMI_LAUNCH_P(P.esz, k_fft_dir_hot<pc_>, nblocks, nthr, fc.lds, st, P.g, P.ftab, lc, d_flds, nfld, (RT *)FB, ldf, nproma);               \
    break;
      EMI_HOT_PLAN_LIST(EMI_HOT_LAUNCH)
#undef EMI_HOT_LAUNCH
      default:
        if (inverse)
          EMI_LAUNCH_P(P.esz, k_fft_inv, nblocks, nthr, fc.lds, st, P.g, P.ftab, lc, d_flds, nfld, (const RT *)FB, ldf, nproma);
        else
          EMI_LAUNCH_P(P.esz, k_fft_dir, nblocks, nthr, fc.lds, st, P.g, P.ftab, lc, d_flds, nfld, (RT *)FB, ldf, nproma);
    }
  }
  return 0;
}

// Two library-owned streams software-pipeline the field batches of one call: the Legendre kernels
// (MFMA-bound) of batch b+1 run on stream A while the FFT kernels (fp64-VALU/LDS-bound) of batch b
// run on stream B; the Fourier buffer is double-buffered.  Both are forked from / joined to the
// caller's stream with events, so the call keeps ordinary stream semantics.
struct Pipeline {
#ifndef EMI_CPU_EMU
  hipStream_t sA = nullptr, sB = nullptr, sX = nullptr;  // Legendre, FFT, exchange
  std::vector<hipEvent_t> ev;
  hipEvent_t fork = nullptr, joinA = nullptr, joinB = nullptr, joinX = nullptr;
  int init() {
    if (sA) return 0;
    EMI_CHECK(hipStreamCreateWithFlags(&sA, hipStreamNonBlocking));
    EMI_CHECK(hipStreamCreateWithFlags(&sB, hipStreamNonBlocking));
    EMI_CHECK(hipStreamCreateWithFlags(&sX, hipStreamNonBlocking));
    EMI_CHECK(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
    EMI_CHECK(hipEventCreateWithFlags(&joinA, hipEventDisableTiming));
    EMI_CHECK(hipEventCreateWithFlags(&joinB, hipEventDisableTiming));
    EMI_CHECK(hipEventCreateWithFlags(&joinX, hipEventDisableTiming));
    return 0;
  }
  hipEvent_t event(size_t i) {
    while (ev.size() <= i) {
      hipEvent_t e;
      (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
      ev.push_back(e);
    }
    return ev[i];
  }
  void begin(emi_stream_t user) {
    (void)hipEventRecord(fork, user);
    (void)hipStreamWaitEvent(sA, fork, 0);
    (void)hipStreamWaitEvent(sB, fork, 0);
    (void)hipStreamWaitEvent(sX, fork, 0);
  }
  void end(emi_stream_t user) {
    (void)hipEventRecord(joinA, sA);
    (void)hipEventRecord(joinB, sB);
    (void)hipEventRecord(joinX, sX);
    (void)hipStreamWaitEvent(user, joinA, 0);
    (void)hipStreamWaitEvent(user, joinB, 0);
    (void)hipStreamWaitEvent(user, joinX, 0);
  }
  void signal(size_t i, emi_stream_t s) { (void)hipEventRecord(event(i), s); }
  void wait(size_t i, emi_stream_t s) { (void)hipStreamWaitEvent(s, event(i), 0); }
#else
  void *sA = nullptr, *sB = nullptr, *sX = nullptr;
  int init() { return 0; }
  void begin(emi_stream_t) {}
  void end(emi_stream_t) {}
  void signal(size_t, emi_stream_t) {}
  void wait(size_t, emi_stream_t) {}
#endif
};
static Pipeline g_pipe;

// number of field batches to pipeline (1 = plain sequential execution on the caller's stream)
static int pipeline_depth(const Plan &P, int nfields) {
  // one task: sequential.  Co-running the two kernel families of neighbouring field batches was measured SLOWER on MI355X
  // (TCo1279/KF=1645: 555 vs 531 ms per pair with 4 batches; round 2: 400.7 vs 391.7) -- the FFT kernels need all 16 waves per CU
  // to hide latency and the Legendre kernels lose MFMA issue slots.
  const int cfg = (test_paths() & 2) ? 4 : 1;
#ifdef EMI_CPU_EMU
  (void)P;
  (void)nfields;
  return 1;
#else
  if (nfields < 256) return 1;
  if (P.nproc > 1) {
    // several tasks: the all-to-all-v of batch b (xGMI) runs on its own stream under the Legendre kernels
    // of batch b+1 and the FFT kernels of batch b-1 -- with 2 or 4 GPUs the exchange is as long as the
    // compute (one or three links per GPU), so hiding it is worth more than the co-running penalty.
    // EMI_PIPELINE_DIST: batches per call (1 = sequential), default 4
    static int dcfg = -1;
    if (dcfg < 0) {
      const char *e = getenv("EMI_PIPELINE_DIST");
      dcfg = e ? atoi(e) : 4;
      if (dcfg < 1) dcfg = 1;
    }
    return dcfg;
  }
  return cfg;
#endif
}

#ifndef EMI_CPU_EMU
static int set_lds_attrs() {
  static bool done = false;
  if (done) return 0;
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f64::k_leg_dir, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f32::k_leg_dir, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
#define EMI_HOT_ATTR(pc_, S_, nf_, a_, b_, c_, d_, e_, nfl_)                                                                                  \
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f64::k_fft_inv_hot<pc_>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));  \
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f64::k_fft_dir_hot<pc_>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));  \
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f32::k_fft_inv_hot<pc_>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));  \
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f32::k_fft_dir_hot<pc_>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_HOT_PLAN_LIST(EMI_HOT_ATTR)
#undef EMI_HOT_ATTR
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f64::k_lam_inv, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f64::k_lam_dir, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f32::k_lam_inv, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f32::k_lam_dir, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f64::k_lam_inv_ad, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f64::k_lam_dir_ad, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f32::k_lam_inv_ad, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f32::k_lam_dir_ad, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f64::k_fft_inv, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f64::k_fft_dir, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f32::k_fft_inv, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f32::k_fft_dir, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  // direct mixed-radix plans hold up to 160 KiB per field (mr_choose) and have no global-scratch variant: fp64 rows such as
  // n = 8704 (half-length 4352 = 16 x 16 x 17) need 69 888 B
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f64::k_fft_inv_mr, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f64::k_fft_dir_mr, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f32::k_fft_inv_mr, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f32::k_fft_dir_mr, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
#define EMI_R16_ATTR(r_)                                                                                                                     \
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f64::k_fft_inv_r16<r_>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));  \
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f64::k_fft_dir_r16<r_>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));  \
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f32::k_fft_inv_r16<r_>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));  \
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f32::k_fft_dir_r16<r_>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_R16_LIST(EMI_R16_ATTR)
#undef EMI_R16_ATTR
#define EMI_R16P_ATTR(r_)                                                                                                                    \
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f64::k_fft_inv_r16p<r_>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); \
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f64::k_fft_dir_r16p<r_>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); \
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f32::k_fft_inv_r16p<r_>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); \
  EMI_CHECK(hipFuncSetAttribute((const void *)emi_f32::k_fft_dir_r16p<r_>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EMI_R16S_LIST(EMI_R16P_ATTR)
#undef EMI_R16P_ATTR
  done = true;
  return 0;
}
#else
static int set_lds_attrs() { return 0; }
#endif

// scalar field enumeration shared by both directions: PSPSCALAR, or PSPSC2 + PSPSC3A + PSPSC3B
// (ltinv_mod.F90:203-240 / updsp_mod.F90:128-160 ordering)
struct ScalarRef {
  int arr;  // 0 scalar, 1 sc2, 2 sc3a, 3 sc3b
  int lev, var;
};

template <class ARGS>
static int enumerate_scalars(const ARGS &a, const char *who, std::vector<ScalarRef> &sc) {
  sc.clear();
  if (a.spscalar) {
    if (a.spsc3a || a.spsc3b || a.spsc2) EMI_FAIL(EMI_ERR_ARG, "%s : PSPSCALAR AND PSPSC3A/PSPSC3B/PSPSC2 BOTH PRESENT", who);
    for (int i = 0; i < a.nf_scalar; i++) sc.push_back({0, i, 0});
  } else {
    if (a.spsc2)
      for (int i = 0; i < a.nf_sc2; i++) sc.push_back({1, i, 0});
    if (a.spsc3a)
      for (int v = 0; v < a.sc3a_nvar; v++)
        for (int l = 0; l < a.sc3a_nlev; l++) sc.push_back({2, l, v});
    if (a.spsc3b)
      for (int v = 0; v < a.sc3b_nvar; v++)
        for (int l = 0; l < a.sc3b_nlev; l++) sc.push_back({3, l, v});
  }
  return 0;
}

// The reference's extent checks (inv_trans.F90:476-600, dir_trans.F90:370-491) on the extents the caller reports.
// nvar_uv = IF_UV_PAR; dmul = 3 with LDSCDERS (IF_SC2_G, IF_SC3A_G3 and IF_SC3B_G3 are tripled, inv_trans.F90:371-376).
// *uv_dim3: the third extent of PGPUV to address with (>= nvar_uv).
template <class ARGS>
static int check_extents(const char *who, const ARGS &a, int nspec2, int nproma, int ngpblks, int nuv, int nvar_uv, int dmul,
                         int *uv_dim3) {
  *uv_dim3 = nvar_uv;
  const emi_extents_t *e = a.ext;
  if (!e) return 0;
  if (e->sp_dim2 > 0 && e->sp_dim2 < nspec2)
    EMI_FAIL(EMI_ERR_ARG, "%s : SECOND DIMENSION OF A SPECTRAL ARRAY TOO SMALL (%d < NSPEC2 = %d)", who, e->sp_dim2, nspec2);
  auto lead = [&](const char *nm, int d1) {
    if (d1 < nproma) {
      emi_set_error("%s:FIRST DIMENSION OF %s TOO SMALL (%d < %d)", who, nm, d1, nproma);
      return -1;
    }
    if (d1 != nproma) {
      emi_set_error("%s: first extent of %s is %d, NPROMA is %d: pass a packed copy at the C-ABI (the Fortran shim does)", who, nm, d1, nproma);
      return -1;
    }
    return 0;
  };
  if (a.gp) {
    if (lead("PGP", e->gp[0])) return EMI_ERR_ARG;
    if (e->gp[1] != a.gp_nfld) EMI_FAIL(EMI_ERR_ARG, "%s: gp_nfld (%d) is not the second extent of PGP (%d)", who, a.gp_nfld, e->gp[1]);
    if (e->gp[2] < ngpblks) EMI_FAIL(EMI_ERR_ARG, "%s:THIRD DIMENSION OF PGP TOO SMALL (%d < %d)", who, e->gp[2], ngpblks);
  }
  if (a.gpuv) {
    if (lead("PGPUV", e->gpuv[0])) return EMI_ERR_ARG;
    if (e->gpuv[1] != a.nf_uv) EMI_FAIL(EMI_ERR_ARG, "%s:SEC. DIMENSION OF PGPUV INCONSISTENT (%d, IF_UV_G = %d)", who, e->gpuv[1], a.nf_uv);
    if (e->gpuv[2] < nvar_uv) EMI_FAIL(EMI_ERR_ARG, "%s:THIRD DIMENSION OF PGPUV TOO SMALL (%d < %d)", who, e->gpuv[2], nvar_uv);
    if (e->gpuv[3] < ngpblks) EMI_FAIL(EMI_ERR_ARG, "%s:FOURTH DIMENSION OF PGPUV TOO SMALL (%d < %d)", who, e->gpuv[3], ngpblks);
    *uv_dim3 = e->gpuv[2];
    (void)nuv;
  }
  if (a.gp2 && a.nf_sc2 > 0) {
    if (lead("PGP2", e->gp2[0])) return EMI_ERR_ARG;
    if (e->gp2[1] != a.nf_sc2 * dmul) EMI_FAIL(EMI_ERR_ARG, "%s:SEC. DIMENSION OF PGP2 INCONSISTENT (%d, IF_SC2_G = %d)", who, e->gp2[1], a.nf_sc2 * dmul);
    if (e->gp2[2] < ngpblks) EMI_FAIL(EMI_ERR_ARG, "%s:THIRD DIMENSION OF PGP2 TOO SMALL (%d < %d)", who, e->gp2[2], ngpblks);
  }
  if (a.gp3a && a.sc3a_nlev * a.sc3a_nvar > 0) {
    if (lead("PGP3A", e->gp3a[0])) return EMI_ERR_ARG;
    if (e->gp3a[1] != a.sc3a_nlev) EMI_FAIL(EMI_ERR_ARG, "%s:SEC. DIMENSION OF PGP3A INCONSISTENT (%d, IF_SC3A_G2 = %d)", who, e->gp3a[1], a.sc3a_nlev);
    if (e->gp3a[2] != a.sc3a_nvar * dmul)
      EMI_FAIL(EMI_ERR_ARG, "%s:THIRD DIMENSION OF PGP3A INCONSISTENT (%d, IF_SC3A_G3 = %d)", who, e->gp3a[2], a.sc3a_nvar * dmul);
    if (e->gp3a[3] < ngpblks) EMI_FAIL(EMI_ERR_ARG, "%s:FOURTH DIMENSION OF PGP3A TOO SMALL (%d < %d)", who, e->gp3a[3], ngpblks);
  }
  if (a.gp3b && a.sc3b_nlev * a.sc3b_nvar > 0) {
    if (lead("PGP3B", e->gp3b[0])) return EMI_ERR_ARG;
    if (e->gp3b[1] != a.sc3b_nlev) EMI_FAIL(EMI_ERR_ARG, "%s:SEC. DIMENSION OF PGP3B INCONSISTENT (%d, IF_SC3B_G2 = %d)", who, e->gp3b[1], a.sc3b_nlev);
    if (e->gp3b[2] != a.sc3b_nvar * dmul)
      EMI_FAIL(EMI_ERR_ARG, "%s:THIRD DIMENSION OF PGP3B INCONSISTENT (%d, IF_SC3B_G3 = %d)", who, e->gp3b[2], a.sc3b_nvar * dmul);
    if (e->gp3b[3] < ngpblks) EMI_FAIL(EMI_ERR_ARG, "%s:FOURTH DIMENSION OF PGP3B TOO SMALL (%d < %d)", who, e->gp3b[3], ngpblks);
  }
  return 0;
}

// One transform call, whichever public block it came in: emi_invtrans_t (INV_TRANS, INV_TRANSAD) or emi_dirtrans_t (DIR_TRANS,
// DIR_TRANSAD).  The pipeline that runs it decides which side is read: the spectral arrays (inverse) or the grid arrays (direct).
struct Call {
  int mem_space;
  emi_stream_t stream;
  const emi_extents_t *ext;
  const emi_vsets_t *vsets;
  int kproma;
  void *spvor, *spdiv, *spscalar, *spsc3a, *spsc3b, *spsc2;
  int nf_uv, nf_scalar, sc3a_nlev, sc3a_nvar, sc3b_nlev, sc3b_nvar, nf_sc2;
  void *gp, *gpuv, *gp3a, *gp3b, *gp2;
  int gp_nfld;
  int ldscders, ldvorgp, lddivgp, lduvder;  // LDSCDERS, LDVORGP, LDDIVGP, LDUVDER: 0 from an emi_dirtrans_t
  int ldlatlon;                             // LDLATLON: 0 from an emi_dirtrans_t
  void *meanu, *meanv;                      // EINV_TRANS / EDIR_TRANS: PMEANU / PMEANV(nf_uv), reals of the library precision where the other arrays live
};
template <class A>
static Call to_call(const A &a) {
  Call c{a.mem_space, (emi_stream_t)a.stream, a.ext, a.vsets, a.kproma,
         (void *)a.spvor, (void *)a.spdiv, (void *)a.spscalar, (void *)a.spsc3a, (void *)a.spsc3b, (void *)a.spsc2,
         a.nf_uv, a.nf_scalar, a.sc3a_nlev, a.sc3a_nvar, a.sc3b_nlev, a.sc3b_nvar, a.nf_sc2,
         (void *)a.gp, (void *)a.gpuv, (void *)a.gp3a, (void *)a.gp3b, (void *)a.gp2, a.gp_nfld, 0, 0, 0, 0, 0, nullptr, nullptr};
  if constexpr (std::is_same<A, emi_invtrans_t>::value)
    c.ldscders = a.ldscders, c.ldvorgp = a.ldvorgp, c.lddivgp = a.lddivgp, c.lduvder = a.lduvder, c.ldlatlon = a.ldlatlon;
  return c;
}

struct VGroups {  // the global fields of a call with V-sets (v_groups)
  int nuv_g = 0;
  std::vector<int> ouv;            // owner V-set (0-based) of every global u/v field
  std::vector<ScalarRef> sc_g;     // global scalars in the reference's order
  std::vector<int> osc;            // their owners
  int nsc_g[4] = {0, 0, 0, 0};     // global counts: PSPSCALAR fields, PSPSC2 fields, PSPSC3A levels, PSPSC3B levels
  int nvar3a = 0, nvar3b = 0;      // variables of PSPSC3A / PSPSC3B = IF_SC3A_G3 / IF_SC3B_G3 (inv_trans.F90:277, 310): the same on every task
};

// Field accounting of a call (inv_trans.F90:230-387, dir_trans.F90:290-303) over the call's own arrays (vg == nullptr) or over the
// global fields of all V-sets (vg), and the reference's checks that the grid arrays these fields need are present.
struct Fields {
  int nuv = 0;                // u/v fields (IF_UV)
  std::vector<ScalarRef> sc;  // scalar fields in the reference's order
  int nf2 = 0, nlev3a = 0, nvar3a = 0, nlev3b = 0, nvar3b = 0;  // the layout of PGP2 / PGP3A / PGP3B (before the factor dmul)
  bool scders = false, vorgp = false, divgp = false, uvder = false;  // the options in effect
  // IF_UV_PAR; 3 with LDSCDERS (IF_SC2_G, IF_SC3A_G3 and IF_SC3B_G3 are tripled, inv_trans.F90:371-376); IF_GP
  int nvar_uv = 2, dmul = 1, if_gp = 0;
};
static int account(const Call &c, const char *who, bool inverse, const VGroups *vg, Fields &f) {
  int need[4];  // fields of PSPSCALAR, PSPSC2, PSPSC3A, PSPSC3B that need a grid array
  if (vg) {
    f.nuv = vg->nuv_g, f.sc = vg->sc_g;
    f.nf2 = vg->nsc_g[1], f.nlev3a = vg->nsc_g[2], f.nvar3a = vg->nvar3a, f.nlev3b = vg->nsc_g[3], f.nvar3b = vg->nvar3b;
    need[0] = vg->nsc_g[0], need[1] = f.nf2, need[2] = f.nlev3a * f.nvar3a, need[3] = f.nlev3b * f.nvar3b;
  } else {
    f.nuv = (c.spvor || c.spdiv) ? c.nf_uv : 0;
    if (inverse && f.nuv > 0 && !c.spvor) EMI_FAIL(EMI_ERR_ARG, "%s : IF_UV > 0 BUT PSPVOR MISSING", who);
    if (inverse && f.nuv > 0 && !c.spdiv) EMI_FAIL(EMI_ERR_ARG, "%s : IF_UV > 0 BUT PSPDIV MISSING", who);
    if (!inverse && f.nuv > 0 && (!c.spvor || !c.spdiv)) EMI_FAIL(EMI_ERR_ARG, "%s : IF_UV > 0 BUT PSPVOR OR PSPDIV MISSING", who);
    if (enumerate_scalars(c, who, f.sc)) return EMI_ERR_ARG;
    f.nf2 = c.nf_sc2, f.nlev3a = c.sc3a_nlev, f.nvar3a = c.sc3a_nvar, f.nlev3b = c.sc3b_nlev, f.nvar3b = c.sc3b_nvar;
    need[0] = c.spscalar ? (int)f.sc.size() : 0, need[1] = c.spsc2 ? f.nf2 : 0;
    need[2] = c.spsc3a ? f.nlev3a * f.nvar3a : 0, need[3] = c.spsc3b ? f.nlev3b * f.nvar3b : 0;
  }
  const int nuv = f.nuv, nsc = (int)f.sc.size();
  f.scders = c.ldscders && nsc > 0;
  f.vorgp = c.ldvorgp && nuv > 0;
  f.divgp = (c.lddivgp || c.ldvorgp) && nuv > 0;  // inv_trans.F90:350
  f.uvder = c.lduvder && nuv > 0;
  f.nvar_uv = 2 + (f.vorgp ? 1 : 0) + (f.divgp ? 1 : 0) + (f.uvder ? 2 : 0);
  f.dmul = f.scders ? 3 : 1;
  f.if_gp = nuv * f.nvar_uv + nsc * f.dmul;
  if (vg && f.if_gp == 0) return 0;  // V-sets: no fields on any task, no array to check
  if (c.gp) {
    if (c.gpuv || c.gp3a || c.gp3b || c.gp2) EMI_FAIL(EMI_ERR_ARG, "%s:PGP AND PGPUV/PGP3A/PGP3B/PGP2 CAN NOT BOTH BE PRESENT", who);
    if (c.gp_nfld < f.if_gp) EMI_FAIL(EMI_ERR_ARG, "%s:SECOND DIMENSION OF PGP TOO SMALL (%d < %d)", who, c.gp_nfld, f.if_gp);
  } else {
    if (nuv > 0 && !c.gpuv) EMI_FAIL(EMI_ERR_ARG, "%s:PGPUV MISSING", who);
    if (need[0] > 0) EMI_FAIL(EMI_ERR_ARG, "%s:PGP MISSING (PSPSCALAR needs PGP)", who);
    if (need[1] > 0 && !c.gp2) EMI_FAIL(EMI_ERR_ARG, "%s:PGP2 MISSING", who);
    if (need[2] > 0 && !c.gp3a) EMI_FAIL(EMI_ERR_ARG, "%s:PGP3A MISSING", who);
    if (need[3] > 0 && !c.gp3b) EMI_FAIL(EMI_ERR_ARG, "%s:PGP3B MISSING", who);
  }
  return 0;
}

// The grid-point fields of a call in the reference's order (inv_trans.F90:352-387, ftinv_ctl_mod.F90:228-262, trltog_mod.F90:632-690):
// [vor] [div] u v scalars [N-S derivatives] [u, v E-W derivatives] [scalar E-W derivatives], over PGP or over PGPUV (uv_dim3
// variables) / PGP2 / PGP3A / PGP3B.  Every field carries its group and its index in the group (the level of a u/v group, the
// position in Fields::sc of a scalar group).
enum { GF_VOR, GF_DIV, GF_U, GF_V, GF_SC, GF_NSD, GF_UEW, GF_VEW, GF_SCEW, GF_N };
static bool gf_uv(int grp) { return grp != GF_SC && grp != GF_NSD && grp != GF_SCEW; }
struct GridRef {
  GridFld g;
  int grp, i;
};
static void grid_fields(const Fields &f, const Call &d, int uv_dim3, std::vector<GridRef> &out) {
  out.clear();
  const int nuv = f.nuv;
  int uvvar = 0;  // the next variable of PGPUV
  auto add = [&](int grp, int i, int mode, void *base, int nf_arr, int fidx) {
    GridFld g{};
    if (d.gp) base = d.gp, nf_arr = d.gp_nfld, fidx = (int)out.size();
    g.base = base, g.nf_arr = nf_arr, g.fidx = fidx, g.mode = mode;
    out.push_back({g, grp, i});
  };
  auto uv = [&](int grp, int mode) {
    for (int i = 0; i < nuv; i++) add(grp, i, mode, d.gpuv, nuv * uv_dim3, uvvar * nuv + i);
    uvvar++;
  };
  auto sc = [&](int grp, int kder, int mode) {  // derivative block kder of every scalar (0 value, 1 N-S, 2 E-W)
    for (int i = 0; i < (int)f.sc.size(); i++) {
      const ScalarRef &r = f.sc[i];
      if (r.arr == 1) add(grp, i, mode, d.gp2, f.nf2 * f.dmul, r.lev + kder * f.nf2);
      else if (r.arr == 2) add(grp, i, mode, d.gp3a, f.nlev3a * f.nvar3a * f.dmul, (r.var + kder * f.nvar3a) * f.nlev3a + r.lev);
      else add(grp, i, mode, d.gp3b, f.nlev3b * f.nvar3b * f.dmul, (r.var + kder * f.nvar3b) * f.nlev3b + r.lev);
    }
  };
  if (f.vorgp) uv(GF_VOR, GM_PLAIN);
  if (f.divgp) uv(GF_DIV, GM_PLAIN);
  uv(GF_U, GM_ACOS);
  uv(GF_V, GM_ACOS);
  sc(GF_SC, 0, GM_PLAIN);
  if (f.scders) sc(GF_NSD, 1, GM_ACOS);
  if (f.uvder) uv(GF_UEW, GM_EWDER_UV), uv(GF_VEW, GM_EWDER_UV);
  if (f.scders) sc(GF_SCEW, 2, GM_EWDER);
}

// The arrays of a call on the device (d: c with device pointers).  Host arrays are staged through device memory, the input side
// (the spectral arrays of the inverse, the grid arrays of the direct) copied in.  An output array is preloaded where the call
// does not write all of it: the padding of the last NPROMA block (gpad), a PGP with more fields than IF_GP, a PGPUV with more
// variables than IF_UV_PAR.  uv_sp: stage PSPVOR / PSPDIV (the W-set transform only with u/v fields, the V-set one always).
static int stage(const Plan &P, HostStage &hs, const Call &c, const char *who, bool inverse, bool uv_sp, const Fields &f, size_t gsz, bool gpad,
                 int uv_dim3, Call &d) {
  const bool host = c.mem_space == EMI_MEM_HOST;
  const emi_stream_t st = c.stream;
  const size_t ns2 = P.nspec2;
  auto sp = [&](void *h, size_t nf, bool on) { return inverse ? (void *)hs.in(h, ns2 * nf, on, st) : hs.out(h, ns2 * nf, on, false, st); };
  auto gr = [&](void *h, size_t nf, bool on, bool pre) { return inverse ? hs.out(h, gsz * nf, on, pre, st) : (void *)hs.in(h, gsz * nf, on, st); };
  d = c;
  d.mem_space = EMI_MEM_DEVICE;
  d.spvor = sp(c.spvor, c.nf_uv, uv_sp), d.spdiv = sp(c.spdiv, c.nf_uv, uv_sp);
  d.spscalar = sp(c.spscalar, c.nf_scalar, host), d.spsc2 = sp(c.spsc2, c.nf_sc2, host);
  d.spsc3a = sp(c.spsc3a, (size_t)c.sc3a_nlev * c.sc3a_nvar, host), d.spsc3b = sp(c.spsc3b, (size_t)c.sc3b_nlev * c.sc3b_nvar, host);
  d.gp = gr(c.gp, c.gp_nfld, host, gpad || c.gp_nfld > f.if_gp);
  d.gpuv = gr(c.gpuv, (size_t)f.nuv * uv_dim3, host && f.nuv, gpad || uv_dim3 > f.nvar_uv);
  d.gp2 = gr(c.gp2, (size_t)f.nf2 * f.dmul, host, gpad);
  d.gp3a = gr(c.gp3a, (size_t)f.nlev3a * f.nvar3a * f.dmul, host, gpad);
  d.gp3b = gr(c.gp3b, (size_t)f.nlev3b * f.nvar3b * f.dmul, host, gpad);
  if (hs.failed) EMI_FAIL(EMI_ERR_RUNTIME, "%s: cannot stage the host arrays through device memory (%s)", who, emi_last_error());
  return 0;
}

// One field batch of a call: its row width, its field descriptors in the call's upload and its Legendre tile map.
struct Batch {
  int ldw = 0, ntiles = 0;                 // row width (2 x 64 x its column tiles); the column tiles that hold fields
  size_t off_g = 0, off_s = 0, off_f = 0;  // offsets of its GridFld, of its SpecSrc (inverse) or SpecDst (direct), of its FuseDst
  int ng = 0, ns = 0;                      // numbers of GridFld and of SpecSrc / SpecDst
  size_t off_l = 0, off_c = 0;             // EINV_TRANSAD: offsets of its LamSlot and of its chunk starts (nchunk + 1 of them)
  int nchunk = 0;
  LegMaps *maps = nullptr;
};
// appends n descriptors to the upload of a call, 256-byte aligned, and returns their offset
template <class T>
static size_t append_desc(std::vector<char> &hdesc, const T *p, size_t n) {
  const size_t off = hdesc.size();
  hdesc.resize(off + (n * sizeof(T) + 255) / 256 * 256);
  if (n) memcpy(hdesc.data() + off, p, n * sizeof(T));
  return off;
}

// Runs the batches of a call: first(batch, stream, FBl, FBf), the exchange between the Fourier buffers (several tasks), then
// last(batch, stream, FBl, FBf, done).  The inverse runs Legendre (stream A), TRMTOL, FFT (stream B); the direct FFT (B), TRLTOM,
// Legendre (A).  Several batches are software-pipelined over the three library streams (A, B, X for the exchange), forked from
// and joined to the caller's stream.  Events of batch ib: 3 ib = first stage done, 3 ib + 1 = last stage done (recorded where the
// last stage calls done()), 3 ib + 2 = exchange done.  Both Fourier buffers are double buffered ([ib & 1]); one task: FBf == FBl
// and there is no exchange.
template <class First, class Last>
static int run_batches(Plan &P, emi_stream_t st, bool inverse, bool piped, int bfpad, std::vector<Batch> &bats, const std::vector<char> &hdesc,
                       First first, Last last) {
  if (ensure_work(P, bfpad, piped ? 2 : 1, st)) return EMI_ERR_RUNTIME;
  // Legendre tile maps per batch: a batch with fewer fields than the row width (the last one of a call) only
  // gets the column tiles that hold fields (built before anything is queued or forked: a new map is a blocking upload)
  for (Batch &bt : bats)
    if (!P.lam && leg_tilemaps(P, bt.ntiles, &bt.maps)) return EMI_ERR_RUNTIME;
  if (upload_desc(P, hdesc, st)) return EMI_ERR_RUNTIME;
  emi_stream_t sA = st, sB = st, sX = st;
  if (piped) {
    if (g_pipe.init()) return EMI_ERR_RUNTIME;
    sA = (emi_stream_t)g_pipe.sA;
    sB = (emi_stream_t)g_pipe.sB;
    sX = (emi_stream_t)g_pipe.sX;
    g_pipe.begin(st);
  }
  g_pt.begin(G.profile != 0, G.profile == 2);
  const emi_stream_t s1 = inverse ? sA : sB, s2 = inverse ? sB : sA;  // first and last stage
  const bool dist = P.nproc > 1;
  // buffer strides for the widest batch (+ the zero row DIR_TRANS keeps behind the Legendre-side rows)
  const int ldw_max = 2 * bfpad;
  const size_t lstride = (size_t)((dist ? P.lrows : P.frows) + 1) * ldw_max * P.esz, fstride = (size_t)P.frows * ldw_max * P.esz;
  int rc = EMI_SUCCESS;
  for (int ib = 0; ib < (int)bats.size(); ib++) {
    const Batch &bt = bats[ib];
    char *FBl = P.d_FBL + (piped ? (size_t)(ib & 1) * lstride : 0);
    char *FBf = dist ? P.d_FBF + (piped ? (size_t)(ib & 1) * fstride : 0) : FBl;
    // the buffer the first stage writes was last read by the last stage (one task) or by the exchange (several tasks) of batch ib-2
    if (piped && ib >= 2) g_pipe.wait(3 * (ib - 2) + (dist ? 2 : 1), s1);
    if (first(bt, s1, FBl, FBf)) {
      rc = EMI_ERR_RUNTIME;
      break;
    }
    if (piped) g_pipe.signal(3 * ib, s1);
    if (dist) {
      // stream X: the buffer the exchange writes was last read by the last stage of batch ib-2
      if (piped) g_pipe.wait(3 * ib, sX);
      if (piped && ib >= 2) g_pipe.wait(3 * (ib - 2) + 1, sX);
      EmiRange rg(inverse ? EMI_LBL_TRMTOL : EMI_LBL_TRLTOM);  // GSTATS 152 / 153
      if (exchange(P, inverse, bt.ldw, sX, FBl, FBf)) {
        rc = EMI_ERR_RUNTIME;
        break;
      }
      if (piped) g_pipe.signal(3 * ib + 2, sX);
    }
    if (piped) g_pipe.wait(3 * ib + (dist ? 2 : 0), s2);
    auto done = [&] {
      if (piped) g_pipe.signal(3 * ib + 1, s2);
    };
    if (last(bt, s2, FBl, FBf, done)) {
      rc = EMI_ERR_RUNTIME;
      break;
    }
  }
  if (piped) g_pipe.end(st);  // the three streams were forked from the caller's: join them, also when giving up
  return rc;
}

// INV_TRANS, and DIR_TRANSAD when adj: the adjoint of DIR_TRANS (for the inner products of the
// reference's adjoint tests: plain sum over grid points, SPECNORM weights in spectral space) is the same
// spectral -> grid pipeline with the Gaussian weight and 1/NLOEN applied per latitude (ledirad_mod.F90:151,183,
// ftdirad_mod.F90:84-89) and the adjoint of UVTVD in place of VDTUV.
static int inv_pipeline(Plan &P, const Call &d, const Fields &f, std::vector<GridRef> &gl, int nproma, bool adj) {
  const size_t ns2 = P.nspec2;
  const int nuv = f.nuv;
  // ---- Legendre-space fields (ltinv_mod.F90:166-262): [vor][div] u v scalars [nsders]
  std::vector<SpecSrc> lt;
  auto sc_src = [&](const ScalarRef &r, int kind) {
    SpecSrc s{};
    s.kind = kind;
    switch (r.arr) {
      case 0: s.a = d.spscalar; s.sa = d.nf_scalar; s.ia = r.lev; break;
      case 1: s.a = d.spsc2; s.sa = d.nf_sc2; s.ia = r.lev; break;
      case 2: s.a = (const char *)d.spsc3a + (size_t)r.var * ns2 * d.sc3a_nlev * P.esz; s.sa = d.sc3a_nlev; s.ia = r.lev; break;
      default: s.a = (const char *)d.spsc3b + (size_t)r.var * ns2 * d.sc3b_nlev * P.esz; s.sa = d.sc3b_nlev; s.ia = r.lev; break;
    }
    return s;
  };
  auto uvsrc = [&](int i, int kind) {
    SpecSrc s{};
    s.kind = kind;
    s.a = d.spvor; s.sa = d.nf_uv; s.ia = i;
    s.b = d.spdiv; s.sb = d.nf_uv; s.ib = i;
    if (kind == SPK_COPY + 100) { s.kind = SPK_COPY; s.a = d.spdiv; }
    return s;
  };
  int l0[GF_N] = {};  // the first Legendre-space field of every group of grid fields
  if (f.vorgp) { l0[GF_VOR] = (int)lt.size(); for (int i = 0; i < nuv; i++) lt.push_back(uvsrc(i, SPK_COPY)); }
  if (f.divgp) { l0[GF_DIV] = (int)lt.size(); for (int i = 0; i < nuv; i++) lt.push_back(uvsrc(i, SPK_COPY + 100)); }
  l0[GF_U] = (int)lt.size(); for (int i = 0; i < nuv; i++) lt.push_back(uvsrc(i, adj ? SPK_U_AD : SPK_U));
  l0[GF_V] = (int)lt.size(); for (int i = 0; i < nuv; i++) lt.push_back(uvsrc(i, adj ? SPK_V_AD : SPK_V));
  l0[GF_SC] = (int)lt.size(); for (auto &r : f.sc) lt.push_back(sc_src(r, SPK_COPY));
  if (f.scders) { l0[GF_NSD] = (int)lt.size(); for (auto &r : f.sc) lt.push_back(sc_src(r, SPK_NSD)); }
  l0[GF_UEW] = l0[GF_U], l0[GF_VEW] = l0[GF_V], l0[GF_SCEW] = l0[GF_SC];  // the E-W derivatives are taken in Fourier space
  for (GridRef &r : gl) r.g.src = l0[r.grp] + r.i;
  const int nlt = (int)lt.size();

  // ---- batches over Legendre-space fields
  const int depth = pipeline_depth(P, nlt);
  const int bsz = pick_batch(P, nlt, depth);
  const int nbat = (nlt + bsz - 1) / bsz;
  // The 64-field column tiles of the call are dealt evenly to the batches and every batch has its own row width
  // (2 x its tiles x 64 reals): no batch computes, stores or exchanges columns of another batch's width (with
  // batches of ceil(fields / nbat) rounded up to 64 the 4 x 448 columns of a 1645-field call were 9 % padding).
  const int tiles_total = (nlt + 63) / 64;
  const int bfpad = 64 * ((tiles_total + nbat - 1) / nbat);  // widest batch
  // all descriptors of the call in one upload
  std::vector<Batch> bats;
  std::vector<char> hdesc;
  for (int ibat = 0, b0 = 0; ibat < nbat; ibat++) {
    const int tiles_b = tiles_total / nbat + (ibat < tiles_total % nbat ? 1 : 0);
    const int nb = std::min(64 * tiles_b, nlt - b0);
    std::vector<GridFld> bg;
    for (const GridRef &r : gl)
      if (r.g.src >= b0 && r.g.src < b0 + nb) {
        bg.push_back(r.g);
        bg.back().src -= b0;
      }
    Batch bt{};
    bt.ldw = 2 * 64 * tiles_b;
    bt.ntiles = (nb + 63) / 64;
    bt.ns = nb, bt.off_s = append_desc(hdesc, lt.data() + b0, nb);
    bt.ng = (int)bg.size(), bt.off_g = append_desc(hdesc, bg.data(), bg.size());
    bats.push_back(bt);
    b0 += nb;
  }
  // stream A: spectral pack + Legendre
  auto legendre = [&](const Batch &bt, emi_stream_t s, char *FBl, char *) -> int {
    EmiRange rg(EMI_LBL_LTINV);  // GSTATS 102: PRFI1B / VDTUV / SPNSDE + LEINV + ASRE1B
    const int ldw = bt.ldw, bfpad_b = bt.ldw / 2;  // this batch's row width
    const SpecSrc *d_bl = (const SpecSrc *)((char *)P.d_desc + bt.off_s);
    if (P.lam) {
      // limited-area handle: EPRFI1B / EVDTUV / ESPNSDE + ELEINV + EASRE1B in one kernel, from the caller's arrays to the Fourier buffer;
      // the y-direction FFT is timed in the Legendre slot
      const int nchunk = (bt.ns + P.lamdev.fbk - 1) / P.lamdev.fbk;
      const int ivl = g_pt.start(1, s);
      if (adj)
        EMI_LAUNCH_P(P.esz, k_lam_inv_ad, (long long)P.nump * nchunk, P.lam_nthr, P.lam_lds, s, P.g, P.lamdev, P.ftab, d_bl, bt.ns, (const RT *)d.meanu, (const RT *)d.meanv,
                     (RT *)FBl, ldw, nchunk);
      else
        EMI_LAUNCH_P(P.esz, k_lam_inv, (long long)P.nump * nchunk, P.lam_nthr, P.lam_lds, s, P.g, P.lamdev, P.ftab, d_bl, bt.ns, (const RT *)d.meanu, (const RT *)d.meanv,
                     (RT *)FBl, ldw, nchunk);
      g_pt.stop(ivl, s);
      return 0;
    }
    int iv = g_pt.start(0, s);
    {
      long long nblk = (long long)P.wrows_total * ((bfpad_b + 255) / 256);
      EMI_LAUNCH_P(P.esz, k_prepack_inv, nblk, 256, 0, s, P.g, d_bl, bt.ns, bfpad_b, (RT *)P.d_W, ldw, (long long)P.wrows_total);
    }
    g_pt.stop(iv, s);
    iv = g_pt.start(1, s);
    LegMaps *lmaps = bt.maps;
    // (the wide tiles first: they are the longest of the call)
    if (lmaps->n_inv_wide > 0)
      EMI_LAUNCH(emi_f32::k_leg_inv_wide, lmaps->n_inv_wide, LG_THREADS, LG_LDS_BYTES + 512, s, P.g, (const int2 *)lmaps->d_inv_wide, (const float *)P.d_W, ldw, (float *)FBl, ldw);
    if (lmaps->n_inv > 0)
      EMI_LAUNCH_P(P.esz, k_leg_inv, lmaps->n_inv, LG_THREADS, LG_LDS_BYTES + 512, s, P.g, (const int2 *)lmaps->d_inv, (const RT *)P.d_W, ldw, (RT *)FBl, ldw);
    g_pt.stop(iv, s);
    return 0;
  };
  // stream B: FFTs
  auto fft = [&](const Batch &bt, emi_stream_t s, char *, char *FBf, auto &&done) -> int {
    EmiRange rgf(EMI_LBL_FTINV);  // GSTATS 107: FOURIER_IN + FSC + FTINV + TRLTOG
    const int iv = g_pt.start(2, s);
    if (launch_fft(P, true, adj, (const GridFld *)((char *)P.d_desc + bt.off_g), bt.ng, FBf, bt.ldw, nproma, s)) return EMI_ERR_RUNTIME;
    g_pt.stop(iv, s);
    done();
    return 0;
  };
  return run_batches(P, d.stream, true, depth > 1 && nbat > 1, bfpad, bats, hdesc, legendre, fft);
}

// DIR_TRANS, and INV_TRANSAD when adj: the adjoint of INV_TRANS is the same grid -> spectral pipeline
// without the Gaussian weight and the 1/NLOEN (ftinvad_mod.F90:77-83: "change of metric") and with the
// adjoint of VDTUV (= -RLAPIN x UVTVD) in place of UVTVD.  INV_TRANSAD with derivative / vorticity / divergence inputs: the grid
// arrays have INV_TRANS's layout (inv_trans.F90:352-387).
static int dir_pipeline(Plan &P, const Call &d, const Fields &f, const std::vector<GridRef> &gl, int nproma, bool adj) {
  const size_t ns2 = P.nspec2;
  const int nuv = f.nuv, nsc = (int)f.sc.size();
  // Fourier-space fields: u(nuv) v(nuv) scalars (dir_trans.F90:301, ftdir_ctl_mod.F90); INV_TRANSAD with options adds
  // the grid vorticity / divergence, the N-S derivatives of the scalars and the E-W derivatives as further fields
  // field numbers: u_i = i, v_i = nuv + i, scalar_j = 2 nuv + j (as DIR_TRANS), then the adjoint-only inputs
  std::vector<GridFld> gin;
  std::vector<int> num[GF_N];  // the field number of every member of a group (-1: absent)
  for (int grp = 0; grp < GF_N; grp++) num[grp].assign(gf_uv(grp) ? nuv : nsc, -1);
  for (int grp : {GF_U, GF_V, GF_SC, GF_VOR, GF_DIV, GF_UEW, GF_VEW, GF_NSD, GF_SCEW})
    for (const GridRef &r : gl)
      if (r.grp == grp) {
        num[grp][r.i] = (int)gin.size();
        gin.push_back(r.g);
      }
  const int kf_total = (int)gin.size();
  // batches of whole atoms: {u_i, v_i [, their adjoint-only companions]} and {scalar_j [, its N-S and E-W inputs]}
  const int natoms = nuv + nsc;
  const int depth = pipeline_depth(P, kf_total);
  const int cap = pick_batch(P, kf_total, depth);
  std::vector<std::vector<int>> batches;  // Fourier field indices
  {
    std::vector<int> cur;
    for (int at = 0; at < natoms; at++) {
      std::vector<int> fl;
      if (at < nuv) {
        fl = {at, nuv + at};
        for (int x : {num[GF_VOR][at], num[GF_DIV][at], num[GF_UEW][at], num[GF_VEW][at]})
          if (x >= 0) fl.push_back(x);
      } else {
        fl = {2 * nuv + (at - nuv)};
        for (int x : {num[GF_NSD][at - nuv], num[GF_SCEW][at - nuv]})
          if (x >= 0) fl.push_back(x);
      }
      if (!cur.empty() && (int)(cur.size() + fl.size()) > cap) {
        batches.push_back(cur);
        cur.clear();
      }
      cur.insert(cur.end(), fl.begin(), fl.end());
    }
    if (!cur.empty()) batches.push_back(cur);
  }
  int maxb = 0;
  for (auto &b : batches) maxb = std::max(maxb, (int)b.size());
  const int bfpad = roundup(maxb, 64);  // every batch has its own row width (2 x its fields rounded up to 64)
  const bool fuse_dir = !(test_paths() & 4) && !P.lam;  // plain-copy fields leave k_leg_dir's epilogue straight for the caller's arrays
  // EINV_TRANSAD: k_lam_dir_ad holds whole atoms in its work array -- {u, v [, vor] [, div]} and {scalar [, N-S input]}, the E-W inputs
  // folded into their base fields.  An atom larger than the fields per workgroup of the handle takes a larger work array where the
  // LDS holds one.
  const bool lam_ad = P.lam && adj;
  int lam_cap = P.lamdev.fbk;
  size_t lam_lds = P.lam_lds;
  if (lam_ad) {
    const size_t per_field = P.lam_lds / P.lamdev.fbk;
    const int need = std::max(nuv ? 2 + (f.vorgp ? 1 : 0) + (f.divgp ? 1 : 0) : 0, nsc ? 1 + (f.scders ? 1 : 0) : 0);
    if (need > lam_cap) {
      if (need * per_field > 160 * 1024)
        EMI_FAIL(EMI_ERR_UNSUPPORTED,
                 "EINV_TRANSAD: LDVORGP / LDDIVGP WITH KDGL = %d: A WIND FIELD NEEDS %d FIELDS OF %zu BYTES IN ONE WORK ARRAY, THE LDS HOLDS 160 KIB (LDVORGP NEEDS 4 "
                 "FIELDS, LDDIVGP ALONE 3, NEITHER 2)",
                 P.ndgl, need, per_field);
      lam_cap = need, lam_lds = need * per_field;
    }
  }
  const int lam_nthr = std::min(512, fft_threads(lam_lds));
  std::vector<Batch> bats;
  std::vector<char> hdesc;
  for (auto &b : batches) {
    std::vector<GridFld> bg;
    std::vector<SpecDst> bo;
    std::vector<FuseDst> bf(bfpad, FuseDst{nullptr, 0, 0});  // per W field of the batch
    std::map<int, int> loc;
    for (size_t i = 0; i < b.size(); i++) {
      loc[b[i]] = (int)i;
      bg.push_back(gin[b[i]]);
    }
    auto at_ = [&](int x) { return x >= 0 ? loc[x] : -1; };  // field number -> position in this batch's W
    std::vector<LamSlot> bsl;
    std::vector<int> bcs;
    if (lam_ad) {  // the slots of the batch, atom by atom, and the chunks of whole atoms; loc: field number -> slot from here on
      std::map<int, int> sloc;
      auto slot = [&](int fn, int few) {
        if (fn < 0) return;
        sloc[fn] = (int)bsl.size();
        bsl.push_back(LamSlot{loc[fn], at_(few)});
      };
      bcs.push_back(0);
      for (size_t i = 0; i < b.size(); i++) {
        const int fn = b[i], n0 = (int)bsl.size();
        if (fn < nuv) {
          slot(fn, num[GF_UEW][fn]), slot(nuv + fn, num[GF_VEW][fn]), slot(num[GF_VOR][fn], -1), slot(num[GF_DIV][fn], -1);
        } else if (fn >= 2 * nuv && fn < 2 * nuv + nsc) {
          slot(fn, num[GF_SCEW][fn - 2 * nuv]), slot(num[GF_NSD][fn - 2 * nuv], -1);
        }
        if ((int)bsl.size() - bcs.back() > lam_cap) bcs.push_back(n0);
      }
      bcs.push_back((int)bsl.size());
      for (size_t i = 0; i < b.size(); i++) {  // (the E-W inputs have no slot: they are not sources any more)
        auto it = sloc.find(b[i]);
        loc[b[i]] = it == sloc.end() ? -1 : it->second;
      }
    }
    for (size_t i = 0; i < b.size(); i++) {
      int fn = b[i];
      if (fn < nuv) {  // u_i -> vor_i and div_i outputs
        SpecDst v{};
        v.dst = d.spvor; v.stride = d.nf_uv; v.idx = fn; v.kind = adj ? SPO_VOR_AD : SPO_VOR; v.src0 = loc[fn]; v.src1 = loc[nuv + fn];
        v.src2 = at_(num[GF_UEW][fn]); v.src3 = at_(num[GF_VEW][fn]); v.src4 = at_(num[GF_VOR][fn]);
        bo.push_back(v);
        v.dst = d.spdiv; v.kind = adj ? SPO_DIV_AD : SPO_DIV; v.src4 = at_(num[GF_DIV][fn]);
        bo.push_back(v);
      } else if (fn >= 2 * nuv && fn < 2 * nuv + nsc) {
        const int isc = fn - 2 * nuv;
        const ScalarRef &r = f.sc[isc];
        SpecDst sd{};
        sd.kind = SPO_COPY; sd.src0 = loc[fn]; sd.src1 = sd.src2 = sd.src3 = sd.src4 = -1;
        switch (r.arr) {
          case 0: sd.dst = d.spscalar; sd.stride = d.nf_scalar; sd.idx = r.lev; break;
          case 1: sd.dst = d.spsc2; sd.stride = d.nf_sc2; sd.idx = r.lev; break;
          case 2: sd.dst = (char *)d.spsc3a + (size_t)r.var * ns2 * d.sc3a_nlev * P.esz; sd.stride = d.sc3a_nlev; sd.idx = r.lev; break;
          default: sd.dst = (char *)d.spsc3b + (size_t)r.var * ns2 * d.sc3b_nlev * P.esz; sd.stride = d.sc3b_nlev; sd.idx = r.lev; break;
        }
        if (f.scders) {  // value + adjoint of SPNSDE on the N-S input + (-i m) x the E-W input: k_postpack_dir
          sd.kind = SPO_SC_AD; sd.src1 = at_(num[GF_NSD][isc]); sd.src2 = at_(num[GF_SCEW][isc]);
          bo.push_back(sd);
        } else if (fuse_dir) {
          bf[i] = FuseDst{sd.dst, sd.stride, sd.idx};  // written by the epilogue of k_leg_dir
        } else {
          bo.push_back(sd);
        }
      }
    }
    Batch bt{};
    bt.ldw = 2 * roundup((int)b.size(), 64);
    bt.ntiles = ((int)b.size() + 63) / 64;  // per batch: only the column tiles that hold fields (as INV_TRANS)
    bt.ng = (int)bg.size(), bt.off_g = append_desc(hdesc, bg.data(), bg.size());
    bt.ns = (int)bo.size(), bt.off_s = append_desc(hdesc, bo.data(), bo.size());
    bt.off_f = append_desc(hdesc, bf.data(), bf.size());
    if (lam_ad) {
      bt.off_l = append_desc(hdesc, bsl.data(), bsl.size());
      bt.off_c = append_desc(hdesc, bcs.data(), bcs.size());
      bt.nchunk = (int)bcs.size() - 1;
    }
    bats.push_back(bt);
  }
  // stream B: FFTs
  auto fft = [&](const Batch &bt, emi_stream_t s, char *, char *FBf) -> int {
    EmiRange rg(EMI_LBL_FTDIR);  // GSTATS 106: TRGTOL + FTDIR + FOURIER_OUT
    const int iv = g_pt.start(2, s);
    if (launch_fft(P, false, adj, (const GridFld *)((char *)P.d_desc + bt.off_g), bt.ng, FBf, bt.ldw, nproma, s)) return EMI_ERR_RUNTIME;
    g_pt.stop(iv, s);
    return 0;
  };
  // stream A: Legendre + spectral unpack
  auto legendre = [&](const Batch &bt, emi_stream_t s, char *FBl, char *, auto &&done) -> int {
    EmiRange rgl(EMI_LBL_LTDIR);  // GSTATS 103: PRFI2B + LEDIR + UVTVD + UPDSP
    const int ldw = bt.ldw;  // this batch's row width
    const long long lrows_call = P.nproc > 1 ? P.lrows : P.frows;
    if (P.lam) {
      // limited-area handle: EPRFI2B + ELEDIR + EUVTVD + EUPDSP in one kernel, from the Fourier buffer to the caller's arrays (bt.ns outputs
      // in the order of their source fields, bt.ng fields in the buffer); timed in the Legendre slot
      const int nchunk = (bt.ng + P.lamdev.fbk - 1) / P.lamdev.fbk;
      const int ivl = g_pt.start(1, s);
      if (lam_ad)
        EMI_LAUNCH_P(P.esz, k_lam_dir_ad, (long long)P.nump * bt.nchunk, lam_nthr, lam_lds, s, P.g, P.lamdev, P.ftab, (const SpecDst *)((char *)P.d_desc + bt.off_s), bt.ns,
                     (const LamSlot *)((char *)P.d_desc + bt.off_l), (const int *)((char *)P.d_desc + bt.off_c), (RT *)d.meanu, (RT *)d.meanv, (const RT *)FBl, ldw, bt.nchunk);
      else
        EMI_LAUNCH_P(P.esz, k_lam_dir, (long long)P.nump * nchunk, P.lam_nthr, P.lam_lds, s, P.g, P.lamdev, P.ftab, (const SpecDst *)((char *)P.d_desc + bt.off_s), bt.ns, bt.ng,
                     (RT *)d.meanu, (RT *)d.meanv, (const RT *)FBl, ldw, nchunk);
      g_pt.stop(ivl, s);
      done();
      return 0;
    }
    int iv = g_pt.start(1, s);
    // the zero row of this batch: row `lrows_call` in the batch's own row width (the buffer held other data before)
    emi_dev_memset(FBl + (size_t)lrows_call * ldw * P.esz, 0, (size_t)ldw * P.esz, s);
    const FuseDst *d_bf = fuse_dir ? (const FuseDst *)((char *)P.d_desc + bt.off_f) : nullptr;
    LegMaps *lmaps = bt.maps;
    if (lmaps->n_dir_wide > 0)  // (the double-precision tiles first: they are the longest of the call)
      EMI_LAUNCH(emi_f32::k_leg_dir_wide, lmaps->n_dir_wide, LG_THREADS, leg_dir_lds_bytes(P), s, P.g, (const int2 *)lmaps->d_dir_wide, (const float *)FBl, (int)lrows_call, ldw, (float *)P.d_W, ldw,
                 d_bf);
    if (lmaps->n_dir > 0)
      EMI_LAUNCH_P(P.esz, k_leg_dir, lmaps->n_dir, LG_THREADS, leg_dir_lds_bytes(P), s, P.g, (const int2 *)lmaps->d_dir, (const RT *)FBl, (int)lrows_call, ldw, (RT *)P.d_W, ldw, d_bf);
    g_pt.stop(iv, s);
    done();
    iv = g_pt.start(0, s);
    if (bt.ns > 0) {  // vorticity / divergence from the wind fields left in W
      const SpecDst *d_bo = (const SpecDst *)((char *)P.d_desc + bt.off_s);
      long long nblk = ((long long)P.wrows_total + 3) / 4 * ((bt.ns + 63) / 64);  // block = 4 rows x 64 fields
      EMI_LAUNCH_P(P.esz, k_postpack_dir, nblk, 256, 0, s, P.g, d_bo, bt.ns, (const RT *)P.d_W, ldw, (long long)P.wrows_total);
    }
    g_pt.stop(iv, s);
    return 0;
  };
  return run_batches(P, d.stream, false, depth > 1 && batches.size() > 1, bfpad, bats, hdesc, fft, legendre);
}

// The transform of the fields of one W-set (all fields without V-sets): checks, staging, the pipeline of the direction
static int wset_transform(Plan &P, const Call &c, bool inverse, bool adj, const char *who) {
  Fields f;
  if (account(c, who, inverse, nullptr, f)) return EMI_ERR_ARG;
  if (f.if_gp == 0) return EMI_SUCCESS;
  const int nproma = c.kproma > 0 ? c.kproma : P.ngptot;
  const int ngpblks = (P.ngptot - 1) / nproma + 1;
  int uv_dim3 = f.nvar_uv;
  if (check_extents(who, c, P.nspec2, nproma, ngpblks, f.nuv, f.nvar_uv, f.dmul, &uv_dim3)) return EMI_ERR_ARG;
  if (set_lds_attrs()) return EMI_ERR_RUNTIME;
  const emi_stream_t st = c.stream;
  if (plan_begin(P, st)) return EMI_ERR_RUNTIME;
  const bool host = c.mem_space == EMI_MEM_HOST;
  HostStage hs(P.esz);
  const size_t gsz = (size_t)nproma * ngpblks;
  const bool gpad = gsz != (size_t)P.ngptot;  // last NPROMA block padded: those elements are not written
  Call d;
  int rc = stage(P, hs, c, who, inverse, host && f.nuv, f, gsz, gpad, uv_dim3, d);
  if (rc == EMI_SUCCESS && P.lam && f.nuv > 0) {
    // PMEANU / PMEANV travel with the arrays, or are host arrays beside device-resident fields (a Fortran caller's small dummies): each is
    // staged where it is in host memory.  The direct transform fills them on the task that owns m = 0 and leaves them alone elsewhere.
    const bool hu = host || emi_ptr_space(c.meanu) == EMI_MEM_HOST, hv = host || emi_ptr_space(c.meanv) == EMI_MEM_HOST;
    d.meanu = inverse ? (void *)hs.in(c.meanu, f.nuv, hu, st) : hs.out(c.meanu, f.nuv, hu, true, st);
    d.meanv = inverse ? (void *)hs.in(c.meanv, f.nuv, hv, st) : hs.out(c.meanv, f.nuv, hv, true, st);
    if (hs.failed) rc = EMI_ERR_RUNTIME;
  }
  if (rc == EMI_SUCCESS) {
    std::vector<GridRef> gl;
    grid_fields(f, d, uv_dim3, gl);
    if (P.lam)  // plane geometry: no 1 / (a cos) on u, v and the N-S derivatives, one factor i m EXWN on every E-W derivative
      for (GridRef &r : gl) r.g.mode = r.g.mode == GM_ACOS ? GM_PLAIN : (r.g.mode == GM_EWDER_UV ? GM_EWDER : r.g.mode);
    rc = inverse ? inv_pipeline(P, d, f, gl, nproma, adj) : dir_pipeline(P, d, f, gl, nproma, adj);
  }
  if (plan_end(P, st) && rc == EMI_SUCCESS) rc = EMI_ERR_RUNTIME;
  if (rc != EMI_SUCCESS) return rc;
  if (host || !hs.outs.empty()) hs.flush(st);  // (outputs beside device-resident arrays: the host means of EDIR_TRANS)
#ifndef EMI_CPU_EMU
  EMI_CHECK(hipGetLastError());
#endif
  return EMI_SUCCESS;
}

// With emi_set_profile(1) the kernel of a SPECNORM call (k_specnorm, k_specnorm_met) is bracketed by events on the null stream, and
// emi_specnorm_last_ms gives the device time of the last call's kernel alone (tools/specnorm_met_rate.py).
static double g_specnorm_ms = 0.0;
struct SpecnormTimer {
#ifndef EMI_CPU_EMU
  hipEvent_t e0 = nullptr, e1 = nullptr;
  void start() {
    if (G.profile == 0 || hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return;
    (void)hipEventRecord(e0, (hipStream_t)0);
  }
  void stop() {
    if (e1) (void)hipEventRecord(e1, (hipStream_t)0);
  }
  ~SpecnormTimer() {  // (the stream has been synchronised)
    float ms = 0.f;
    if (e1 && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) g_specnorm_ms = ms;
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
#else
  void start() {}
  void stop() {}
#endif
};
extern "C" int emi_specnorm_last_ms(double *ms) {
  if (!ms) EMI_FAIL(EMI_ERR_ARG, "emi_specnorm_last_ms: bad arguments");
  *ms = g_specnorm_ms;
  return EMI_SUCCESS;
}

static int specnorm_sumsq(Plan &P, int mem_space, const void *spec, int nfld, double *sumsq) {
  if (resolve_space("SPECNORM", mem_space, {spec}, &mem_space)) return EMI_ERR_ARG;
  SpecnormTimer tm;
  HostStage hs(P.esz);
  // SPECNORM has no stream argument: it runs on the null stream behind the last transform of this resolution
  // (which may have been queued on a non-blocking stream, e.g. the DIR_TRANS that produced `spec`)
  if (plan_begin(P, (emi_stream_t)0)) return EMI_ERR_RUNTIME;
  const void *d_sp = hs.in(spec, (size_t)P.nspec2 * nfld, mem_space == EMI_MEM_HOST, 0);
  if (hs.failed) EMI_FAIL(EMI_ERR_RUNTIME, "SPECNORM: cannot stage the host array through device memory");
  void *d_out = nullptr;
  if (emi_dev_malloc(&d_out, (size_t)nfld * 8)) return EMI_ERR_RUNTIME;
  tm.start();
  EMI_LAUNCH_P(P.esz, k_specnorm, nfld, 256, 256 * 8, (emi_stream_t)0, P.g, (long long)P.nspec2, (const RT *)d_sp, nfld, (double *)d_out);
  tm.stop();
  emi_d2h(sumsq, d_out, (size_t)nfld * 8, 0);
  emi_stream_sync(0);
  emi_dev_free(d_out);
  return EMI_SUCCESS;
}

// V-sets: the fields of PSPEC are this V-set's (spnorm_ctl_mod.F90: KVSET); their wavenumbers are spread over the NPRTRW tasks that
// share the V-set.  The host collective spans all tasks, and the V-sets may hold different numbers of fields: field counts first,
// then the partial sums; byv[v][k] = sum over the W-sets of field k of V-set v (the same on every task).
static int specnorm_vsets(Plan &P, const double *partial, int nfld, std::vector<std::vector<double>> &byv) {
  if (!G.hc_gather) EMI_FAIL(EMI_ERR_STATE, "SPECNORM: several tasks and no host collectives (emi_set_host_collectives)");
  const int NA = G.nproc_all;
  std::vector<long long> one(NA, 8), d1(NA);
  for (int t = 0; t < NA; t++) d1[t] = 8LL * t;
  std::vector<long long> nf_all(NA, 0);
  long long mine = nfld;
  if (G.hc_gather(G.hc_user, &mine, 8, nf_all.data(), one.data(), d1.data(), NA)) EMI_FAIL(EMI_ERR_RUNTIME, "SPECNORM: all-gather-v failed");
  std::vector<long long> cnt(NA), dsp(NA);
  long long tot = 0;
  for (int t = 0; t < NA; t++) cnt[t] = nf_all[t] * 8, dsp[t] = tot, tot += cnt[t];
  std::vector<double> all((size_t)(tot / 8) + 1);
  double dummy = 0.0;
  if (G.hc_gather(G.hc_user, nfld ? (const void *)partial : (const void *)&dummy, cnt[G.myproc_all - 1], all.data(), cnt.data(), dsp.data(), NA))
    EMI_FAIL(EMI_ERR_RUNTIME, "SPECNORM: all-gather-v failed");
  byv.assign(P.nprv, {});
  for (int v = 0; v < P.nprv; v++) {
    const long long nfv = nf_all[v];  // task (W-set 1, V-set v)
    byv[v].assign((size_t)nfv, 0.0);
    for (int w = 0; w < P.nproc; w++) {
      const int t = w * P.nprv + v;
      if (nf_all[t] != nfv) EMI_FAIL(EMI_ERR_ARG, "SPECNORM: tasks %d and %d of V-set %d pass %lld and %lld fields", v + 1, t + 1, v + 1, nfv, nf_all[t]);
      for (long long i = 0; i < nfv; i++) byv[v][(size_t)i] += all[(size_t)(dsp[t] / 8 + i)];
    }
  }
  return 0;
}

extern "C" int emi_specnorm(int kresol, int mem_space, const void *spec, int nfld, double *norms) {
  Plan *Pp = get_plan(kresol);
  if (!Pp) EMI_FAIL(EMI_ERR_STATE, "SPECNORM: unknown resolution %d", kresol);
  if (Pp->lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: resolution %d is a limited-area handle (ESETUP_TRANS): this routine serves the spherical transforms only", "SPECNORM", kresol);
  // V-sets: a task whose V-set holds none of the fields still takes part in the collective (nfld = 0)
  if (nfld < 0 || (nfld > 0 && (!spec || !norms)) || (nfld == 0 && Pp->nprv == 1)) EMI_FAIL(EMI_ERR_ARG, "SPECNORM: bad arguments");
  if (Pp->nproc > 1 && Pp->nprv == 1 && !G.hc_gather)
    EMI_FAIL(EMI_ERR_STATE, "SPECNORM: several tasks and no host collectives (emi_set_host_collectives): use emi_specnorm_partial and sum over tasks");
  if (nfld > 0) {
    const int rc = specnorm_sumsq(*Pp, mem_space, spec, nfld, norms);
    if (rc) return rc;
  }
  if (Pp->nproc > 1 && Pp->nprv == 1) {  // spnormc_mod.F90:49-85 gathers the partial sums on the master; here every task gets the norms
    const int NP = Pp->nproc;
    std::vector<double> all((size_t)NP * nfld);
    std::vector<long long> cnt(NP, (long long)nfld * 8), dsp(NP);
    for (int t = 0; t < NP; t++) dsp[t] = (long long)t * nfld * 8;
    if (G.hc_gather(G.hc_user, norms, cnt[0], all.data(), cnt.data(), dsp.data(), NP)) EMI_FAIL(EMI_ERR_RUNTIME, "SPECNORM: all-gather-v failed");
    for (int i = 0; i < nfld; i++) {
      double s = 0.0;
      for (int t = 0; t < NP; t++) s += all[(size_t)t * nfld + i];  // task order: the same sum on every task
      norms[i] = s;
    }
  } else if (Pp->nprv > 1) {
    std::vector<std::vector<double>> byv;
    if (specnorm_vsets(*Pp, norms, nfld, byv)) return EMI_ERR_RUNTIME;
    for (int i = 0; i < nfld; i++) norms[i] = byv[Pp->mev][i];
  }
  for (int i = 0; i < nfld; i++) norms[i] = std::sqrt(norms[i]);
  return EMI_SUCCESS;
}

// SPECNORM with KVSET (specnorm.h:12, spnorm_ctl_mod.F90): PSPEC holds this V-set's fields, PNORM the norms of ALL nfld_g fields
// (on every task; the reference fills it on the master), kvset[f] the V-set of global field f
extern "C" int emi_specnorm_kvset(int kresol, int mem_space, const void *spec, int nfld, const int *kvset, int nfld_g, double *norms_g) {
  Plan *Pp = get_plan(kresol);
  if (!Pp) EMI_FAIL(EMI_ERR_STATE, "SPECNORM: unknown resolution %d", kresol);
  if (Pp->lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: resolution %d is a limited-area handle (ESETUP_TRANS): this routine serves the spherical transforms only", "SPECNORM", kresol);
  Plan &P = *Pp;
  if (nfld < 0 || nfld_g < 0 || (nfld_g > 0 && (!kvset || !norms_g)) || (nfld > 0 && !spec)) EMI_FAIL(EMI_ERR_ARG, "SPECNORM: bad arguments");
  int mine = 0;
  for (int f = 0; f < nfld_g; f++) {
    if (kvset[f] < 1 || kvset[f] > P.nprv) EMI_FAIL(EMI_ERR_ARG, "SPECNORM:KVSET CONTAINS VALUES OUTSIDE RANGE");
    mine += kvset[f] == P.mev + 1;
  }
  if (mine != nfld) EMI_FAIL(EMI_ERR_ARG, "SPECNORM: %d fields of KVSET belong to this V-set, PSPEC holds %d", mine, nfld);
  if (P.nprv == 1) return emi_specnorm(kresol, mem_space, spec, nfld, norms_g);
  std::vector<double> part((size_t)nfld + 1, 0.0);
  if (nfld > 0) {
    const int rc = specnorm_sumsq(P, mem_space, spec, nfld, part.data());
    if (rc) return rc;
  }
  std::vector<std::vector<double>> byv;
  if (specnorm_vsets(P, part.data(), nfld, byv)) return EMI_ERR_RUNTIME;
  std::vector<int> k(P.nprv, 0);
  for (int f = 0; f < nfld_g; f++) {
    const int v = kvset[f] - 1;
    if ((size_t)k[v] >= byv[v].size()) EMI_FAIL(EMI_ERR_ARG, "SPECNORM: V-set %d passed fewer fields than KVSET names", v + 1);
    norms_g[f] = std::sqrt(byv[v][(size_t)k[v]++]);
  }
  return EMI_SUCCESS;
}
// V-set decomposition (sump_trans0_mod.F90:49, pe2set_mod.F90:111-112): NPRTRW, NPRTRV, MYSETW, MYSETV
extern "C" int emi_inq_vsets(int *nprtrw, int *nprtrv, int *mysetw, int *mysetv) {
  if (!G.init) EMI_FAIL(EMI_ERR_STATE, "emi_inq_vsets: SETUP_TRANS0 has not been called");
  if (nprtrw) *nprtrw = G.nproc;
  if (nprtrv) *nprtrv = G.nprtrv;
  if (mysetw) *mysetw = G.myproc;
  if (mysetv) *mysetv = G.mysetv;
  return EMI_SUCCESS;
}

// this task's contribution (sum over its wavenumbers of the weighted squares, spnormd_mod.F90);
// the caller sums over tasks and takes the square root (spnormc_mod.F90 gathers to the master)
extern "C" int emi_specnorm_partial(int kresol, int mem_space, const void *spec, int nfld, double *sumsq) {
  Plan *Pp = get_plan(kresol);
  if (!Pp) EMI_FAIL(EMI_ERR_STATE, "SPECNORM: unknown resolution %d", kresol);
  if (Pp->lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: resolution %d is a limited-area handle (ESETUP_TRANS): this routine serves the spherical transforms only", "SPECNORM", kresol);
  if (!spec || nfld <= 0 || !sumsq) EMI_FAIL(EMI_ERR_ARG, "SPECNORM: bad arguments");
  return specnorm_sumsq(*Pp, mem_space, spec, nfld, sumsq);
}

// SPECNORM with PMET (specnorm.h:12, spnorm_ctl_mod.F90, spnormd_mod.F90:36-53): the metric PMET(0:NSMAX) weights the coefficients of
// total wavenumber n.  sums[ml][f], ml over this task's wavenumbers in MYMS order: k_specnorm_met.  pmet: host array of the handle's
// precision with at least NSMAX + 1 elements; it is small and is uploaded with every call.  The unweighted call keeps k_specnorm.
static int specnorm_met_check(int kresol, const void *pmet, int npmet, Plan **Pp) {
  Plan *P = get_plan(kresol);
  if (!P) EMI_FAIL(EMI_ERR_STATE, "SPECNORM: unknown resolution %d", kresol);
  if (P->lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: resolution %d is a limited-area handle (ESETUP_TRANS): this routine serves the spherical transforms only", "SPECNORM", kresol);
  if (P->ldll) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: not available on a handle set up with LDLL (it serves INV_TRANS with LDLATLON only)", "SPECNORM with PMET");
  if (!pmet) EMI_FAIL(EMI_ERR_ARG, "SPECNORM: PMET NOT PRESENT");
  if (npmet < P->nsmax + 1) EMI_FAIL(EMI_ERR_ARG, "SPECNORM: PMET TOO SMALL (%d elements, %d are needed)", npmet, P->nsmax + 1);
  *Pp = P;
  return 0;
}
static int specnorm_met_sums(Plan &P, int mem_space, const void *spec, int nfld, const void *pmet, double *sums) {
  if (resolve_space("SPECNORM", mem_space, {spec}, &mem_space)) return EMI_ERR_ARG;
  if (P.nump == 0 || nfld == 0) return EMI_SUCCESS;
  SpecnormTimer tm;
  HostStage hs(P.esz);
  if (plan_begin(P, (emi_stream_t)0)) return EMI_ERR_RUNTIME;  // the null stream, behind the last transform of this resolution (SPECNORM)
  const void *d_sp = hs.in(spec, (size_t)P.nspec2 * nfld, mem_space == EMI_MEM_HOST, 0);
  if (hs.failed) EMI_FAIL(EMI_ERR_RUNTIME, "SPECNORM: cannot stage the host array through device memory");
  // the sums and the metric live in one buffer of the plan, grown on demand: every call ends synchronised, so the next one may reuse it
  const size_t nout = (size_t)P.nump * nfld, nmet = (size_t)P.nsmax + 1, need = nout * 8 + nmet * P.esz;
  if (need > P.cap_normws) {
    emi_dev_free(P.d_normws);
    P.d_normws = nullptr, P.cap_normws = 0;
    if (emi_dev_malloc(&P.d_normws, need)) return EMI_ERR_RUNTIME;
    P.cap_normws = need;
  }
  void *d_out = P.d_normws, *d_met = (char *)P.d_normws + nout * 8;
  int rc = EMI_SUCCESS;
  if (emi_h2d(d_met, pmet, nmet * P.esz, 0)) {
    rc = EMI_ERR_RUNTIME;
  } else {
    const int ntile = (nfld + 63) / 64;
    tm.start();
    EMI_LAUNCH_P(P.esz, k_specnorm_met, (long long)P.nump * ntile, 256, 3 * 64 * 8, (emi_stream_t)0, P.g.mval, P.g.nasm0, P.nsmax, ntile, (const RT *)d_sp, nfld,
                 (const RT *)d_met, (double *)d_out);
    tm.stop();
    if (emi_d2h(sums, d_out, nout * 8, 0)) rc = EMI_ERR_RUNTIME;
  }
  if (emi_stream_sync(0)) rc = EMI_ERR_RUNTIME;  // (also: the caller's pmet has been read)
  return rc;
}
extern "C" int emi_specnorm_met_partial(int kresol, int mem_space, const void *spec, int nfld, const void *pmet, int npmet, double *sums) {
  Plan *Pp = nullptr;
  if (int rc = specnorm_met_check(kresol, pmet, npmet, &Pp)) return rc;
  if (!spec || nfld <= 0 || !sums) EMI_FAIL(EMI_ERR_ARG, "SPECNORM: bad arguments");
  return specnorm_met_sums(*Pp, mem_space, spec, nfld, pmet, sums);
}
// The per-wavenumber sums of all tasks are gathered and added for m = 0 .. NSMAX in ascending order on every task, as ESPECNORM does:
// the norms do not depend on the number of W-set tasks, and every task gets them.  kvset == NULL: spec holds the nfld fields whose
// norms are wanted (nfld_g is not read).  With kvset (NPRTRV > 1), as emi_specnorm_kvset: spec holds this V-set's fields, norms the
// nfld_g norms of all fields; wavenumber m of a field of V-set v comes from the task (W-set of m, v).
extern "C" int emi_specnorm_met(int kresol, int mem_space, const void *spec, int nfld, const void *pmet, int npmet, const int *kvset, int nfld_g, double *norms) {
  Plan *Pp = nullptr;
  if (int rc = specnorm_met_check(kresol, pmet, npmet, &Pp)) return rc;
  Plan &P = *Pp;
  if (!kvset) nfld_g = nfld;
  if (nfld < 0 || nfld_g < 0 || (nfld > 0 && !spec) || (nfld_g > 0 && !norms) || (nfld == 0 && P.nprv == 1)) EMI_FAIL(EMI_ERR_ARG, "SPECNORM: bad arguments");
  if (kvset) {
    int mine = 0;
    for (int f = 0; f < nfld_g; f++) {
      if (kvset[f] < 1 || kvset[f] > P.nprv) EMI_FAIL(EMI_ERR_ARG, "SPECNORM:KVSET CONTAINS VALUES OUTSIDE RANGE");
      mine += kvset[f] == P.mev + 1;
    }
    if (mine != nfld) EMI_FAIL(EMI_ERR_ARG, "SPECNORM: %d fields of KVSET belong to this V-set, PSPEC holds %d", mine, nfld);
  }
  const int NW = P.nproc, NV = P.nprv, NA = NW * NV, M = P.nsmax;
  if (NA > 1 && !G.hc_gather)
    EMI_FAIL(EMI_ERR_STATE, "SPECNORM: several tasks and no host collectives (emi_set_host_collectives): use emi_specnorm_met_partial and gather the sums");
  std::vector<double> mine((size_t)std::max(P.nump, 1) * std::max(nfld, 1), 0.0), all;
  if (int rc = specnorm_met_sums(P, mem_space, spec, nfld, pmet, mine.data())) return rc;
  std::vector<int> lidx(M + 1, 0), numpp(NW, 0);
  for (int m = 0; m <= M; m++) lidx[m] = numpp[P.procm[m]]++;
  // task t = w * NPRTRV + v (specnorm_vsets); the V-sets may hold different numbers of fields: field counts first, then the sums
  std::vector<long long> nf_all(NA, nfld), cnt(NA, 0), dsp(NA, 0);
  const double *base = mine.data();
  if (NA > 1) {
    const int me = NV > 1 ? G.myproc_all - 1 : P.me;
    if (NV > 1) {
      std::vector<long long> one(NA, 8), d1(NA);
      for (int t = 0; t < NA; t++) d1[t] = 8LL * t;
      long long nf = nfld;
      if (G.hc_gather(G.hc_user, &nf, 8, nf_all.data(), one.data(), d1.data(), NA)) EMI_FAIL(EMI_ERR_RUNTIME, "SPECNORM: all-gather-v failed");
    }
    long long tot = 0;
    for (int t = 0; t < NA; t++) cnt[t] = 8LL * numpp[t / NV] * nf_all[t], dsp[t] = tot, tot += cnt[t];
    all.resize((size_t)(tot / 8) + 1);
    if (G.hc_gather(G.hc_user, mine.data(), cnt[me], all.data(), cnt.data(), dsp.data(), NA)) EMI_FAIL(EMI_ERR_RUNTIME, "SPECNORM: all-gather-v failed");
    base = all.data();
  }
  // the squared norm of field k of V-set v
  auto sumsq = [&](int v, long long k) {
    double s = 0.0;
    for (int m = 0; m <= M; m++) {
      const int t = P.procm[m] * NV + v;
      s += base[(size_t)(dsp[t] / 8) + (size_t)lidx[m] * (size_t)nf_all[t] + (size_t)k];
    }
    return s;
  };
  for (int v = 0; v < NV; v++)
    for (int w = 1; w < NW; w++)
      if (nf_all[w * NV + v] != nf_all[v])
        EMI_FAIL(EMI_ERR_ARG, "SPECNORM: tasks %d and %d of V-set %d pass %lld and %lld fields", v + 1, w * NV + v + 1, v + 1, nf_all[v], nf_all[w * NV + v]);
  if (!kvset) {
    for (int f = 0; f < nfld; f++) norms[f] = std::sqrt(sumsq(NV > 1 ? P.mev : 0, f));
    return EMI_SUCCESS;
  }
  std::vector<long long> k(NV, 0);
  for (int f = 0; f < nfld_g; f++) {
    const int v = kvset[f] - 1;
    if (k[v] >= nf_all[v]) EMI_FAIL(EMI_ERR_ARG, "SPECNORM: V-set %d passed fewer fields than KVSET names", v + 1);
    norms[f] = std::sqrt(sumsq(v, k[v]++));
  }
  return EMI_SUCCESS;
}

// ESPECNORM (etrans/cpu/external/especnorm.F90, internal/espnorm_ctl_mod.F90, espnormd_mod.F90): the spectral norms of a limited-area
// handle.  sums[ml][f], ml over this task's wavenumbers in MYMS order: k_especnorm.  pmet: host array of the handle's precision, read
// zero-based at NPME(m) + n (element 0 is never read), or NULL for weights of 1; it is small and is uploaded with every call.
static int especnorm_check(const char *who, int kresol, const void *spec, int nfld, const void *pmet, int npmet, const void *out, Plan **Pp) {
  Plan *P = get_plan(kresol);
  if (!P) EMI_FAIL(EMI_ERR_STATE, "%s: unknown resolution %d", who, kresol);
  if (!P->lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: resolution %d is not a limited-area handle: it was not set up by ESETUP_TRANS", who, kresol);
  if (nfld <= 0 || !spec) EMI_FAIL(EMI_ERR_ARG, "ESPECNORM: PSPEC NOT PRESENT");
  if (!out) EMI_FAIL(EMI_ERR_ARG, "ESPECNORM: PNORM NOT PRESENT");
  if (pmet && npmet < 1 + P->nspec2g / 4)  // NPME(KMSMAX) + KNTMP(KMSMAX) + 1
    EMI_FAIL(EMI_ERR_ARG, "ESPECNORM: PMET TOO SMALL (%d elements, %d are needed)", npmet, 1 + P->nspec2g / 4);
  *Pp = P;
  return 0;
}
static int especnorm_sums(Plan &P, int mem_space, const void *spec, int nfld, const void *pmet, int npmet, double *sums) {
  if (resolve_space("ESPECNORM", mem_space, {spec}, &mem_space)) return EMI_ERR_ARG;
  if (P.nump == 0) return EMI_SUCCESS;
  HostStage hs(P.esz);
  if (plan_begin(P, (emi_stream_t)0)) return EMI_ERR_RUNTIME;  // the null stream, behind the last transform of this resolution (SPECNORM)
  const void *d_sp = hs.in(spec, (size_t)P.nspec2 * nfld, mem_space == EMI_MEM_HOST, 0);
  if (hs.failed) EMI_FAIL(EMI_ERR_RUNTIME, "ESPECNORM: cannot stage the host array through device memory");
  void *d_out = nullptr, *d_met = nullptr;
  const size_t nout = (size_t)P.nump * nfld;
  int rc = EMI_SUCCESS;
  if (emi_dev_malloc(&d_out, nout * 8) || (pmet && (emi_dev_malloc(&d_met, (size_t)npmet * P.esz) || emi_h2d(d_met, pmet, (size_t)npmet * P.esz, 0)))) {
    rc = EMI_ERR_RUNTIME;
  } else {
    const int ntile = (nfld + 63) / 64;
    EMI_LAUNCH_P(P.esz, k_especnorm, (long long)P.nump * ntile, 256, 3 * 64 * 8, (emi_stream_t)0, P.lamdev.kntmp, P.lamdev.nesm0, P.d_npme, ntile, (const RT *)d_sp, nfld,
                 (const RT *)d_met, (double *)d_out);
    if (emi_d2h(sums, d_out, nout * 8, 0)) rc = EMI_ERR_RUNTIME;
  }
  if (emi_stream_sync(0)) rc = EMI_ERR_RUNTIME;  // (also: the caller's pmet has been read)
  emi_dev_free(d_out);
  emi_dev_free(d_met);
  return rc;
}
extern "C" int emi_especnorm_partial(int kresol, int mem_space, const void *spec, int nfld, const void *pmet, int npmet, double *sums) {
  Plan *Pp = nullptr;
  if (int rc = especnorm_check("ESPECNORM", kresol, spec, nfld, pmet, npmet, sums, &Pp)) return rc;
  return especnorm_sums(*Pp, mem_space, spec, nfld, pmet, npmet, sums);
}
// The per-wavenumber sums of all tasks are gathered (SPNORMC) and added for m = 0 .. KMSMAX in ascending order on every task, the
// reference's SUM(ZGM,DIM=2) (espnorm_ctl_mod.F90:64-69): the norms do not depend on the number of tasks, and every task gets them.
extern "C" int emi_especnorm(int kresol, int mem_space, const void *spec, int nfld, const void *pmet, int npmet, double *norms) {
  Plan *Pp = nullptr;
  if (int rc = especnorm_check("ESPECNORM", kresol, spec, nfld, pmet, npmet, norms, &Pp)) return rc;
  Plan &P = *Pp;
  const int NP = P.nproc, M = P.nsmax;
  if (NP > 1 && !G.hc_gather)
    EMI_FAIL(EMI_ERR_STATE, "ESPECNORM: several tasks and no host collectives (emi_set_host_collectives): use emi_especnorm_partial and gather the sums");
  std::vector<double> mine((size_t)std::max(P.nump, 1) * nfld, 0.0), all;
  if (int rc = especnorm_sums(P, mem_space, spec, nfld, pmet, npmet, mine.data())) return rc;
  std::vector<long long> cnt(NP, 0), dsp(NP, 0);
  std::vector<int> lidx(M + 1, 0), numpp(NP, 0);
  for (int m = 0; m <= M; m++) lidx[m] = numpp[P.procm[m]]++;
  const double *base = mine.data();
  if (NP > 1) {
    long long tot = 0;
    for (int t = 0; t < NP; t++) cnt[t] = 8LL * numpp[t] * nfld, dsp[t] = tot, tot += cnt[t];
    all.resize((size_t)(tot / 8));
    if (G.hc_gather(G.hc_user, mine.data(), cnt[P.me], all.data(), cnt.data(), dsp.data(), NP)) EMI_FAIL(EMI_ERR_RUNTIME, "ESPECNORM: all-gather-v failed");
    base = all.data();
  }
  for (int f = 0; f < nfld; f++) {
    double s = 0.0;
    for (int m = 0; m <= M; m++) s += base[(size_t)(dsp[P.procm[m]] / 8) + (size_t)lidx[m] * nfld + f];
    norms[f] = std::sqrt(s);
  }
  return EMI_SUCCESS;
}

// GPNORM_TRANS (cpu/external/gpnorm_trans.F90:11-96, cpu/internal/gpnorm_trans_ctl_mod.F90): area-weighted average, minimum and maximum of
// `kfields` grid fields of PGP(nproma, gp_nfld, ngpblks).  Per latitude the sum over the longitudes in double times RW / NLOEN on the
// task that holds the latitude (whole latitudes here, so the reference's TRGTOL is not needed); the per-latitude values of all tasks
// are gathered and summed in latitude order on every task (the reference: on task 1), so the average does not depend on the
// decomposition.  ave_only (LDAVE_ONLY): pmin / pmax come in as the caller's local extrema and are only reduced over the tasks.
// Host arrays are staged whole (all gp_nfld fields of PGP, although only the first kfields are reduced): a diagnostic, not a hot path.
// The rows, their weights RW and their lengths come from the plan: Gaussian latitudes and weights (GPNORM_TRANS), or the NDGL rows of a
// limited-area handle, extension zone included, with RW = 1 / NDGL (EGPNORM_TRANS, etrans/cpu/external/egpnorm_trans.F90:94-97).
static int gpnorm_impl(Plan &P, const char *who, int mem_space, const void *gp, int gp_nfld, int kfields, int kproma, double *ave, double *pmin, double *pmax,
                       int ave_only) {
  if (kfields <= 0 || !gp || !ave || !pmin || !pmax) EMI_FAIL(EMI_ERR_ARG, "%s: bad arguments", who);
  if (gp_nfld < kfields) EMI_FAIL(EMI_ERR_ARG, "GPNORM_TRANS_CTL:SECOND DIMENSION OF PGP TOO SMALL (%d < %d)", gp_nfld, kfields);
  if (G.nproc_all > 1 && !G.hc_gather) EMI_FAIL(EMI_ERR_STATE, "%s: several tasks and no host collectives (emi_set_host_collectives)", who);
  if (resolve_space(who, mem_space, {gp}, &mem_space)) return EMI_ERR_ARG;
  const int j0 = P.vfirst(P.me, P.mev), j1 = P.vlast(P.me, P.mev), nl = j1 - j0;
  std::vector<int> rowoff(nl + 1, 0);
  for (int j = 0; j < nl; j++) rowoff[j + 1] = rowoff[j] + P.nloen[j0 + j];
  const long long myp = rowoff[nl];
  const int nproma = kproma > 0 ? kproma : (int)std::max<long long>(myp, 1);
  const long long ngpblks = myp > 0 ? (myp - 1) / nproma + 1 : 0;
  std::vector<double> loc((size_t)3 * kfields * std::max(nl, 1), 0.0);
  int lerr = 0;
  if (nl > 0) {
    HostStage hs(P.esz);
    if (plan_begin(P, (emi_stream_t)0)) return EMI_ERR_RUNTIME;  // behind the transform that produced the fields
    const void *d_gp = hs.in(gp, (size_t)nproma * gp_nfld * ngpblks, mem_space == EMI_MEM_HOST, 0);
    int *d_off = nullptr;
    void *d_out = nullptr;
    // a local failure must not leave the other tasks waiting in the gather below: it travels as a status word of this task's block
    if (hs.failed || upload(rowoff, &d_off) || emi_dev_malloc(&d_out, loc.size() * 8)) {
      lerr = 1;
    } else {
      EMI_LAUNCH_P(P.esz, k_gpnorm, (long long)nl * kfields, 256, 3 * 256 * 8, (emi_stream_t)0, (const int *)d_off, nl, (const RT *)d_gp, gp_nfld, kfields, nproma,
                   (double *)d_out);
      if (emi_d2h(loc.data(), d_out, loc.size() * 8, 0) || emi_stream_sync(0)) lerr = 1;
    }
    emi_dev_free(d_off);
    emi_dev_free(d_out);
  }
  // this task's block: [field][latitude] RW / NLOEN x row sums, then the field minima and maxima, then the status word
  const size_t nn = (size_t)kfields * nl;
  std::vector<double> blk(nn + 2 * (size_t)kfields + 1);
  blk.back() = (double)lerr;
  for (int f = 0; f < kfields; f++) {
    double mn = ave_only ? pmin[f] : 0.0, mx = ave_only ? pmax[f] : 0.0;
    for (int j = 0; j < nl; j++) {
      const double rwj = P.esz == 4 ? (double)(float)P.rw[j0 + j] : P.rw[j0 + j];  // REAL(PW(IGL),JPRB), gpnorm_trans_ctl_mod.F90:206
      blk[(size_t)f * nl + j] = loc[(size_t)f * nl + j] * rwj / (double)P.nloen[j0 + j];
      if (!ave_only) {
        const double a = loc[nn + (size_t)f * nl + j], b = loc[2 * nn + (size_t)f * nl + j];
        mn = j == 0 ? a : std::min(mn, a), mx = j == 0 ? b : std::max(mx, b);
      }
    }
    blk[nn + f] = mn, blk[nn + kfields + f] = mx;
  }
  const int NA = G.nproc_all;
  std::vector<double> all;
  std::vector<long long> cnt(NA, 0), dsp(NA, 0);
  std::vector<int> nlat_of(NA, 0);
  if (NA > 1) {
    long long tot = 0;
    for (int w = 0; w < P.nproc; w++)
      for (int v = 0; v < P.nprv; v++) {
        const int t = w * P.nprv + v;
        nlat_of[t] = P.vlast(w, v) - P.vfirst(w, v);
        cnt[t] = 8LL * ((long long)kfields * nlat_of[t] + 2 * kfields + 1), dsp[t] = tot, tot += cnt[t];
      }
    all.resize((size_t)(tot / 8));
    if (G.hc_gather(G.hc_user, blk.data(), cnt[G.myproc_all - 1], all.data(), cnt.data(), dsp.data(), NA)) EMI_FAIL(EMI_ERR_RUNTIME, "%s: all-gather-v failed", who);
  } else {
    nlat_of[0] = nl, cnt[0] = 8LL * (long long)blk.size();
    all = blk;
  }
  for (int t = 0; t < NA; t++)
    if (all[(size_t)(dsp[t] / 8) + (size_t)kfields * nlat_of[t] + 2 * (size_t)kfields] != 0.0)
      EMI_FAIL(EMI_ERR_RUNTIME, "%s: task %d could not stage or reduce its fields (no device memory?)", who, t + 1);
  for (int f = 0; f < kfields; f++) {  // latitude order = task order (bands and sub-bands ascend with the task number)
    double a = 0.0, mn = 0.0, mx = 0.0;
    bool first = true;
    for (int t = 0; t < NA; t++) {
      const double *b = all.data() + dsp[t] / 8;
      const int nlt = nlat_of[t];
      for (int j = 0; j < nlt; j++) a += b[(size_t)f * nlt + j];
      if (nlt > 0 || ave_only) {
        const double tmn = b[(size_t)kfields * nlt + f], tmx = b[(size_t)kfields * nlt + kfields + f];
        mn = first ? tmn : std::min(mn, tmn), mx = first ? tmx : std::max(mx, tmx), first = false;
      }
    }
    ave[f] = a, pmin[f] = mn, pmax[f] = mx;
  }
  return EMI_SUCCESS;
}

extern "C" int emi_gpnorm(int kresol, int mem_space, const void *gp, int gp_nfld, int kfields, int kproma, double *ave, double *pmin, double *pmax,
                          int ave_only) {
  Plan *Pp = get_plan(kresol);
  if (!Pp) EMI_FAIL(EMI_ERR_STATE, "GPNORM_TRANS: unknown resolution %d", kresol);
  if (Pp->lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: resolution %d is a limited-area handle (ESETUP_TRANS): this routine serves the spherical transforms only", "GPNORM_TRANS", kresol);
  if (Pp->ldll) EMI_FAIL(EMI_ERR_UNSUPPORTED, "GPNORM_TRANS: not available on a handle set up with LDLL (it keeps no Gaussian weights)");
  return gpnorm_impl(*Pp, "GPNORM_TRANS", mem_space, gp, gp_nfld, kfields, kproma, ave, pmin, pmax, ave_only);
}
// EGPNORM_TRANS: PAVE = sum over all NDGL rows of (1 / NDGL) (row sum) / NDLON; the reference's EGPNORM_OLD variant is not provided
extern "C" int emi_egpnorm(int kresol, int mem_space, const void *gp, int gp_nfld, int kfields, int kproma, double *ave, double *pmin, double *pmax,
                           int ave_only) {
  Plan *Pp = get_plan(kresol);
  if (!Pp) EMI_FAIL(EMI_ERR_STATE, "EGPNORM_TRANS: unknown resolution %d", kresol);
  if (!Pp->lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: resolution %d is not a limited-area handle: it was not set up by ESETUP_TRANS", "EGPNORM_TRANS", kresol);
  return gpnorm_impl(*Pp, "EGPNORM_TRANS", mem_space, gp, gp_nfld, kfields, kproma, ave, pmin, pmax, ave_only);
}

// VORDIV_TO_UV (cpu/external/vordiv_to_uv.F90:11-178): spectral vorticity / divergence -> spectral U = u cos(theta), V = v cos(theta), for the
// wavenumbers of this task's W-set (suwavedi_mod.F90:118-137), n <= KSMAX.  Needs SETUP_TRANS0 only (the reference sets up and releases a
// spectral-only resolution inside the call); precision: 8 or 4 bytes per real of the four arrays PSP*(nfld, nspec2).
extern "C" int emi_vordiv_to_uv(int ksmax, int precision, int mem_space, const void *spvor, const void *spdiv, void *spu, void *spv, int nfld, int nspec2_ext) {
  if (!G.init) EMI_FAIL(EMI_ERR_STATE, "VORDIV_TO_UV: SETUP_TRANS0 has not been called");
  if (ksmax < 0 || (precision != 8 && precision != 4)) EMI_FAIL(EMI_ERR_ARG, "VORDIV_TO_UV: bad arguments (KSMAX = %d, precision = %d)", ksmax, precision);
  if (nfld <= 0) return EMI_SUCCESS;
  if (!spvor || !spdiv || !spu || !spv) EMI_FAIL(EMI_ERR_ARG, "VORDIV_TO_UV : PSPVOR / PSPDIV / PSPU / PSPV MISSING");
  const int N = ksmax, NP = G.nproc, me = G.myproc - 1;
  std::vector<int> mval, nasm0, ebase, pairm;
  std::vector<double> eps, lapin(N + 4, 0.0);
  {
    int ik = 0, ind = 1, ipos = 0;
    for (int m = 0; m <= N; m++) {  // the zig-zag of SETUP_TRANS (suwavedi_mod.F90:118-137)
      ik += ind;
      if (ik > NP) ik = NP, ind = -1;
      else if (ik < 1) ik = 1, ind = 1;
      if (ik - 1 != me) continue;
      const int ml = (int)mval.size();
      mval.push_back(m), nasm0.push_back(ipos), ebase.push_back((int)eps.size());
      for (int n = m; n <= N; n++) pairm.push_back(ml);
      ipos += 2 * (N - m + 1);
      for (int n = m; n <= N + 2; n++) eps.push_back(std::sqrt((double)(n * n - m * m) / (double)(4 * n * n - 1)));  // REPSNM (pre_suleg_mod.F90:55-63)
    }
  }
  for (int n = 1; n <= N + 2; n++) lapin[n + 1] = -(G.ra * G.ra / (double)(n * (n + 1)));  // RLAPIN (pre_suleg_mod.F90:64-69)
  const int nspec2 = 2 * (int)pairm.size();
  if (nspec2 == 0) return EMI_SUCCESS;
  if (nspec2_ext < nspec2)
    EMI_FAIL(EMI_ERR_ARG, "VORDIV_TO_UV:SECOND DIMENSION OF PSPVOR / PSPDIV / PSPU / PSPV TOO SMALL (%d < %d spectral coefficients at KSMAX = %d)", nspec2_ext, nspec2,
             ksmax);
  if (resolve_space("VORDIV_TO_UV", mem_space, {spvor, spdiv, spu, spv}, &mem_space)) return EMI_ERR_ARG;
  HostStage hs(precision);
  const bool host = mem_space == EMI_MEM_HOST;
  const void *d_vor = hs.in(spvor, (size_t)nspec2 * nfld, host, 0), *d_div = hs.in(spdiv, (size_t)nspec2 * nfld, host, 0);
  void *d_u = hs.out(spu, (size_t)nspec2 * nfld, host), *d_v = hs.out(spv, (size_t)nspec2 * nfld, host);
  int *d_pairm = nullptr, *d_mval = nullptr, *d_nasm0 = nullptr, *d_ebase = nullptr;
  double *d_eps = nullptr, *d_lapin = nullptr;
  int rc = EMI_SUCCESS;
  if (hs.failed || upload(pairm, &d_pairm) || upload(mval, &d_mval) || upload(nasm0, &d_nasm0) || upload(ebase, &d_ebase) || upload(eps, &d_eps) ||
      upload(lapin, &d_lapin)) {
    emi_set_error("VORDIV_TO_UV: no device memory");
    rc = EMI_ERR_RUNTIME;
  } else {
    Vd2uvDev d{d_pairm, d_mval, d_nasm0, d_ebase, d_eps, d_lapin, N, nspec2, nfld, 1.0 / G.ra};
    const long long nthr = (long long)(nspec2 / 2) * nfld;
    EMI_LAUNCH_P(precision, k_vd2uv, (nthr + 255) / 256, 256, 0, (emi_stream_t)0, d, (const RT *)d_vor, (const RT *)d_div, (RT *)d_u, (RT *)d_v);
    hs.flush(0);
    emi_stream_sync(0);
  }
  for (void *q : {(void *)d_pairm, (void *)d_mval, (void *)d_nasm0, (void *)d_ebase, (void *)d_eps, (void *)d_lapin}) emi_dev_free(q);
  return rc;
}

// ------------------------------------------------------------------------------------------
// Biperiodicisation: FPBIPERE, ETIBIHIE, HORIZ_FIELD (etrans/cpu/biper; kernels: emi_biper_body.h).  No resolution handle: the
// routines act on whole fields of one task.  They run on the null stream behind the last transform of every resolution and return
// when the device has finished; scratch memory is allocated per call and freed on every way out.
// ------------------------------------------------------------------------------------------
static int biper_begin() {
  for (auto &p : G.plans)
    if (p && plan_begin(*p, (emi_stream_t)0)) return -1;
  return 0;
}
// With emi_set_profile(1) the kernels of a call are bracketed by events and emi_biper_last_ms gives the device time of the last call by
// kernel: k_biper_spline_x, k_biper_spline_y, k_biper_smooth, k_biper_copy (tools/biper_rate.py).
static double g_biper_ms[4] = {0.0, 0.0, 0.0, 0.0};
struct BiperTimer {
#ifndef EMI_CPU_EMU
  std::vector<std::pair<hipEvent_t, int>> ev;  // (event, the kernel launched before it; -1: the start)
  bool on;
  BiperTimer() : on(G.profile != 0) { mark(-1); }
  void mark(int k) {
    if (!on) return;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, (hipStream_t)0);
    ev.push_back({e, k});
  }
  ~BiperTimer() {  // (the stream has been synchronised)
    if (on)
      for (int k = 0; k < 4; k++) g_biper_ms[k] = 0.0;
    for (size_t i = 0; i < ev.size(); i++) {
      float ms = 0.f;
      if (i > 0 && hipEventElapsedTime(&ms, ev[i - 1].first, ev[i].first) == hipSuccess) g_biper_ms[ev[i].second] += ms;
    }
    for (auto &e : ev) (void)hipEventDestroy(e.first);
  }
#else
  void mark(int) {}
#endif
};
extern "C" int emi_biper_last_ms(double *ms4) {
  for (int k = 0; k < 4; k++) ms4[k] = g_biper_ms[k];
  return EMI_SUCCESS;
}
// spline extension + smoothing of nf fields whose element (x, f, y), zero-based, is w[x + f sf + y sy] (ESPLINE, ESMOOTHE)
static int biper_core(int esz, void *w, long long sf, long long sy, int X, int Y, int UX, int UY, int nf, bool bix, bool biy) {
  const int EX = X - UX, EY = Y - UY;
  int X1 = X, X2 = X, Y1 = Y, Y2 = Y;
  if (bix && !biy) Y1 = Y2 = UY;
  if (biy && !bix) X1 = X2 = UX;
  const int iend = (std::max(EX, EY) + 1) / 2;
  const size_t band_elems = (size_t)std::max((long long)(X1 - UX) * Y2, (long long)(Y1 - UY) * X2) * nf;
  void *band = nullptr;
  if (band_elems && emi_dev_malloc(&band, band_elems * esz)) return -1;
  const emi_stream_t st = (emi_stream_t)0;
  int rc;
  {
    BiperTimer tm;
    if (bix && EX > 0) {
      EMI_LAUNCH_P(esz, k_biper_spline_x, ((long long)EX * UY * nf + 255) / 256, 256, 0, st, (RT *)w, sf, sy, X, UX, UY, nf);
      tm.mark(0);
    }
    if (biy && EY > 0) {
      const int ncols = bix ? X : UX;
      EMI_LAUNCH_P(esz, k_biper_spline_y, ((long long)ncols * nf + 255) / 256, 256, 0, st, (RT *)w, sf, sy, ncols, Y, UY, EX + 1, nf);
      tm.mark(1);
    }
    for (int l = 1; l <= iend; l++) {
      for (int half = 0; half < 2; half++) {
        const int x0 = half ? 0 : UX + l - 1, nx = half ? X2 : (X1 - UX) - 2 * l + 2;
        const int y0 = half ? UY + l - 1 : 0, ny = half ? (Y1 - UY) - 2 * l + 2 : Y2;
        if (nx <= 0 || ny <= 0) continue;
        const long long nblk = ((long long)nx * ny * nf + 255) / 256;
        EMI_LAUNCH_P(esz, k_biper_smooth, nblk, 256, 0, st, (const RT *)w, sf, sy, X, Y, x0, nx, y0, ny, nf, (RT *)band);
        tm.mark(2);
        EMI_LAUNCH_P(esz, k_biper_copy, nblk, 256, 0, st, (RT *)w + x0 + (long long)y0 * sy, sf, sy, (const RT *)band, (long long)nx * ny, (long long)nx, nx, ny, nf);
        tm.mark(3);
      }
    }
    rc = emi_stream_sync(st);
  }
  emi_dev_free(band);
  return rc;
}
static int biper_sizes(const char *who, int esz, int X, int Y, int UX, int UY, bool bix, bool biy, int kdadd) {
  if (!G.init) EMI_FAIL(EMI_ERR_STATE, "%s: SETUP_TRANS0 has not been called", who);
  if (esz != 8 && esz != 4) EMI_FAIL(EMI_ERR_ARG, "%s: element size %d (8 or 4)", who, esz);
  if (kdadd != 0) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: KDADD = %d NOT SUPPORTED (the self-test of the externalised biperiodicisation changes the array shape)", who, kdadd);
  if (X < 1 || Y < 1 || UX < 1 || UY < 1) EMI_FAIL(EMI_ERR_ARG, "%s: KDLON, KDGL, KDLUX, KDGUX = %d, %d, %d, %d MUST BE POSITIVE", who, X, Y, UX, UY);
  if (UX > X || UY > Y) EMI_FAIL(EMI_ERR_ARG, "%s: KDLUX > KDLON OR KDGUX > KDGL (%d > %d, %d > %d)", who, UX, X, UY, Y);
  if ((bix && UX < 2) || (biy && UY < 2))
    EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: KDLUX = %d, KDGUX = %d: FEWER THAN 2 POINTS IN A PERIODICISED DIRECTION (the 2-D vertical-plane case is not supported)", who, UX, UY);
  if (!bix && UX != X) EMI_FAIL(EMI_ERR_ARG, "%s: LDBIX = .FALSE. REQUIRES KDLUX = KDLON (%d, %d)", who, UX, X);
  if (!biy && UY != Y) EMI_FAIL(EMI_ERR_ARG, "%s: LDBIY = .FALSE. REQUIRES KDGUX = KDGL (%d, %d)", who, UY, Y);
  return 0;
}

/* The weights of Boyd's window (ewindowe_mod.F90:107-131) in the precision esz, on the host. */
extern "C" int emi_boyd_window(int n, double scale, int esz, void *out) {
  if (n < 0 || (esz != 8 && esz != 4) || (n > 0 && !out)) EMI_FAIL(EMI_ERR_ARG, "emi_boyd_window: bad arguments (n = %d, element size %d)", n, esz);
  for (int j = 1; j <= n; j++) {
    if (esz == 8) {
      const double t = (double)(-n - 1 + 2 * j) / (double)(n + 1), l = t / std::sqrt(1.0 - (t * t));
      ((double *)out)[j - 1] = (1.0 + std::erf(scale * l)) / 2.0;
    } else {
      const float t = (float)(-n - 1 + 2 * j) / (float)(n + 1), l = t / std::sqrt(1.0f - (t * t));
      ((float *)out)[j - 1] = (1.0f + std::erf((float)scale * l)) / 2.0f;
    }
  }
  return EMI_SUCCESS;
}

/* HORIZ_FIELD (biper/external/horiz_field.F90:67-73): the expression as Fortran types it -- default-real literals and integers with
 * PPI, a JPRB parameter of the default-real value 3.141592.  esz = 4: all of it in float; esz = 8: (jx + 0.5 imax), (jy + 0.7 imax) and
 * the literal 0.1 are float values, the rest is double. */
extern "C" int emi_horiz_field(int kx, int ky, int esz, void *out) {
  if (kx < 1 || ky < 1 || (esz != 8 && esz != 4) || !out) EMI_FAIL(EMI_ERR_ARG, "HORIZ_FIELD: bad arguments (KX = %d, KY = %d, element size %d)", kx, ky, esz);
  const int imax = std::max(kx, ky);
  for (int jy = 1; jy <= ky; jy++)
    for (int jx = 1; jx <= kx; jx++) {
      const float a = (float)jx + 0.5f * (float)imax, b = (float)jy + 0.7f * (float)imax;
      const size_t i = (size_t)(jy - 1) * kx + (jx - 1);
      if (esz == 8) {
        const double ppi = (double)3.141592f;
        ((double *)out)[i] = 280.0 * (1.0 + (double)0.1f * std::sin(ppi * (double)a * (double)b / (double)(imax * imax) + 1.0));
      } else {
        ((float *)out)[i] = 280.0f * (1.0f + 0.1f * std::sin(3.141592f * a * b / (float)(imax * imax) + 1.0f));
      }
    }
  return EMI_SUCCESS;
}

extern "C" int emi_fpbipere(int mem_space, int esz, void *pgpbi, int kdlux, int kdgux, int kdlon, int kdgl, int knubi, int kd1, int kdadd, int ldzon, int ldboyd,
                            const int *kdboyd, const double *plboyd) {
  const char *who = "FPBIPERE";
  const int X = kdlon, Y = kdgl, UX = kdlux, UY = kdgux;
  if (int rc = biper_sizes(who, esz, X, Y, UX, UY, true, true, kdadd)) return rc;
  int Wx = 0, Wy = 0;
  long long need = (long long)X * Y;
  if (ldboyd) {
    if (!kdboyd) EMI_FAIL(EMI_ERR_ARG, "FPBIPERE: Boyd periodization requires KDBOYD argument");
    if (!plboyd) EMI_FAIL(EMI_ERR_ARG, "FPBIPERE: Boyd periodization requires PLBOYD argument");
    const int bwx = kdboyd[2], bwy = kdboyd[5];
    if (bwx < 0 || bwy < 0) EMI_FAIL(EMI_ERR_ARG, "FPBIPERE: KDBOYD(3), KDBOYD(6) = %d, %d MUST NOT BE NEGATIVE", bwx, bwy);
    Wx = 2 * bwx + (X - UX), Wy = 2 * bwy + (Y - UY);
    if (X - UX != Y - UY)
      EMI_FAIL(EMI_ERR_UNSUPPORTED,
               "FPBIPERE: BOYD WINDOW WITH KDLON - KDLUX = %d /= KDGL - KDGUX = %d NOT SUPPORTED (EWINDOWE strides its rows by KDLUX + 2 (KBWX + KDGL - KDGUX): the row "
               "length only where the two zones are equally wide)",
               X - UX, Y - UY);
    if (Wx > X || Wy > Y) EMI_FAIL(EMI_ERR_UNSUPPORTED, "FPBIPERE: BOYD WINDOW WIDER THAN THE DOMAIN (%d > %d OR %d > %d): THE BLENDED ZONES WOULD OVERLAP", Wx, X, Wy, Y);
    need = (long long)(X + Wx) * (Y + Wy);
    if (kd1 != need && knubi != 1)
      EMI_FAIL(EMI_ERR_UNSUPPORTED, "FPBIPERE: BOYD WINDOW NEEDS KD1 = (KDLON + WX) (KDGL + WY) = %lld OR KNUBI = 1 (KD1 = %d: EWINDOWE re-declares PGPBI with that first extent)",
               need, kd1);
  }
  if (kd1 < need) EMI_FAIL(EMI_ERR_ARG, "FPBIPERE: KD1 = %d TOO SMALL (%lld points are needed)", kd1, need);
  if (knubi <= 0) return EMI_SUCCESS;
  if (!pgpbi) EMI_FAIL(EMI_ERR_ARG, "FPBIPERE: PGPBI NOT PRESENT");
  if (resolve_space(who, mem_space, {pgpbi}, &mem_space)) return EMI_ERR_ARG;
  HostStage hs(esz);
  if (biper_begin()) return EMI_ERR_RUNTIME;
  void *d = hs.out(pgpbi, (size_t)kd1 * knubi, mem_space == EMI_MEM_HOST, true, 0);
  if (hs.failed) EMI_FAIL(EMI_ERR_RUNTIME, "FPBIPERE: cannot stage the host array through device memory");
  const emi_stream_t st = (emi_stream_t)0;
  int rc = EMI_SUCCESS;
  if (ldboyd) {
    std::vector<char> bh((size_t)(Wx + Wy) * esz + 8);
    emi_boyd_window(Wx, *plboyd, esz, bh.data());
    emi_boyd_window(Wy, *plboyd, esz, bh.data() + (size_t)Wx * esz);
    void *db = nullptr;
    if (emi_dev_malloc(&db, bh.size()) || emi_h2d(db, bh.data(), bh.size(), st)) {
      rc = EMI_ERR_RUNTIME;
    } else {
      const int ld = X + Wx, nrow = Y + Wy;
      if (Wx > 0) EMI_LAUNCH_P(esz, k_biper_boyd, ((long long)Wx * nrow * knubi + 255) / 256, 256, 0, st, (RT *)d, (long long)kd1, ld, 0, X, Wx, nrow, knubi, (const RT *)db);
      if (Wy > 0) EMI_LAUNCH_P(esz, k_biper_boyd, ((long long)Wy * ld * knubi + 255) / 256, 256, 0, st, (RT *)d, (long long)kd1, ld, 1, Y, Wy, ld, knubi, (const RT *)db + Wx);
      if (emi_stream_sync(st)) rc = EMI_ERR_RUNTIME;
    }
    emi_dev_free(db);
  } else {
    if (!ldzon && UX != X) {  // the rows move from KDLUX to KDLON apart, in place: through a copy of C+I, as the reference's ZGPBI
      void *c = nullptr;
      const long long ci = (long long)UX * UY, nblk = (ci * knubi + 255) / 256;
      if (emi_dev_malloc(&c, (size_t)ci * knubi * esz)) {
        rc = EMI_ERR_RUNTIME;
      } else {
        EMI_LAUNCH_P(esz, k_biper_copy, nblk, 256, 0, st, (RT *)c, ci, (long long)UX, (const RT *)d, (long long)kd1, (long long)UX, UX, UY, knubi);
        EMI_LAUNCH_P(esz, k_biper_copy, nblk, 256, 0, st, (RT *)d, (long long)kd1, (long long)X, (const RT *)c, ci, (long long)UX, UX, UY, knubi);
        if (emi_stream_sync(st)) rc = EMI_ERR_RUNTIME;
      }
      emi_dev_free(c);
    }
    if (rc == EMI_SUCCESS && biper_core(esz, d, kd1, X, X, Y, UX, UY, knubi, true, true)) rc = EMI_ERR_RUNTIME;
  }
  if (rc == EMI_SUCCESS) hs.flush(st);
  else emi_set_error("FPBIPERE: device memory or a launch failed");
  return rc;
}

extern "C" int emi_etibihie(int mem_space, int esz, void *pgpbi, int kdlon, int kdgl, int knubi, int kdlux, int kdgux, int kstart, int kdlsm, int ldbix, int ldbiy,
                            int kdadd) {
  const char *who = "ETIBIHIE";
  if (int rc = biper_sizes(who, esz, kdlon, kdgl, kdlux, kdgux, ldbix != 0, ldbiy != 0, kdadd)) return rc;
  if (kstart > 1 || kdlsm < kdlon) EMI_FAIL(EMI_ERR_ARG, "ETIBIHIE: KSTART = %d > 1 OR KDLSM = %d < KDLON = %d: THE ROWS DO NOT HOLD 1 .. KDLON", kstart, kdlsm, kdlon);
  if (knubi <= 0 || (!ldbix && !ldbiy)) return EMI_SUCCESS;
  if (!pgpbi) EMI_FAIL(EMI_ERR_ARG, "ETIBIHIE: PGPBI NOT PRESENT");
  if (resolve_space(who, mem_space, {pgpbi}, &mem_space)) return EMI_ERR_ARG;
  const long long L = (long long)kdlsm - kstart + 1;
  HostStage hs(esz);
  if (biper_begin()) return EMI_ERR_RUNTIME;
  void *d = hs.out(pgpbi, (size_t)L * knubi * kdgl, mem_space == EMI_MEM_HOST, true, 0);
  if (hs.failed) EMI_FAIL(EMI_ERR_RUNTIME, "ETIBIHIE: cannot stage the host array through device memory");
  if (biper_core(esz, (char *)d + (size_t)(1 - kstart) * esz, L, L * knubi, kdlon, kdgl, kdlux, kdgux, knubi, ldbix != 0, ldbiy != 0))
    EMI_FAIL(EMI_ERR_RUNTIME, "ETIBIHIE: device memory or a launch failed");
  hs.flush((emi_stream_t)0);
  return EMI_SUCCESS;
}

extern "C" int emi_work_model(int kresol, int nfields, double *leg, double *fft, double *fbytes) {
  Plan *Pp = get_plan(kresol);
  if (!Pp) EMI_FAIL(EMI_ERR_STATE, "emi_work_model: unknown resolution %d", kresol);
  if (Pp->lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: resolution %d is a limited-area handle (ESETUP_TRANS): this routine serves the spherical transforms only", "emi_work_model", kresol);
  Plan &P = *Pp;
  // LT flops/direction = KF * sum_m 2*NDGLU(m)*(N-m+2)*c_m, c_0=1, c_{m>0}=2 (this
  // task's wavenumbers); FFT ~ 2.5 n log2 n per row; Fourier bytes of this task's latitudes
  double s = 0.0;
  for (int ml = 0; ml < P.nump; ml++) {
    const int m = P.mval[ml];
    s += 2.0 * std::min(P.ndgnh, P.ndglu[m]) * (double)(P.nsmax - m + 2) * (m == 0 ? 1.0 : 2.0);
  }
  if (leg) *leg = s * nfields;
  double f = 0.0;
  for (int j = P.lat0; j < P.lat0 + P.nlat; j++) f += 2.5 * P.nloen[j] * std::log2((double)std::max(2, P.nloen[j]));
  if (fft) *fft = f * nfields;
  if (fbytes) *fbytes = (double)P.frows * 2.0 * P.esz * nfields;
  return EMI_SUCCESS;
}

extern "C" int emi_last_phase_ms(double *ms3) {
  int l[4];
  double ms[4];
  g_pt.resolve(ms, l);
  for (int i = 0; i < 3; i++) ms3[i] = ms[i];
  return EMI_SUCCESS;
}

extern "C" int emi_last_phase_launches(int *l3) {
  double ms[4];
  int l[4];
  g_pt.resolve(ms, l);
  for (int i = 0; i < 3; i++) l3[i] = l[i];
  return EMI_SUCCESS;
}

// TRMTOL / TRLTOM (and, with V-sets, TRLTOG / TRGTOL) of the calls since emi_set_profile: device time between an event in front of
// and one behind the all-to-all-v hook on the stream the hook was given, the number of exchanges, the bytes this task sent.
extern "C" int emi_last_exchange(double *ms, int *calls, double *bytes_sent) {
  double m4[4];
  int l[4];
  g_pt.resolve(m4, l);
  if (ms) *ms = m4[3];
  if (calls) *calls = l[3];
  if (bytes_sent) *bytes_sent = g_pt.xbytes;
  return EMI_SUCCESS;
}

// kernel launches of the FFT phases since emi_set_profile (one FTINV or FTDIR of one field batch launches one kernel per length class)
extern "C" int emi_last_fft_launches(long long *kernels) {
  if (kernels) *kernels = g_pt.fft_kernels;
  return EMI_SUCCESS;
}

extern "C" int emi_set_profile(int on) {
  G.profile = on;
  g_pt.n = 0;  // a new measurement starts here
  g_pt.xbytes = 0;
  g_pt.fft_kernels = 0;
  return EMI_SUCCESS;
}

extern "C" int emi_set_max_batch(int max_fields) {
  G.max_batch = max_fields;
  return EMI_SUCCESS;
}

// ------------------------------------------------------------------------------------------
// DIST_SPEC / GATH_SPEC / DIST_GRID / GATH_GRID: host-side re-layouts + two host collectives
// ------------------------------------------------------------------------------------------
extern "C" int emi_set_host_collectives(emi_bcast_fn bcast, emi_allgatherv_fn allgatherv, void *user) {
  G.hc_bcast = bcast;
  G.hc_gather = allgatherv;
  G.hc_user = user;
  return EMI_SUCCESS;
}
// broadcast of host bytes from task `root` (1-based) over the attached transport: what the drop-in layers above need where the
// reference sends a small array from its master task (GPNORM_TRANSAD: gpnorm_trans_ctlad_mod.F90)
extern "C" int emi_bcast_host(void *buf, long long bytes, int root) {
  if (!G.init) EMI_FAIL(EMI_ERR_STATE, "emi_bcast_host: SETUP_TRANS0 has not been called");
  if (root < 1 || root > G.nproc_all || bytes < 0 || (bytes > 0 && !buf)) EMI_FAIL(EMI_ERR_ARG, "emi_bcast_host: bad arguments");
  if (G.nproc_all == 1 || bytes == 0) return EMI_SUCCESS;
  if (!G.hc_bcast) EMI_FAIL(EMI_ERR_STATE, "emi_bcast_host: several tasks and no host collectives (emi_set_host_collectives)");
  if (G.hc_bcast(G.hc_user, buf, bytes, root - 1)) EMI_FAIL(EMI_ERR_RUNTIME, "emi_bcast_host: broadcast failed");
  return EMI_SUCCESS;
}
extern "C" int emi_inq_init(int *kmax_resol, double *prad) {
  if (!G.init) EMI_FAIL(EMI_ERR_STATE, "emi_inq_init: SETUP_TRANS0 has not been called");
  if (kmax_resol) *kmax_resol = G.max_resol;
  if (prad) *prad = G.ra;
  return EMI_SUCCESS;
}
extern "C" int emi_inq_tasks(int *nproc, int *myproc) {
  if (!G.init) EMI_FAIL(EMI_ERR_STATE, "emi_inq_tasks: SETUP_TRANS0 has not been called");
  if (nproc) *nproc = G.nproc_all;
  if (myproc) *myproc = G.myproc_all;
  return EMI_SUCCESS;
}
namespace {
struct TaskLayout {  // global <-> per-task positions of one resolution, over all NPROC = NPRTRW x NPRTRV tasks (task t = w NPRTRV + v)
  std::vector<long long> iasm0g;              // [N+1] global start of wavenumber m
  std::vector<long long> mlen;                // [N+1] reals of wavenumber m: 2 (NSMAX - m + 1), or 4 (KNTMP(m) + 1) on a limited-area handle
  std::vector<std::vector<int>> ms;           // [W-set] its wavenumbers, ascending
  std::vector<std::vector<long long>> start;  // [W-set][i] local start of ms[W-set][i]
  std::vector<int> wset;                      // [task] its W-set: a task's spectral layout is that of its W-set
  std::vector<long long> nspec2, gp0, ngp;    // [task] (grid: its band, or its sub-band with V-sets)
  int nt = 1, me = 0;                         // tasks; this task
};
TaskLayout task_layout(const Plan &P) {
  TaskLayout L;
  const int N = P.nsmax, NW = P.nproc, NV = P.nprv;
  L.nt = NW * NV, L.me = P.me * NV + P.mev;
  L.iasm0g.assign(N + 2, 0);
  L.mlen.assign(N + 1, 0);
  for (int m = 0; m <= N; m++) {  // (a limited-area handle: N = KMSMAX; the global field is the one-task layout, NCPL4M(m) reals per m)
    L.mlen[m] = P.lam ? 4LL * (P.kntmp[m] + 1) : 2LL * (N - m + 1);
    L.iasm0g[m + 1] = L.iasm0g[m] + L.mlen[m];
  }
  L.ms.assign(NW, {});
  L.start.assign(NW, {});
  std::vector<long long> wspec2(NW, 0);
  for (int m = 0; m <= N; m++) {
    const int w = P.procm[m];
    L.ms[w].push_back(m);
    L.start[w].push_back(wspec2[w]);
    wspec2[w] += L.mlen[m];
  }
  std::vector<long long> cum(P.ndgl + 1, 0);
  for (int j = 0; j < P.ndgl; j++) cum[j + 1] = cum[j] + P.nloen[j];
  L.wset.assign(L.nt, 0);
  L.nspec2.assign(L.nt, 0);
  L.gp0.assign(L.nt, 0);
  L.ngp.assign(L.nt, 0);
  for (int t = 0; t < L.nt; t++) {  // latitude order = task order
    const int w = t / NV, v = t % NV;
    L.wset[t] = w;
    L.nspec2[t] = wspec2[w];
    L.gp0[t] = cum[P.vfirst(w, v)];
    L.ngp[t] = cum[P.vlast(w, v)] - cum[P.vfirst(w, v)];
  }
  return L;
}
// Which task holds which field in its local array.  A grid field, and every field with NPRTRV = 1, lives on all tasks; with V-sets
// a spectral field lives on the NPRTRW tasks of ONE V-set (KVSET of dist_spec.h / gath_spec.h): PSPEC of a task holds the fields
// of its own V-set in ascending order, which may be none (dist_spec_control_mod.F90:96, gath_spec_control_mod.F90).
struct FieldSets {
  int nprv = 1;
  std::vector<int> vs;    // [field] its V-set (0-based); -1: every task holds it
  std::vector<int> lidx;  // [field] its position among the local fields of a task that holds it
  bool holds(int t, int f) const { return vs[f] < 0 || vs[f] == t % nprv; }
  int nlocal(int t) const {
    int n = 0;
    for (size_t f = 0; f < vs.size(); f++) n += holds(t, (int)f) ? 1 : 0;
    return n;
  }
  unsigned hash() const {  // FNV-1a of the V-sets: what the tasks of a call compare
    unsigned h = 2166136261u;
    for (int v : vs) h = (h ^ (unsigned)(v + 1)) * 16777619u;
    return h;
  }
};
int field_sets(const Plan &P, bool spec, int nfld, const int *kvset, const char *who, FieldSets &F) {
  F.nprv = P.nprv;
  F.vs.assign(std::max(nfld, 0), -1);
  F.lidx.assign(std::max(nfld, 0), 0);
  if (spec && P.nprv > 1 && !kvset) EMI_FAIL(EMI_ERR_ARG, "%s:KVSET MISSING, NPRTRV > 1", who);
  std::vector<int> seen(P.nprv, 0);
  for (int f = 0; f < nfld; f++) {
    if (spec && kvset && (kvset[f] < 1 || kvset[f] > P.nprv))  // (also with NPRTRV = 1, as gath_spec.F90:169-172)
      EMI_FAIL(EMI_ERR_ARG, "%s:KVSET CONTAINS VALUES OUTSIDE RANGE (KVSET(%d) = %d, NPRTRV = %d)", who, f + 1, kvset[f], P.nprv);
    if (spec && P.nprv > 1) {
      F.vs[f] = kvset[f] - 1;
      F.lidx[f] = seen[F.vs[f]]++;
    } else {
      F.lidx[f] = f;
    }
  }
  return 0;
}
int check_tasks(const Plan &P, const int *k, int nfld, const char *who, bool host_path = true) {
  const int NT = P.nproc * P.nprv;
  if (nfld < 0 || (nfld > 0 && !k)) EMI_FAIL(EMI_ERR_ARG, "%s: task list missing", who);
  for (int f = 0; f < nfld; f++)
    if (k[f] < 1 || k[f] > NT) EMI_FAIL(EMI_ERR_ARG, "%s: task %d of field %d outside 1..%d", who, k[f], f + 1, NT);
  if (host_path && NT > 1 && (!G.hc_bcast || !G.hc_gather))
    EMI_FAIL(EMI_ERR_STATE, "%s: %d tasks but no host collectives registered (emi_set_host_collectives)", who, NT);
  if (!host_path && NT > 1 && !G.a2a) EMI_FAIL(EMI_ERR_STATE, "%s: %d tasks but no all-to-all-v hook registered (emi_set_alltoallv)", who, NT);
  return 0;
}
int slot_of(const int *ksort, int f, int nfld, const char *who, int *slot) {
  *slot = ksort ? ksort[f] - 1 : f;
  if (*slot < 0 || *slot >= nfld) EMI_FAIL(EMI_ERR_ARG, "%s: KSORT(%d) = %d outside 1..%d", who, f + 1, *slot + 1, nfld);
  return 0;
}
}  // namespace

// global fields on their source tasks -> every task's share.  One broadcast per source task, over all tasks: a task outside the
// V-set of a spectral field takes part and drops it.
template <bool SPEC>
static int dist_impl(int kresol, const void *glob, int nfld, const int *kfrom, const int *kvset, const int *ksort, int kproma, void *loc, const char *who,
                     bool lam = false) {
  Plan *Pp = get_plan(kresol);
  if (!Pp) EMI_FAIL(EMI_ERR_STATE, "%s: unknown resolution %d", who, kresol);
  if (Pp->lam && !lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: resolution %d is a limited-area handle (ESETUP_TRANS): this routine serves the spherical transforms only", who, kresol);
  if (!Pp->lam && lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: resolution %d is not a limited-area handle: it was not set up by ESETUP_TRANS", who, kresol);
  Plan &P = *Pp;
  FieldSets F;
  if (field_sets(P, SPEC, nfld, kvset, who, F)) return EMI_ERR_ARG;
  if (check_tasks(P, kfrom, nfld, who)) return EMI_ERR_ARG;
  const TaskLayout L = task_layout(P);
  const int me = L.me, nfl = F.nlocal(me);  // nfl: the fields of PSPEC / PGP on this task
  if (!loc && (nfl > 0 || P.nprv == 1)) EMI_FAIL(EMI_ERR_ARG, "%s: local array missing", who);
  const size_t esz = P.esz;
  const long long nglob = SPEC ? (long long)P.nspec2g : (long long)P.ngptotg;
  const int nproma = kproma > 0 ? kproma : (int)L.ngp[me];
  std::vector<char> tmp;
  long long mine_done = 0;  // global fields of this task consumed so far
  for (int root = 0; root < L.nt; root++) {
    std::vector<int> fl;
    for (int f = 0; f < nfld; f++)
      if (kfrom[f] == root + 1) fl.push_back(f);
    if (fl.empty()) continue;
    const long long bytes = (long long)fl.size() * nglob * (long long)esz;
    const char *buf;
    if (root == me) {
      if (!glob) EMI_FAIL(EMI_ERR_ARG, "%s: this task is the source of %zu fields but passes no global array", who, fl.size());
      buf = (const char *)glob + (size_t)mine_done * nglob * esz;
      mine_done += (long long)fl.size();
      if (L.nt > 1 && G.hc_bcast(G.hc_user, (void *)buf, bytes, root)) EMI_FAIL(EMI_ERR_RUNTIME, "%s: broadcast failed", who);
    } else {
      tmp.resize((size_t)bytes);
      if (G.hc_bcast(G.hc_user, tmp.data(), bytes, root)) EMI_FAIL(EMI_ERR_RUNTIME, "%s: broadcast failed", who);
      buf = tmp.data();
    }
    for (size_t i = 0; i < fl.size(); i++) {
      if (!F.holds(me, fl[i])) continue;
      int slot;  // KSORT is indexed by the local field (dist_spec_control_mod.F90:255, 288)
      if (slot_of(ksort, F.lidx[fl[i]], nfl, who, &slot)) return EMI_ERR_ARG;
      const char *g = buf + i * (size_t)nglob * esz;
      if (SPEC) {  // PSPEC(nfl, nspec2): element (slot, isp)
        const std::vector<int> &ms = L.ms[L.wset[me]];
        for (size_t k = 0; k < ms.size(); k++) {
          const long long cnt = L.mlen[ms[k]], gs = L.iasm0g[ms[k]], ls = L.start[L.wset[me]][k];
          for (long long e = 0; e < cnt; e++) memcpy((char *)loc + ((size_t)(ls + e) * nfl + slot) * esz, g + (size_t)(gs + e) * esz, esz);
        }
      } else {  // PGP(nproma, nfl, ngpblks): point p -> block p / nproma
        const long long g0 = L.gp0[me], ng = L.ngp[me];
        for (long long p0 = 0; p0 < ng; p0 += nproma) {
          const long long w = std::min<long long>(nproma, ng - p0), blk = p0 / nproma;
          memcpy((char *)loc + ((size_t)(blk * nfl + slot) * nproma) * esz, g + (size_t)(g0 + p0) * esz, (size_t)w * esz);
        }
      }
    }
  }
  return EMI_SUCCESS;
}

// every task's share -> global fields on their target tasks.  An all-gather-v of the packed local fields per chunk of fields: a task
// sends the fields of the chunk that it holds (with V-sets a spectral field comes from the tasks of its V-set only).
template <bool SPEC>
static int gath_impl(int kresol, void *glob, int nfld, const int *kto, const int *kvset, int kproma, const void *loc, const char *who, bool lam = false) {
  Plan *Pp = get_plan(kresol);
  if (!Pp) EMI_FAIL(EMI_ERR_STATE, "%s: unknown resolution %d", who, kresol);
  if (Pp->lam && !lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: resolution %d is a limited-area handle (ESETUP_TRANS): this routine serves the spherical transforms only", who, kresol);
  if (!Pp->lam && lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: resolution %d is not a limited-area handle: it was not set up by ESETUP_TRANS", who, kresol);
  Plan &P = *Pp;
  FieldSets F;
  if (field_sets(P, SPEC, nfld, kvset, who, F)) return EMI_ERR_ARG;
  if (check_tasks(P, kto, nfld, who)) return EMI_ERR_ARG;
  const TaskLayout L = task_layout(P);
  const int NT = L.nt, me = L.me, nfl = F.nlocal(me);
  if (!loc && (nfl > 0 || P.nprv == 1)) EMI_FAIL(EMI_ERR_ARG, "%s: local array missing", who);
  const size_t esz = P.esz;
  const int nproma = kproma > 0 ? kproma : (int)L.ngp[me];
  const long long nglob = SPEC ? (long long)P.nspec2g : (long long)P.ngptotg;
  auto nloc = [&](int t) { return SPEC ? L.nspec2[t] : L.ngp[t]; };
  // Fields in chunks whose gathered image stays below 256 MiB: every task receives every field of a chunk whatever KTO says (the
  // host collectives offer an all-gather-v only), so an unchunked GATH_GRID of 137 levels at TCo1279 would put 7 GB on every task.
  const long long per_field = nglob * (long long)esz;
  const long long budget = (getenv("EMI_GATH_CHUNK") && *getenv("EMI_GATH_CHUNK")) ? atoll(getenv("EMI_GATH_CHUNK")) : (256LL << 20);  // bytes (tests: a few fields per chunk)
  const int chunk = (int)std::max<long long>(1, std::min<long long>(nfld, budget / std::max<long long>(per_field, 1)));
  long long i_mine = 0;
  std::vector<char> mine, all;
  std::vector<long long> cnt(NT), dsp(NT);
  std::vector<int> held(NT);  // fields of the chunk that task t holds
  for (int fa = 0; fa < nfld; fa += chunk) {
    const int nf = std::min(chunk, nfld - fa);
    for (int t = 0; t < NT; t++) {
      held[t] = 0;
      for (int f = fa; f < fa + nf; f++) held[t] += F.holds(t, f) ? 1 : 0;
    }
    // pack [held field][local element]
    mine.resize((size_t)held[me] * nloc(me) * esz);
    for (int f = fa, fc = 0; f < fa + nf; f++) {
      if (!F.holds(me, f)) continue;
      const int lf = F.lidx[f];
      char *dst = mine.data() + (size_t)fc++ * nloc(me) * esz;
      if (SPEC) {
        for (long long e = 0; e < nloc(me); e++) memcpy(dst + (size_t)e * esz, (const char *)loc + ((size_t)e * nfl + lf) * esz, esz);
      } else {
        for (long long p0 = 0; p0 < nloc(me); p0 += nproma) {
          const long long w = std::min<long long>(nproma, nloc(me) - p0), blk = p0 / nproma;
          memcpy(dst + (size_t)p0 * esz, (const char *)loc + ((size_t)(blk * nfl + lf) * nproma) * esz, (size_t)w * esz);
        }
      }
    }
    const char *base = mine.data();
    if (NT > 1) {
      long long tot = 0;
      for (int t = 0; t < NT; t++) {
        cnt[t] = (long long)held[t] * nloc(t) * (long long)esz;
        dsp[t] = tot;
        tot += cnt[t];
      }
      all.resize((size_t)tot);
      if (G.hc_gather(G.hc_user, mine.data(), cnt[me], all.data(), cnt.data(), dsp.data(), NT)) EMI_FAIL(EMI_ERR_RUNTIME, "%s: all-gather-v failed", who);
      base = all.data();
    } else {
      dsp[0] = 0;
    }
    for (int f = fa; f < fa + nf; f++) {
      if (kto[f] != me + 1) continue;
      if (!glob) EMI_FAIL(EMI_ERR_ARG, "%s: this task is the target of field %d but passes no global array", who, f + 1);
      char *g = (char *)glob + (size_t)i_mine * nglob * esz;
      i_mine++;
      for (int t = 0; t < NT; t++) {
        if (!F.holds(t, f)) continue;
        int fc = 0;  // position of field f in the block of task t
        for (int h = fa; h < f; h++) fc += F.holds(t, h) ? 1 : 0;
        const char *src = base + dsp[t] + (size_t)fc * nloc(t) * esz;
        if (SPEC) {
          const int w = L.wset[t];
          for (size_t k = 0; k < L.ms[w].size(); k++) {
            const long long cnte = L.mlen[L.ms[w][k]];
            memcpy(g + (size_t)L.iasm0g[L.ms[w][k]] * esz, src + (size_t)L.start[w][k] * esz, (size_t)cnte * esz);
          }
        } else {
          memcpy(g + (size_t)L.gp0[t] * esz, src, (size_t)L.ngp[t] * esz);
        }
      }
    }
  }
  return EMI_SUCCESS;
}

extern "C" int emi_dist_spec(int kresol, const void *specg, int nfld, const int *kfrom, const int *ksort, void *spec) {
  return dist_impl<true>(kresol, specg, nfld, kfrom, nullptr, ksort, 0, spec, "DIST_SPEC");
}
extern "C" int emi_gath_spec(int kresol, void *specg, int nfld, const int *kto, const void *spec) {
  return gath_impl<true>(kresol, specg, nfld, kto, nullptr, 0, spec, "GATH_SPEC");
}
extern "C" int emi_dist_grid(int kresol, const void *gpg, int nfld, const int *kfrom, const int *ksort, int kproma, void *gp) {
  return dist_impl<false>(kresol, gpg, nfld, kfrom, nullptr, ksort, kproma, gp, "DIST_GRID");
}
extern "C" int emi_gath_grid(int kresol, void *gpg, int nfld, const int *kto, int kproma, const void *gp) {
  return gath_impl<false>(kresol, gpg, nfld, kto, nullptr, kproma, gp, "GATH_GRID");
}
// EDIST_SPEC / EGATH_SPEC / EDIST_GRID / EGATH_GRID: the same on a limited-area handle.  A global spectral field is the one-task layout,
// m = 0 .. KMSMAX ascending with 4 (KNTMP(m) + 1) reals each (gath_spec_control_mod.F90:108-113 with KN = NCPL4M); a global grid field
// the NDGL x NDLON points row after row, the tasks' bands of whole rows in task order.
extern "C" int emi_edist_spec(int kresol, const void *specg, int nfld, const int *kfrom, const int *ksort, void *spec) {
  return dist_impl<true>(kresol, specg, nfld, kfrom, nullptr, ksort, 0, spec, "EDIST_SPEC", true);
}
extern "C" int emi_egath_spec(int kresol, void *specg, int nfld, const int *kto, const void *spec) {
  return gath_impl<true>(kresol, specg, nfld, kto, nullptr, 0, spec, "EGATH_SPEC", true);
}
extern "C" int emi_edist_grid(int kresol, const void *gpg, int nfld, const int *kfrom, const int *ksort, int kproma, void *gp) {
  return dist_impl<false>(kresol, gpg, nfld, kfrom, nullptr, ksort, kproma, gp, "EDIST_GRID", true);
}
extern "C" int emi_egath_grid(int kresol, void *gpg, int nfld, const int *kto, int kproma, const void *gp) {
  return gath_impl<false>(kresol, gpg, nfld, kto, nullptr, kproma, gp, "EGATH_GRID", true);
}

// CRC-64/ECMA-182, table driven (ectrans-benchmark.F90:1455-1600 calls fiat's crc64, un-vendored)
extern "C" int emi_crc64(const void *data, size_t bytes, unsigned long long *crc) {
  if ((!data && bytes) || !crc) EMI_FAIL(EMI_ERR_ARG, "emi_crc64: null argument");
  static unsigned long long tab[256];
  static bool init = false;
  if (!init) {
    for (int i = 0; i < 256; i++) {
      unsigned long long c = (unsigned long long)i << 56;
      for (int k = 0; k < 8; k++) c = (c & 0x8000000000000000ULL) ? (c << 1) ^ 0x42F0E1EBA9EA3693ULL : (c << 1);
      tab[i] = c;
    }
    init = true;
  }
  unsigned long long c = *crc;
  const unsigned char *p = (const unsigned char *)data;
  for (size_t i = 0; i < bytes; i++) c = tab[((c >> 56) ^ p[i]) & 0xff] ^ (c << 8);
  *crc = c;
  return EMI_SUCCESS;
}

// ------------------------------------------------------------------------------------------
// V-sets (NPRTRV > 1): INV_TRANS / DIR_TRANS of task (MYSETW, MYSETV).
// Spectral and Fourier space hold the fields of ONE V-set on the wavenumbers / latitude band of the W-set; grid space holds ALL
// fields on the task's sub-band (inv_trans.F90:212-300, trltog_mod.F90, trgtol_mod.F90).  The transform of the local fields is
// the W-set transform above, run into / out of a band-sized device array; TRLTOG / TRGTOL between the NPRTRV tasks of the band
// is one all-to-all-v of dense [field][point] blocks, packed and unpacked by k_gridcopy.  Field order everywhere: the
// reference's ([vor] [div] u v scalars [N-S derivatives] [u, v E-W derivatives] [scalar E-W derivatives]); a V-set's fields
// are the global ones it owns, in global order, group by group.
// ------------------------------------------------------------------------------------------
struct StageBuf {  // device scratch from the staging pool
  void *p = nullptr;
  explicit StageBuf(size_t bytes) { p = bytes ? emi_stage::acquire(bytes) : nullptr; }
  ~StageBuf() {
    if (p) emi_stage::release(p);
  }
};
template <class ARGS>
static int v_groups(const Plan &P, const ARGS &a, const char *who, VGroups &vg) {
  const emi_vsets_t *vs = a.vsets;
  if (!vs) EMI_FAIL(EMI_ERR_ARG, "%s: NPRTRV = %d but no KVSET arrays (emi_vsets_t)", who, P.nprv);
  auto owners = [&](const int *k, int n, const char *nm, std::vector<int> &out) {
    out.clear();
    for (int i = 0; i < n; i++) {
      if (!k || k[i] < 1 || k[i] > P.nprv) {
        emi_set_error("%s:%s TOO LONG OR CONTAINS VALUES OUTSIDE RANGE", who, nm);
        return -1;
      }
      out.push_back(k[i] - 1);
    }
    return 0;
  };
  vg.nuv_g = vs->kvsetuv ? vs->nuv_g : 0;
  if (owners(vs->kvsetuv, vg.nuv_g, "KVSETUV", vg.ouv)) return EMI_ERR_ARG;
  const int mine_uv = (int)std::count(vg.ouv.begin(), vg.ouv.end(), P.mev);
  if (mine_uv != ((a.spvor || a.spdiv) ? a.nf_uv : 0))
    EMI_FAIL(EMI_ERR_ARG, "%s: %d fields of KVSETUV belong to this V-set, the spectral arrays hold %d", who, mine_uv, (a.spvor || a.spdiv) ? a.nf_uv : 0);
  std::vector<int> o;
  vg.sc_g.clear(), vg.osc.clear();
  auto check_local = [&](const char *nm, int mine, int have) {
    if (mine != have) {
      emi_set_error("%s: %d fields of %s belong to this V-set, the spectral array holds %d", who, mine, nm, have);
      return -1;
    }
    return 0;
  };
  if (vs->kvsetsc) {  // PSPSCALAR form
    if (vs->kvsetsc2 || vs->kvsetsc3a || vs->kvsetsc3b) EMI_FAIL(EMI_ERR_ARG, "%s : PSPSCALAR AND PSPSC3A/PSPSC3B/PSPSC2 BOTH PRESENT", who);
    if (owners(vs->kvsetsc, vs->nsc_g, "KVSETSC", o)) return EMI_ERR_ARG;
    vg.nsc_g[0] = vs->nsc_g;
    for (int i = 0; i < vs->nsc_g; i++) vg.sc_g.push_back({0, i, 0}), vg.osc.push_back(o[i]);
    if (check_local("KVSETSC", (int)std::count(o.begin(), o.end(), P.mev), a.spscalar ? a.nf_scalar : 0)) return EMI_ERR_ARG;
  } else {
    if (vs->kvsetsc2) {
      if (owners(vs->kvsetsc2, vs->nsc2_g, "KVSETSC2", o)) return EMI_ERR_ARG;
      vg.nsc_g[1] = vs->nsc2_g;
      for (int i = 0; i < vs->nsc2_g; i++) vg.sc_g.push_back({1, i, 0}), vg.osc.push_back(o[i]);
      if (check_local("KVSETSC2", (int)std::count(o.begin(), o.end(), P.mev), a.spsc2 ? a.nf_sc2 : 0)) return EMI_ERR_ARG;
    }
    if (vs->kvsetsc3a) {
      if (owners(vs->kvsetsc3a, vs->nsc3a_g, "KVSETSC3A", o)) return EMI_ERR_ARG;
      vg.nsc_g[2] = vs->nsc3a_g;
      // The reference takes the variable count from UBOUND(PSPSC3A,3), which a task whose V-set owns no level still passes as a
      // zero-level array (inv_trans.F90:272-277 aborts without it).  Here such a task may have no spectral array at all, so the
      // count also travels in the KVSET block (from the grid array); without either the peers would disagree on the field list.
      // the count is UBOUND(PSPSC3A,3) wherever the task names one (also with zero levels), and the third extent of PGP3A (/ 3 with
      // LDSCDERS) must EQUAL it: inv_trans.F90:557, :587 and dir_trans.F90:451, :481 abort on `IUBOUND(3) /= IF_SC3A_G3`.  A grid array with
      // spare room would also let a task that names no PSPSC3A (count taken from the grid array) list other global fields than its peers.
      vg.nvar3a = a.sc3a_nvar > 0 ? a.sc3a_nvar : vs->nvar3a_g;
      if (vg.nvar3a <= 0) EMI_FAIL(EMI_ERR_ARG, "%s:KVSETSC3A BUT NOT PSPSC3A (number of variables unknown: pass sc3a_nvar or emi_vsets_t.nvar3a_g)", who);
      if (vs->nvar3a_g > 0 && vs->nvar3a_g != vg.nvar3a)
        EMI_FAIL(EMI_ERR_ARG, "%s:THIRD DIMENSION OF PGP3A INCONSISTENT (%d variables, IF_SC3A_G3 = %d)", who, vs->nvar3a_g, vg.nvar3a);
      for (int v = 0; v < vg.nvar3a; v++)
        for (int l = 0; l < vs->nsc3a_g; l++) vg.sc_g.push_back({2, l, v}), vg.osc.push_back(o[l]);
      if (check_local("KVSETSC3A", (int)std::count(o.begin(), o.end(), P.mev), a.spsc3a ? a.sc3a_nlev : 0)) return EMI_ERR_ARG;
    }
    if (vs->kvsetsc3b) {
      if (owners(vs->kvsetsc3b, vs->nsc3b_g, "KVSETSC3B", o)) return EMI_ERR_ARG;
      vg.nsc_g[3] = vs->nsc3b_g;
      // the count is UBOUND(PSPSC3B,3) wherever the task names one (also with zero levels), and the third extent of PGP3B (/ 3 with
      // LDSCDERS) must EQUAL it: inv_trans.F90:557, :587 and dir_trans.F90:451, :481 abort on `IUBOUND(3) /= IF_SC3B_G3`.  A grid array with
      // spare room would also let a task that names no PSPSC3B (count taken from the grid array) list other global fields than its peers.
      vg.nvar3b = a.sc3b_nvar > 0 ? a.sc3b_nvar : vs->nvar3b_g;
      if (vg.nvar3b <= 0) EMI_FAIL(EMI_ERR_ARG, "%s:KVSETSC3B BUT NOT PSPSC3B (number of variables unknown: pass sc3b_nvar or emi_vsets_t.nvar3b_g)", who);
      if (vs->nvar3b_g > 0 && vs->nvar3b_g != vg.nvar3b)
        EMI_FAIL(EMI_ERR_ARG, "%s:THIRD DIMENSION OF PGP3B INCONSISTENT (%d variables, IF_SC3B_G3 = %d)", who, vs->nvar3b_g, vg.nvar3b);
      for (int v = 0; v < vg.nvar3b; v++)
        for (int l = 0; l < vs->nsc3b_g; l++) vg.sc_g.push_back({3, l, v}), vg.osc.push_back(o[l]);
      if (check_local("KVSETSC3B", (int)std::count(o.begin(), o.end(), P.mev), a.spsc3b ? a.sc3b_nlev : 0)) return EMI_ERR_ARG;
    }
  }
  return 0;
}
// pack / unpack one block of the V-exchange: nf fields x npts points between two lists of grid-field descriptors
static int v_copy(Plan &P, const std::vector<GridFld> &src, const std::vector<GridFld> &dst, long long sp0, long long dp0, long long npts, long long snp,
                  long long dnp, std::vector<StageBuf *> &keep, emi_stream_t st) {
  const int nf = (int)src.size();
  if (nf == 0 || npts == 0) return 0;
  StageBuf *d = new StageBuf(2 * (size_t)nf * sizeof(GridFld));
  keep.push_back(d);
  if (!d->p) EMI_FAIL(EMI_ERR_RUNTIME, "V-set exchange: no device memory for %d field descriptors", nf);
  std::vector<GridFld> both(src);
  both.insert(both.end(), dst.begin(), dst.end());
  if (emi_h2d(d->p, both.data(), both.size() * sizeof(GridFld), st)) return EMI_ERR_RUNTIME;
  const long long nblk = ((long long)nf * npts + 255) / 256;
  EMI_LAUNCH_P(P.esz, k_gridcopy, nblk, 256, 0, st, (const GridFld *)d->p, (const GridFld *)d->p + nf, nf, sp0, dp0, (int)npts, (int)snp, (int)dnp);
  return 0;
}
static GridFld dense_field(void *base, size_t field, long long npts, int esz) {
  GridFld g{};
  g.base = (char *)base + field * (size_t)npts * esz;
  g.nf_arr = 1;
  g.fidx = 0;
  return g;
}

// The transform with V-sets: the W-set transform of this V-set's fields runs into (inverse) or out of (direct) a band-sized array,
// and TRLTOG (inverse) / TRGTOL (direct) moves the fields between that array and the caller's grid arrays.
static int vset_transform(Plan &P, const Call &c, bool inverse, bool adj, const char *who) {
  if (!inverse && (c.ldscders || c.ldvorgp || c.lddivgp || c.lduvder))
    EMI_FAIL(EMI_ERR_UNSUPPORTED, "INV_TRANSAD: LDSCDERS / LDVORGP / LDDIVGP / LDUVDER are not supported with NPRTRV > 1");
  VGroups vg;
  if (v_groups(P, c, who, vg)) return EMI_ERR_ARG;
  Fields f;
  if (account(c, who, inverse, &vg, f)) return EMI_ERR_ARG;
  if (f.if_gp == 0) return EMI_SUCCESS;
  const long long myp = P.vpoints(P.me, P.mev), bandp = P.ngptot;
  const int nproma = c.kproma > 0 ? c.kproma : (int)myp;
  const int ngpblks = (int)((myp - 1) / nproma + 1);
  const emi_stream_t st = c.stream;
  const bool host = c.mem_space == EMI_MEM_HOST;
  // ---- the caller's arrays on the device (spectral: local fields; grid: all fields on this task's points)
  HostStage hs(P.esz);
  const size_t gsz = (size_t)nproma * ngpblks;
  Call in;
  if (stage(P, hs, c, who, inverse, host, f, gsz, gsz != (size_t)myp, f.nvar_uv, in)) return EMI_ERR_RUNTIME;
  std::vector<GridRef> gl;
  grid_fields(f, in, f.nvar_uv, gl);
  std::vector<int> owner, nl(P.nprv, 0);  // the owner V-set of every grid field; the grid fields every V-set computes
  for (const GridRef &r : gl) {
    owner.push_back(gf_uv(r.grp) ? vg.ouv[r.i] : vg.osc[r.i]);
    nl[owner.back()]++;
  }
  const int nlm = nl[P.mev];
  // ---- the band-sized array [field][band point] of the W-set transform, and the two sides of the exchange
  StageBuf tband((size_t)nlm * bandp * P.esz), xband((size_t)nlm * bandp * P.esz), xgrid((size_t)f.if_gp * myp * P.esz);
  if ((nlm && (!tband.p || !xband.p)) || !xgrid.p) EMI_FAIL(EMI_ERR_RUNTIME, "%s: no device memory for the exchange between the V-sets", who);
  in.ext = nullptr;
  in.vsets = nullptr;
  in.gp = tband.p, in.gp_nfld = nlm, in.gpuv = in.gp3a = in.gp3b = in.gp2 = nullptr, in.kproma = (int)bandp;
  // ---- TRLTOG / TRGTOL: one all-to-all-v among the NPRTRV tasks of the band.  The block with V-set v is, on the band side, the
  // local fields on the points of sub-band v and, on the grid side, the fields of V-set v on this task's points.
  std::vector<StageBuf *> keep;
  std::vector<long long> nbb(P.nprv), ngb(P.nprv);  // bytes of the band-side and grid-side blocks
  for (int v = 0; v < P.nprv; v++) nbb[v] = (long long)nlm * P.vpoints(P.me, v) * P.esz, ngb[v] = (long long)nl[v] * myp * P.esz;
  // pack (k_gridcopy into the dense [field][point] blocks at buf) or unpack one side
  auto copy = [&](bool band, void *buf, bool pack) {
    size_t off = 0;
    for (int v = 0; v < P.nprv; v++) {
      std::vector<GridFld> arr, blk;  // the fields of block v in the band array / the caller's arrays, and in the block
      long long np = myp, p0 = 0, anp = nproma;  // points of the block; its first point and NPROMA in the arrays
      if (band) {
        np = P.vpoints(P.me, v), p0 = P.voffset(v), anp = bandp;
        for (int j = 0; j < nlm; j++) arr.push_back(GridFld{tband.p, nlm, j, 0, 0});
      } else {
        for (size_t k = 0; k < gl.size(); k++)
          if (owner[k] == v) arr.push_back(gl[k].g);
      }
      for (size_t j = 0; j < arr.size(); j++) blk.push_back(dense_field((char *)buf + off, j, np, P.esz));
      if (pack ? v_copy(P, arr, blk, p0, 0, np, anp, np, keep, st) : v_copy(P, blk, arr, 0, p0, np, np, anp, keep, st)) return true;
      off += blk.size() * (size_t)np * P.esz;
    }
    return false;
  };
  auto trans_v = [&](bool to_grid) {
    const bool bad = to_grid ? copy(true, xband.p, true) || hook_alltoallv(xband.p, nbb, xgrid.p, ngb, P.nprv, 1, P.me * P.nprv, st) || copy(false, xgrid.p, false)
                             : copy(false, xgrid.p, true) || hook_alltoallv(xgrid.p, ngb, xband.p, nbb, P.nprv, 1, P.me * P.nprv, st) || copy(true, xband.p, false);
    return bad ? EMI_ERR_RUNTIME : EMI_SUCCESS;
  };
  int rc;
  if (inverse) {
    if (nlm && (rc = wset_transform(P, in, true, adj, who)) != EMI_SUCCESS) return rc;
    rc = trans_v(true);
  } else {
    rc = trans_v(false);
    if (rc == EMI_SUCCESS && nlm) rc = wset_transform(P, in, false, adj, who);
  }
  if (host && rc == EMI_SUCCESS) hs.flush(st);
  else emi_stream_sync(st);  // the scratch buffers go back to the pool below
  for (StageBuf *k : keep) delete k;
  return rc;
}

// EMI_MEM_AUTO of a transform call: every array of the argument block is classified (emi_ptr_space); the call then runs as
// EMI_MEM_DEVICE (arrays used in place) or EMI_MEM_HOST (staged) -- or is refused when the arrays are in both places
// EMI_MEM_AUTO with several tasks: every task learns whether ANY task found its arrays in both memories, and then all of them fail together
// with the text of the offending task (one 4-byte word per task over the host collectives; host and device callers may mix between tasks,
// staging is local).  Without registered collectives (a host that drives the exchange hook only) the outcome must be identical on every
// task by the caller's construction, as include/ectrans_mi.h says.
static int agree_on_mixed_arrays(const char *who, int ndev, int nhost) {
  const int mixed = (ndev && nhost) ? 1 : 0;
  if (G.nproc_all > 1 && G.hc_gather) {
    const int NA = G.nproc_all;
    std::vector<int> all(NA, 0);
    std::vector<long long> cnt(NA, 4), dsp(NA);
    for (int r = 0; r < NA; r++) dsp[r] = 4LL * r;
    if (G.hc_gather(G.hc_user, &mixed, 4, all.data(), cnt.data(), dsp.data(), NA)) EMI_FAIL(EMI_ERR_RUNTIME, "%s: all-gather-v failed", who);
    for (int r = 0; r < NA; r++)
      if (all[r] && !mixed)
        EMI_FAIL(EMI_ERR_ARG, "%s: ARRAYS OF THE CALL ARE IN DEVICE MEMORY AND IN HOST MEMORY ON TASK %d (all of them must live in one place)", who, r + 1);
  }
  if (mixed)
    EMI_FAIL(EMI_ERR_ARG, "%s: %d ARRAYS OF THE CALL ARE IN DEVICE MEMORY AND %d IN HOST MEMORY (all of them must live in one place)", who, ndev, nhost);
  return 0;
}
// ------------------------------------------------------------------------------------------
// DIST_* / GATH_* with the local array in device memory (emi_dist_spec_m ... emi_egath_grid_m).
// Wire format of one chunk of fields: a task's send buffer holds one block per peer, in task order; a block holds the fields that
// travel between the two tasks, ascending, each as the dense run of its elements on the task that holds the local side -- GATH_*:
// the sender's nloc(me) elements of the fields whose target is the peer; DIST_*: the peer's nloc(t) elements of the fields whose
// source is the sender.  One all-to-all-v per chunk moves every field once, to where it is wanted.  The local side is packed /
// unpacked by k_spec_fields (PSPEC is field-fastest) or k_gridcopy (PGP is NPROMA-blocked); the global side by k_run_copy over
// the runs of TaskLayout, straight into / out of the caller's global array where that lives in device memory, else through a
// staged image and one copy per chunk.
// V-sets (NPRTRV > 1): the tasks are all NPROC = NPRTRW x NPRTRV, a grid field lives on every task's sub-band, a spectral field on the
// NPRTRW tasks of its V-set only (FieldSets): a block holds the fields that travel between the two tasks AND that the local side holds.
// ------------------------------------------------------------------------------------------
static int gs_run_copy(Plan &P, const void *src, void *dst, std::vector<CopyRun> &runs, int nf, std::vector<StageBuf *> &keep, emi_stream_t st) {
  if (runs.empty() || nf == 0) return 0;
  long long nblk = 0;
  for (CopyRun &r : runs) {
    r.blk0 = (int)nblk;
    nblk += (r.n + 255) / 256;
  }
  if (nblk * nf >= (1LL << 31)) EMI_FAIL(EMI_ERR_UNSUPPORTED, "global fields: %lld workgroups in one launch (lower EMI_GATH_CHUNK)", nblk * nf);
  StageBuf *d = new StageBuf(runs.size() * sizeof(CopyRun));
  keep.push_back(d);
  if (!d->p || emi_h2d(d->p, runs.data(), runs.size() * sizeof(CopyRun), st)) EMI_FAIL(EMI_ERR_RUNTIME, "global fields: no device memory for %zu runs", runs.size());
  EMI_LAUNCH_P(P.esz, k_run_copy, nblk * nf, 256, 0, st, (const RT *)src, (RT *)dst, (const CopyRun *)d->p, (int)runs.size(), (int)nblk, nf);
  return 0;
}
// the local array <-> the dense fields [w][nloc] at `wire`; slots[w]: the field of PSPEC / PGP that is wire field w
template <bool SPEC>
static int gs_local(Plan &P, void *loc, void *wire, const std::vector<int> &slots, int nfld, long long nloc, int nproma, bool to_wire, std::vector<StageBuf *> &keep,
                    emi_stream_t st) {
  const int nf = (int)slots.size();
  if (nf == 0 || nloc == 0) return 0;
  if (SPEC) {
    std::vector<SpecFld> tab(nf);
    for (int w = 0; w < nf; w++) tab[w] = SpecFld{(long long)w * nloc, slots[w], 0};
    StageBuf *d = new StageBuf(tab.size() * sizeof(SpecFld));
    keep.push_back(d);
    if (!d->p || emi_h2d(d->p, tab.data(), tab.size() * sizeof(SpecFld), st)) EMI_FAIL(EMI_ERR_RUNTIME, "spectral fields: no device memory for %d field descriptors", nf);
    const long long ntf = (nf + SF_T - 1) / SF_T, nte = (nloc + SF_T - 1) / SF_T;
    EMI_LAUNCH_P(P.esz, k_spec_fields, nte * ntf, 256, SF_LDS_BYTES(P.esz), st, (RT *)loc, (RT *)wire, (const SpecFld *)d->p, nfld, nf, nloc, (int)ntf,
                 to_wire ? 1 : 0);
    return 0;
  }
  std::vector<GridFld> arr, blk;
  for (int w = 0; w < nf; w++) {
    arr.push_back(GridFld{loc, nfld, slots[w], 0, 0});
    blk.push_back(dense_field(wire, (size_t)w, nloc, P.esz));
  }
  return to_wire ? v_copy(P, arr, blk, 0, 0, nloc, nproma, nloc, keep, st) : v_copy(P, blk, arr, 0, 0, nloc, nloc, nproma, keep, st);
}
// gath: every task's share -> global fields on their targets; else global fields on their sources -> every task's share.
// nfld counts the GLOBAL fields; the local array holds the F.nlocal(me) of them that live on this task (FieldSets).
template <bool SPEC>
static int gs_device(Plan &P, bool gath, void *glob, bool glob_dev, int nfld, const int *ktask, const FieldSets &F, const int *ksort, int kproma, void *loc,
                     const char *who) {
  const TaskLayout L = task_layout(P);
  const int esz = P.esz, NT = L.nt, me = L.me, nfl = F.nlocal(me), nproma = kproma > 0 ? kproma : (int)L.ngp[me];
  const long long nglob = SPEC ? (long long)P.nspec2g : (long long)P.ngptotg;
  auto nloc = [&](int t) { return SPEC ? L.nspec2[t] : L.ngp[t]; };
  std::vector<int> slot(nfld);
  for (int f = 0; f < nfld; f++)  // (KSORT and the presence of the arrays: checked by gs_local_args before the tasks compared)
    slot[f] = (gath || !ksort || !F.holds(me, f)) ? F.lidx[f] : ksort[F.lidx[f]] - 1;
  // the chunk rule of the host path, the same on every task: the global image of a chunk stays below 256 MiB / EMI_GATH_CHUNK
  const long long per_field = nglob * (long long)esz;
  const long long budget = (getenv("EMI_GATH_CHUNK") && *getenv("EMI_GATH_CHUNK")) ? atoll(getenv("EMI_GATH_CHUNK")) : (256LL << 20);
  const int chunk = (int)std::max<long long>(1, std::min<long long>(nfld, budget / std::max<long long>(per_field, 1)));
  // V-sets: the fields of mine that a peer holds are not evenly spaced in the global image, so every (field, run) is a run of its own
  const bool run_per_field = SPEC && P.nprv > 1;
  const emi_stream_t st = (emi_stream_t)0;
  if (plan_begin(P, st)) return EMI_ERR_RUNTIME;  // behind the last transform of the handle
  g_pt.begin(G.profile != 0, G.profile == 2);
  long long i_mine = 0;
  int rc = EMI_SUCCESS;
  for (int fa = 0; fa < nfld && rc == EMI_SUCCESS; fa += chunk) {
    const int nf = std::min(chunk, nfld - fa);
    // the fields of the chunk that this task holds, by (peer, field); cnt: of them per peer; minef: the global fields of mine;
    // held[t]: of those, the ones task t holds
    std::vector<int> order, cnt(NT, 0), minef, held(NT, 0);
    for (int t = 0; t < NT; t++)
      for (int f = fa; f < fa + nf; f++)
        if (ktask[f] == t + 1 && F.holds(me, f)) order.push_back(f), cnt[t]++;
    for (int f = fa; f < fa + nf; f++)
      if (ktask[f] == me + 1) minef.push_back(f);
    const int nmine = (int)minef.size(), nord = (int)order.size();
    std::vector<long long> boff(NT + 1, 0);  // elements of the global-side blocks of the tasks below t
    for (int t = 0; t < NT; t++) {
      for (int f : minef) held[t] += F.holds(t, f) ? 1 : 0;
      boff[t + 1] = boff[t] + (long long)held[t] * nloc(t);
    }
    std::vector<int> wslots;
    for (int f : order) wslots.push_back(slot[f]);
    // locb: the dense fields [w][nloc(me)] of the local side; globb: the blocks [task][field of mine it holds][nloc(task)] of the global side
    const size_t locbytes = (size_t)nord * nloc(me) * esz, globbytes = (size_t)nmine * nglob * esz, blkbytes = (size_t)boff[NT] * esz;
    StageBuf locb(locbytes), globb(NT > 1 ? blkbytes : 0), img(glob_dev ? 0 : globbytes);
    if ((locbytes && !locb.p) || (NT > 1 && blkbytes && !globb.p) || (!glob_dev && globbytes && !img.p))
      EMI_FAIL(EMI_ERR_RUNTIME, "%s: no device memory for the exchange buffers of %d fields", who, nf);
    void *gb = NT > 1 ? globb.p : locb.p;  // one task: the two sides are one buffer, [field][nglob]
    char *gcall = glob ? (char *)glob + (size_t)i_mine * nglob * esz : nullptr;
    void *gimg = glob_dev ? (void *)gcall : img.p;
    std::vector<StageBuf *> keep;
    std::vector<CopyRun> runs;
    for (int t = 0; t < NT && nmine; t++) {  // (global position, position in the block of task t) of every run
      if (!held[t]) continue;
      const int w = L.wset[t];
      if (run_per_field) {
        for (int j = 0, jt = 0; j < nmine; j++) {
          if (!F.holds(t, minef[j])) continue;
          for (size_t k = 0; k < L.ms[w].size(); k++) {
            const int m = L.ms[w][k];
            if (L.mlen[m] > 0) runs.push_back(CopyRun{(long long)j * nglob + L.iasm0g[m], boff[t] + (long long)jt * nloc(t) + L.start[w][k], nglob, nloc(t), (int)L.mlen[m], 0});
          }
          jt++;
        }
      } else if (SPEC) {
        for (size_t k = 0; k < L.ms[w].size(); k++) {
          const int m = L.ms[w][k];
          if (L.mlen[m] > 0) runs.push_back(CopyRun{L.iasm0g[m], boff[t] + L.start[w][k], nglob, nloc(t), (int)L.mlen[m], 0});
        }
      } else if (L.ngp[t] > 0) {
        runs.push_back(CopyRun{L.gp0[t], boff[t], nglob, nloc(t), (int)L.ngp[t], 0});
      }
    }
    const int nrf = run_per_field ? 1 : nmine;  // fields that every run stands for
    std::vector<long long> cl(NT), cg(NT);  // bytes of the local-side and the global-side block with every task
    for (int t = 0; t < NT; t++) cl[t] = (long long)cnt[t] * nloc(me) * esz, cg[t] = (long long)held[t] * nloc(t) * esz;
    bool bad;
    if (gath) {
      bad = gs_local<SPEC>(P, loc, locb.p, wslots, nfl, nloc(me), nproma, true, keep, st) || (NT > 1 && hook_alltoallv(locb.p, cl, gb, cg, NT, 1, 0, st));
      for (CopyRun &r : runs) std::swap(r.src0, r.dst0), std::swap(r.sfs, r.dfs);
      bad = bad || gs_run_copy(P, gb, gimg, runs, nrf, keep, st) || (!glob_dev && globbytes && emi_d2h(gcall, gimg, globbytes, st));
    } else {
      bad = (!glob_dev && globbytes && emi_h2d(gimg, gcall, globbytes, st)) || gs_run_copy(P, gimg, gb, runs, nrf, keep, st) ||
            (NT > 1 && hook_alltoallv(gb, cg, locb.p, cl, NT, 1, 0, st)) || gs_local<SPEC>(P, loc, locb.p, wslots, nfl, nloc(me), nproma, false, keep, st);
    }
    if (emi_stream_sync(st) && !bad) {  // the call waits for its stream: the buffers go back to the pool, the caller needs no emi_wait
      emi_set_error("%s: the kernels or copies of the call did not complete", who);
      bad = true;
    }
    for (StageBuf *k : keep) delete k;
    if (bad) rc = EMI_ERR_RUNTIME;
    i_mine += nmine;
  }
  return rc;
}
static int gs_handle(int kresol, const char *who, bool lam, Plan **out) {
  Plan *Pp = get_plan(kresol);
  if (!Pp) EMI_FAIL(EMI_ERR_STATE, "%s: unknown resolution %d", who, kresol);
  if (Pp->lam && !lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: resolution %d is a limited-area handle (ESETUP_TRANS): this routine serves the spherical transforms only", who, kresol);
  if (!Pp->lam && lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: resolution %d is not a limited-area handle: it was not set up by ESETUP_TRANS", who, kresol);
  *out = Pp;
  return 0;
}
// The local array alone selects the path; every task of a call must take the same one.  With registered host collectives the tasks
// compare (one word each) and fail together; without them it is the caller's duty, as for EMI_MEM_AUTO of the transforms.
// What one task alone can find wrong with the arguments of a device-path call, found BEFORE the tasks compare: a task that returned on its own
// would leave its peers waiting in the exchange.  The message stays in the error text of this task.
static int gs_local_args(const Plan &P, bool gath, const void *glob, int nfld, const int *ktask, const FieldSets &F, const int *ksort, const void *loc, bool host_path,
                         const char *who) {
  if (check_tasks(P, ktask, nfld, who, host_path)) return EMI_ERR_ARG;
  const int me = P.me * P.nprv + P.mev, nfl = F.nlocal(me);
  if (!loc && (nfl > 0 || P.nprv == 1)) EMI_FAIL(EMI_ERR_ARG, "%s: local array missing", who);
  int n_glob = 0, slot;
  for (int f = 0; f < nfld; f++) {
    if (!gath && F.holds(me, f) && slot_of(ksort, F.lidx[f], nfl, who, &slot)) return EMI_ERR_ARG;
    if (ktask[f] == me + 1) n_glob++;
  }
  if (n_glob && !glob)
    EMI_FAIL(EMI_ERR_ARG, gath ? "%s: this task is the target of %d fields but passes no global array" : "%s: this task is the source of %d fields but passes no global array", who, n_glob);
  return 0;
}
// mine: 0 host path, 1 device path, 2 a device global array beside a host local array, 3 arguments refused on this task (gs_local_args),
// 4 no local field on this task (a V-set that owns none of the fields): it follows the others.  kvhash: FieldSets::hash, the V-sets of
// the fields as this task names them -- tasks that disagreed on KVSET would wait for blocks that nobody sends.  *path: the agreed path.
static int gs_agree_on_path(const char *who, int mine, unsigned kvhash, int *path) {
  const int word[2] = {mine, (int)kvhash};
  std::vector<int> all(word, word + 2);
  if (G.nproc_all > 1 && G.hc_gather) {
    const int NA = G.nproc_all;
    all.assign(2 * (size_t)NA, 0);
    std::vector<long long> cnt(NA, 8), dsp(NA);
    for (int r = 0; r < NA; r++) dsp[r] = 8LL * r;
    if (G.hc_gather(G.hc_user, word, 8, all.data(), cnt.data(), dsp.data(), NA)) EMI_FAIL(EMI_ERR_RUNTIME, "%s: all-gather-v failed", who);
  }
  const size_t n = all.size() / 2;
  if (mine == 3) return EMI_ERR_ARG;  // (with this task's own message)
  for (size_t r = 0; r < n; r++)
    if (all[2 * r] == 3) EMI_FAIL(EMI_ERR_ARG, "%s: TASK %d REFUSED ITS ARGUMENTS (its error text says why); no task of the call went on", who, (int)r + 1);
  for (size_t r = 0; r < n; r++)
    if (all[2 * r + 1] != word[1]) EMI_FAIL(EMI_ERR_ARG, "%s: KVSET DIFFERS BETWEEN TASKS (here and on task %d); no task of the call went on", who, (int)r + 1);
  for (size_t r = 0; r < n; r++)
    if (all[2 * r] == 2)
      EMI_FAIL(EMI_ERR_ARG, "%s: THE GLOBAL ARRAY IS IN DEVICE MEMORY AND THE LOCAL ARRAY IN HOST MEMORY ON TASK %d (a host local array takes the host path)", who,
               n > 1 ? (int)r + 1 : G.myproc_all);
  *path = -1;
  for (size_t r = 0; r < n; r++) {
    if (all[2 * r] == 4) continue;
    if (*path < 0) *path = all[2 * r];
    if (mine != 4 && all[2 * r] != mine)
      EMI_FAIL(EMI_ERR_ARG, "%s: THE LOCAL ARRAY IS IN %s MEMORY HERE AND IN %s MEMORY ON TASK %d (every task of a call must take the same path)", who,
               mine ? "DEVICE" : "HOST", mine ? "HOST" : "DEVICE", (int)r + 1);
    if (mine == 4 && all[2 * r] != *path)
      EMI_FAIL(EMI_ERR_ARG, "%s: THE LOCAL ARRAY IS IN HOST MEMORY ON SOME TASKS AND IN DEVICE MEMORY ON OTHERS, AS ON TASK %d (every task of a call must take the same path)",
               who, (int)r + 1);
  }
  return 0;
}
template <bool SPEC>
static int gs_m(bool gath, int kresol, int glob_space, const void *glob, int nfld, const int *ktask, const int *kvset, const int *ksort, int kproma, int loc_space,
                const void *loc, const char *who, bool lam) {
  Plan *Pp;
  if (int rc = gs_handle(kresol, who, lam, &Pp)) return rc;
  for (int sp : {glob_space, loc_space})
    if (sp != EMI_MEM_HOST && sp != EMI_MEM_DEVICE && sp != EMI_MEM_AUTO)
      EMI_FAIL(EMI_ERR_ARG, "%s: memory space %d (EMI_MEM_HOST, EMI_MEM_DEVICE or EMI_MEM_AUTO)", who, sp);
  if (lam && kvset) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: KVSET: V-sets are not available on a limited-area handle", who);
  if (glob_space == EMI_MEM_AUTO) glob_space = emi_ptr_space(glob);
  if (loc_space == EMI_MEM_AUTO) loc_space = emi_ptr_space(loc);
  const bool glob_dev = glob && glob_space == EMI_MEM_DEVICE, loc_dev = loc_space == EMI_MEM_DEVICE;
  const Plan &P = *Pp;
  // With V-sets the arguments are looked at on both paths before the tasks compare (a task of another V-set sees nothing wrong with
  // a field it does not hold); with NPRTRV = 1 the host path finds its own errors, as it always did.
  FieldSets F;
  int word;
  if (field_sets(P, SPEC, nfld, kvset, who, F))
    word = 3;
  else if (P.nprv > 1 && F.nlocal(P.me * P.nprv + P.mev) == 0 && !gs_local_args(P, gath, glob, nfld, ktask, F, ksort, loc, !loc_dev, who))
    word = 4;
  else if (!loc_dev && glob_dev)
    word = 2;
  else if (!loc_dev)
    word = (P.nprv > 1 && gs_local_args(P, gath, glob, nfld, ktask, F, ksort, loc, true, who)) ? 3 : 0;
  else
    word = gs_local_args(P, gath, glob, nfld, ktask, F, ksort, loc, false, who) ? 3 : 1;
  int path = 0;
  if (gs_agree_on_path(who, word, F.hash(), &path)) return EMI_ERR_ARG;
  if (path < 0) path = loc_dev ? 1 : 0;  // (no task holds a field: nothing moves)
  if (word == 4 && path == 0 && glob_dev) EMI_FAIL(EMI_ERR_ARG, "%s: THE GLOBAL ARRAY IS IN DEVICE MEMORY AND THE CALL TAKES THE HOST PATH", who);
  if (path == 0)
    return gath ? gath_impl<SPEC>(kresol, (void *)glob, nfld, ktask, kvset, kproma, loc, who, lam)
                : dist_impl<SPEC>(kresol, glob, nfld, ktask, kvset, ksort, kproma, (void *)loc, who, lam);
  return gs_device<SPEC>(*Pp, gath, (void *)glob, glob_dev, nfld, ktask, F, ksort, kproma, (void *)loc, who);
}
#define EMI_GS_M(pre, PRE, lam)                                                                                                                                          \
  extern "C" int emi_##pre##dist_spec_m(int kresol, int glob_space, const void *specg, int nfld, const int *kfrom, const int *ksort, int loc_space, void *spec) {          \
    return gs_m<true>(false, kresol, glob_space, specg, nfld, kfrom, nullptr, ksort, 0, loc_space, spec, PRE "DIST_SPEC", lam);                                                    \
  }                                                                                                                                                                        \
  extern "C" int emi_##pre##gath_spec_m(int kresol, int glob_space, void *specg, int nfld, const int *kto, int loc_space, const void *spec) {                             \
    return gs_m<true>(true, kresol, glob_space, specg, nfld, kto, nullptr, nullptr, 0, loc_space, spec, PRE "GATH_SPEC", lam);                                                    \
  }                                                                                                                                                                        \
  extern "C" int emi_##pre##dist_grid_m(int kresol, int glob_space, const void *gpg, int nfld, const int *kfrom, const int *ksort, int kproma, int loc_space, void *gp) { \
    return gs_m<false>(false, kresol, glob_space, gpg, nfld, kfrom, nullptr, ksort, kproma, loc_space, gp, PRE "DIST_GRID", lam);                                                  \
  }                                                                                                                                                                        \
  extern "C" int emi_##pre##gath_grid_m(int kresol, int glob_space, void *gpg, int nfld, const int *kto, int kproma, int loc_space, const void *gp) {                     \
    return gs_m<false>(true, kresol, glob_space, gpg, nfld, kto, nullptr, nullptr, kproma, loc_space, gp, PRE "GATH_GRID", lam);                                                  \
  }
EMI_GS_M(, "", false)
EMI_GS_M(e, "E", true)
#undef EMI_GS_M
// DIST_SPEC / GATH_SPEC with KVSET (dist_spec.h, gath_spec.h): the _m forms with the V-set of every global field.  kvset NULL with
// NPRTRV = 1: the _m calls.
extern "C" int emi_dist_spec_v(int kresol, int glob_space, const void *specg, int nfld_g, const int *kfrom, const int *kvset, const int *ksort, int loc_space,
                               void *spec) {
  return gs_m<true>(false, kresol, glob_space, specg, nfld_g, kfrom, kvset, ksort, 0, loc_space, spec, "DIST_SPEC", false);
}
extern "C" int emi_gath_spec_v(int kresol, int glob_space, void *specg, int nfld_g, const int *kto, const int *kvset, int loc_space, const void *spec) {
  return gs_m<true>(true, kresol, glob_space, specg, nfld_g, kto, kvset, nullptr, 0, loc_space, spec, "GATH_SPEC", false);
}

template <class A>
static int resolve_call(const char *who, const A *ap, A &a) {
  if (!ap) EMI_FAIL(EMI_ERR_ARG, "%s: null argument block", who);
  a = *ap;
  return resolve_space(who, ap->mem_space, {ap->spvor, ap->spdiv, ap->spscalar, ap->spsc3a, ap->spsc3b, ap->spsc2, ap->gp, ap->gpuv, ap->gp3a, ap->gp3b, ap->gp2},
                       &a.mem_space, true);
}
// INV_TRANS / DIR_TRANSAD run the inverse pipeline, DIR_TRANS / INV_TRANSAD the direct one
static int transform(int kresol, const Call &c, bool inverse, bool adj, bool lam = false) {
  const char *who = lam ? (inverse ? (adj ? "EDIR_TRANSAD" : "EINV_TRANS") : (adj ? "EINV_TRANSAD" : "EDIR_TRANS")) : inverse ? (adj ? "DIR_TRANSAD" : "INV_TRANS") : (adj ? "INV_TRANSAD" : "DIR_TRANS");
  Plan *Pp = get_plan(kresol);
  if (!Pp) EMI_FAIL(EMI_ERR_STATE, "%s: unknown resolution %d", who, kresol);
  if (Pp->lam && !lam)
    EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: resolution %d is a limited-area handle (ESETUP_TRANS): it serves EINV_TRANS, EDIR_TRANS and their adjoints", who, kresol);
  if (!Pp->lam && lam) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: resolution %d is not a limited-area handle: it was not set up by ESETUP_TRANS", who, kresol);
  if (lam && c.vsets) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: KVSET arguments: V-sets are not available on a limited-area handle", who);
  // A handle set up with LDLL holds the inverse panels of its lat-lon rows and nothing else: no Gaussian grid beside them (the
  // reference keeps both on one handle), no Gaussian weights, no panels of the direct transform
  if (Pp->ldll && !(inverse && !adj))
    EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: not available on a handle set up with LDLL (it serves INV_TRANS with LDLATLON only)", who);
  if (Pp->ldll && !c.ldlatlon)
    EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: a handle set up with LDLL holds no Gaussian grid: call it with LDLATLON=.TRUE.", who);
  if (!Pp->ldll && c.ldlatlon) EMI_FAIL(EMI_ERR_UNSUPPORTED, "%s: LDLATLON needs a handle set up with LDLL", who);
  return G.nprtrv > 1 ? vset_transform(*Pp, c, inverse, adj, who) : wset_transform(*Pp, c, inverse, adj, who);
}
extern "C" int emi_inv_trans(int kresol, const emi_invtrans_t *args) {
  EmiRange rg(EMI_LBL_INV);  // GSTATS 4
  emi_invtrans_t a;
  if (resolve_call("INV_TRANS", args, a)) return EMI_ERR_ARG;
  return transform(kresol, to_call(a), true, false);
}
extern "C" int emi_dir_trans(int kresol, const emi_dirtrans_t *args) {
  EmiRange rg(EMI_LBL_DIR);  // GSTATS 5
  emi_dirtrans_t a;
  if (resolve_call("DIR_TRANS", args, a)) return EMI_ERR_ARG;
  return transform(kresol, to_call(a), false, false);
}
// EINV_TRANS / EDIR_TRANS (etrans/include/etrans/einv_trans.h, edir_trans.h): the argument blocks of INV_TRANS / DIR_TRANS on a handle of
// ESETUP_TRANS, plus the mean wind PMEANU / PMEANV(nf_uv) -- the (0, 0) coefficients of u and v, which vorticity and divergence do not hold
extern "C" int emi_einv_trans(int kresol, const emi_invtrans_t *args, const void *meanu, const void *meanv) {
  EmiRange rg(EMI_LBL_INV);
  emi_invtrans_t a;
  if (resolve_call("EINV_TRANS", args, a)) return EMI_ERR_ARG;
  if (a.ldlatlon) EMI_FAIL(EMI_ERR_UNSUPPORTED, "EINV_TRANS: LDLATLON is not available on a limited-area handle");
  Call c = to_call(a);
  c.meanu = (void *)meanu, c.meanv = (void *)meanv;
  return transform(kresol, c, true, false, true);
}
extern "C" int emi_edir_trans(int kresol, const emi_dirtrans_t *args, void *meanu, void *meanv) {
  EmiRange rg(EMI_LBL_DIR);
  emi_dirtrans_t a;
  if (resolve_call("EDIR_TRANS", args, a)) return EMI_ERR_ARG;
  Call c = to_call(a);
  c.meanu = meanu, c.meanv = meanv;
  return transform(kresol, c, false, false, true);
}
// EINV_TRANSAD / EDIR_TRANSAD (etrans/include/etrans/einv_transad.h, edir_transad.h): the argument blocks of the forward routines with the
// intents swapped, for plain Euclidean inner products on both sides (the means among the spectral entries).  Outputs are overwritten.
extern "C" int emi_einv_transad(int kresol, const emi_invtrans_t *args, void *meanu, void *meanv) {
  emi_invtrans_t a;
  if (resolve_call("EINV_TRANSAD", args, a)) return EMI_ERR_ARG;
  if (a.ldlatlon) EMI_FAIL(EMI_ERR_UNSUPPORTED, "EINV_TRANSAD: LDLATLON is not available on a limited-area handle");
  Call c = to_call(a);
  c.meanu = meanu, c.meanv = meanv;
  return transform(kresol, c, false, true, true);
}
extern "C" int emi_edir_transad(int kresol, const emi_dirtrans_t *args, const void *meanu, const void *meanv) {
  emi_dirtrans_t a;
  if (resolve_call("EDIR_TRANSAD", args, a)) return EMI_ERR_ARG;
  Call c = to_call(a);
  c.meanu = (void *)meanu, c.meanv = (void *)meanv;
  return transform(kresol, c, true, true, true);
}
extern "C" int emi_wait(int kresol) {
  if (!G.init) EMI_FAIL(EMI_ERR_STATE, "emi_wait: SETUP_TRANS0 has not been called");
  if (kresol > 0) {
    Plan *Pp = get_plan(kresol);
    if (!Pp) EMI_FAIL(EMI_ERR_STATE, "emi_wait: unknown resolution %d", kresol);
    if (const int rc = plan_quiesce(*Pp)) EMI_FAIL(EMI_ERR_RUNTIME, "emi_wait: the last call of resolution %d did not complete (%s)", kresol, emi_rt_errstr(rc));
    return EMI_SUCCESS;
  }
  for (size_t i = 0; i < G.plans.size(); i++) {
    Plan *Pp = G.plans[i].get();
    if (!Pp) continue;
    if (const int rc = plan_quiesce(*Pp)) EMI_FAIL(EMI_ERR_RUNTIME, "emi_wait: the last call of resolution %d did not complete (%s)", (int)i, emi_rt_errstr(rc));
  }
  return EMI_SUCCESS;
}

// INV_TRANSAD (include/ectrans/inv_transad.h): arguments of INV_TRANS with the intents swapped.  LDSCDERS / LDVORGP / LDDIVGP /
// LDUVDER: the grid arrays then carry the derivative / vorticity / divergence inputs in INV_TRANS's layout (ltinvad_mod.F90:149-225,
// spnsdead_mod.F90, fscad_mod.F90)
extern "C" int emi_inv_transad(int kresol, const emi_invtrans_t *ap) {
  emi_invtrans_t a;
  if (resolve_call("INV_TRANSAD", ap, a)) return EMI_ERR_ARG;
  return transform(kresol, to_call(a), false, true);
}
// DIR_TRANSAD (include/ectrans/dir_transad.h): arguments of DIR_TRANS with the intents swapped
extern "C" int emi_dir_transad(int kresol, const emi_dirtrans_t *ap) {
  emi_dirtrans_t d;
  if (resolve_call("DIR_TRANSAD", ap, d)) return EMI_ERR_ARG;
  return transform(kresol, to_call(d), true, true);
}

#if defined(EMI_MR_STAMP) && !defined(EMI_CPU_EMU)
// experiments only (-DEMI_MR_STAMP): read and clear the stage clocks of k_fft_dir_mr
extern "C" int emi_debug_mr_stamps(unsigned long long *out) {
  hipDeviceSynchronize();
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(emi_mr_stamp), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
  unsigned long long z[16] = {0};
  return hipMemcpyToSymbol(HIP_SYMBOL(emi_mr_stamp), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif
