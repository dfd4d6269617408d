"""ectrans_amd -- Python host mirror of the ecTrans API over libectrans_mi.so (C-ABI, HIP).

The names and argument meaning follow the reference Fortran interface
(/root/reference/src/trans/include/ectrans/{setup_trans0,setup_trans,inv_trans,dir_trans,
trans_inq,specnorm}.h): ``setup_trans0``, ``setup_trans`` (returns KRESOL), ``inv_trans``,
``dir_trans``, ``trans_inq``, ``specnorm``, ``trans_release``, ``trans_end``.  Errors that the
reference reports through ABORT_TRANS are raised as :class:`TransError` with the same text.

Arrays are passed with the *Fortran* index order reversed (C-contiguous):
``PSPEC(nfld, nspec2)`` is a ``(nspec2, nfld)`` array, ``PGP(nproma, nfld, ngpblks)`` is
``(ngpblks, nfld, nproma)``, ``PSPSC3A(nlev, nspec2, nvar)`` is ``(nvar, nspec2, nlev)``,
``PGPUV(nproma, nlev, nvar, ngpblks)`` is ``(ngpblks, nvar, nlev, nproma)``.
numpy arrays are staged through PCIe (EMI_MEM_HOST); torch CUDA tensors are used in place
(EMI_MEM_DEVICE); the ``mem_space`` keyword of the calls that take arrays overrides this.  There is no CPU implementation in this package: without the HIP library
and a GPU every call fails loudly.
"""
import ctypes as C
import os

import numpy as np

__all__ = ["TransError", "setup_trans0", "setup_trans", "inv_trans", "dir_trans", "trans_inq", "specnorm",
           "trans_release", "trans_end", "lib", "build", "esetup_trans", "einv_trans", "edir_trans", "etrans_inq",
           "einv_transad", "edir_transad", "fpbipere", "etibihie", "horiz_field", "boyd_window"]

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.path.join(_HERE, "libectrans_mi.so")
_L = None

EMI_MEM_HOST, EMI_MEM_DEVICE, EMI_MEM_AUTO = 0, 1, 2


class TransError(RuntimeError):
    """What the reference would have reported through ABORT_TRANS."""


class _Init(C.Structure):
    _fields_ = [("kmax_resol", C.c_int), ("kprintlev", C.c_int), ("prad", C.c_double), ("nproc", C.c_int),
                ("myproc", C.c_int), ("device", C.c_int), ("nprtrv", C.c_int)]


class _VSets(C.Structure):  # emi_vsets_t
    _fields_ = [("kvsetuv", C.POINTER(C.c_int)), ("nuv_g", C.c_int), ("kvsetsc", C.POINTER(C.c_int)), ("nsc_g", C.c_int),
                ("kvsetsc2", C.POINTER(C.c_int)), ("nsc2_g", C.c_int), ("kvsetsc3a", C.POINTER(C.c_int)), ("nsc3a_g", C.c_int),
                ("kvsetsc3b", C.POINTER(C.c_int)), ("nsc3b_g", C.c_int), ("nvar3a_g", C.c_int), ("nvar3b_g", C.c_int)]


class _LegpolIO(C.Structure):
    _fields_ = [("io", C.c_char_p), ("fname", C.c_char_p), ("ptr", C.c_void_p), ("len", C.c_size_t)]


class _Setup(C.Structure):
    _fields_ = [("ksmax", C.c_int), ("kdgl", C.c_int), ("kloen", C.POINTER(C.c_int)), ("kdlon", C.c_int),
                ("precision", C.c_int), ("lduseflt", C.c_int), ("ldll", C.c_int), ("ldstretch", C.c_int),
                ("lduserpnm", C.c_int), ("ldshiftll", C.c_int)]


class _ESetup(C.Structure):  # emi_esetup_t
    _fields_ = [("kmsmax", C.c_int), ("ksmax", C.c_int), ("kdgl", C.c_int), ("kloen", C.POINTER(C.c_int)), ("kdlon", C.c_int),
                ("kdgux", C.c_int), ("pexwn", C.c_double), ("peywn", C.c_double), ("precision", C.c_int)]


class _Ext(C.Structure):  # emi_extents_t
    _fields_ = [("sp_dim2", C.c_int), ("gp", C.c_int * 3), ("gpuv", C.c_int * 4), ("gp3a", C.c_int * 4),
                ("gp3b", C.c_int * 4), ("gp2", C.c_int * 3)]


class _Inv(C.Structure):
    _fields_ = [("mem_space", C.c_int), ("spvor", C.c_void_p), ("spdiv", C.c_void_p), ("nf_uv", C.c_int),
                ("spscalar", C.c_void_p), ("nf_scalar", C.c_int), ("spsc3a", C.c_void_p), ("sc3a_nlev", C.c_int),
                ("sc3a_nvar", C.c_int), ("spsc3b", C.c_void_p), ("sc3b_nlev", C.c_int), ("sc3b_nvar", C.c_int),
                ("spsc2", C.c_void_p), ("nf_sc2", C.c_int), ("ldscders", C.c_int), ("ldvorgp", C.c_int),
                ("lddivgp", C.c_int), ("lduvder", C.c_int), ("kproma", C.c_int), ("gp", C.c_void_p),
                ("gp_nfld", C.c_int), ("gpuv", C.c_void_p), ("gp3a", C.c_void_p), ("gp3b", C.c_void_p),
                ("gp2", C.c_void_p), ("stream", C.c_void_p), ("ext", C.POINTER(_Ext)), ("vsets", C.POINTER(_VSets)),
                ("ldlatlon", C.c_int)]


class _Dir(C.Structure):
    _fields_ = [("mem_space", C.c_int), ("spvor", C.c_void_p), ("spdiv", C.c_void_p), ("nf_uv", C.c_int),
                ("spscalar", C.c_void_p), ("nf_scalar", C.c_int), ("spsc3a", C.c_void_p), ("sc3a_nlev", C.c_int),
                ("sc3a_nvar", C.c_int), ("spsc3b", C.c_void_p), ("sc3b_nlev", C.c_int), ("sc3b_nvar", C.c_int),
                ("spsc2", C.c_void_p), ("nf_sc2", C.c_int), ("kproma", C.c_int), ("gp", C.c_void_p),
                ("gp_nfld", C.c_int), ("gpuv", C.c_void_p), ("gp3a", C.c_void_p), ("gp3b", C.c_void_p),
                ("gp2", C.c_void_p), ("stream", C.c_void_p), ("ext", C.POINTER(_Ext)), ("vsets", C.POINTER(_VSets))]


def build(force=False):
    """Compile libectrans_mi.so for gfx950 with hipcc (in-tree)."""
    import subprocess
    src = os.path.join(_HERE, "csrc", "ectrans_mi.hip")
    deps = [src] + [os.path.join(_HERE, "csrc", f) for f in ("emi_kernels.h", "emi_kernels_body.h", "emi_mr_body.h", "emi_biper_body.h", "emi_mr_tables.h", "emi_types.h", "emi_rt.h", "emi_setup.h", "emi_stage.h")]
    deps.append(os.path.join(os.path.dirname(_HERE), "include", "ectrans_mi.h"))
    if not force and os.path.exists(_LIBPATH) and all(os.path.getmtime(_LIBPATH) >= os.path.getmtime(d) for d in deps):
        return _LIBPATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-o", _LIBPATH, src]
    subprocess.check_call(cmd)
    return _LIBPATH


def source_hash():
    """First 16 hex digits of the SHA-256 over the library sources (csrc/* and the C-ABI header): profiles/*_pmc_traffic.json
    is stamped with it, and bench.py quotes a counter file only for the build it was taken on."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc")))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "ectrans_mi.h"))
    for f in files:
        if os.path.isfile(f):
            h.update(os.path.basename(f).encode() + b"\0" + open(f, "rb").read())
    return h.hexdigest()[:16]


def _bind(L):
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.emi_init.argtypes = [C.POINTER(_Init)]
    L.emi_setup.argtypes = [C.POINTER(_Setup), ip]
    L.emi_setup_legpol.argtypes = [C.POINTER(_Setup), C.POINTER(_LegpolIO), ip]
    L.emi_inq_int.argtypes = [C.c_int, C.c_char_p, ip]
    L.emi_inq_int_array.argtypes = [C.c_int, C.c_char_p, ip, C.c_int]
    L.emi_inq_real_array.argtypes = [C.c_int, C.c_char_p, dp, C.c_int]
    L.emi_inq_legendre.argtypes = [C.c_int, C.c_int, C.c_int, dp, ip, ip]
    L.emi_inv_trans.argtypes = [C.c_int, C.POINTER(_Inv)]
    L.emi_dir_trans.argtypes = [C.c_int, C.POINTER(_Dir)]
    L.emi_specnorm.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, dp]
    L.emi_inv_transad.argtypes = [C.c_int, C.POINTER(_Inv)]
    L.emi_dir_transad.argtypes = [C.c_int, C.POINTER(_Dir)]
    L.emi_release.argtypes = [C.c_int]
    L.emi_finalize.argtypes = []
    L.emi_trim_cache.argtypes = []
    L.emi_last_error.restype = C.c_char_p
    L.emi_work_model.argtypes = [C.c_int, C.c_int, dp, dp, dp]
    L.emi_last_phase_ms.argtypes = [dp]
    L.emi_set_max_batch.argtypes = [C.c_int]
    L.emi_specnorm_partial.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, dp]
    L.emi_gpnorm.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, dp, dp, dp, C.c_int]
    L.emi_vordiv_to_uv.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    if hasattr(L, "emi_ptr_space"):  # (an older build loaded for an A/B run, tools/ab_libs.sh)
        L.emi_ptr_space.argtypes = [C.c_void_p]
        L.emi_wait.argtypes = [C.c_int]
    L.emi_specnorm_kvset.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, dp]
    L.emi_set_alltoallv.argtypes = [C.c_void_p, C.c_void_p]
    L.emi_set_profile.argtypes = [C.c_int]
    L.emi_last_phase_launches.argtypes = [ip]
    if hasattr(L, "emi_last_exchange"):  # (an older build loaded for an A/B run)
        L.emi_last_exchange.argtypes = [dp, ip, dp]
        L.emi_last_fft_launches.argtypes = [C.POINTER(C.c_longlong)]
    L.emi_crc64.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_ulonglong)]
    L.emi_set_host_collectives.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.emi_dist_spec.argtypes = [C.c_int, C.c_void_p, C.c_int, ip, ip, C.c_void_p]
    L.emi_gath_spec.argtypes = [C.c_int, C.c_void_p, C.c_int, ip, C.c_void_p]
    L.emi_dist_grid.argtypes = [C.c_int, C.c_void_p, C.c_int, ip, ip, C.c_int, C.c_void_p]
    L.emi_gath_grid.argtypes = [C.c_int, C.c_void_p, C.c_int, ip, C.c_int, C.c_void_p]
    L.emi_inq_tasks.argtypes = [ip, ip]
    if hasattr(L, "emi_dist_spec_m"):  # (an older build loaded for an A/B run)
        for e in ("", "e"):
            getattr(L, "emi_%sdist_spec_m" % e).argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, ip, ip, C.c_int, C.c_void_p]
            getattr(L, "emi_%sgath_spec_m" % e).argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, ip, C.c_int, C.c_void_p]
            getattr(L, "emi_%sdist_grid_m" % e).argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, ip, ip, C.c_int, C.c_int, C.c_void_p]
            getattr(L, "emi_%sgath_grid_m" % e).argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, ip, C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "emi_dist_spec_v"):  # (an older build loaded for an A/B run)
        L.emi_dist_spec_v.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, ip, ip, ip, C.c_int, C.c_void_p]
        L.emi_gath_spec_v.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, ip, ip, C.c_int, C.c_void_p]
    L.emi_inq_init.argtypes = [ip, dp]
    L.emi_set_nprtrv.argtypes = [C.c_int]
    if hasattr(L, "emi_esetup"):  # (an older build loaded for an A/B run)
        L.emi_esetup.argtypes = [C.POINTER(_ESetup), ip]
        L.emi_einv_trans.argtypes = [C.c_int, C.POINTER(_Inv), C.c_void_p, C.c_void_p]
        L.emi_edir_trans.argtypes = [C.c_int, C.POINTER(_Dir), C.c_void_p, C.c_void_p]
        L.emi_einv_transad.argtypes = [C.c_int, C.POINTER(_Inv), C.c_void_p, C.c_void_p]
        L.emi_edir_transad.argtypes = [C.c_int, C.POINTER(_Dir), C.c_void_p, C.c_void_p]
    if hasattr(L, "emi_especnorm"):  # (an older build loaded for an A/B run)
        L.emi_especnorm.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, dp]
        L.emi_especnorm_partial.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, dp]
        L.emi_egpnorm.argtypes = L.emi_gpnorm.argtypes
        L.emi_edist_spec.argtypes = L.emi_dist_spec.argtypes
        L.emi_egath_spec.argtypes = L.emi_gath_spec.argtypes
        L.emi_edist_grid.argtypes = L.emi_dist_grid.argtypes
        L.emi_egath_grid.argtypes = L.emi_gath_grid.argtypes
    if hasattr(L, "emi_specnorm_met"):  # (an older build loaded for an A/B run)
        L.emi_specnorm_met.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, dp]
        L.emi_specnorm_met_partial.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, dp]
        L.emi_specnorm_last_ms.argtypes = [dp]
    if hasattr(L, "emi_fpbipere"):  # (an older build loaded for an A/B run)
        L.emi_fpbipere.argtypes = [C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 9 + [ip, dp]
        L.emi_etibihie.argtypes = [C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 10
        L.emi_boyd_window.argtypes = [C.c_int, C.c_double, C.c_int, C.c_void_p]
        L.emi_horiz_field.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.emi_biper_last_ms.argtypes = [dp]
    return L


_EMULATOR = [False]  # set by _use_library_for_tests alone


def lib():
    """The HIP shared library.  No fallback: a missing library is an error."""
    global _L
    if _L is None:
        _EMULATOR[0] = False
        if not os.path.exists(_LIBPATH):
            raise TransError("libectrans_mi.so is not built (run __graft_entry__.build()); "
                             "ectrans_amd has no CPU implementation")
        _L = _bind(C.CDLL(_LIBPATH))
    return _L


def _use_library_for_tests(path):
    """tests/emu only: point the wrapper at the CPU functional emulator build."""
    global _L
    _L = _bind(C.CDLL(path))
    _EMULATOR[0] = True
    return _L


def _chk(rc):
    if rc != 0:
        raise TransError(lib().emi_last_error().decode())


def _is_torch(a):
    return a is not None and type(a).__module__.startswith("torch")


def _ptr(a, space):
    """(pointer, keep-alive object) of an array living in `space`."""
    if a is None:
        return None, None
    if _is_torch(a):
        if not a.is_contiguous() or str(a.dtype) != "torch." + space[1]:
            raise TransError("device arrays must be contiguous %s tensors" % space[1])
        if space[0] is None:
            space[0] = EMI_MEM_DEVICE if a.is_cuda else EMI_MEM_HOST
        elif space[0] != (EMI_MEM_DEVICE if a.is_cuda else EMI_MEM_HOST):
            raise TransError("all arrays of one call must live in the same memory space")
        return a.data_ptr(), a
    if not (isinstance(a, np.ndarray) and a.dtype == np.dtype(space[1]) and a.flags.c_contiguous):
        raise TransError("host arrays must be C-contiguous %s numpy arrays" % space[1])
    if space[0] is None:
        space[0] = EMI_MEM_HOST
    elif space[0] != EMI_MEM_HOST:
        raise TransError("all arrays of one call must live in the same memory space")
    return a.ctypes.data, a


def _space(mem_space, space):
    """The memory space of a call: `mem_space` where the caller gives one, else what the arrays said (host where there are none)."""
    return int(mem_space) if mem_space is not None else space[0] if space[0] is not None else EMI_MEM_HOST


_DIST = {"nproc": 1, "nprtrv": 1, "group": None, "device": None}


def setup_trans0(kmax_resol=1, kprintlev=0, prad=None, device=-1, kprtrw=1, myproc=1, group=None, alltoallv=None,
                 transport="torch", kprtrv=1, **unsupported):
    """SETUP_TRANS0 (setup_trans0.h:12-89).

    kprtrw > 1: this process is task `myproc` (1-based) of a W-set of `kprtrw` tasks, one per GPU
    (NPRTRV = NPRGPEW = 1); the all-to-all-v between them defaults to torch.distributed on `group`
    (RCCL for CUDA devices, gloo on the CPU test tier) -- see ectrans_amd.dist.
    kprtrv > 1: NPRTRV V-sets (sump_trans0_mod.F90:49): kprtrw x kprtrv tasks, task `myproc` is (MYSETW, MYSETV) =
    ((myproc - 1) // kprtrv + 1, (myproc - 1) % kprtrv + 1); fields are dealt to the V-sets by the kvset* arguments of the
    transforms.
    transport="rccl": the native transport of ectrans_amd/rccl instead (what a Fortran host attaches: grouped
    ncclSend / ncclRecv on the library's stream, no Python callback per field batch); `group` only carries the
    128-byte unique id and the small reductions of SPECNORM."""
    for k, v in unsupported.items():
        if k.lower() in ("kprgpns", "kprgpew") and v not in (None, 1, kprtrw, kprtrw * kprtrv):
            raise TransError("SETUP_TRANS0: %s=%r: only the W-set decomposition (KPRTRW tasks) is supported" % (k, v))
    nproc_all = kprtrw * max(1, kprtrv)
    if transport == "rccl":
        from . import dist as _dist
        if kprtrv > 1:
            _chk(lib().emi_set_nprtrv(int(kprtrv)))
        _dist.rccl_native_attach(nproc_all, myproc, kmax_resol, kprintlev, prad, device, group)  # calls emi_init itself
        _DIST.update(nproc=nproc_all, nprtrv=max(1, kprtrv), group=group if nproc_all > 1 else None,
                     device=("cuda:%d" % device) if nproc_all > 1 and device is not None and device >= 0 else None)
        return
    if nproc_all > 1:
        from . import dist as _dist
        dev = ("cuda:%d" % device) if device is not None and device >= 0 else "cpu"
        hook = alltoallv if alltoallv is not None else _dist.make_alltoallv_hook(group, dev, p2p=kprtrv > 1)
        _chk(lib().emi_set_alltoallv(C.cast(hook, C.c_void_p), None))
        bc, ag = _dist.make_host_collectives(group, dev)  # DIST_x / GATH_x, SPECNORM over several tasks
        _chk(lib().emi_set_host_collectives(C.cast(bc, C.c_void_p), C.cast(ag, C.c_void_p), None))
        _DIST.update(nproc=nproc_all, nprtrv=max(1, kprtrv), group=group, device=dev)
    else:
        _DIST.update(nproc=1, nprtrv=1, group=None, device=None)
    cfg = _Init(kmax_resol, kprintlev, prad if prad else 0.0, nproc_all, myproc, device if device is not None else -1, max(1, kprtrv))
    _chk(lib().emi_init(C.byref(cfg)))


def inq_init():
    """(KMAX_RESOL, PRAD) the library was initialised with (emi_inq_init): what a host that adopts an attached transport's
    initialisation compares its own SETUP_TRANS0 arguments with."""
    k, r = C.c_int(0), C.c_double(0.0)
    _chk(lib().emi_inq_init(C.byref(k), C.byref(r)))
    return k.value, r.value


_PREC = {}  # kresol -> array dtype name of that resolution


def setup_trans(ksmax, kdgl, kloen=None, kdlon=0, lduseflt=False, ldll=False, pstret=None, precision=8,
                cdio_legpol=None, cdlegpolfname=None, klegpolptr=None, klegpolptr_len=None, lduserpnm=False,
                ldshiftll=False):
    """SETUP_TRANS (setup_trans.h:12-115); returns KRESOL.

    cdio_legpol: "writef" writes the Legendre polynomials of this setup to `cdlegpolfname`, "readf" takes
    them from that file, "membuf" from the file image `klegpolptr` (bytes-like or numpy array, or an
    address with `klegpolptr_len`) -- the reference's format (write_legpol_mod.F90), one task only.

    precision: 8 = the reference's double-precision library (libtrans_dp, JPRB=JPRD), arrays are
    float64; 4 = its single-precision library (libtrans_sp, JPRB=JPRM), arrays are float32 (setup --
    Gaussian latitudes, Legendre recurrences -- still runs in double, as in the reference).

    ldll: a regular latitude-longitude grid for ``inv_trans(..., ldlatlon=True)`` with the reference's argument conventions
    (setup_trans.F90:258-271): ``kdlon`` = nlon; unshifted, ``kdgl`` = nlat - 1 (nlat odd) and the handle has NDGL = kdgl + 2
    rows, pole to pole with the equator held twice; ``ldshiftll``: ``kdgl`` = nlat (even), rows and longitudes offset by half a
    cell.  The series is evaluated exactly on those rows.  Such a handle serves no other transform."""
    if precision not in (4, 8):
        raise TransError("SETUP_TRANS: precision must be 4 or 8")
    cfg = _Setup()
    cfg.ksmax, cfg.kdgl, cfg.kdlon, cfg.precision = int(ksmax), int(kdgl), int(kdlon), int(precision)
    keep = None
    if kloen is not None:
        keep = np.ascontiguousarray(kloen, dtype=np.int32)
        if keep.size < kdgl:
            raise TransError("SETUP_TRANS: KLOEN TOO SHORT")
        cfg.kloen = keep.ctypes.data_as(C.POINTER(C.c_int))
    cfg.lduseflt, cfg.ldll = int(bool(lduseflt)), int(bool(ldll))
    cfg.ldshiftll = int(bool(ldshiftll))
    cfg.lduserpnm = int(bool(lduserpnm))  # True: Belousov's generator (the Fortran API's default); False: SUPOLF, as the benchmark
    cfg.ldstretch = int(pstret is not None and abs(pstret - 1.0) > 100 * np.finfo(float).eps)
    kresol = C.c_int(0)
    if cdio_legpol is None:
        _chk(lib().emi_setup(C.byref(cfg), C.byref(kresol)))
    else:
        io = _LegpolIO(str(cdio_legpol).encode(), None if cdlegpolfname is None else str(cdlegpolfname).encode(), None, 0)
        seg = None
        if klegpolptr is not None:
            if isinstance(klegpolptr, int):
                io.ptr, io.len = klegpolptr, int(klegpolptr_len or 0)
            else:
                seg = np.frombuffer(klegpolptr, dtype=np.uint8) if not isinstance(klegpolptr, np.ndarray) \
                    else np.ascontiguousarray(klegpolptr).view(np.uint8).reshape(-1)
                io.ptr, io.len = seg.ctypes.data, seg.size if klegpolptr_len is None else int(klegpolptr_len)
        _chk(lib().emi_setup_legpol(C.byref(cfg), C.byref(io), C.byref(kresol)))
        del seg  # the library has copied what it needs
    _PREC[kresol.value] = "float32" if precision == 4 else "float64"
    return kresol.value


def real_dtype(kresol):
    """numpy dtype name of the arrays of resolution `kresol` ("float64" or "float32")."""
    return _PREC.get(kresol, "float64")


_INT_SCALARS = ("nspec2", "nspec2g", "nspec2mx", "nspec", "nspecg", "ngptot", "ngptotg", "ngptotmx", "nump", "ndgl",
                "nsmax", "ndlon", "nproc", "myproc", "nfrstlat", "nlstlat", "nprtrw", "nprtrv", "mysetw", "mysetv", "ngptot_band",
                "ldll", "lshiftll")
_INT_ARRAYS = {"nloen": "ndgl", "nmen": "ndgl", "ndglu": "nsmax+1", "nasm0": "nsmax+1", "myms": "nump",
               "procm": "nsmax+1", "latlo": "nproc+1", "fftwork": "ndgl", "fftplan": "ndgl*5", "fftfac": "ndgl*15"}
_REAL_ARRAYS = {"rmu": "ndgl", "pmu": "ndgl", "rgw": "ndgl", "pgw": "ndgl", "racthe": "ndgl"}


def trans_inq(kresol, name):
    """TRANS_INQ (trans_inq.h): one quantity by (lower-case) name.  Three diagnostics beside the reference's names: "fftwork" (per
    latitude the work length of its FFT), "fftplan" ((ndgl, 5): kernel family -- 0 generic, 1 specialised in place, 2 register-resident,
    3 split, 4 direct mixed radix, 5 global scratch --, the mixed-radix factors A, B, C (0 for the other families), fields per workgroup)
    and "fftfac" ((ndgl, 15): the pass count and the factors of the FFT in pass order)."""
    L = lib()
    name = name.lower()
    if name in _INT_SCALARS:
        v = C.c_int(0)
        _chk(L.emi_inq_int(kresol, name.encode(), C.byref(v)))
        return v.value
    dims = {"ndgl": trans_inq(kresol, "ndgl"), "nsmax+1": trans_inq(kresol, "nsmax") + 1,
            "nump": trans_inq(kresol, "nump"), "nproc+1": trans_inq(kresol, "nproc") + 1}
    dims["ndgl*5"], dims["ndgl*15"] = dims["ndgl"] * 5, dims["ndgl"] * 15
    if name in _INT_ARRAYS:
        out = np.zeros(dims[_INT_ARRAYS[name]], dtype=np.int32)
        _chk(L.emi_inq_int_array(kresol, name.encode(), out.ctypes.data_as(C.POINTER(C.c_int)), out.size))
        return out.reshape(-1, 5) if name == "fftplan" else out.reshape(-1, 15) if name == "fftfac" else out  # per latitude: family, A, B, C, fields per workgroup; pass count, factors
    if name in _REAL_ARRAYS:
        out = np.zeros(dims[_REAL_ARRAYS[name]])
        _chk(L.emi_inq_real_array(kresol, name.encode(), out.ctypes.data_as(C.POINTER(C.c_double)), out.size))
        return out
    raise TransError("TRANS_INQ: unknown quantity %r" % name)


def legendre_panel(kresol, m, symmetric):
    """S%FA(m)%RPNMS / RPNMA as the reference lays them out; numpy [col(n desc)][lat]."""
    L = lib()
    r, c = C.c_int(), C.c_int()
    _chk(L.emi_inq_legendre(kresol, m, int(symmetric), None, C.byref(r), C.byref(c)))
    out = np.zeros((c.value, r.value))
    if out.size:
        _chk(L.emi_inq_legendre(kresol, m, int(symmetric), out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(r),
                                C.byref(c)))
    return out


def _fill_spec(a, space, keep, pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2, nspec2):
    def chk2(x, nm):
        if x is not None and (x.ndim != 2 or x.shape[0] != nspec2):
            raise TransError("%s must have shape (nspec2=%d, nfld)" % (nm, nspec2))

    chk2(pspvor, "PSPVOR"), chk2(pspdiv, "PSPDIV"), chk2(pspscalar, "PSPSCALAR"), chk2(pspsc2, "PSPSC2")
    for x, nm in ((pspsc3a, "PSPSC3A"), (pspsc3b, "PSPSC3B")):
        if x is not None and (x.ndim != 3 or x.shape[1] != nspec2):
            raise TransError("%s must have shape (nvar, nspec2=%d, nlev)" % (nm, nspec2))
    if (pspvor is None) != (pspdiv is None):
        raise TransError("PSPVOR and PSPDIV must be given together")
    if pspvor is not None and pspvor.shape != pspdiv.shape:
        raise TransError("PSPVOR and PSPDIV shapes differ")
    for nm, x in (("spvor", pspvor), ("spdiv", pspdiv), ("spscalar", pspscalar), ("spsc3a", pspsc3a),
                  ("spsc3b", pspsc3b), ("spsc2", pspsc2)):
        p, k = _ptr(x, space)
        setattr(a, nm, p)
        keep.append(k)
    a.nf_uv = 0 if pspvor is None else pspvor.shape[1]
    a.nf_scalar = 0 if pspscalar is None else pspscalar.shape[1]
    a.nf_sc2 = 0 if pspsc2 is None else pspsc2.shape[1]
    a.sc3a_nvar, a.sc3a_nlev = (0, 0) if pspsc3a is None else (pspsc3a.shape[0], pspsc3a.shape[2])
    a.sc3b_nvar, a.sc3b_nlev = (0, 0) if pspsc3b is None else (pspsc3b.shape[0], pspsc3b.shape[2])


def _fill_grid(a, space, keep, pgp, pgpuv, pgp3a, pgp3b, pgp2, nproma, ngpblks, specs=()):
    """Grid arrays + the extents block (emi_extents_t): the library makes the reference's extent checks
    (inv_trans.F90:476-600) on the real shapes.  numpy/torch shapes are the Fortran extents reversed."""
    ext = _Ext()
    for nm, x, rank in (("gp", pgp, 3), ("gpuv", pgpuv, 4), ("gp3a", pgp3a, 4), ("gp3b", pgp3b, 4), ("gp2", pgp2, 3)):
        if x is not None:
            if x.ndim != rank:
                raise TransError("P%s must have %d dimensions, got shape %s" % (nm.upper(), rank, tuple(x.shape)))
            for i, n in enumerate(reversed(tuple(x.shape))):
                getattr(ext, nm)[i] = int(n)
        p, k = _ptr(x, space)
        setattr(a, nm, p)
        keep.append(k)
    sp2 = [x.shape[-2] if x.ndim == 3 else x.shape[0] for x in specs if x is not None]
    ext.sp_dim2 = int(min(sp2)) if sp2 else 0
    a.gp_nfld = 0 if pgp is None else pgp.shape[1]
    a.ext = C.pointer(ext)
    keep.append(ext)


def _fill_vsets(a, keep, kvsetuv, kvsetsc, kvsetsc2, kvsetsc3a, kvsetsc3b, pgp3a=None, pgp3b=None, dmul=1):
    """KVSETUV / KVSETSC / KVSETSC2 / KVSETSC3A / KVSETSC3B (inv_trans.h:84-101): the V-set (1..NPRTRV) of every GLOBAL field;
    with them the spectral arrays hold this task's V-set only, the grid arrays all fields."""
    if all(k is None for k in (kvsetuv, kvsetsc, kvsetsc2, kvsetsc3a, kvsetsc3b)):
        return
    vs = _VSets()
    for nm, cnt, k in (("kvsetuv", "nuv_g", kvsetuv), ("kvsetsc", "nsc_g", kvsetsc), ("kvsetsc2", "nsc2_g", kvsetsc2),
                       ("kvsetsc3a", "nsc3a_g", kvsetsc3a), ("kvsetsc3b", "nsc3b_g", kvsetsc3b)):
        if k is not None:
            arr = np.ascontiguousarray(k, dtype=np.int32)
            keep.append(arr)
            setattr(vs, nm, arr.ctypes.data_as(C.POINTER(C.c_int)))
            setattr(vs, cnt, int(arr.size))
    # the variable count of the 3-D arrays from the GRID side (every task holds all fields there), so that a task whose V-set owns
    # no level -- and passes no PSPSC3A -- still lists the same global fields as its peers (the reference: UBOUND(PSPSC3A,3))
    vs.nvar3a_g = 0 if pgp3a is None or pgp3a.ndim != 4 else int(pgp3a.shape[1]) // dmul
    vs.nvar3b_g = 0 if pgp3b is None or pgp3b.ndim != 4 else int(pgp3b.shape[1]) // dmul
    keep.append(vs)
    a.vsets = C.pointer(vs)
    a.ext = None  # the extents block describes one-V-set calls (local == global field counts)


def inv_trans(kresol, pspvor=None, pspdiv=None, pspscalar=None, pspsc3a=None, pspsc3b=None, pspsc2=None,
              ldscders=False, ldvorgp=False, lddivgp=False, lduvder=False, kproma=None, pgp=None, pgpuv=None,
              pgp3a=None, pgp3b=None, pgp2=None, stream=None, kvsetuv=None, kvsetsc=None, kvsetsc2=None, kvsetsc3a=None,
              kvsetsc3b=None, ldlatlon=False, mem_space=None):
    """INV_TRANS (inv_trans.h:12-163): spectral -> grid point, results written into pgp*/...

    ldlatlon: the output is the lat-lon grid of a handle set up with ``ldll`` (required there, refused elsewhere).
    mem_space: overrides the memory space derived from the arrays (EMI_MEM_AUTO; on the CPU emulator of the tests EMI_MEM_DEVICE uses
    numpy arrays in place, the path device tensors take on a GPU)."""
    a, space, keep = _Inv(), [None, real_dtype(kresol)], []
    nspec2, ngptot = trans_inq(kresol, "nspec2"), trans_inq(kresol, "ngptot")
    nproma = int(kproma) if kproma else ngptot
    ngpblks = (ngptot - 1) // nproma + 1
    _fill_spec(a, space, keep, pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2, nspec2)
    _fill_grid(a, space, keep, pgp, pgpuv, pgp3a, pgp3b, pgp2, nproma, ngpblks,
               (pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2))
    a.ldscders, a.ldvorgp, a.lddivgp, a.lduvder = int(ldscders), int(ldvorgp), int(lddivgp), int(lduvder)
    a.kproma = nproma
    a.ldlatlon = int(bool(ldlatlon))
    a.mem_space = _space(mem_space, space)
    a.stream = stream
    _fill_vsets(a, keep, kvsetuv, kvsetsc, kvsetsc2, kvsetsc3a, kvsetsc3b, pgp3a, pgp3b, 3 if ldscders else 1)
    _chk(lib().emi_inv_trans(kresol, C.byref(a)))


def dir_trans(kresol, pspvor=None, pspdiv=None, pspscalar=None, pspsc3a=None, pspsc3b=None, pspsc2=None,
              kproma=None, pgp=None, pgpuv=None, pgp3a=None, pgp3b=None, pgp2=None, stream=None, kvsetuv=None, kvsetsc=None,
              kvsetsc2=None, kvsetsc3a=None, kvsetsc3b=None, mem_space=None):
    """DIR_TRANS (dir_trans.h:12-140): grid point -> spectral, results written into psp*.
    mem_space: overrides the memory space derived from the arrays (EMI_MEM_AUTO; on the CPU emulator of the tests EMI_MEM_DEVICE uses
    numpy arrays in place, the path device tensors take on a GPU)."""
    a, space, keep = _Dir(), [None, real_dtype(kresol)], []
    nspec2, ngptot = trans_inq(kresol, "nspec2"), trans_inq(kresol, "ngptot")
    nproma = int(kproma) if kproma else ngptot
    ngpblks = (ngptot - 1) // nproma + 1
    _fill_spec(a, space, keep, pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2, nspec2)
    _fill_grid(a, space, keep, pgp, pgpuv, pgp3a, pgp3b, pgp2, nproma, ngpblks,
               (pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2))
    a.kproma = nproma
    a.mem_space = _space(mem_space, space)
    a.stream = stream
    _fill_vsets(a, keep, kvsetuv, kvsetsc, kvsetsc2, kvsetsc3a, kvsetsc3b, pgp3a, pgp3b)
    _chk(lib().emi_dir_trans(kresol, C.byref(a)))


def inv_transad(kresol, pspvor=None, pspdiv=None, pspscalar=None, pspsc3a=None, pspsc3b=None, pspsc2=None,
                ldscders=False, ldvorgp=False, lddivgp=False, lduvder=False,
                kproma=None, pgp=None, pgpuv=None, pgp3a=None, pgp3b=None, pgp2=None, stream=None, kvsetuv=None, kvsetsc=None,
                kvsetsc2=None, kvsetsc3a=None, kvsetsc3b=None, mem_space=None):
    """INV_TRANSAD (inv_transad.h:12): adjoint of INV_TRANS -- reads pgp*, writes psp* (overwritten).
    Inner products: plain sum in grid-point space, SPECNORM weights (1 for m = 0, 2 for m > 0) in
    spectral space, as tests/trans/test_invtrans_adjoint.F90:243-315.  With ldscders / ldvorgp / lddivgp / lduvder the
    grid arrays carry the derivative / vorticity / divergence inputs in INV_TRANS's layout (inv_trans.h:66-76).
    mem_space: overrides the memory space derived from the arrays (EMI_MEM_AUTO; on the CPU emulator of the tests EMI_MEM_DEVICE uses
    numpy arrays in place, the path device tensors take on a GPU)."""
    a, space, keep = _Inv(), [None, real_dtype(kresol)], []
    nspec2, ngptot = trans_inq(kresol, "nspec2"), trans_inq(kresol, "ngptot")
    nproma = int(kproma) if kproma else ngptot
    _fill_spec(a, space, keep, pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2, nspec2)
    _fill_grid(a, space, keep, pgp, pgpuv, pgp3a, pgp3b, pgp2, nproma, (ngptot - 1) // nproma + 1,
               (pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2))
    a.ldscders, a.ldvorgp, a.lddivgp, a.lduvder = int(ldscders), int(ldvorgp), int(lddivgp), int(lduvder)
    a.kproma = nproma
    a.mem_space = _space(mem_space, space)
    a.stream = stream
    _fill_vsets(a, keep, kvsetuv, kvsetsc, kvsetsc2, kvsetsc3a, kvsetsc3b, pgp3a, pgp3b, 3 if ldscders else 1)
    _chk(lib().emi_inv_transad(kresol, C.byref(a)))


def dir_transad(kresol, pspvor=None, pspdiv=None, pspscalar=None, pspsc3a=None, pspsc3b=None, pspsc2=None,
                kproma=None, pgp=None, pgpuv=None, pgp3a=None, pgp3b=None, pgp2=None, stream=None, kvsetuv=None, kvsetsc=None,
                kvsetsc2=None, kvsetsc3a=None, kvsetsc3b=None, mem_space=None):
    """DIR_TRANSAD (dir_transad.h:12): adjoint of DIR_TRANS -- reads psp*, writes pgp*.
    mem_space: overrides the memory space derived from the arrays (EMI_MEM_AUTO; on the CPU emulator of the tests EMI_MEM_DEVICE uses
    numpy arrays in place, the path device tensors take on a GPU)."""
    a, space, keep = _Dir(), [None, real_dtype(kresol)], []
    nspec2, ngptot = trans_inq(kresol, "nspec2"), trans_inq(kresol, "ngptot")
    nproma = int(kproma) if kproma else ngptot
    _fill_spec(a, space, keep, pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2, nspec2)
    _fill_grid(a, space, keep, pgp, pgpuv, pgp3a, pgp3b, pgp2, nproma, (ngptot - 1) // nproma + 1,
               (pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2))
    a.kproma = nproma
    a.mem_space = _space(mem_space, space)
    a.stream = stream
    _fill_vsets(a, keep, kvsetuv, kvsetsc, kvsetsc2, kvsetsc3a, kvsetsc3b, pgp3a, pgp3b)
    _chk(lib().emi_dir_transad(kresol, C.byref(a)))


# ---------------------------------------------------------------------------------------------
# ESETUP_TRANS / EINV_TRANS / EDIR_TRANS / ETRANS_INQ: the limited-area, bi-Fourier transforms (etrans/include/etrans/*.h).
# INTEGRATION.md ("Limited-area transforms") holds the definitions.
# ---------------------------------------------------------------------------------------------
def esetup_trans(kmsmax, ksmax, kdgl, kdgux=None, kloen=None, kdlon=0, pexwn=1.0, peywn=1.0, precision=8, ldsplit=False,
                 ktmax=None, pweight=None, ldgridonly=False, knoextzl=0, knoextzg=0, ldusefftw=False, ld_all_fftw=False):
    """ESETUP_TRANS (esetup_trans.h); returns KRESOL, from the same numbering as ``setup_trans``.

    kmsmax, ksmax: truncation in x and y; kdgl rows of one length (``kloen`` with equal entries, or ``kdlon``); pexwn, peywn: the
    wavenumber units 2 pi / (ndlon dx), 2 pi / (kdgl dy).  ldusefftw, ld_all_fftw are accepted and have no effect; ldsplit: rows
    are never split between tasks."""
    who = "ESETUP_TRANS"
    if precision not in (4, 8):
        raise TransError("%s: precision must be 4 or 8" % who)
    if pweight is not None:
        raise TransError("%s: PWEIGHT (weighted distribution) is not supported" % who)
    if ldgridonly:
        raise TransError("%s: LDGRIDONLY is not supported" % who)
    if knoextzl or knoextzg:
        raise TransError("%s: KNOEXTZL / KNOEXTZG (no extension zone) are not supported" % who)
    if ktmax is not None and int(ktmax) != int(ksmax):
        raise TransError("%s: KTMAX /= KSMAX is not supported" % who)
    cfg = _ESetup()
    cfg.kmsmax, cfg.ksmax, cfg.kdgl, cfg.kdlon = int(kmsmax), int(ksmax), int(kdgl), int(kdlon)
    cfg.kdgux = int(kdgl if kdgux is None else kdgux)
    cfg.pexwn, cfg.peywn, cfg.precision = float(pexwn), float(peywn), int(precision)
    keep = None
    if kloen is not None:
        keep = np.ascontiguousarray(kloen, dtype=np.int32)
        if keep.size < kdgl:
            raise TransError("%s: KLOEN TOO SHORT" % who)
        cfg.kloen = keep.ctypes.data_as(C.POINTER(C.c_int))
    kresol = C.c_int(0)
    _chk(lib().emi_esetup(C.byref(cfg), C.byref(kresol)))
    _PREC[kresol.value] = "float32" if precision == 4 else "float64"
    return kresol.value


def _mean_ptr(x, nuv, space, keep, nm):
    if x is None:
        return None
    if x.ndim != 1 or x.shape[0] < nuv:
        raise TransError("%s must have shape (nf_uv=%d,)" % (nm, nuv))
    p, k = _ptr(x, space)
    keep.append(k)
    return p


def einv_trans(kresol, pspvor=None, pspdiv=None, pspscalar=None, pspsc3a=None, pspsc3b=None, pspsc2=None, fspgl_proc=None,
               ldscders=False, ldvorgp=False, lddivgp=False, lduvder=False, kproma=None, pgp=None, pgpuv=None, pgp3a=None,
               pgp3b=None, pgp2=None, pmeanu=None, pmeanv=None, stream=None, kvsetuv=None, kvsetsc=None, kvsetsc2=None,
               kvsetsc3a=None, kvsetsc3b=None, mem_space=None):
    """EINV_TRANS (einv_trans.h): spectral -> grid point on a handle of ``esetup_trans``; arrays as ``inv_trans``.
    pmeanu, pmeanv: (nf_uv,) arrays where the other arrays live, the mean wind (the (0, 0) coefficients of u and v).
    mem_space: overrides the memory space derived from the arrays (EMI_MEM_AUTO; on the CPU emulator of the tests EMI_MEM_DEVICE uses
    numpy arrays in place, the path device tensors take on a GPU)."""
    if fspgl_proc is not None:
        raise TransError("EINV_TRANS: FSPGL_PROC is not supported")
    if any(k is not None for k in (kvsetuv, kvsetsc, kvsetsc2, kvsetsc3a, kvsetsc3b)) and _DIST.get("nprtrv", 1) > 1:
        raise TransError("EINV_TRANS: KVSET arguments: V-sets are not available on a limited-area handle")
    a, space, keep = _Inv(), [None, real_dtype(kresol)], []
    nspec2, ngptot = trans_inq(kresol, "nspec2"), trans_inq(kresol, "ngptot")
    nproma = int(kproma) if kproma else ngptot
    _fill_spec(a, space, keep, pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2, nspec2)
    _fill_grid(a, space, keep, pgp, pgpuv, pgp3a, pgp3b, pgp2, nproma, (ngptot - 1) // nproma + 1,
               (pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2))
    a.ldscders, a.ldvorgp, a.lddivgp, a.lduvder = int(ldscders), int(ldvorgp), int(lddivgp), int(lduvder)
    a.kproma = nproma
    mu, mv = _mean_ptr(pmeanu, a.nf_uv, space, keep, "PMEANU"), _mean_ptr(pmeanv, a.nf_uv, space, keep, "PMEANV")
    a.mem_space = _space(mem_space, space)
    a.stream = stream
    _chk(lib().emi_einv_trans(kresol, C.byref(a), mu, mv))


def edir_trans(kresol, pspvor=None, pspdiv=None, pspscalar=None, pspsc3a=None, pspsc3b=None, pspsc2=None, kproma=None,
               pgp=None, pgpuv=None, pgp3a=None, pgp3b=None, pgp2=None, pmeanu=None, pmeanv=None, aux_proc=None, stream=None,
               kvsetuv=None, kvsetsc=None, kvsetsc2=None, kvsetsc3a=None, kvsetsc3b=None, mem_space=None):
    """EDIR_TRANS (edir_trans.h): grid point -> spectral on a handle of ``esetup_trans``; pmeanu, pmeanv receive the mean wind."""
    if aux_proc is not None:
        raise TransError("EDIR_TRANS: AUX_PROC is not supported")
    if any(k is not None for k in (kvsetuv, kvsetsc, kvsetsc2, kvsetsc3a, kvsetsc3b)) and _DIST.get("nprtrv", 1) > 1:
        raise TransError("EDIR_TRANS: KVSET arguments: V-sets are not available on a limited-area handle")
    a, space, keep = _Dir(), [None, real_dtype(kresol)], []
    nspec2, ngptot = trans_inq(kresol, "nspec2"), trans_inq(kresol, "ngptot")
    nproma = int(kproma) if kproma else ngptot
    _fill_spec(a, space, keep, pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2, nspec2)
    _fill_grid(a, space, keep, pgp, pgpuv, pgp3a, pgp3b, pgp2, nproma, (ngptot - 1) // nproma + 1,
               (pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2))
    a.kproma = nproma
    mu, mv = _mean_ptr(pmeanu, a.nf_uv, space, keep, "PMEANU"), _mean_ptr(pmeanv, a.nf_uv, space, keep, "PMEANV")
    a.mem_space = _space(mem_space, space)
    a.stream = stream
    _chk(lib().emi_edir_trans(kresol, C.byref(a), mu, mv))


def einv_transad(kresol, pspvor=None, pspdiv=None, pspscalar=None, pspsc3a=None, pspsc3b=None, pspsc2=None, fspgl_proc=None,
                 ldscders=False, ldvorgp=False, lddivgp=False, lduvder=False, kproma=None, pgp=None, pgpuv=None, pgp3a=None,
                 pgp3b=None, pgp2=None, pmeanu=None, pmeanv=None, stream=None, kvsetuv=None, kvsetsc=None, kvsetsc2=None,
                 kvsetsc3a=None, kvsetsc3b=None, mem_space=None):
    """EINV_TRANSAD (einv_transad.h): the transpose of ``einv_trans`` -- reads pgp*, writes psp*, pmeanu and pmeanv (overwritten;
    the reference adds to them).  Inner products: plain sums over the grid points and over the NSPEC2 reals and the means, no weights.
    With ldscders / ldvorgp / lddivgp / lduvder the grid arrays carry the derivative / vorticity / divergence inputs in
    EINV_TRANS's layout.  Entries that do not enter EINV_TRANS come back as zeros."""
    if fspgl_proc is not None:
        raise TransError("EINV_TRANSAD: FSPGL_PROC is not supported")
    if any(k is not None for k in (kvsetuv, kvsetsc, kvsetsc2, kvsetsc3a, kvsetsc3b)) and _DIST.get("nprtrv", 1) > 1:
        raise TransError("EINV_TRANSAD: KVSET arguments: V-sets are not available on a limited-area handle")
    a, space, keep = _Inv(), [None, real_dtype(kresol)], []
    nspec2, ngptot = trans_inq(kresol, "nspec2"), trans_inq(kresol, "ngptot")
    nproma = int(kproma) if kproma else ngptot
    _fill_spec(a, space, keep, pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2, nspec2)
    _fill_grid(a, space, keep, pgp, pgpuv, pgp3a, pgp3b, pgp2, nproma, (ngptot - 1) // nproma + 1,
               (pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2))
    a.ldscders, a.ldvorgp, a.lddivgp, a.lduvder = int(ldscders), int(ldvorgp), int(lddivgp), int(lduvder)
    a.kproma = nproma
    mu, mv = _mean_ptr(pmeanu, a.nf_uv, space, keep, "PMEANU"), _mean_ptr(pmeanv, a.nf_uv, space, keep, "PMEANV")
    a.mem_space = _space(mem_space, space)
    a.stream = stream
    _chk(lib().emi_einv_transad(kresol, C.byref(a), mu, mv))


def edir_transad(kresol, pspvor=None, pspdiv=None, pspscalar=None, pspsc3a=None, pspsc3b=None, pspsc2=None, kproma=None,
                 pgp=None, pgpuv=None, pgp3a=None, pgp3b=None, pgp2=None, pmeanu=None, pmeanv=None, aux_proc=None, stream=None,
                 kvsetuv=None, kvsetsc=None, kvsetsc2=None, kvsetsc3a=None, kvsetsc3b=None, mem_space=None):
    """EDIR_TRANSAD (edir_transad.h): the transpose of ``edir_trans`` -- reads psp*, pmeanu and pmeanv, writes pgp* (overwritten).
    The entries that EDIR_TRANS writes as structural zeros are not read."""
    if aux_proc is not None:
        raise TransError("EDIR_TRANSAD: AUX_PROC is not supported")
    if any(k is not None for k in (kvsetuv, kvsetsc, kvsetsc2, kvsetsc3a, kvsetsc3b)) and _DIST.get("nprtrv", 1) > 1:
        raise TransError("EDIR_TRANSAD: KVSET arguments: V-sets are not available on a limited-area handle")
    a, space, keep = _Dir(), [None, real_dtype(kresol)], []
    nspec2, ngptot = trans_inq(kresol, "nspec2"), trans_inq(kresol, "ngptot")
    nproma = int(kproma) if kproma else ngptot
    _fill_spec(a, space, keep, pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2, nspec2)
    _fill_grid(a, space, keep, pgp, pgpuv, pgp3a, pgp3b, pgp2, nproma, (ngptot - 1) // nproma + 1,
               (pspvor, pspdiv, pspscalar, pspsc3a, pspsc3b, pspsc2))
    a.kproma = nproma
    mu, mv = _mean_ptr(pmeanu, a.nf_uv, space, keep, "PMEANU"), _mean_ptr(pmeanv, a.nf_uv, space, keep, "PMEANV")
    a.mem_space = _space(mem_space, space)
    a.stream = stream
    _chk(lib().emi_edir_transad(kresol, C.byref(a), mu, mv))


_E_INT_SCALARS = ("nspec", "nspec2", "nspec2g", "nspec2mx", "nump", "ngptot", "ngptotg", "ngptotmx", "nprtrw", "mysetw", "mysetv",
                  "nsmax", "nmsmax", "ndgl", "ndlon", "ndgux", "ldlam", "nfrstlat", "nlstlat", "nproc", "myproc")
_E_INT_ARRAYS = {"myms": "nump", "kntmp": "m", "ncpl2m": "m", "ncpl4m": "m", "npme": "m", "nesm0": "m", "ndim0g": "m", "nallms": "m",
                 "procm": "m", "numpp": "w", "nptrms": "w", "npossp": "w+1", "latlo": "w+1", "nloen": "ndgl", "fftwork": "ndgl", "fftplan": "ndgl*5", "fftfac": "ndgl*15"}


def etrans_inq(kresol, name):
    """ETRANS_INQ (etrans_inq.h): one quantity of a limited-area handle by lower-case name.  Arrays over the x-wavenumbers have
    KMSMAX + 1 entries (positions 1-based as in the reference, -99 in "nesm0" for the wavenumbers of other tasks); "latlo" holds the
    0-based first row of every task's band (KPTRFRSTLAT - 1) and NDGL; "rlepinm" is FALD%RLEPINM."""
    L = lib()
    name = name.lower()
    v = C.c_int(0)
    _chk(L.emi_inq_int(kresol, b"ldlam", C.byref(v)))
    if not v.value:
        raise TransError("ETRANS_INQ: resolution %d is not a limited-area handle (ESETUP_TRANS)" % kresol)
    if name in _E_INT_SCALARS:
        _chk(L.emi_inq_int(kresol, name.encode(), C.byref(v)))
        return v.value
    q = lambda n: etrans_inq(kresol, n)
    if name in _E_INT_ARRAYS:
        dims = {"nump": "nump", "ndgl": "ndgl"}
        k = _E_INT_ARRAYS[name]
        n = q("nmsmax") + 1 if k == "m" else q("nprtrw") if k == "w" else q("nprtrw") + 1 if k == "w+1" else \
            5 * q("ndgl") if k == "ndgl*5" else 15 * q("ndgl") if k == "ndgl*15" else q(dims[k])
        out = np.zeros(n, dtype=np.int32)
        _chk(L.emi_inq_int_array(kresol, name.encode(), out.ctypes.data_as(C.POINTER(C.c_int)), out.size))
        return out.reshape(-1, 5) if name == "fftplan" else out.reshape(-1, 15) if name == "fftfac" else out  # per row: family, A, B, C, fields per workgroup; pass count, factors
    if name in ("rlepinm", "plepinm"):
        out = np.zeros(q("nspec2g") // 4)
        _chk(L.emi_inq_real_array(kresol, name.encode(), out.ctypes.data_as(C.POINTER(C.c_double)), out.size))
        return out
    raise TransError("ETRANS_INQ: unknown quantity %r" % name)


def _especnorm_args(kresol, pspec, pmet, mem_space):
    space = [None, real_dtype(kresol)]
    if pspec is None or getattr(pspec, "ndim", 0) != 2 or pspec.shape[1] == 0:
        p, keep, nf = None, None, 0
        space[0] = EMI_MEM_HOST
    else:
        p, keep = _ptr(pspec, space)
        space[0] = _space(mem_space, space)
        nf = int(pspec.shape[1])
    met = None
    if pmet is not None:  # a small host array, whatever memory the fields live in
        met = np.ascontiguousarray(_np(pmet), dtype=space[1]).reshape(-1)
    return space[0], p, nf, met, keep


def especnorm(kresol, pspec, pmet=None, mem_space=None):
    """ESPECNORM (especnorm.h): the spectral norm of every field of pspec (nspec2, nfld) on a handle of ``esetup_trans``, as a
    numpy array, on every task (the reference: on KMASTER).  PNORM(f)^2 = sum over m, n of w(m, n) (a_r^2 + a_i^2 + b_r^2 + b_i^2);
    pmet: the metric, a host array read zero-based at NPME(m) + n (etrans_inq "npme"; at least NSPEC2G / 4 + 1 elements, element 0
    is never read), or None for w = 1.  Several tasks: the library gathers the per-wavenumber sums over the host collectives.
    mem_space: as ``specnorm``."""
    space, p, nf, met, keep = _especnorm_args(kresol, pspec, pmet, mem_space)
    out = np.zeros(nf)
    _chk(lib().emi_especnorm(kresol, space, p, nf, None if met is None else met.ctypes.data, 0 if met is None else met.size,
                             out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def especnorm_partial(kresol, pspec, pmet=None, mem_space=None):
    """emi_especnorm_partial: (nump, nfld) sums S(f, m) of this task's x-wavenumbers, in MYMS order; arguments as ``especnorm``."""
    space, p, nf, met, keep = _especnorm_args(kresol, pspec, pmet, mem_space)
    out = np.zeros((trans_inq(kresol, "nump"), nf))
    _chk(lib().emi_especnorm_partial(kresol, space, p, nf, None if met is None else met.ctypes.data, 0 if met is None else met.size,
                                     out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def egpnorm_trans(kresol, pgp, kfields=None, kproma=None, ldave_only=False, pmin=None, pmax=None, mem_space=None):
    """EGPNORM_TRANS (egpnorm_trans.h): (PAVE, PMIN, PMAX) as ``gpnorm_trans`` on a handle of ``esetup_trans``: the average over all
    NDGL x NDLON points, extension zone included, each row weighted 1 / NDGL."""
    return _gpnorm("emi_egpnorm", kresol, pgp, kfields, kproma, ldave_only, pmin, pmax, mem_space)


def specnorm(kresol, pspec, kvset=None, mem_space=None, pmet=None):
    """SPECNORM (specnorm.h:12): per-field spectral L2 norm, returned as a numpy array (on every
    task; the reference returns it on the master only).  kvset (NPRTRV > 1, specnorm.F90:82-101): V-set of every GLOBAL
    field; pspec holds this task's fields of its own V-set and the norms of all len(kvset) fields come back.
    mem_space: overrides the memory space derived from the arrays (EMI_MEM_AUTO; on the CPU emulator of the tests EMI_MEM_DEVICE uses
    numpy arrays in place, the path device tensors take on a GPU).
    pmet: the metric PMET(0:NSMAX), a host array of at least NSMAX + 1 elements read from element n = 0 (spnormd_mod.F90):
    PNORM(f)^2 = sum over m of c_m sum over n of pmet[n] (re^2 + im^2).  Several tasks: the library gathers the per-wavenumber sums
    over the host collectives, and the norms are the bytes of one task."""
    space = [None, real_dtype(kresol)]
    if pspec.shape[1] == 0:
        p, keep, space[0] = None, None, EMI_MEM_HOST
    else:
        p, keep = _ptr(pspec, space)
        space[0] = _space(mem_space, space)
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    if pmet is not None:  # a small host array, whatever memory the fields live in
        met = np.ascontiguousarray(_np(pmet), dtype=space[1]).reshape(-1)
        kv = None
        if kvset is not None and _DIST.get("nprtrv", 1) > 1:
            kv = np.ascontiguousarray(kvset, dtype=np.int32)
        out = np.zeros(pspec.shape[1] if kv is None else kv.size)
        _chk(lib().emi_specnorm_met(kresol, space[0], p, pspec.shape[1], met.ctypes.data, met.size,
                                    None if kv is None else kv.ctypes.data_as(C.POINTER(C.c_int)), 0 if kv is None else kv.size, pd(out)))
        return out
    if kvset is not None and _DIST.get("nprtrv", 1) > 1:
        kv = np.ascontiguousarray(kvset, dtype=np.int32)
        out = np.zeros(kv.size)
        _chk(lib().emi_specnorm_kvset(kresol, space[0], p, pspec.shape[1], kv.ctypes.data_as(C.POINTER(C.c_int)), kv.size, pd(out)))
        return out
    out = np.zeros(pspec.shape[1])
    if _DIST["nproc"] == 1 or _DIST.get("nprtrv", 1) > 1:
        # several V-sets: the library sums over the tasks of this V-set itself (host collectives)
        _chk(lib().emi_specnorm(kresol, space[0], p, pspec.shape[1], pd(out)))
        return out
    from . import dist as _dist
    _chk(lib().emi_specnorm_partial(kresol, space[0], p, pspec.shape[1], pd(out)))
    return np.sqrt(_dist.all_reduce_sum(out, _DIST["group"], _DIST["device"]))  # every task gets the norms


def specnorm_met_partial(kresol, pspec, pmet, mem_space=None):
    """emi_specnorm_met_partial: (nump, nfld) sums of this task's zonal wavenumbers, in MYMS order, c_m and the metric applied;
    arguments as ``specnorm`` with pmet.  Needs no collectives: sum over m (and tasks) and take the root."""
    space = [None, real_dtype(kresol)]
    p, keep = _ptr(pspec, space)
    space[0] = _space(mem_space, space)
    met = np.ascontiguousarray(_np(pmet), dtype=space[1]).reshape(-1)
    out = np.zeros((trans_inq(kresol, "nump"), int(pspec.shape[1])))
    _chk(lib().emi_specnorm_met_partial(kresol, space[0], p, int(pspec.shape[1]), met.ctypes.data, met.size,
                                        out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def specnorm_last_ms():
    """emi_specnorm_last_ms: with ``set_profile(1)``, the device time (ms) of the kernel alone of the last ``specnorm`` call."""
    v = C.c_double(0.0)
    _chk(lib().emi_specnorm_last_ms(C.byref(v)))
    return v.value


def gpnorm_trans(kresol, pgp, kfields=None, kproma=None, ldave_only=False, pmin=None, pmax=None, mem_space=None):
    """GPNORM_TRANS (gpnorm_trans.h:12): (PAVE, PMIN, PMAX) of the first `kfields` fields of pgp[ngpblks, nfld, nproma] -- the
    area-weighted average over the sphere (Gaussian weights), minimum and maximum -- as numpy arrays, on every task (the
    reference: task 1).  ldave_only: pmin / pmax are the caller's local extrema and are only reduced over the tasks.
    mem_space: overrides the memory space derived from the arrays (EMI_MEM_AUTO; on the CPU emulator of the tests EMI_MEM_DEVICE uses
    numpy arrays in place, the path device tensors take on a GPU)."""
    return _gpnorm("emi_gpnorm", kresol, pgp, kfields, kproma, ldave_only, pmin, pmax, mem_space)


def _gpnorm(fn, kresol, pgp, kfields, kproma, ldave_only, pmin, pmax, mem_space):
    """gpnorm_trans / egpnorm_trans over the entry point `fn`"""
    space = [None, real_dtype(kresol)]
    p, keep = _ptr(pgp, space)
    space[0] = _space(mem_space, space)
    if pgp.ndim != 3:
        raise TransError("PGP must have 3 dimensions (ngpblks, fields, nproma), got shape %s" % (tuple(pgp.shape),))
    nf = int(pgp.shape[1]) if kfields is None else int(kfields)
    nproma = int(kproma) if kproma else int(pgp.shape[2])
    ave, mn, mx = np.zeros(nf), np.zeros(nf), np.zeros(nf)
    if ldave_only:
        mn[:], mx[:] = np.asarray(pmin, dtype=np.float64)[:nf], np.asarray(pmax, dtype=np.float64)[:nf]
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    _chk(getattr(lib(), fn)(kresol, space[0], p, int(pgp.shape[1]), nf, nproma, pd(ave), pd(mn), pd(mx), int(bool(ldave_only))))
    return ave, mn, mx


def vordiv_to_uv(pspvor, pspdiv, ksmax, pspu=None, pspv=None, mem_space=None):
    """VORDIV_TO_UV (vordiv_to_uv.h:12): spectral vorticity / divergence [nspec2, nfld] -> spectral (U, V) = (u, v) cos(theta), total
    wavenumbers n <= ksmax, for the zonal wavenumbers of this task.  Needs setup_trans0 only; returns (pspu, pspv).
    mem_space: overrides the memory space derived from the arrays (EMI_MEM_AUTO; on the CPU emulator of the tests EMI_MEM_DEVICE uses
    numpy arrays in place, the path device tensors take on a GPU)."""
    is64 = str(pspvor.dtype).endswith("float64")
    space = [None, "float64" if is64 else "float32"]
    pv_, k1 = _ptr(pspvor, space)
    pd_, k2 = _ptr(pspdiv, space)
    if pspu is None:
        pspu = pspvor.clone() if _is_torch(pspvor) else np.zeros_like(pspvor)
    if pspv is None:
        pspv = pspvor.clone() if _is_torch(pspvor) else np.zeros_like(pspvor)
    pu_, k3 = _ptr(pspu, space)
    pw_, k4 = _ptr(pspv, space)
    if not (tuple(pspvor.shape) == tuple(pspdiv.shape) == tuple(pspu.shape) == tuple(pspv.shape)) or pspvor.ndim != 2:
        raise TransError("VORDIV_TO_UV: PSPVOR, PSPDIV, PSPU, PSPV must be [nspec2, nfld] arrays of one shape")
    _chk(lib().emi_vordiv_to_uv(int(ksmax), 8 if is64 else 4, _space(mem_space, space), pv_, pd_, pu_, pw_, int(pspvor.shape[1]), int(pspvor.shape[0])))
    return pspu, pspv


# ---------------------------------------------------------------------------------------------
# Biperiodicisation (etrans/cpu/biper): FPBIPERE, ETIBIHIE, HORIZ_FIELD.  No resolution handle, setup_trans0 only.
# ---------------------------------------------------------------------------------------------
def _biper_array(who, pgpbi, ndim):
    name = str(pgpbi.dtype).replace("torch.", "")
    if name not in ("float64", "float32") or pgpbi.ndim != ndim:
        raise TransError("%s: PGPBI must be a %d-dimensional float64 or float32 array" % (who, ndim))
    space = [None, name]
    p, keep = _ptr(pgpbi, space)
    return p, keep, space, 8 if name == "float64" else 4


def fpbipere(pgpbi, kdlux, kdgux, kdlon, kdgl, ldzon=False, ldboyd=False, kdboyd=None, plboyd=None, mem_space=None, kdadd=0):
    """FPBIPERE (biper/external/fpbipere.F90): the fields PGPBI(KD1, KNUBI) = ``pgpbi[knubi, kd1]``, known on C+I (kdlux x kdgux), are
    made doubly periodic on C+I+E (kdlon x kdgl), in place.  ldzon: the C+I rows lie kdlon apart on input (else kdlux apart, packed);
    on output they always lie kdlon apart.  ldboyd: Boyd's window with ``kdboyd`` (6 integers) and ``plboyd`` instead of spline and
    smoothing.  A numpy array is staged, a torch tensor on the device is used in place; the precision is the array's dtype."""
    p, keep, space, esz = _biper_array("FPBIPERE", pgpbi, 2)
    kb = None if kdboyd is None else np.ascontiguousarray(kdboyd, dtype=np.int32)
    if kb is not None and kb.size < 6:
        raise TransError("FPBIPERE: KDBOYD must hold 6 integers")
    pl = None if plboyd is None else C.c_double(float(plboyd))
    _chk(lib().emi_fpbipere(_space(mem_space, space), esz, p, int(kdlux), int(kdgux), int(kdlon), int(kdgl), int(pgpbi.shape[0]), int(pgpbi.shape[1]),
                            int(kdadd), int(bool(ldzon)), int(bool(ldboyd)), None if kb is None else kb.ctypes.data_as(C.POINTER(C.c_int)),
                            None if pl is None else C.byref(pl)))
    return pgpbi


def etibihie(pgpbi, kdlon, kdgl, kdlux, kdgux, kstart, kdlsm, ldbix, ldbiy, mem_space=None, kdadd=0):
    """ETIBIHIE (biper/external/etibihie.F90): the same on PGPBI(KSTART:KDLSM, KNUBI, KDGL) = ``pgpbi[kdgl, knubi, kdlsm - kstart + 1]``,
    in place; ldbix / ldbiy switch the directions.  The columns outside 1 .. kdlon are not touched."""
    p, keep, space, esz = _biper_array("ETIBIHIE", pgpbi, 3)
    if int(pgpbi.shape[0]) != int(kdgl) or int(pgpbi.shape[2]) != int(kdlsm) - int(kstart) + 1:
        raise TransError("ETIBIHIE: PGPBI must be [kdgl, knubi, kdlsm - kstart + 1] = [%d, :, %d]" % (kdgl, kdlsm - kstart + 1))
    _chk(lib().emi_etibihie(_space(mem_space, space), esz, p, int(kdlon), int(kdgl), int(pgpbi.shape[1]), int(kdlux), int(kdgux), int(kstart), int(kdlsm),
                            int(bool(ldbix)), int(bool(ldbiy)), int(kdadd)))
    return pgpbi


def horiz_field(kx, ky, dtype):
    """HORIZ_FIELD (biper/external/horiz_field.F90): the test field PHFIELD(KX, KY) as a host array ``[ky, kx]``."""
    out = np.zeros((int(ky), int(kx)), dtype=np.dtype(dtype))
    if out.dtype not in (np.dtype("float64"), np.dtype("float32")):
        raise TransError("HORIZ_FIELD: dtype must be float64 or float32")
    _chk(lib().emi_horiz_field(int(kx), int(ky), out.dtype.itemsize, out.ctypes.data))
    return out


def boyd_window(n, scale, dtype):
    """The weights b(1 .. n) of Boyd's window (ewindowe_mod.F90:107-131) in the precision ``dtype``, as the library computes them."""
    out = np.zeros(int(n), dtype=np.dtype(dtype))
    if out.dtype not in (np.dtype("float64"), np.dtype("float32")):
        raise TransError("boyd_window: dtype must be float64 or float32")
    _chk(lib().emi_boyd_window(int(n), float(scale), out.dtype.itemsize, out.ctypes.data))
    return out


def biper_last_ms():
    """With set_profile(1): device ms of the last fpbipere / etibihie call by kernel (spline x, spline y, smoothing, band copy)."""
    ms = (C.c_double * 4)()
    _chk(lib().emi_biper_last_ms(ms))
    return list(ms)


# ---------------------------------------------------------------------------------------------
# DIST_SPEC / GATH_SPEC / DIST_GRID / GATH_GRID: global <-> distributed arrays.
# Not on the transform hot path: host (numpy) arrays, moved with torch.distributed collectives.
# Global spectral order (dist_spec_control_mod.F90:158-161, IASM0G): m = 0..N, n = m..N, (re, im).
# Global grid order: latitudes north to south = the tasks' latitude bands in task order.
# ---------------------------------------------------------------------------------------------
def _np(a):
    return a.detach().cpu().numpy() if _is_torch(a) else np.asarray(a)


def _global_spec_index(kresol):
    """indices into the global spectral array of this task's coefficients, in local order"""
    n, myms = trans_inq(kresol, "nsmax"), trans_inq(kresol, "myms")
    iasm0g = np.concatenate([[0], np.cumsum([2 * (n - m + 1) for m in range(n + 1)])])
    return np.concatenate([np.arange(iasm0g[m], iasm0g[m] + 2 * (n - m + 1)) for m in myms]) if len(myms) else \
        np.zeros(0, dtype=np.int64)


def _roots(k, nfld, what):
    k = np.ascontiguousarray(np.broadcast_to(np.asarray(k, dtype=np.int32), (nfld,))) if np.ndim(k) <= 1 else None
    if k is None or (nfld and (k.min() < 1 or k.max() > _DIST["nproc"])):
        raise TransError("%s: task numbers must be 1..%d" % (what, _DIST["nproc"]))
    return k


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _on_emulator():
    """tests/emu only: the CPU functional emulator is loaded (_use_library_for_tests), whose "device" memory is host memory (numpy
    arrays in place)"""
    return _EMULATOR[0]


def _gs_device_of(like):
    import torch
    if _is_torch(like) and like.is_cuda:
        return like.device
    return torch.device(_DIST["device"] if _DIST["device"] and str(_DIST["device"]).startswith("cuda") else "cuda")


def _gs_zeros(shape, dt, on_device, like=None):
    """a zero array for a result of the _m routines: a device tensor, or numpy (host memory; the emulator's device memory too)"""
    if not on_device or _on_emulator():
        return np.zeros(shape, dtype=dt)
    import torch
    return torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device=_gs_device_of(like))


def _gs_move(a, dt, on_device, like=None):
    """array `a` (numpy or torch, any memory) as a C-contiguous array of dtype dt in the wanted memory"""
    if not on_device or _on_emulator():
        return np.ascontiguousarray(_np(a), dtype=dt)
    import torch
    t = a if _is_torch(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=dt))
    return t.to(device=_gs_device_of(like if like is not None else a), dtype=getattr(torch, np.dtype(dt).name)).contiguous()


def _gs_ptr(a, dt, who, name):
    """pointer of an array of the _m routines used in place: a contiguous numpy array or torch tensor of the handle's precision"""
    if a is None:
        return None
    if _is_torch(a):
        if not a.is_contiguous() or str(a.dtype) != "torch." + np.dtype(dt).name:
            raise TransError("%s: %s must be a contiguous %s tensor" % (who, name, np.dtype(dt).name))
        return a.data_ptr()
    if not (isinstance(a, np.ndarray) and a.dtype == np.dtype(dt) and a.flags.c_contiguous):
        raise TransError("%s: %s must be a C-contiguous %s array" % (who, name, np.dtype(dt).name))
    return a.ctypes.data


def _gs_spaces(who, mem_space, glob_space, glob=None):
    """(loc_space, glob_space) of a call with mem_space= or glob_space=; glob: the global array where the caller passes one"""
    ls = EMI_MEM_AUTO if mem_space is None else int(mem_space)
    if glob_space is None:
        gs = EMI_MEM_DEVICE if (_is_torch(glob) and glob.is_cuda) else EMI_MEM_HOST
    else:
        gs = int(glob_space)
    if gs == EMI_MEM_AUTO:
        gs = EMI_MEM_DEVICE if (_is_torch(glob) and glob.is_cuda) else EMI_MEM_HOST
    if ls not in (EMI_MEM_HOST, EMI_MEM_DEVICE, EMI_MEM_AUTO) or gs not in (EMI_MEM_HOST, EMI_MEM_DEVICE):
        raise TransError("%s: mem_space / glob_space must be EMI_MEM_HOST, EMI_MEM_DEVICE or EMI_MEM_AUTO" % who)
    return ls, gs


def _kvset_local(kresol, kvset, nfld, who):
    """(kvset as int32, fields of PSPEC on this task): with NPRTRV > 1 the fields whose V-set is this task's, else all of them"""
    kv = np.ascontiguousarray(kvset, dtype=np.int32)
    if kv.shape != (nfld,):
        raise TransError("%s: KVSET must name the V-set of each of the %d fields" % (who, nfld))
    if trans_inq(kresol, "nprtrv") == 1:
        return kv, nfld
    return kv, int((kv == trans_inq(kresol, "mysetv")).sum())


def dist_spec(kresol, pspecg, kfdistg, kfrom=1, mem_space=None, glob_space=None, kvset=None):
    """DIST_SPEC (dist_spec.h:11) over emi_dist_spec: global spectral fields `pspecg` (nspec2g, kfdistg), field f held
    by task kfrom[f] (1-based; the columns of other tasks' fields are not read, the array may be None on a task that is
    the source of none), -> this task's (nspec2, kfdistg) local array.
    kvset (NPRTRV > 1, emi_dist_spec_v): the V-set of every one of the kfdistg GLOBAL fields; the result holds the fields of this
    task's own V-set, (nspec2, COUNT(kvset == mysetv)), which may be no field at all.  kfrom[f] may be any of the NPRTRW x NPRTRV tasks.
    mem_space=EMI_MEM_DEVICE (emi_dist_spec_m): the local array is laid out on the device and returned as a device tensor (a numpy
    array on the CPU emulator of the tests); glob_space: the memory the global image is consumed from (default: where `pspecg` lives).
    The local array is created by the call, so there is nothing for EMI_MEM_AUTO to classify: mem_space=EMI_MEM_AUTO, and glob_space=
    given alone, mean EMI_MEM_DEVICE; only mem_space=EMI_MEM_HOST gives a numpy result through the host path."""
    return _dist_spec("", kresol, pspecg, kfdistg, kfrom, None, mem_space, glob_space, kvset)


def _dist_spec(_e, kresol, pspecg, kfdistg, kfrom, ksort, mem_space=None, glob_space=None, kvset=None):
    """dist_spec (_e = "") / edist_spec (_e = "e")"""
    dt = real_dtype(kresol)
    ns2g, ns2, me = trans_inq(kresol, "nspec2g"), trans_inq(kresol, "nspec2"), trans_inq(kresol, "myproc")
    who = _e.upper() + "DIST_SPEC"
    kfrom = _roots(kfrom, kfdistg, who + ":KFROM")
    mine = np.flatnonzero(kfrom == me)
    ks = None if ksort is None else np.ascontiguousarray(ksort, dtype=np.int32)
    kv, nfl = (None, kfdistg) if kvset is None else _kvset_local(kresol, kvset, kfdistg, who)
    if mem_space is not None or glob_space is not None or kv is not None:
        host = mem_space is None and glob_space is None  # (kvset alone: host arrays through the general entry point)
        ls, gs = (EMI_MEM_HOST, EMI_MEM_HOST) if host else _gs_spaces(who, mem_space, glob_space, pspecg)
        g = None
        if mine.size:
            if pspecg.shape[0] != ns2g:
                raise TransError("%s: PSPECG must have shape (nspec2g=%d, nfld)" % (who, ns2g))
            g = _gs_move(pspecg[:, mine.tolist()].T, dt, gs == EMI_MEM_DEVICE)  # [n_mine][nspec2g]
        out = _gs_zeros((ns2, nfl), dt, ls != EMI_MEM_HOST, pspecg)
        a = (kresol, gs, _gs_ptr(g, dt, who, "PSPECG"), kfdistg, _iptr(kfrom))
        b = (None if ks is None else _iptr(ks), EMI_MEM_HOST if ls == EMI_MEM_HOST else EMI_MEM_DEVICE, _gs_ptr(out, dt, who, "PSPEC") if nfl else None)
        _chk(getattr(lib(), "emi_%sdist_spec_m" % _e)(*a, *b) if kv is None else lib().emi_dist_spec_v(*a, _iptr(kv), *b))
        return out
    g = None
    if mine.size:
        a = _np(pspecg)
        if a.shape[0] != ns2g:
            raise TransError("%s: PSPECG must have shape (nspec2g=%d, nfld)" % (who, ns2g))
        g = np.ascontiguousarray(a[:, mine].T, dtype=dt)  # [n_mine][nspec2g]
    out = np.zeros((ns2, kfdistg), dtype=dt)
    _chk(getattr(lib(), "emi_%sdist_spec" % _e)(kresol, None if g is None else g.ctypes.data, kfdistg, _iptr(kfrom),
                                                None if ks is None else _iptr(ks), out.ctypes.data))
    return out


def gath_spec(kresol, pspec, kfgathg, kto=1, mem_space=None, glob_space=None, kvset=None):
    """GATH_SPEC (gath_spec.h:11) over emi_gath_spec: local (nspec2, kfgathg) -> global (nspec2g, n_mine) holding the
    fields this task is the target of (None if it is the target of none).
    kvset (NPRTRV > 1, emi_gath_spec_v): the V-set of every one of the kfgathg GLOBAL fields; `pspec` holds the fields of this task's
    own V-set, (nspec2, COUNT(kvset == mysetv)), and may be None on a task whose V-set owns none (it still takes part).
    mem_space=EMI_MEM_DEVICE (emi_gath_spec_m): `pspec` is a contiguous device tensor used in place (a numpy array on the CPU emulator
    of the tests); glob_space: the memory of the returned global image (default host: a numpy array; EMI_MEM_DEVICE: a device
    tensor, the (nspec2g, n_mine) view of the [n_mine][nspec2g] image)."""
    return _gath_spec("", kresol, pspec, kfgathg, kto, mem_space, glob_space, kvset)


def _gath_spec(_e, kresol, pspec, kfgathg, kto, mem_space=None, glob_space=None, kvset=None):
    """gath_spec (_e = "") / egath_spec (_e = "e")"""
    dt = real_dtype(kresol)
    ns2g, me = trans_inq(kresol, "nspec2g"), trans_inq(kresol, "myproc")
    who = _e.upper() + "GATH_SPEC"
    kto = _roots(kto, kfgathg, who + ":KTO")
    nm = int((kto == me).sum())
    kv, nfl = (None, kfgathg) if kvset is None else _kvset_local(kresol, kvset, kfgathg, who)
    if mem_space is not None or glob_space is not None or kv is not None:
        host = mem_space is None and glob_space is None  # (kvset alone: host arrays through the general entry point)
        ls, gs = (EMI_MEM_HOST, EMI_MEM_HOST) if host else _gs_spaces(who, mem_space, glob_space)
        if host and pspec is not None:
            pspec = np.ascontiguousarray(_np(pspec), dtype=dt)
        if nfl == 0 and (pspec is None or pspec.shape[-1] == 0):
            pspec = None  # a task whose V-set owns no field: no local array, and it follows the path of the others
        elif pspec is None or pspec.ndim != 2 or pspec.shape[1] != nfl or pspec.shape[0] != trans_inq(kresol, "nspec2"):
            raise TransError("%s: PSPEC must have shape (nspec2, %d)" % (who, nfl))
        g = _gs_zeros((nm, ns2g), dt, gs == EMI_MEM_DEVICE, pspec) if nm else None
        a = (kresol, gs, _gs_ptr(g, dt, who, "PSPECG"), kfgathg, _iptr(kto))
        b = (ls, _gs_ptr(pspec, dt, who, "PSPEC"))
        _chk(getattr(lib(), "emi_%sgath_spec_m" % _e)(*a, *b) if kv is None else lib().emi_gath_spec_v(*a, _iptr(kv), *b))
        return None if g is None else (g.t() if _is_torch(g) else np.ascontiguousarray(g.T))
    loc = np.ascontiguousarray(_np(pspec), dtype=dt)
    g = np.zeros((nm, ns2g), dtype=dt) if nm else None
    _chk(getattr(lib(), "emi_%sgath_spec" % _e)(kresol, None if g is None else g.ctypes.data, kfgathg, _iptr(kto), loc.ctypes.data))
    return None if g is None else np.ascontiguousarray(g.T)


def gath_grid(kresol, pgp, kfgathg, kto=1, mem_space=None, glob_space=None):
    """GATH_GRID (gath_grid.h:11) over emi_gath_grid: local blocked grid array (ngpblks, kfgathg, nproma) -> global
    (n_mine, ngptotg) of the fields this task is the target of (None if none).
    mem_space=EMI_MEM_DEVICE (emi_gath_grid_m): `pgp` is a contiguous device tensor used in place (a numpy array on the CPU emulator
    of the tests); glob_space: the memory of the returned global image (default host)."""
    return _gath_grid("", kresol, pgp, kfgathg, kto, mem_space, glob_space)


def _gath_grid(_e, kresol, pgp, kfgathg, kto, mem_space=None, glob_space=None):
    """gath_grid (_e = "") / egath_grid (_e = "e")"""
    dt = real_dtype(kresol)
    ngg, me = trans_inq(kresol, "ngptotg"), trans_inq(kresol, "myproc")
    who = _e.upper() + "GATH_GRID"
    kto = _roots(kto, kfgathg, who + ":KTO")
    nm = int((kto == me).sum())
    if mem_space is not None or glob_space is not None:
        ls, gs = _gs_spaces(who, mem_space, glob_space)
        ngl = trans_inq(kresol, "ngptot")
        if pgp.ndim != 3 or pgp.shape[1] != kfgathg or pgp.shape[0] != (ngl - 1) // int(pgp.shape[2]) + 1:
            raise TransError("%s: PGP must have shape (ngpblks, kfgathg=%d, nproma)" % (who, kfgathg))
        g = _gs_zeros((nm, ngg), dt, gs == EMI_MEM_DEVICE, pgp) if nm else None
        _chk(getattr(lib(), "emi_%sgath_grid_m" % _e)(kresol, gs, _gs_ptr(g, dt, who, "PGPG"), kfgathg, _iptr(kto), int(pgp.shape[2]), ls,
                                                      _gs_ptr(pgp, dt, who, "PGP")))
        return g
    loc = np.ascontiguousarray(_np(pgp), dtype=dt)
    if loc.ndim != 3 or loc.shape[1] != kfgathg:
        raise TransError("%s: PGP must have shape (ngpblks, kfgathg=%d, nproma)" % (who, kfgathg))
    g = np.zeros((nm, ngg), dtype=dt) if nm else None
    _chk(getattr(lib(), "emi_%sgath_grid" % _e)(kresol, None if g is None else g.ctypes.data, kfgathg, _iptr(kto), loc.shape[2], loc.ctypes.data))
    return g


def dist_grid(kresol, pgpg, kfdistg, kfrom=1, kproma=None, mem_space=None, glob_space=None):
    """DIST_GRID (dist_grid.h:11) over emi_dist_grid: global (kfdistg, ngptotg) on task kfrom[f] -> this task's blocked
    (ngpblks, kfdistg, nproma) array (padding of the last block zero).
    mem_space=EMI_MEM_DEVICE (emi_dist_grid_m): the local array is laid out on the device and returned as a device tensor (a numpy
    array on the CPU emulator of the tests); glob_space: the memory the global image is consumed from (default: where `pgpg` lives).
    mem_space=EMI_MEM_AUTO, and glob_space= given alone, mean EMI_MEM_DEVICE, as for ``dist_spec``."""
    return _dist_grid("", kresol, pgpg, kfdistg, kfrom, kproma, None, mem_space, glob_space)


def _dist_grid(_e, kresol, pgpg, kfdistg, kfrom, kproma, ksort, mem_space=None, glob_space=None):
    """dist_grid (_e = "") / edist_grid (_e = "e")"""
    dt = real_dtype(kresol)
    ngl, ngg, me = trans_inq(kresol, "ngptot"), trans_inq(kresol, "ngptotg"), trans_inq(kresol, "myproc")
    who = _e.upper() + "DIST_GRID"
    kfrom = _roots(kfrom, kfdistg, who + ":KFROM")
    mine = np.flatnonzero(kfrom == me)
    nproma = int(kproma) if kproma else ngl
    ks = None if ksort is None else np.ascontiguousarray(ksort, dtype=np.int32)
    if mem_space is not None or glob_space is not None:
        ls, gs = _gs_spaces(who, mem_space, glob_space, pgpg)
        g = None
        if mine.size:
            if pgpg.shape[-1] != ngg:
                raise TransError("%s: PGPG must have shape (nfld, ngptotg=%d)" % (who, ngg))
            g = _gs_move(pgpg[mine.tolist()], dt, gs == EMI_MEM_DEVICE)
        out = _gs_zeros(((ngl - 1) // nproma + 1, kfdistg, nproma), dt, ls != EMI_MEM_HOST, pgpg)
        _chk(getattr(lib(), "emi_%sdist_grid_m" % _e)(kresol, gs, _gs_ptr(g, dt, who, "PGPG"), kfdistg, _iptr(kfrom), None if ks is None else _iptr(ks),
                                                      nproma, EMI_MEM_HOST if ls == EMI_MEM_HOST else EMI_MEM_DEVICE, _gs_ptr(out, dt, who, "PGP")))
        return out
    g = None
    if mine.size:
        a = _np(pgpg)
        if a.shape[-1] != ngg:
            raise TransError("%s: PGPG must have shape (nfld, ngptotg=%d)" % (who, ngg))
        g = np.ascontiguousarray(a[mine], dtype=dt)
    out = np.zeros(((ngl - 1) // nproma + 1, kfdistg, nproma), dtype=dt)
    _chk(getattr(lib(), "emi_%sdist_grid" % _e)(kresol, None if g is None else g.ctypes.data, kfdistg, _iptr(kfrom),
                                                None if ks is None else _iptr(ks), nproma, out.ctypes.data))
    return out


def edist_spec(kresol, pspecg, kfdistg, kfrom=1, ksort=None, mem_space=None, glob_space=None):
    """EDIST_SPEC (edist_spec.h): ``dist_spec`` on a handle of ``esetup_trans``.  A global spectral field is the one-task layout:
    m = 0 .. KMSMAX ascending, 4 (KNTMP(m) + 1) reals each.  ksort: field f lands in column ksort[f] (1-based) of the result."""
    return _dist_spec("e", kresol, pspecg, kfdistg, kfrom, ksort, mem_space, glob_space)


def egath_spec(kresol, pspec, kfgathg, kto=1, ksmax=None, kmsmax=None, ldza0ip=False, mem_space=None, glob_space=None):
    """EGATH_SPEC (egath_spec.h): ``gath_spec`` on a handle of ``esetup_trans``.  The whole spectrum only: ksmax / kmsmax are accepted
    where they equal the handle's, and ldza0ip, which addresses the spherical layout, is refused."""
    if (ksmax is not None and int(ksmax) != etrans_inq(kresol, "nsmax")) or (kmsmax is not None and int(kmsmax) != etrans_inq(kresol, "nmsmax")):
        raise TransError("EGATH_SPEC: KSMAX / KMSMAX (truncated gather) not supported")
    if ldza0ip:
        raise TransError("EGATH_SPEC: LDZA0IP not supported")
    return _gath_spec("e", kresol, pspec, kfgathg, kto, mem_space, glob_space)


def edist_grid(kresol, pgpg, kfdistg, kfrom=1, kproma=None, ksort=None, mem_space=None, glob_space=None):
    """EDIST_GRID (edist_grid.h): ``dist_grid`` on a handle of ``esetup_trans``.  A global grid field is the NDGL x NDLON points row
    after row.  ksort: field f lands in slot ksort[f] (1-based) of the result."""
    return _dist_grid("e", kresol, pgpg, kfdistg, kfrom, kproma, ksort, mem_space, glob_space)


def egath_grid(kresol, pgp, kfgathg, kto=1, mem_space=None, glob_space=None):
    """EGATH_GRID (egath_grid.h): ``gath_grid`` on a handle of ``esetup_trans``."""
    return _gath_grid("e", kresol, pgp, kfgathg, kto, mem_space, glob_space)


def trans_release(kresol):
    _chk(lib().emi_release(kresol))


def trim_cache():
    """Frees the idle device staging buffers of host-array calls (emi_trim_cache); TRANS_RELEASE and TRANS_END do it too."""
    _chk(lib().emi_trim_cache())


def trans_end():
    _chk(lib().emi_finalize())
    _DIST.update(nproc=1, nprtrv=1, group=None, device=None)


def work_model(kresol, nfields):
    """Algorithmic work per direction for `nfields` Fourier-space fields."""
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    _chk(lib().emi_work_model(kresol, nfields, C.byref(a), C.byref(b), C.byref(c)))
    return {"legendre_flops": a.value, "fft_flops": b.value, "fourier_bytes": c.value}


def last_phase_ms():
    """Device time (ms) of the last inv_trans/dir_trans call per phase
    [spectral pack/unpack, Legendre MFMA kernel, FFT kernels] -- needs set_profile(True)."""
    out = (C.c_double * 3)()
    lib().emi_last_phase_ms(out)
    return list(out)


def last_phase_launches():
    out = (C.c_int * 3)()
    lib().emi_last_phase_launches(out)
    return list(out)


def last_exchange():
    """(ms, calls, bytes_sent) of the all-to-all-v exchanges since set_profile(): HIP events around the hook on the exchange stream."""
    ms, n, b = C.c_double(), C.c_int(), C.c_double()
    lib().emi_last_exchange(C.byref(ms), C.byref(n), C.byref(b))
    return ms.value, n.value, b.value


def last_fft_launches():
    """kernel launches of the FFT phases since set_profile()"""
    k = C.c_longlong()
    lib().emi_last_fft_launches(C.byref(k))
    return k.value


def set_profile(on):
    """True / 1: HIP-event phase timers per call (last_phase_ms() of the last call); 2: accumulated over all calls
    since this set_profile(2) -- nothing is resolved, so nothing synchronises, between the calls of a timed loop."""
    lib().emi_set_profile(int(on))


def set_max_batch(n):
    lib().emi_set_max_batch(int(n))
