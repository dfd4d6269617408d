"""The Fortran drop-in shim and the transi-style C layer, driven by small native callers on the GPU."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(subdir, target, marker):
    d = os.path.join(ROOT, "ectrans_amd", subdir)
    subprocess.check_call(["make", "-s", "-C", d, target])
    p = subprocess.run([os.path.join(d, target)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert marker in p.stdout


def test_fortran_shim_roundtrip():
    """SETUP_TRANS0/SETUP_TRANS/TRANS_INQ/INV_TRANS/DIR_TRANS/SPECNORM with the reference's keyword
    interfaces (tests/fortran/test_shim.F90): benchmark harmonic, norm drift <= 100 eps."""
    _run("fortran", "test_shim", "FORTRAN SHIM OK")


def test_fortran_shim_single_precision():
    """The same caller compiled with JPRB = real32 against the _sp flavour of the shim (-DEMI_SP):
    SETUP_TRANS selects the fp32 kernels; norm drift <= 100 epsilon(1.0_jprb)."""
    _run("fortran", "test_shim_sp", "FORTRAN SHIM OK (JPRB = real32)")


def test_fortran_shim_both_precisions_in_one_executable():
    """ecTrans 1.7.0 names its entry points per precision (INV_TRANS_DP / INV_TRANS_SP, ...: src/trans/CMakeLists.txt:43-93,
    sedrenames.txt) so that trans_dp and trans_sp live in one executable, as IFS uses them.  tests/fortran/test_shim_both.F90 links
    libectrans_mi_f.so AND libectrans_mi_f_sp.so (+ the common library with SETUP_TRANS0), takes its interface blocks from
    ectrans_amd/fortran/include/*_dp.h / *_sp.h and runs a real64 and a real32 resolution side by side: dp round trip 1e-12, sp against
    dp at float accuracy (and not better: the sp library ran fp32 kernels)."""
    _run("fortran", "test_shim_both", "FORTRAN SHIM OK (dp and sp in one executable)")


def test_fortran_shim_generic_names_through_compat_headers():
    """A caller written against the generic names (`#include "inv_trans.h"`, CALL INV_TRANS) compiled with -Iinclude/trans_dp: the
    backward-compatibility headers of src/trans/CMakeLists.txt:76-85 map it onto the _DP entry points."""
    _run("fortran", "test_shim_compat", "FORTRAN SHIM OK (generic names through include/trans_dp)")


def test_transi_c_api():
    """trans_new/trans_setup/trans_inquire/trans_dirtrans/trans_invtrans/trans_specnorm
    (tests/transi/transi_test.c, modelled on the reference's transi_test_program.c)."""
    _run("transi", "transi_test", "TRANSI API OK")


def test_fortran_shim_device_resident_arrays(tmp_path):
    """Fields that live in DEVICE memory through the reference's own Fortran interface (the reference GPU
    back-end's present-or-copyin, gpu/internal/trltog_mod.F90:501-523, ltinv_mod.F90:334-338): tests/fortran/test_shim_device.F90
    hipMalloc's its call-mode-2 arrays, wraps them with C_F_POINTER and calls INV_TRANS / DIR_TRANS / SPECNORM of the shim
    (EMI_MEM_AUTO -> hipPointerGetAttributes -> used in place).  Harmonic round trip (norm drift <= 100 eps, bit-identical to the
    staged host-array calls) + a dense sample from the ORACLE written here, uploaded by the Fortran program and compared
    element-wise in both directions.  A call with arrays in both memories, and a strided section of a device array, must abort."""
    from oracle.oracle import Oracle
    from tests.common import octahedral, random_spectrum
    N, nf = 47, 5
    nloen = octahedral(N)
    o = Oracle(N, nloen)
    sp = random_spectrum(np.random.default_rng(20251114), o.nasm0, N, o.nspec2, nf, False)
    g = o.inv_trans(spsc=sp)             # [nf, ngptot] = PGP(ngptot, nf, 1)
    back = o.dir_trans(g, nsc=nf)[2]     # [nspec2, nf] = PSPSCALAR(nf, nspec2)
    f = tmp_path / "dense_t47.bin"
    with open(f, "wb") as fh:
        np.array([N, o.nspec2, o.ngptot, nf], dtype=np.int32).tofile(fh)
        np.ascontiguousarray(sp, dtype=np.float64).tofile(fh)
        np.ascontiguousarray(g, dtype=np.float64).tofile(fh)
        np.ascontiguousarray(back, dtype=np.float64).tofile(fh)
    d = os.path.join(ROOT, "ectrans_amd", "fortran")
    subprocess.check_call(["make", "-s", "-C", d, "test_shim_device"])
    exe = os.path.join(d, "test_shim_device")
    p = subprocess.run([exe, "dense", str(f)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "FORTRAN SHIM DEVICE ARRAYS OK" in p.stdout and "DENSE ORACLE SAMPLE OK" in p.stdout, p.stdout + p.stderr
    p = subprocess.run([exe, "mixed"], capture_output=True, text=True, timeout=600)
    assert p.returncode != 0 and "NOT REFUSED" not in p.stdout and "IN DEVICE MEMORY AND" in p.stderr, p.stdout + p.stderr
    p = subprocess.run([exe, "section"], capture_output=True, text=True, timeout=600)
    assert p.returncode != 0 and "NOT REFUSED" not in p.stdout and "IS IN DEVICE MEMORY AND NOT CONTIGUOUS" in p.stderr, p.stdout + p.stderr


def test_transi_device_resident_arrays():
    """The same through the transi-style C layer (tests/transi/transi_test_device.c): rgp / rspscalar / rspvor / rspdiv from
    hipMalloc; bit-identical to the staged host-array calls; a host / device mixture is refused."""
    _run("transi", "transi_test_device", "TRANSI DEVICE ARRAYS OK")


def test_mem_auto_through_the_cabi():
    """EMI_MEM_AUTO of the C-ABI itself (include/ectrans_mi.h): emi_ptr_space classifies device, pinned and pageable
    memory; an AUTO call on device tensors gives the bits of the explicit EMI_MEM_DEVICE call, on numpy arrays the bits of
    the EMI_MEM_HOST call; a mixture returns EMI_ERR_ARG with the abort text."""
    import sys
    code = """
import ctypes as C, numpy as np, torch, sys
sys.path.insert(0, %r)
import ectrans_amd as et
from tests.common import octahedral, random_spectrum
et.setup_trans0(kmax_resol=2, device=0)
N = 31; nloen = octahedral(N)
r = et.setup_trans(N, len(nloen), nloen)
L = et.lib()
ns2, ng = et.trans_inq(r, "nspec2"), et.trans_inq(r, "ngptot")
nasm0 = et.trans_inq(r, "nasm0")
sp = random_spectrum(np.random.default_rng(3), nasm0, N, ns2, 4, False)
dsp = torch.from_numpy(sp).to("cuda:0")
pin = torch.zeros(8, dtype=torch.float64).pin_memory()
assert L.emi_ptr_space(C.c_void_p(dsp.data_ptr())) == 1 and L.emi_ptr_space(C.c_void_p(sp.ctypes.data)) == 0
assert L.emi_ptr_space(C.c_void_p(pin.data_ptr())) == 0 and L.emi_ptr_space(None) == 0
def call(space, spp, gpp):
    a = et._Inv()
    a.mem_space = space; a.spscalar = spp; a.nf_scalar = 4; a.kproma = ng; a.gp = gpp; a.gp_nfld = 4
    return L.emi_inv_trans(r, C.byref(a))
g_dev, g_auto = (torch.zeros((1, 4, ng), dtype=torch.float64, device="cuda:0") for _ in range(2))
assert call(1, dsp.data_ptr(), g_dev.data_ptr()) == 0 and call(2, dsp.data_ptr(), g_auto.data_ptr()) == 0
torch.cuda.synchronize()
assert L.emi_wait(r) == 0 and L.emi_wait(0) == 0
assert torch.equal(g_dev, g_auto)
h_host, h_auto = np.zeros((1, 4, ng)), np.zeros((1, 4, ng))
assert call(0, sp.ctypes.data, h_host.ctypes.data) == 0 and call(2, sp.ctypes.data, h_auto.ctypes.data) == 0
assert np.array_equal(h_host, h_auto) and np.array_equal(h_host, g_dev.cpu().numpy())
assert call(2, dsp.data_ptr(), h_auto.ctypes.data) == -1
msg = L.emi_last_error().decode()
assert "DEVICE MEMORY AND" in msg and "HOST MEMORY" in msg, msg
assert call(7, dsp.data_ptr(), g_auto.data_ptr()) == -1
et.trans_end()
print("MEM AUTO OK")
""" % ROOT
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "MEM AUTO OK" in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("world,nsc,prec", [(2, 2, 8), (4, 2, 8), (2, 300, 8), (3, 300, 8), (2, 300, 4)])
def test_multi_rank_path_on_one_gpu(world, nsc, prec):
    """The N > 1 path with the REAL HIP kernels: `world` ranks share cuda:0 (RCCL cannot put two
    ranks on one device, so the hook stages the all-to-all-v through gloo -- ectrans_amd/dist.py);
    every rank checks its wavenumber/latitude share against the oracle (tests/dist_worker.py).
    With 300 scalar fields the calls run as 4 pipelined batches: Legendre, exchange and FFT of
    different batches on three streams with double-buffered Fourier buffers (EMI_PIPELINE_DIST)."""
    import sys
    port = 29540 + world + (10 if nsc > 2 else 0) + (20 if prec == 4 else 0)
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   EMI_TEST_NSMAX="63", EMI_TEST_DEVICE="cuda", EMI_TEST_NSC=str(nsc), EMI_TEST_PRECISION=str(prec))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ("DIST OK rank %d" % rank) in out, out


@pytest.mark.parametrize("world,nsc,transport", [(2, 2, "rccl"), (2, 300, "rccl"), (4, 300, "rccl"), (8, 300, "rccl"), (2, 300, "torch")])
def test_multi_gpu_native_rccl_exchange(world, nsc, transport):
    """One task per GPU over the native RCCL transport (emi_rccl_alltoallv: grouped ncclSend / ncclRecv over xGMI) -- exactly the
    configuration `bench.py --gpus N` times.  RCCL refuses two tasks on one device, so this runs only where
    torch.cuda.device_count() >= world and is SKIPPED on the one-GPU box: the first driver run on a multi-GPU node exercises the
    exchange here, with every task checked against the oracle (tests/dist_worker.py; 300 fields = 4 pipelined batches on three
    streams), before the bench does.  `torch`: the torch.distributed (nccl) callback transport, the bench's fallback."""
    import sys
    import torch
    if torch.cuda.device_count() < world:
        pytest.skip("%d GPUs needed, %d visible" % (world, torch.cuda.device_count()))
    port = 29700 + world + (10 if nsc > 2 else 0) + (20 if transport == "torch" else 0)
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), EMI_TEST_NSMAX="63",
                   EMI_TEST_DEVICE="cuda_per_rank", EMI_TEST_NSC=str(nsc), EMI_TEST_TRANSPORT=transport, HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_worker.py")], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ("DIST OK rank %d" % rank) in out, out


@pytest.mark.parametrize("nranks", [2, 3])
def test_mpi_host_with_alltoallv_hook(nranks):
    """A C / MPI host of the C-ABI (tests/mpi/test_mpi_hook.c): `mpiexec -n N`, every rank one task of the
    W-set, the all-to-all-v hook of ectrans_amd/mpi/emi_mpi_hook.c (MPI_Alltoallv, staged through pinned host
    memory because this MPICH is not GPU-aware; the ranks share the one GPU).  Skipped without MPI."""
    import shutil
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if not os.path.exists(mpiexec) or not os.path.exists("/opt/conda/lib/libmpi.so"):
        pytest.skip("no MPI installation")
    d = os.path.join(ROOT, "ectrans_amd", "mpi")
    subprocess.check_call(["make", "-s", "-C", d, "test_mpi_hook"])
    env = dict(os.environ, LD_LIBRARY_PATH="/usr/lib/x86_64-linux-gnu:/opt/conda/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([mpiexec, "-n", str(nranks), os.path.join(d, "test_mpi_hook")], capture_output=True, text=True, timeout=600,
                       env=env)
    assert p.returncode == 0 and p.stdout.count("MPI HOOK OK") == nranks, p.stdout + p.stderr


def test_decomposition_invariance_and_checksum_dumps(tmp_path):
    """1 task vs 2 / 4 / 8 tasks with the HIP kernels (the ranks share cuda:0, exchange staged through gloo): the same
    dense fields, gathered with GATH_GRID / GATH_SPEC, agree to 1e-13 and the CRC-64 dumps in the reference's text format
    (ectrans-benchmark.F90:1455-1600) are byte-identical -- the reference's own criterion (tests/compare_checksums.py:11-60).
    TCo63, NPROMA = 1000 (several blocks, a padded last one)."""
    from tests.test_decomposition_invariance import check_invariance, run_decompositions
    res = run_decompositions(tmp_path, (1, 2, 4, 8), "cuda", 63, 29580, extra_env={"EMI_TEST_NPROMA": "1000", "EMI_TEST_NLEV": "3"},
                             nthreads="8")
    check_invariance(res)


@pytest.mark.parametrize("ngpus,nprtrv", [(2, 1), (4, 1), (8, 1), (8, 2), (4, 4)])
def test_bench_multi_rank_launch(ngpus, nprtrv):
    """`bench.py --gpus N` in its test configuration (EMI_BENCH_BACKEND=gloo, EMI_BENCH_ONE_GPU=1: N ranks share the one
    GPU, the exchange is staged through the host) at TCo399: the launcher, the sharded set-up, the timed loop and the
    JSON line -- so that the first run on an 8-GPU node cannot fail for software reasons.  (8, 2) is the split the
    reference's benchmark picks for 8 tasks (ectrans-benchmark.F90:280-306): `--nprtrv 2`, levels dealt to two V-sets."""
    import json
    import sys
    env = dict(os.environ, EMI_BENCH_BACKEND="gloo", EMI_BENCH_ONE_GPU="1", EMI_BENCH_PREFLIGHT="1")  # the T63 pre-flight pair of the exchange too
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(ngpus), "--nsmax", "399", "--nlev", "30", "--nfld", "2",
                        "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--nprtrv", str(nprtrv)], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout + p.stderr
    out = json.loads(lines[0])
    assert out["n_gpus"] == ngpus and out["steps"] == 2 and out["unit"] == "pairs/s" and out["scaling"] == "strong"
    assert out["value"] > 0 and np.isfinite(out["value"]) and abs(out["ms_per_step"] * out["value"] - 1000.0) < 1e-6 * 1000
    assert abs(out["roofline"]["peak"] - ngpus * 78.6) < 1e-9 and 0 < out["roofline"]["frac"] < 1
    assert out["config"]["world_size"] == ngpus and out["config"]["backend"] == "gloo"
    assert out["config"]["nprtrv"] == nprtrv and out["config"]["nprtrw"] * nprtrv == ngpus
    assert out["config"]["exchange_preflight"] == "ok"
    assert out["spectral_norm_rel_error"] < 1e-12
    # the keys that make the first run on an 8-GPU node self-explaining
    assert out["exchange_ms_per_step"] > 0 and (out["overlap_frac"] is None or 0.0 <= out["overlap_frac"] <= 1.0)
    rp = out["rank_phase_ms_per_step"]
    for k in ("ms_per_step", "spectral_pack_unpack", "legendre_mfma", "fft", "exchange"):
        assert 0 <= rp[k]["min"] <= rp[k]["mean"] <= rp[k]["max"], (k, rp[k])
    assert rp["legendre_mfma"]["min"] > 0 and rp["fft"]["min"] > 0
    ex = out["exchange"]
    assert ex["exchanges_per_step"] >= 2 and ex["bytes_sent_per_rank_and_step"] > 0 and ex["links_used_per_rank"] == max(out["config"]["nprtrw"] - 1, 1)
    assert ex["bytes_per_link_per_step"] > 0 and ex["achieved_GBps_per_link"] > 0
    assert out["fft_launches_per_direction"] >= 1


def test_bench_plain_run_and_dump(tmp_path):
    """A plain `bench.py` run (no --full) times only the headline loop: the line carries the driver's keys and none of the side legs;
    --steps sets the timed steps; --dump-outputs writes the arrays of the last timed step, the same values run after run, and the
    spectral ones hold the benchmark harmonic after its round trips."""
    import json
    import sys
    outs = []
    for i in range(2):
        d = tmp_path / ("dump%d" % i)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--nsmax", "159", "--nlev", "10", "--nfld", "2",
                            "--steps", str(3 + i), "--warmup", "1", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout + p.stderr
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout + p.stderr
        out = json.loads(lines[0])
        assert out["steps"] == 3 + i and out["unit"] == "pairs/s" and out["dtype"] == "f64" and out["higher_is_better"] is True
        assert abs(out["ms_per_step"] * out["value"] - 1000.0) < 1e-6 * 1000 and out["spectral_norm_rel_error"] < 1e-12
        for k in ("dense_timing", "api_level", "cpu_baseline", "cpu_baseline_blas", "dense", "fortran_device_resident"):
            assert k not in out, k
        outs.append({n: np.load(str(d / (n + ".npy"))) for n in ("gpuv", "gp3a", "gp2", "spvor", "spdiv", "spsc3a", "spsc2")})
    assert sum(a.nbytes for a in outs[0].values()) <= 64e6
    for n, a in outs[0].items():
        b = outs[1][n]
        assert a.dtype == np.float64 and a.shape == b.shape and np.isfinite(a).all(), n
        assert np.abs(a - b).max() <= 1e-10 * np.abs(a).max(), n
    assert outs[0]["spsc2"].shape == (160 * 161, 1) and abs(outs[0]["spsc2"].max() - 1.0) < 1e-10
    assert outs[0]["gp3a"].shape[:3] == (1, 2, 10) and np.abs(outs[0]["gp3a"]).max() > 0.1


def test_native_rccl_transport():
    """ectrans_amd/rccl/emi_rccl_hook.c: the all-to-all-v as grouped ncclSend / ncclRecv on the library's stream, for hosts
    without Python (tests/rccl/test_rccl_hook.c, the RCCL twin of the MPI host).  One task here exercises
    ncclCommInitRank, SPECNORM's ncclAllReduce path and the exchange entry itself; with `mpiexec -n 2` the unique id
    travels by MPI_Bcast -- RCCL refuses two tasks on one device, so on a one-GPU box that run reports it and is
    accepted as skipped."""
    import shutil
    d = os.path.join(ROOT, "ectrans_amd", "rccl")
    subprocess.check_call(["make", "-s", "-C", d, "all", "test_rccl_hook"])
    p = subprocess.run([os.path.join(d, "test_rccl_hook")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "RCCL HOOK OK rank 0 of 1" in p.stdout, p.stdout + p.stderr
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if os.path.exists(mpiexec) and os.path.exists("/opt/conda/lib/libmpi.so"):
        subprocess.check_call(["make", "-s", "-C", d, "test_rccl_hook_mpi"])
        env = dict(os.environ, LD_LIBRARY_PATH="/usr/lib/x86_64-linux-gnu:/opt/conda/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
        p = subprocess.run([mpiexec, "-n", "2", os.path.join(d, "test_rccl_hook_mpi")], capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, p.stdout + p.stderr
        assert p.stdout.count("RCCL HOOK OK") == 2 or p.stdout.count("RCCL REFUSED") == 2, p.stdout + p.stderr


@pytest.mark.parametrize("ntasks", [1, 2, 3])
def test_fortran_shim_several_tasks(ntasks):
    """The Fortran drop-in with several tasks (tests/fortran/test_shim_mpi.F90 under mpiexec): the MPI transport is
    attached first, SETUP_TRANS0 takes MYPROC / NPROC from the library, and DIST_SPEC -> INV_TRANS -> GATH_GRID ->
    DIST_GRID -> DIR_TRANS -> GATH_SPEC between different source / target tasks returns the dense global fields;
    SPECNORM gives every task the global norms (dist_spec_control_mod.F90, gath_grid_ctl_mod.F90, spnormc_mod.F90).
    Skipped without MPI."""
    import shutil
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if not os.path.exists(mpiexec) or not os.path.exists("/opt/conda/lib/libmpi.so"):
        pytest.skip("no MPI installation")
    d = os.path.join(ROOT, "ectrans_amd", "fortran")
    subprocess.check_call(["make", "-s", "-C", d, "test_shim_mpi"])
    env = dict(os.environ, LD_LIBRARY_PATH="/usr/lib/x86_64-linux-gnu:/opt/conda/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([mpiexec, "-n", str(ntasks), os.path.join(d, "test_shim_mpi")], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0 and p.stdout.count("FORTRAN SHIM MPI OK") == ntasks, p.stdout + p.stderr


@pytest.mark.parametrize("ntasks", [1, 2, 3])
def test_transi_c_api_several_tasks(ntasks):
    """The transi-style C layer with several tasks (tests/transi/transi_test_mpi.c under mpiexec; the reference: transi
    with TRANS_USE_MPI): trans_init adopts the attached MPI transport; trans_distspec -> trans_invtrans ->
    trans_gathgrid -> trans_distgrid -> trans_dirtrans -> trans_gathspec between different source / target tasks
    returns the global fields (1e-10: the octahedral grid's own truncation), trans_specnorm the global norms on every task.  Skipped without MPI."""
    import shutil
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if not os.path.exists(mpiexec) or not os.path.exists("/opt/conda/lib/libmpi.so"):
        pytest.skip("no MPI installation")
    d = os.path.join(ROOT, "ectrans_amd", "transi")
    subprocess.check_call(["make", "-s", "-C", d, "transi_test_mpi"])
    env = dict(os.environ, LD_LIBRARY_PATH="/usr/lib/x86_64-linux-gnu:/opt/conda/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([mpiexec, "-n", str(ntasks), os.path.join(d, "transi_test_mpi")], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0 and p.stdout.count("TRANSI MPI OK") == ntasks, p.stdout + p.stderr


def test_python_host_attaches_the_native_rccl_transport():
    """setup_trans0(transport="rccl") -- what `bench.py --gpus N` uses for N > 1 (round 3): emi_rccl_get_unique_id,
    emi_rccl_attach (communicator, exchange hook, host collectives, emi_init) from a Python host, then a transform pair
    against the oracle.  One task on the one-GPU box (RCCL refuses two ranks on one device); own process: the
    library is initialised once per process."""
    import sys
    code = """
import numpy as np, torch, sys
sys.path.insert(0, %r)
import ectrans_amd as et
from oracle.oracle import Oracle
from tests.common import octahedral, random_spectrum
et.setup_trans0(kmax_resol=2, device=0, kprtrw=1, myproc=1, transport="rccl")
assert et.inq_init()[0] == 2
N = 21; nloen = octahedral(N)
r = et.setup_trans(N, len(nloen), nloen)
o = Oracle(N, nloen)
sp = random_spectrum(np.random.default_rng(2), o.nasm0, N, o.nspec2, 3, False)
gp = torch.zeros((1, 3, o.ngptot), dtype=torch.float64, device="cuda:0")
et.inv_trans(r, pspscalar=torch.from_numpy(sp).to("cuda:0"), pgp=gp)
g = o.inv_trans(spsc=sp)
assert np.abs(gp[0].cpu().numpy() - g).max() / np.abs(g).max() < 1e-12
s2 = torch.zeros((o.nspec2, 3), dtype=torch.float64, device="cuda:0")
et.dir_trans(r, pspscalar=s2, pgp=gp)
ref = o.dir_trans(g, nsc=3)[2]
assert np.abs(s2.cpu().numpy() - ref).max() / np.abs(ref).max() < 1e-12
assert abs(et.specnorm(r, s2)[0] / o.specnorm(ref)[0] - 1) < 1e-13
et.trans_end()
print("NATIVE RCCL ATTACH OK")
""" % ROOT
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "NATIVE RCCL ATTACH OK" in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("world,nprtrv,prec", [(2, 2, 8), (4, 2, 8), (6, 3, 8), (4, 2, 4)])
def test_vset_sharding_on_one_gpu(world, nprtrv, prec):
    """NPRTRV > 1 with the HIP kernels (round 3; sump_trans0_mod.F90:49, inv_trans.F90:212-300): NPRTRW x NPRTRV tasks share cuda:0,
    both exchanges -- TRMTOL / TRLTOM inside a V-set, TRLTOG / TRGTOL between the V-sets of a band (k_gridcopy packs) -- staged through
    gloo; every task checks its wavenumbers x its V-set's fields, and ALL fields on its own latitudes, against the oracle
    (tests/vsets_worker.py), single PGP with every derivative option and call mode 2 with levels dealt to the V-sets."""
    from tests.test_dist_gloo import run_vsets
    run_vsets(world, nprtrv, 29640 + world + nprtrv + (20 if prec == 4 else 0), device="cuda", extra={"EMI_TEST_NSMAX": "63", "EMI_TEST_PRECISION": str(prec)})


@pytest.mark.parametrize("ntasks", [2, 4])
def test_fortran_shim_with_two_vsets(ntasks):
    """The Fortran drop-in with NPRTRV = 2 (tests/fortran/test_shim_vsets.F90 under mpiexec -n 2 / -n 4: 1 x 2 and 2 x 2 tasks):
    SETUP_TRANS0(KPRTRW = NPROC / 2), KVSETSC honoured by INV_TRANS / DIR_TRANS, TRANS_INQ's KMYSETW / KMYSETV / KFRSTLAT, SPECNORM
    with KVSET.  Checks without an oracle: field f = f P_1^0 lands as f sqrt(3) mu in slot f of PGP on every task's own
    latitudes, and dense fields survive INV_TRANS -> DIR_TRANS.  Skipped without MPI."""
    import shutil
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if not os.path.exists(mpiexec) or not os.path.exists("/opt/conda/lib/libmpi.so"):
        pytest.skip("no MPI installation")
    d = os.path.join(ROOT, "ectrans_amd", "fortran")
    subprocess.check_call(["make", "-s", "-C", d, "test_shim_vsets"])
    env = dict(os.environ, LD_LIBRARY_PATH="/usr/lib/x86_64-linux-gnu:/opt/conda/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([mpiexec, "-n", str(ntasks), os.path.join(d, "test_shim_vsets")], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0 and p.stdout.count("FORTRAN SHIM VSETS OK") == ntasks, p.stdout + p.stderr


def test_bench_line_contract():
    """`bench.py --full` on one GPU at a small size with every leg on (oracle port, library BLAS + FFT, dense parity, host-array rate): ONE JSON line
    with the driver's keys and the two blocks this tier adds -- `roofline` (bound, achieved, peak, unit, frac, traffic) and
    `cpu_baseline` (value, unit, cores, kind, sample) -- plus `cpu_baseline_blas`, `fft_bound`, `dense`."""
    import json
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--nsmax", "159", "--nlev", "10", "--nfld", "2", "--steps", "2", "--warmup", "1",
                        "--full"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout + p.stderr
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in out, k
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["warmup"] == 1 and out["unit"] == "pairs/s" and out["dtype"] == "f64" and out["vs_baseline"] is None
    assert "workload" in out["config"] and "model" not in out["config"]
    rf = out["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and "traffic" in rf
    cb = out["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1 and cb["unit"] == "pairs/s" and "sample" in cb
    bl = out["cpu_baseline_blas"]
    assert ("error" in bl) or (bl["value"] > 0 and bl["inv_max_rel_err_vs_oracle"] < 1e-12 and bl["dir_max_rel_err_vs_oracle"] < 1e-12 and bl["cores"] >= 1)
    dt_ = out["dense_timing"]
    assert dt_["ms_per_step"] > 0 and set(dt_["phase_ms_per_step"]) == {"spectral_pack_unpack", "legendre_mfma", "fft"} and 0 < dt_["roofline_frac"] < 1
    assert dt_["spectral_norm_rel_error_round_trip"] < 1e-9
    assert "fft_bound" in out and out["dense"]["inv_max_rel_err"] < 1e-11 and out["dense"]["dir_max_rel_err"] < 1e-11
    assert out["spectral_norm_rel_error"] < 1e-12
