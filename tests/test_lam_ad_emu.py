"""EINV_TRANSAD / EDIR_TRANSAD -- the limited-area adjoints -- on the CPU functional emulator (tests/emu): the same host logic and
kernels as the GPU tier (tests/test_lam_ad_gpu.py), element by element against the NumPy model of tests/lam_ad_ref.py, which
tests/test_lam_ad_model.py holds to the dense transposes of the forward model.  Bounds: 1e-11 of each output field's maximum in
fp64, 3e-5 in fp32 (tests/test_lam_gpu.py); the means against the largest coefficient of the wind."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests.lam_ad_common import ALL, CASES, FLAG_COMBOS, NONE, TOL, dot_identities, flag_id, lam_ad_case
from tests.lam_ref import ellips, zigzag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def et():
    os.environ.setdefault("OMP_NUM_THREADS", "256")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
    import ectrans_amd
    ectrans_amd._use_library_for_tests(os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so"))
    ectrans_amd.setup_trans0(kmax_resol=4)
    yield ectrans_amd
    ectrans_amd.trans_end()
    ectrans_amd._L = None


def check(errs, precision=8):
    print({k: "%.1e" % v for k, v in errs.items()})
    assert max(errs.values()) < TOL[precision], errs
    if precision == 4:
        assert max(errs.values()) > 1e-9  # really computed in float


# ---- 1. parity with the model -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAG_COMBOS, ids=flag_id)
def test_every_flag_combination(et, flags):
    check(lam_ad_case(et, 20, 18, 9, 8, flags=flags, which=("inv",)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_fp64(et, name):
    ndlon, ndgl, M, N, kw = CASES[name]
    check(lam_ad_case(et, ndlon, ndgl, M, N, **kw))


@pytest.mark.parametrize("name", ["ref_size", "prime_y", "prime_x", "m_zero", "n_zero", "atoms_meet_chunks", "call_mode_2", "in_place"])
def test_parity_fp32(et, name):
    ndlon, ndgl, M, N, kw = CASES[name]
    check(lam_ad_case(et, ndlon, ndgl, M, N, precision=4, **kw), 4)


def test_several_batches(et):
    """a field count above the batch limit: whole atoms per batch, chunks of whole atoms inside every batch"""
    et.set_max_batch(64)
    try:
        errs = lam_ad_case(et, 24, 20, 7, 6, nuv=30, nsc=40)
    finally:
        et.set_max_batch(0)
    check(errs)


# ---- 2. the dot-product identities -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("flags", [ALL, NONE], ids=flag_id)
def test_dot_product_identities(et, precision, flags):
    """<y, EINV_TRANS x> = <EINV_TRANSAD y, x> and <s, EDIR_TRANS g> = <EDIR_TRANSAD s, g>, the means among the spectral entries, sums
    with math.fsum: below 20000 eps of the precision, the tolerance of the reference's adjoint tests (tests/trans/test_adjoint.F90)."""
    eps = np.finfo(np.float64 if precision == 8 else np.float32).eps
    rel = dot_identities(et, 20, 18, 9, 8, flags=flags, precision=precision)
    print("relative differences: inverse pair %.3e, direct pair %.3e (bound %.3e)" % (rel[0], rel[1], 20000 * eps))
    assert max(rel) < 20000 * eps, rel


# ---- 3. the LDS limit --------------------------------------------------------------------------------------------------------------------
LONG = dict(scders=True, vorgp=False, divgp=False, uvder=True)
DIVGP = dict(scders=False, vorgp=False, divgp=True, uvder=False)


@pytest.mark.parametrize("ndgl,flags,need", [(1296, LONG, 0), (1296, DIVGP, 0), (1296, ALL, 0), (5103, DIVGP, 3), (1499, ALL, 4)],
                         ids=["1296-no_vordiv", "1296-divgp", "1296-all", "5103-divgp", "1499-all"])
def test_long_columns(et, ndgl, flags, need):
    """NDGL = 1296: 20 KiB a field in fp64, so the handle's workgroups hold two fields; a wind field with LDDIVGP / LDVORGP takes a work
    array of three / four.  NDGL = 5103 = 3^6 7, the longest column ESETUP_TRANS takes in fp64: two fields fill the LDS, and with
    LDDIVGP EINV_TRANSAD refuses and names the limit.  NDGL = 1499 (prime: convolution length 3000, 47 KiB a field): three fields
    fit, LDVORGP (four) is refused.  need: the fields named by the refusal, 0: parity.  (tests/test_lam_ad_gpu.py runs the parity
    cases of 1499 and 5103.)"""
    if need == 0:
        check(lam_ad_case(et, 8, ndgl, 3, 3, nuv=1, nsc=1, flags=flags, which=("inv",)))
    else:
        with pytest.raises(et.TransError, match="EINV_TRANSAD: LDVORGP / LDDIVGP WITH KDGL = %d: A WIND FIELD NEEDS %d FIELDS .* THE LDS HOLDS 160 KIB" % (ndgl, need)):
            lam_ad_case(et, 8, ndgl, 3, 3, nuv=1, nsc=1, flags=flags, which=("inv",))


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(et, monkeypatch):
    T = et.TransError
    r = et.esetup_trans(7, 6, 20, kdlon=24, pexwn=1.0, peywn=1.0)
    sc, gp = np.zeros((et.etrans_inq(r, "nspec2"), 1)), np.zeros((1, 1, 480))
    with pytest.raises(T, match="EINV_TRANSAD: FSPGL_PROC"):
        et.einv_transad(r, pspscalar=sc, pgp=gp, fspgl_proc=print)
    with pytest.raises(T, match="EDIR_TRANSAD: AUX_PROC"):
        et.edir_transad(r, pspscalar=sc, pgp=gp, aux_proc=print)
    monkeypatch.setitem(et._DIST, "nprtrv", 2)  # (ESETUP_TRANS itself refuses NPRTRV > 1)
    for fn, who in ((et.einv_transad, "EINV_TRANSAD"), (et.edir_transad, "EDIR_TRANSAD")):
        with pytest.raises(T, match=who + ": KVSET arguments: V-sets are not available on a limited-area handle"):
            fn(r, pspscalar=sc, pgp=gp, kvsetsc=np.ones(1, dtype=np.int32))
    monkeypatch.undo()
    # the spherical adjoints keep refusing a limited-area handle
    for fn, who in ((et.inv_transad, "INV_TRANSAD"), (et.dir_transad, "DIR_TRANSAD")):
        with pytest.raises(T, match=who + ": resolution %d is a limited-area handle" % r):
            fn(r, pspscalar=sc, pgp=gp)
    et.trans_release(r)
    # ... and the limited-area adjoints a Gaussian handle
    r = et.setup_trans(5, 8)
    sc, gp = np.zeros((et.trans_inq(r, "nspec2"), 1)), np.zeros((1, 1, et.trans_inq(r, "ngptot")))
    for fn, who in ((et.einv_transad, "EINV_TRANSAD"), (et.edir_transad, "EDIR_TRANSAD")):
        with pytest.raises(T, match=who + ": resolution %d is not a limited-area handle" % r):
            fn(r, pspscalar=sc, pgp=gp)
    et.trans_release(r)


# ---- 5. several tasks ----------------------------------------------------------------------------------------------------------------------
def _run_workers(nproc, outdir):
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="256")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        env["MASTER_PORT"] = str(s.getsockname()[1])
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "lam_ad_worker.py"), str(rank), str(nproc), outdir], env=env)
             for rank in range(nproc)]
    codes = [p.wait(timeout=600) for p in procs]
    assert codes == [0] * nproc, codes
    return [np.load(os.path.join(outdir, "lamad_%d_of_%d.npz" % (rank, nproc))) for rank in range(nproc)]


@pytest.fixture(scope="module")
def one_task(tmp_path_factory):
    return _run_workers(1, str(tmp_path_factory.mktemp("lamad1")))[0]


@pytest.mark.parametrize("nproc", [2, 3])
def test_tasks_assemble_to_the_one_task_result(nproc, one_task, tmp_path):
    """2 and 3 tasks over gloo on a 60 x 50 grid (wind, scalars, all flags, both adjoints): the per-task pieces, assembled, are
    byte-identical to the one-task result; the task that owns m = 0 writes the means and the others leave them alone"""
    from tests.lam_ad_worker import M, N, NDLON
    one, parts = one_task, _run_workers(nproc, str(tmp_path))
    kn, procm = ellips(M, N), zigzag(M, nproc)
    nesm0_one = np.concatenate([[0], np.cumsum(4 * (kn + 1))[:-1]])
    grid = np.zeros_like(one["grid"])
    spec = {k: np.zeros_like(one[k]) for k in ("vor", "div", "sc")}
    mean = None
    for w, p in enumerate(parts):
        myms = np.flatnonzero(procm == w)
        assert np.array_equal(p["myms"], myms)
        grid[:, p["rows"][0] * NDLON:p["rows"][1] * NDLON] = p["grid"]
        pos = 0
        for m in myms:
            n4 = 4 * (kn[m] + 1)
            for k in spec:
                spec[k][nesm0_one[m]:nesm0_one[m] + n4] = p[k][pos:pos + n4]
            pos += n4
        if 0 in myms:
            mean = p["mean"]
    assert grid.tobytes() == one["grid"].tobytes()
    for k in spec:
        assert spec[k].tobytes() == one[k].tobytes(), k
    assert mean.tobytes() == one["mean"].tobytes()
