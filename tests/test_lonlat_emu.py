"""INV_TRANS(LDLATLON) on a handle set up with LDLL -- regular latitude-longitude grids -- on the CPU functional emulator (tests/emu):
the same host logic and kernels as the GPU tier (tests/test_lonlat_gpu.py), against the direct summation of tests/lonlat_ref.py.
The frozen oracle has no lat-lon path, so the summation is first pinned to the oracle on full Gaussian grids."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.common import random_spectrum, rel_err
from tests.lonlat_ref import SeriesRef, field_groups, lonlat_case, lonlat_rows, spectra, wind_spectrum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12  # fp64, of the field maximum (the emulator tier's bound, tests/test_emu_parity.py)
FLAGS = dict(scders=True, vorgp=True, divgp=True, uvder=True)


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


# ---- 1. the helper, pinned to the oracle on full Gaussian grids ------------------------------------------------------------------
@pytest.mark.parametrize("nsmax,ndgl,nlon", [(21, 32, 64), (63, 96, 192), (255, 384, 768), (255, 384, 400)])
def test_series_helper_matches_oracle_on_gaussian_grids(nsmax, ndgl, nlon):
    """scalars, u, v, E-W and N-S derivatives, grid vorticity and divergence; 1e-12 of the field maximum (measured: 5e-15 at T21,
    2e-14 at T63, 1.1e-13 and 2.8e-13 at T255 -- the T255 grids pin the helper at the size of the GPU tier)"""
    nloen = np.full(ndgl, nlon, dtype=np.int32)
    o = Oracle(nsmax, nloen, lazy=nsmax > 100)
    rng = np.random.default_rng(5)
    vor = wind_spectrum(rng, o.nasm0, nsmax, o.nspec2, 1)
    div = wind_spectrum(rng, o.nasm0, nsmax, o.nspec2, 1)
    sc = random_spectrum(rng, o.nasm0, nsmax, o.nspec2, 2, False)
    u, v = o.vordiv_to_uv(vor, div)
    gref = o.inv_trans(spvor=vor, spdiv=div, spsc=sc, **FLAGS)
    ref = SeriesRef(nsmax, o.nasm0, o.rmu, nlon)
    g = ref.inv_trans(spvor=vor, spdiv=div, spsc=sc, spu=u, spv=v, **FLAGS)
    assert g.shape == gref.shape
    for nm, f0, cnt, acos in field_groups(1, 2):
        a, b = g[f0:f0 + cnt].reshape(cnt, ndgl, nlon), gref[f0:f0 + cnt].reshape(cnt, ndgl, nlon)
        e = rel_err(a.reshape(cnt, -1), b.reshape(cnt, -1), axis=1)
        print("helper vs oracle T%d %dx%d %-9s %.2e" % (nsmax, ndgl, nlon, nm, e))
        if nsmax == 255 and acos:
            # The oracle's polynomials are the reference's SUPOLF: undoing its 1e+-100 rescaling floors values below 2.2e-16 to 2.2e-16, so
            # next to the poles its panels hold 2.2e-16 for high m where the function is 1e-110 (the helper has 0).  A full Gaussian grid
            # reads those entries, and u, v and the derivatives multiply them by 1 / cos(lat) = 160 on the first row of 384: measured there
            # 4.7e-13 (u), 2.6e-12 (v) of the field maximum, 5.3e-13 and less from the second row on.  That is the oracle's error, not the
            # helper's, so the first row at each pole is left out of these fields at this size (all rows of vor, div and the scalars stay).
            e = rel_err(a[:, 1:-1].reshape(cnt, -1), b[:, 1:-1].reshape(cnt, -1), axis=1)
            print("   without the first and the last row: %.2e" % e)
        assert e < 1e-12, (nm, e)
    if nsmax == 21:
        for m in (0, 1, 5, 21):
            pol = ref.legpol(m)
            for jgl in (1, 7, 16):
                assert np.abs(pol[:, jgl - 1] - o.legpol(m, jgl)).max() < 1e-12


# ---- 2. parity ------------------------------------------------------------------------------------------------------------------
LL_CASES = {
    "t21_33x64": (21, 33, 64, None),
    "t21_32x64_shifted": (21, 32, 64, None),
    "t31_45x90": (31, 45, 90, None),            # row length with an odd half: another FFT family
    "t31_46x90_shifted": (31, 46, 90, None),
    "t21_33x36_nmen17": (21, 33, 36, None),     # NMEN = 17 < NSMAX
    "t21_33x64_nproma": (21, 33, 64, 37),       # KPROMA blocks that cut rows
    "t21_32x64_shifted_nproma": (21, 32, 64, 50),
}


@pytest.mark.parametrize("name", sorted(LL_CASES))
def test_latlon_inverse_matches_series(et, name):
    nsmax, nlat, nlon, nproma = LL_CASES[name]
    errs, _ = lonlat_case(et, nsmax, nlat, nlon, nproma)
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("name", ["t21_33x64", "t21_32x64_shifted", "t31_45x90", "t21_33x36_nmen17"])
def test_latlon_inverse_fp32_library(et, name):
    nsmax, nlat, nlon, nproma = LL_CASES[name]
    errs, _ = lonlat_case(et, nsmax, nlat, nlon, nproma, precision=4)
    assert max(errs.values()) < 2e-5, errs
    assert max(errs.values()) > 1e-9  # really computed in float


@pytest.mark.parametrize("name", ["t21_33x64", "t21_32x64_shifted"])
def test_latlon_inverse_belousov_generator(et, name):
    """LDUSERPNM=.TRUE. (the Fortran API's default): the panels from Belousov's recurrence on the host"""
    nsmax, nlat, nlon, nproma = LL_CASES[name]
    errs, g = lonlat_case(et, nsmax, nlat, nlon, nproma, setup_kw=dict(lduserpnm=True))
    assert max(errs.values()) < TOL, errs
    _, g2 = lonlat_case(et, nsmax, nlat, nlon, nproma)
    inner = slice(None) if nlat % 2 == 0 else slice(nlon, -nlon)  # u, v: not the pole rows
    assert rel_err(g[[0, 1, 4, 5]], g2[[0, 1, 4, 5]], axis=1) < 1e-11 and rel_err(g[2:4, inner], g2[2:4, inner], axis=1) < 1e-11


# ---- 3. structure ---------------------------------------------------------------------------------------------------------------
def test_latlon_grid_structure(et):
    nsmax, nlat, nlon = 21, 33, 64
    _, g = lonlat_case(et, nsmax, nlat, nlon)
    ndgl = nlat + 1
    rows = g.reshape(g.shape[0], ndgl, nlon)
    assert np.array_equal(rows[:, ndgl // 2 - 1], rows[:, ndgl // 2])  # the equator, held twice, bit for bit
    for f in (0, 1, 4, 5):  # vor, div and the two scalars: one value on a pole row
        for j in (0, ndgl - 1):
            assert np.abs(rows[f, j] - rows[f, j, 0]).max() < 1e-12 * np.abs(rows[f]).max()


def test_latlon_handles_inquiry_and_coexistence(et):
    nloen = np.full(32, 64, dtype=np.int32)
    rg = et.setup_trans(21, 32, nloen)
    ru = et.setup_trans(21, 32, kdlon=64, ldll=True)
    rs = et.setup_trans(21, 32, kdlon=64, ldll=True, ldshiftll=True)
    try:
        assert len({rg, ru, rs}) == 3
        assert (et.trans_inq(rg, "ldll"), et.trans_inq(ru, "ldll"), et.trans_inq(rs, "ldll")) == (0, 1, 1)
        assert (et.trans_inq(rg, "lshiftll"), et.trans_inq(ru, "lshiftll"), et.trans_inq(rs, "lshiftll")) == (0, 0, 1)
        assert et.trans_inq(ru, "ndgl") == 34 and et.trans_inq(ru, "ngptot") == 34 * 64 == et.trans_inq(ru, "ngptotg")
        assert et.trans_inq(rs, "ndgl") == 32 and et.trans_inq(rs, "ngptot") == 32 * 64
        j = np.arange(1, 18)
        lat_u = np.deg2rad(90.0 - (j - 1) * 180.0 / 32)
        pmu = et.trans_inq(ru, "pmu")
        assert np.abs(pmu[:17] - np.sin(lat_u)).max() < 1e-15 and np.array_equal(pmu[17:], -pmu[:17][::-1])
        assert pmu[0] == 1.0 and pmu[16] == 0.0 and pmu[17] == 0.0
        j = np.arange(1, 33)
        assert np.abs(et.trans_inq(rs, "pmu") - np.sin(np.deg2rad(90.0 - (j - 0.5) * 180.0 / 32))).max() < 1e-15
        assert (et.trans_inq(ru, "nmen") == 21).all() and (et.trans_inq(ru, "ndglu") == 17).all()
        with pytest.raises(et.TransError, match="LDLL"):
            et.trans_inq(ru, "pgw")
        # the panels of the lat-lon rows: P_n^m(mu) of the series helper
        o = Oracle(21, nloen)
        ref = SeriesRef(21, o.nasm0, pmu[:17], 64, cth=lonlat_rows(33, False)[1][:17])
        for m in (0, 1, 2, 9, 21):
            pol = ref.legpol(m)  # [n - m][lat]
            for sym in (1, 0):
                pan = et.legendre_panel(ru, m, sym)  # [col: n descending][lat]
                ns = np.arange(m, 22)[(np.arange(m, 22) - m) % 2 == (0 if sym else 1)]
                assert pan.shape[1] == 17
                for c, n in enumerate(ns[::-1]):
                    assert np.abs(pan[pan.shape[0] - len(ns) + c] - pol[n - m]).max() < 1e-12, (m, sym, n)
        # the Gaussian handle beside them still transforms
        sc = random_spectrum(np.random.default_rng(1), o.nasm0, 21, o.nspec2, 1, False)
        gp = np.zeros((1, 1, o.ngptot))
        et.inv_trans(rg, pspscalar=sc, pgp=gp)
        assert rel_err(gp[0], o.inv_trans(spsc=sc), axis=1) < TOL
    finally:
        et.trans_release(ru)
        r2 = et.setup_trans(21, 32, kdlon=64, ldll=True)  # a released handle's number is used again
        assert r2 == ru
        for r in (rg, r2, rs):
            et.trans_release(r)


def test_latlon_setup_argument_checks(et):
    with pytest.raises(et.TransError, match="LDLL"):
        et.setup_trans(21, 32, np.array([64] * 16 + [60] * 16, dtype=np.int32), ldll=True)  # one row length only
    with pytest.raises(et.TransError, match="LDSHIFTLL"):
        et.setup_trans(21, 32, kdlon=64, ldshiftll=True)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["inv_trans_without_ldlatlon", "dir_trans", "inv_transad", "dir_transad", "gpnorm_trans", "cdio_legpol"])
def test_latlon_handle_refuses(et, what, tmp_path):
    if what == "cdio_legpol":
        with pytest.raises(et.TransError, match="LDLL"):
            et.setup_trans(21, 32, kdlon=64, ldll=True, cdio_legpol="writef", cdlegpolfname=str(tmp_path / "legpol"))
        return
    r = et.setup_trans(21, 32, kdlon=64, ldll=True)
    try:
        ns2, ng = et.trans_inq(r, "nspec2"), et.trans_inq(r, "ngptot")
        sc, gp = np.zeros((ns2, 1)), np.zeros((1, 1, ng))
        with pytest.raises(et.TransError, match="LDLL"):
            if what == "inv_trans_without_ldlatlon":
                et.inv_trans(r, pspscalar=sc, pgp=gp)
            elif what == "dir_trans":
                et.dir_trans(r, pspscalar=sc, pgp=gp)
            elif what == "inv_transad":
                et.inv_transad(r, pspscalar=sc, pgp=gp)
            elif what == "dir_transad":
                et.dir_transad(r, pspscalar=sc, pgp=gp)
            else:
                et.gpnorm_trans(r, gp)
        et.inv_trans(r, pspscalar=sc, pgp=gp, ldlatlon=True)  # the handle is intact
    finally:
        et.trans_release(r)


def test_ldlatlon_on_gaussian_handle_is_refused(et):
    r = et.setup_trans(21, 32, np.full(32, 64, dtype=np.int32))
    try:
        ns2, ng = et.trans_inq(r, "nspec2"), et.trans_inq(r, "ngptot")
        with pytest.raises(et.TransError, match="LDLATLON"):
            et.inv_trans(r, pspscalar=np.zeros((ns2, 1)), pgp=np.zeros((1, 1, ng)), ldlatlon=True)
    finally:
        et.trans_release(r)


# ---- 5. two tasks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifted", [0, 1])
def test_latlon_two_tasks_over_gloo(et, shifted, tmp_path):
    """W-sets 1 and 2 on the emulator with the exchange over gloo (tests/lonlat_dist_worker.py): the gathered lat-lon fields equal the
    fields of one task, computed here (byte-identical by design; asserted to 1e-12), and both generators of the polynomials agree"""
    nsmax, nlat, nlon = 21, 32 if shifted else 33, 64
    o, vor, div, sc, _, _ = spectra(nsmax)
    _, g = lonlat_case(et, nsmax, nlat, nlon)
    np.savez(tmp_path / "one_task.npz", dims=np.array([nsmax, nlat, nlon]), vor=vor, div=div, sc=sc, grid=g, norms=o.specnorm(sc))
    port = 29560 + shifted
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1024",
                   EMI_TEST_SHIFTED=str(shifted), EMI_TEST_REF=str(tmp_path / "one_task.npz"))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "lonlat_dist_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=900)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    print(outs[0])
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "LONLAT DIST OK rank %d" % rank in out, out
