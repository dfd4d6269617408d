"""INV_TRANS(LDLATLON) on regular lat-lon grids on the GPU: the HIP path through the C-ABI against the direct summation of
tests/lonlat_ref.py (pinned to the oracle in tests/test_lonlat_emu.py, at T255 too).  Bounds as tests/test_gpu_parity.py: 1e-11 of the
field maximum in fp64, 3e-5 in fp32.  Left out: the two pole rows of the unshifted grid, in the fields that carry 1 / cos(lat)."""
import numpy as np
import pytest

from tests.lonlat_ref import lonlat_case

pytestmark = pytest.mark.gpu
TOL = {8: 1e-11, 4: 3e-5}


@pytest.fixture(scope="module")
def et():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ectrans_amd
    ectrans_amd.lib()  # fails loudly if the HIP library is missing
    ectrans_amd.setup_trans0(kmax_resol=4, device=0)
    yield ectrans_amd
    ectrans_amd.trans_end()


def mover(memory, precision):
    """(to, back) for arrays of the call in `memory`"""
    dt = np.float32 if precision == 4 else np.float64
    if memory == "host":
        return (lambda a: np.ascontiguousarray(a, dtype=dt)), (lambda a: np.asarray(a, dtype=np.float64))
    import torch
    return (lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda:0")), (lambda t: t.cpu().numpy().astype(np.float64))


GRIDS = {
    "t255_361x720": (255, 361, 720),          # 0.5 degrees with poles and equator
    "t255_360x720_shifted": (255, 360, 720),
    "t255_37x3600": (255, 37, 3600),          # the long-row FFT kernels; few latitudes keep the reference cheap
}


@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("memory", ["device", "host"])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_latlon_inverse_matches_series(et, grid, memory, precision):
    nsmax, nlat, nlon = GRIDS[grid]
    to, back = mover(memory, precision)
    errs, _ = lonlat_case(et, nsmax, nlat, nlon, precision=precision, to=to, back=back)
    assert max(errs.values()) < TOL[precision], errs
    if precision == 4:
        assert max(errs.values()) > 1e-9  # really computed in float


def test_latlon_inverse_with_nproma_blocks_and_belousov_panels(et):
    """KPROMA blocks that cut the rows, and LDUSERPNM=.TRUE. (the panels of the lat-lon rows from Belousov's recurrence on the host)"""
    to, back = mover("device", 8)
    errs, g = lonlat_case(et, 255, 361, 720, nproma=1000, to=to, back=back)
    assert max(errs.values()) < TOL[8], errs
    rows = g.reshape(g.shape[0], 362, 720)
    assert np.array_equal(rows[:, 180], rows[:, 181])  # the equator, held twice
    errs, _ = lonlat_case(et, 255, 361, 720, to=to, back=back, setup_kw=dict(lduserpnm=True))
    assert max(errs.values()) < TOL[8], errs


def test_latlon_handle_leaks_no_device_memory_and_holds_one_panel_set(et):
    """Free device memory over SETUP_TRANS(LDLL) / INV_TRANS(LDLATLON) / TRANS_RELEASE cycles, measured as
    test_no_device_memory_leak_over_setup_release_cycles of tests/test_gpu_parity.py measures it; and what a T255 361 x 720 handle
    holds against a full Gaussian handle with the same rows per hemisphere (362 x 720), which carries the transposed panels of the
    direct transform beside the inverse ones: about half."""
    import torch
    to, back = mover("device", 8)
    rng = np.random.default_rng(0)

    def free():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info()[0]

    def cycle(nf, shifted):
        r = et.setup_trans(63, 90, kdlon=180, ldll=True, ldshiftll=shifted)
        ns2, ng = et.trans_inq(r, "nspec2"), et.trans_inq(r, "ngptot")
        sp = rng.uniform(-1, 1, (ns2, nf))
        gp = np.zeros((1, nf, ng))
        et.inv_trans(r, pspscalar=sp, pgp=gp, ldlatlon=True)  # host arrays
        tsp, tgp = to(sp), to(gp)
        et.inv_trans(r, pspscalar=tsp, pgp=tgp, ldlatlon=True)  # device arrays
        torch.cuda.synchronize()
        et.trans_release(r)
        del tsp, tgp
        return free()

    levels = [cycle(70 if i % 2 else 7, bool(i % 3 == 0)) for i in range(16)]
    assert max(levels[8:]) - min(levels[8:]) == 0 and levels[0] - levels[-1] <= 64 << 20, levels

    f0 = free()
    r = et.setup_trans(255, 360, kdlon=720, ldll=True)
    held_ll = f0 - free()
    et.trans_release(r)
    f0 = free()
    r = et.setup_trans(255, 362, np.full(362, 720, dtype=np.int32))
    held_g = f0 - free()
    et.trans_release(r)
    print("device memory of a T255 handle: lat-lon 361x720 %.1f MiB, Gaussian 362x720 %.1f MiB" % (held_ll / 2**20, held_g / 2**20))
    assert 0 < held_ll < 0.7 * held_g, (held_ll, held_g)
