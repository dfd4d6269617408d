"""One task of the several-task test of the limited-area adjoints (launched by tests/test_lam_ad_emu.py: argv = rank, tasks, output
directory): W-sets on the CPU functional emulator with the all-to-all-v over gloo.  Every task runs EINV_TRANSAD (all flags) on its rows
of the same global white grid fields and EDIR_TRANSAD on its wavenumbers of the same global spectra, and saves its pieces; the launching
test assembles them and compares with what one task saved."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch.distributed as dist  # noqa: E402

import ectrans_amd as et  # noqa: E402
from tests.lam_ad_common import ALL, grid_groups  # noqa: E402
from tests.lam_ad_ref import LamAdRef  # noqa: E402
from tests.lam_common import units  # noqa: E402

NDLON, NDGL, M, N, NUV, NSC = 60, 50, 19, 16, 2, 3


def main():
    rank, world, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    et._use_library_for_tests(os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so"))
    et.setup_trans0(kmax_resol=2, kprtrw=world, myproc=rank + 1, device=None)
    exwn, eywn = units(NDLON, NDGL)
    r = et.esetup_trans(M, N, NDGL, kdlon=NDLON, pexwn=exwn, peywn=eywn)
    q = lambda n: et.etrans_inq(r, n)
    one = LamAdRef(NDLON, NDGL, M, N, exwn, eywn)
    myms = q("myms")
    idx = np.concatenate([np.arange(one.nesm0[m] - 1, one.nesm0[m] - 1 + 4 * (one.kntmp[m] + 1)) for m in myms])
    lat0, lat1 = q("nfrstlat") - 1, q("nlstlat")
    rows = slice(lat0 * NDLON, lat1 * NDLON)
    # ---- EINV_TRANSAD: this task's rows in, this task's wavenumbers out; the task that owns m = 0 writes the means
    nf = sum(c for _, c in grid_groups(NUV, NSC, ALL))
    gw = np.random.default_rng(41).uniform(-1.0, 1.0, (nf, NDLON * NDGL))
    nan = lambda *sh: np.full(sh, np.nan)
    vor, div, sc, mean = nan(len(idx), NUV), nan(len(idx), NUV), nan(len(idx), NSC), np.full((2, NUV), -5.0)
    et.einv_transad(r, pspvor=vor, pspdiv=div, pspscalar=sc, pmeanu=mean[0], pmeanv=mean[1], pgp=np.ascontiguousarray(gw[None, :, rows]),
                    ldscders=True, ldvorgp=True, lddivgp=True, lduvder=True)
    assert not np.isnan(vor).any() and not np.isnan(div).any() and not np.isnan(sc).any()
    if 0 not in myms:
        assert np.all(mean == -5.0)
    # against the global model, and the structural zeros
    want = one.inv_transad(gw.reshape(-1, NDGL, NDLON), nuv=NUV, nsc=NSC, **ALL)
    for got, w in ((vor, want[0]), (div, want[1]), (sc, want[2])):
        e = np.abs(got - w[idx]).max(axis=0) / np.abs(w).max(axis=0)
        assert e.max() < 1e-11, e
        glob = np.zeros_like(w)
        glob[idx] = got
        assert np.array_equal(one.clean(glob), glob)
    if 0 in myms:
        assert max(np.abs(mean[0] - want[3]).max(), np.abs(mean[1] - want[4]).max()) < 1e-11 * one.wind_max
    # ---- EDIR_TRANSAD: this task's wavenumbers in (every task holds the means; the owner of m = 0 reads them), this task's rows out
    rng = np.random.default_rng(42)
    sv, sd, ss = rng.uniform(-0.5, 0.5, (one.nspec2, NUV)), rng.uniform(-0.5, 0.5, (one.nspec2, NUV)), rng.uniform(-0.5, 0.5, (one.nspec2, NSC))
    mu, mv = np.array([2.5, -1.0]), np.array([0.5, 1.5])
    loc = lambda a: np.ascontiguousarray(a[idx])
    gp = nan(1, 2 * NUV + NSC, q("ngptot"))
    et.edir_transad(r, pspvor=loc(sv), pspdiv=loc(sd), pspscalar=loc(ss), pmeanu=mu, pmeanv=mv, pgp=gp)
    wg = one.dir_transad(sv, sd, ss, mu, mv).reshape(2 * NUV + NSC, -1)
    e = np.abs(gp[0] - wg[:, rows]).max(axis=1) / np.abs(wg).max(axis=1)
    assert e.max() < 1e-11, e
    np.savez(os.path.join(outdir, "lamad_%d_of_%d.npz" % (rank, world)), grid=gp[0], vor=vor, div=div, sc=sc, mean=mean, myms=myms,
             rows=np.array([lat0, lat1]))
    et.trans_end()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    print("LAM AD DIST OK rank %d of %d" % (rank, world), flush=True)


if __name__ == "__main__":
    main()
