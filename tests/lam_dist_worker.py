"""One task of the several-task limited-area test (launched by tests/test_lam_emu.py: argv = rank, tasks, output directory): W-sets on
the CPU functional emulator with the all-to-all-v over gloo.  Every task runs EINV_TRANS and EDIR_TRANS on its share of a 60 x 50
grid -- wind with means, scalars, every derivative -- and saves its pieces and its inquiry arrays; the launching test assembles them
and compares with what one task saved."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch.distributed as dist  # noqa: E402

import ectrans_amd as et  # noqa: E402
from tests.lam_common import units  # noqa: E402
from tests.lam_ref import LamRef  # noqa: E402

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
    # the global inputs, the same on every task: spectra in the one-task layout, grid fields from the model
    one = LamRef(NDLON, NDGL, M, N, exwn, eywn)
    rng = np.random.default_rng(21)
    vor, div, sc = one.random_spec(rng, NUV), one.random_spec(rng, NUV), one.random_spec(rng, NSC)
    mu, mv = np.array([2.5, -1.0]), np.array([0.5, 1.5])
    gin = one.inv_trans(vor, div, sc, mu, mv).reshape(2 * NUV + NSC, -1)
    # this task's share
    myms, nesm0 = q("myms"), q("nesm0")
    idx = np.concatenate([np.arange(one.nesm0[m] - 1, one.nesm0[m] - 1 + 4 * (one.kntmp[m] + 1)) for m in myms])
    assert len(idx) == q("nspec2") and all(nesm0[m] > 0 for m in myms)
    lat0, lat1 = q("nfrstlat") - 1, q("nlstlat")
    ng = q("ngptot")
    assert ng == (lat1 - lat0) * NDLON and q("ngptotg") == NDLON * NDGL
    loc = lambda a: np.ascontiguousarray(a[idx])
    nf = 6 * NUV + 3 * NSC
    gp = np.zeros((1, nf, ng))
    et.einv_trans(r, pspvor=loc(vor), pspdiv=loc(div), pspscalar=loc(sc), pmeanu=mu, pmeanv=mv, pgp=gp, ldscders=True, ldvorgp=True,
                  lddivgp=True, lduvder=True)
    v2, d2, s2 = np.zeros((len(idx), NUV)), np.zeros((len(idx), NUV)), np.zeros((len(idx), NSC))
    mean = np.full((2, NUV), -5.0)
    et.edir_trans(r, pspvor=v2, pspdiv=d2, pspscalar=s2, pmeanu=mean[0], pmeanv=mean[1],
                  pgp=np.ascontiguousarray(gin[None, :, lat0 * NDLON:lat1 * NDLON]))
    if 0 not in myms:
        assert np.all(mean == -5.0)  # the task that owns m = 0 writes the means
    # the same leg on full-bandwidth input: the same global white fields on every task, this task's rows in, this task's wavenumbers against
    # the global model (the emulator tier's bound, tests/test_lam_emu.py); energy above M in every row and outside the ellipse
    gw = np.random.default_rng(22).uniform(-1.0, 1.0, gin.shape)
    wv, wd, ws, wmu, wmv = one.dir_trans(gw.reshape(-1, NDGL, NDLON), nuv=NUV, nsc=NSC)
    v3, d3, s3 = np.zeros((len(idx), NUV)), np.zeros((len(idx), NUV)), np.zeros((len(idx), NSC))
    mean3 = np.full((2, NUV), -5.0)
    et.edir_trans(r, pspvor=v3, pspdiv=d3, pspscalar=s3, pmeanu=mean3[0], pmeanv=mean3[1],
                  pgp=np.ascontiguousarray(gw[None, :, lat0 * NDLON:lat1 * NDLON]))
    for got, want in ((v3, wv), (d3, wd), (s3, ws)):
        e = np.abs(got - want[idx]).max(axis=0) / np.abs(want).max(axis=0)
        assert e.max() < 1e-12, e
        glob = np.zeros_like(want)
        glob[idx] = got
        assert np.array_equal(one.clean(glob), glob)  # the structural zeros
    if 0 in myms:
        assert max(np.abs(mean3[0] - wmu).max(), np.abs(mean3[1] - wmv).max()) < 1e-12
    else:
        assert np.all(mean3 == -5.0)
    np.savez(os.path.join(outdir, "lam_%d_of_%d.npz" % (rank, world)), grid=gp[0], vor=v2, div=d2, sc=s2, mean=mean,
             **{n: q(n) for n in ("myms", "procm", "latlo", "ndim0g", "nump", "numpp", "nptrms", "nallms", "npossp", "nspec2", "nspec2mx",
                                  "nesm0", "ngptot", "nfrstlat", "nlstlat")})
    et.trans_end()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    print("LAM DIST OK rank %d of %d" % (rank, world), flush=True)


if __name__ == "__main__":
    main()
