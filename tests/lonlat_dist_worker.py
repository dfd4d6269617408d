"""One task of the two-task lat-lon test (launched by tests/test_lonlat_emu.py): W-sets 1 and 2 on the CPU functional emulator with
the all-to-all-v over gloo.  Every task runs INV_TRANS(LDLATLON) on its latitude band, GATH_GRID collects the fields on task 1, which
compares them with the one-task fields the launching test computed (EMI_TEST_REF) and with the series of tests/lonlat_ref.py."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch.distributed as dist  # noqa: E402

import ectrans_amd as et  # noqa: E402
from tests.common import rel_err  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    shifted = bool(int(os.environ.get("EMI_TEST_SHIFTED", "0")))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    et._use_library_for_tests(os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so"))
    et.setup_trans0(kmax_resol=2, kprtrw=world, myproc=rank + 1, device=None)
    ref = np.load(os.environ["EMI_TEST_REF"])  # one task: nsmax, nlat, nlon, the spectral inputs and the fields [fld][point]
    nsmax, nlat, nlon = (int(x) for x in ref["dims"])
    vor, div, sc, gone = ref["vor"], ref["div"], ref["sc"], ref["grid"]
    nasm0g = np.concatenate([[0], np.cumsum([2 * (nsmax - m + 1) for m in range(nsmax + 1)])])
    got = {}
    for userpnm in (False, True):
        r = et.setup_trans(nsmax, nlat if shifted else nlat - 1, kdlon=nlon, ldll=True, ldshiftll=shifted, lduserpnm=userpnm)
        myms = et.trans_inq(r, "myms")
        gidx = np.concatenate([np.arange(nasm0g[m], nasm0g[m] + 2 * (nsmax - m + 1)) for m in myms])
        ng, ndgl = et.trans_inq(r, "ngptot"), et.trans_inq(r, "ndgl")
        lat0, lat1 = et.trans_inq(r, "nfrstlat") - 1, et.trans_inq(r, "nlstlat")
        assert ng == (lat1 - lat0) * nlon and et.trans_inq(r, "ngptotg") == ndgl * nlon == gone.shape[1]
        loc = lambda a: np.ascontiguousarray(a[gidx])
        gp = np.zeros((1, gone.shape[0], ng))
        et.inv_trans(r, pspvor=loc(vor), pspdiv=loc(div), pspscalar=loc(sc), pgp=gp, ldlatlon=True, ldscders=True, ldvorgp=True, lddivgp=True,
                     lduvder=True)
        e_norm = np.abs(et.specnorm(r, loc(sc)) - ref["norms"]).max()
        assert e_norm < 1e-13, e_norm
        got[userpnm] = et.gath_grid(r, gp, gone.shape[0], kto=1)
        et.trans_release(r)
    if rank == 0:
        g = got[False]
        same = np.array_equal(g, gone)
        e = rel_err(g, gone, axis=1)
        print("two tasks vs one task: byte-identical %s, max error %.2e" % (same, e), flush=True)
        assert e < 1e-12, e
        # both generators: all rows of vor, div and the scalars; u, v and the derivatives off the pole rows (1 / cos there is 1 / 2e-13)
        inner = slice(None) if shifted else slice(nlon, -nlon)
        plain = [0, 1, 4, 5]
        rest = [f for f in range(g.shape[0]) if f not in plain]
        e_gen = max(rel_err(got[True][plain], g[plain], axis=1), rel_err(got[True][rest][:, inner], g[rest][:, inner], axis=1))
        print("Belousov vs recurrence: %.2e" % e_gen, flush=True)
        assert e_gen < 1e-11, e_gen
    else:
        assert got[False] is None and got[True] is None
    et.trans_end()
    dist.barrier()
    dist.destroy_process_group()
    print("LONLAT DIST OK rank %d" % rank, flush=True)


if __name__ == "__main__":
    main()
