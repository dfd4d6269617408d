"""ESPECNORM, EGPNORM_TRANS, EDIST_SPEC, EGATH_SPEC, EDIST_GRID and EGATH_GRID on the GPU: the HIP path through the C-ABI against the
NumPy restatements of tests/lam_norm_ref.py, with the cases and the derived bounds of the emulator tier (tests/lam_norms_common.py,
tests/test_lam_norms_emu.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests.lam_norms_common import (HANDLES, NFLDS, check_decomposition_invariance, egpnorm_cases, especnorm_case, independence_case,
                                     placement_case, run_workers, setup)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def et():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ectrans_amd
    ectrans_amd.lib()  # fails loudly if the HIP library is missing
    ectrans_amd.setup_trans0(kmax_resol=4, device=0)
    yield ectrans_amd
    ectrans_amd.trans_end()


def mover(memory):
    """(to, back) for the arrays of a call in `memory`; the dtype is the array's own"""
    if memory == "host":
        return (lambda a: np.ascontiguousarray(a)), (lambda a: np.asarray(a))
    import torch
    return (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")), (lambda t: t.cpu().numpy())


@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("memory", ["device", "host"])
@pytest.mark.parametrize("handle", HANDLES, ids=lambda h: "%dx%d_%dx%d" % h)
def test_especnorm_matches_the_model(et, handle, memory, precision):
    """norms and per-wavenumber sums, with and without PMET, 1 / 63 / 64 / 65 / 130 fields"""
    to, _ = mover(memory)
    r, ref = setup(et, handle, precision)
    try:
        for nf in NFLDS:
            for with_met in (False, True):
                err, bound, worst = especnorm_case(et, r, ref, nf, precision, with_met, to_dev=to)
                print(handle, memory, precision, nf, with_met, "norm %.2e (bound %.2e), per-m sums %.2f of their bounds" % (err, bound, worst))
                assert err <= bound and worst <= 1.0, (nf, with_met, err, bound, worst)
    finally:
        et.trans_release(r)


@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("handle,nf", [((400, 300, 199, 149), 65), ((1536, 1440, 767, 719), 32)], ids=["400x300", "1536x1440"])
def test_especnorm_larger_handles(et, handle, nf, precision):
    """workgroups of every tile shape at sizes a forecast uses: 65 fields (a full tile and one lane) and 32 (half a tile), device arrays"""
    to, _ = mover("device")
    r, ref = setup(et, handle, precision)
    try:
        for with_met in (False, True):
            err, bound, worst = especnorm_case(et, r, ref, nf, precision, with_met, to_dev=to)
            print(handle, precision, nf, with_met, "norm %.2e (bound %.2e), per-m sums %.2f of their bounds" % (err, bound, worst))
            assert err <= bound and worst <= 1.0, (with_met, err, bound, worst)
    finally:
        et.trans_release(r)


@pytest.mark.parametrize("precision", [8, 4])
def test_especnorm_does_not_depend_on_the_other_fields(et, precision):
    to, _ = mover("device")
    r, ref = setup(et, (60, 50, 19, 16), precision)
    try:
        independence_case(et, r, ref, precision, to_dev=to)
    finally:
        et.trans_release(r)


@pytest.mark.parametrize("precision", [8, 4])
def test_especnorm_of_a_placed_input(et, precision):
    to, back = mover("device")
    r, ref = setup(et, (24, 20, 7, 6), precision)
    try:
        placement_case(et, r, ref, precision, to_dev=to, to_host=back)
    finally:
        et.trans_release(r)


def test_especnorm_waits_for_the_transform_before_it(et):
    """ESPECNORM has no stream argument: it runs on the null stream behind the last transform of the handle, here an EDIR_TRANS queued
    on a non-blocking stream whose output it reads (the spherical counterpart: tests/test_gpu_parity.py,
    test_calls_on_different_streams_are_serialised)"""
    import torch
    r, ref = setup(et, (400, 300, 199, 149), 8)
    try:
        nf = 65
        rng = np.random.default_rng(3)
        gp = torch.from_numpy(rng.uniform(-1.0, 1.0, (1, nf, ref.ngptot))).to("cuda:0")
        sa0 = torch.zeros((ref.nspec2, nf), dtype=torch.float64, device="cuda:0")
        et.edir_trans(r, pspscalar=sa0, pgp=gp)
        torch.cuda.synchronize()
        n0 = et.especnorm(r, sa0)
        assert np.all(n0 > 0.0)
        sa = torch.zeros_like(sa0)
        s1 = torch.cuda.Stream(device="cuda:0")
        torch.cuda.synchronize()
        for _ in range(3):
            et.edir_trans(r, pspscalar=sa0, pgp=gp, stream=s1.cuda_stream)
        et.edir_trans(r, pspscalar=sa, pgp=gp, stream=s1.cuda_stream)
        n1 = et.especnorm(r, sa)  # null stream, right behind the direct transform on s1
        torch.cuda.synchronize()
        assert np.abs(n1 / n0 - 1.0).max() < 1e-10, (n0, n1)
    finally:
        et.trans_release(r)


@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("memory", ["device", "host"])
def test_egpnorm_matches_the_model(et, memory, precision):
    to, _ = mover(memory)
    err, bound = egpnorm_cases(et, precision, to_dev=to)
    print("EGPNORM_TRANS", memory, precision, "average %.2e (bound %.2e)" % (err, bound))
    assert err <= bound


def test_tasks_give_the_one_task_bytes(tmp_path):
    """tests/lam_norms_worker.py on 1, 2 and 3 tasks that share cuda:0 (the exchange hook and the host collectives over gloo, as
    tests/test_gpu_shims.py::test_multi_rank_path_on_one_gpu): at most three processes at a time"""
    check_decomposition_invariance({n: run_workers(n, str(tmp_path), where="cuda", timeout=300) for n in (1, 2, 3)})


def test_fortran_shim_lam_norms():
    """tests/fortran/test_shim_lam_norms.F90 on the real library, and one refusal that must abort with the ABORT_TRANS text"""
    d = os.path.join(ROOT, "ectrans_amd", "fortran")
    subprocess.check_call(["make", "-s", "-C", d, "test_shim_lam_norms"])
    exe = os.path.join(d, "test_shim_lam_norms")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "FORTRAN SHIM LAM NORMS OK (dp and sp)" in p.stdout, p.stdout + p.stderr
    p = subprocess.run([exe, "pmet"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "NOT REFUSED" not in p.stdout, p.stdout + p.stderr
    assert "ABORT_TRANS CALLED" in p.stderr and "ESPECNORM: PMET TOO SMALL" in p.stderr, p.stderr
