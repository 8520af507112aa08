"""The host half of the direct Cholesky tests (tests/chol_reference.py; the device half is tests/test_gpu_chol.py), no GPU needed:
the generator and the reference stay inside the bars on their own, every crafted pattern gives the structure it was crafted for
under default switches (lsfm_symbolic_analyse), and the bars tell a slightly wrong factor from a right one."""
import numpy as np
import pytest

import chol_reference as cr
from linearsfm_amd import api

VARIANTS = [(name, False) for name in cr.CASES] + [(name, True) for name, c in cr.CASES.items() if c.fixed_pose]


def test_entry_is_exported():
    assert "lsfm_selftest_chol" in api.EXPORTS
    assert hasattr(api.Context, "selftest_chol")


@pytest.mark.parametrize("name,with_fixed", VARIANTS)
def test_lapack_cholesky_is_within_5e15_of_the_reference(name, with_fixed):
    pb = cr.problem(name, with_fixed)
    w = np.linalg.eigvalsh(pb.A0)
    print(f"{name} fixed={with_fixed}: kappa(A0) {w[-1] / w[0]:.2f}, corrections {pb.corrections}, LAPACK fp64 {pb.lapack_e}, "
          f"its factor in fp32 {pb.lapack_e32}")
    # the refinement has converged far below double precision: the reference's own error is nothing beside the bars
    assert pb.corrections[1] <= 1e-17 and pb.corrections[2] <= 1e-17
    assert np.all(pb.lapack_e <= cr.LAPACK_BAR)
    # what the fp64 bar's kappa <= 13 stands on (1.6 from 40 poses on; the tiny dense cases reach 2.1, where 3 n u is tiny)
    assert w[-1] / w[0] <= (1.7 if pb.m >= 40 else 2.2)
    assert np.all(pb.lapack_e32 > 1e-9) and np.all(pb.lapack_e32 < 1e-6)
    if with_fixed:
        assert pb.fixed.sum() == 7 and np.all(pb.z_ref[:, pb.fixed != 0] == 0.0)
    # the scales really are spread out: the power-of-four scaling has work to do
    assert np.diag(pb.S).max() / np.diag(pb.S).min() > (1e6 if pb.m > 1 else 1e2)


@pytest.mark.parametrize("name", [n for n, c in cr.CASES.items() if c.symbolic_checked])
def test_pattern_gives_the_structure_it_was_made_for(name):
    case = cr.CASES[name]
    rowptr, colidx = case.pattern
    r = api.symbolic_analyse(rowptr, colidx, case.origin)
    info = r["info"]
    got = dict(leaf_tasks=int(info[4]), groups=int(info[2]), group_levels=int(info[3]), max_rows_below=int((np.diff(r["colptr"]) - 1).max()))
    print(name, got)
    for k in ("leaf_tasks", "groups", "group_levels", "max_rows_below"):
        if k in case.expect:
            assert got[k] == case.expect[k], (k, got)
    if case.expect.get("split"):
        assert got["max_rows_below"] > cr.SN_FUSE_MAX
    if name == "dense20":
        # a chain of two groups, the last one narrower than CHOL_GS: 20 = (columns of the leaf task) + 8 + fewer than 8
        colptr = r["colptr"]
        assert int(info[5]) > cr.CHOL_GS and int(info[5]) < 2 * cr.CHOL_GS and np.all(np.diff(colptr) == np.arange(20, 0, -1))


@pytest.mark.parametrize("name,with_fixed", VARIANTS)
def test_checks_pass_a_right_factor(name, with_fixed):
    """LAPACK's factor of the scaled matrix, laid out as the device returns its own, goes through every check the device's does"""
    pb = cr.problem(name, with_fixed)
    res = cr.host_result(pb)
    llt, bar, dinv = cr.check_factor(pb, res)
    e, _ = cr.check_solves(pb, res, fp32=False)
    cr.check_dot(pb, res, pb.case.nseg)
    print(f"{name} fixed={with_fixed}: max|L L^T - S^| {llt:.2e} (bar {bar:.2e}), Dinv {dinv:.2e}, e {e}")


@pytest.mark.parametrize("name", [n for n in cr.CASES if n != "dense1"])
def test_bars_refuse_a_slightly_wrong_factor(name):
    """One off-diagonal block of LAPACK's factor (the largest) times 1 + 1e-6: e lands above 100 x the fp64 bar, the factor check fails"""
    pb = cr.problem(name)
    good = cr.host_result(pb)
    nb = np.linalg.norm(good["L"].reshape(-1, 36), axis=1)
    nb[good["colptr"][:-1]] = 0.0
    blk = int(np.argmax(nb))
    j = int(np.searchsorted(good["colptr"], blk, side="right") - 1)
    i = int(good["rowidx"][blk])
    bad = cr.host_result(pb, (i, j, 1 + 1e-6))
    e = pb.error(bad["z"])
    print(f"{name}: block ({i}, {j}) of the factor off by 1e-6 relative: e {e}")
    assert np.all(e > 100 * cr.FP64_BAR)
    with pytest.raises(AssertionError):
        cr.check_solves(pb, bad, fp32=False)
    with pytest.raises(AssertionError):
        cr.check_factor(pb, bad)


def test_entry_checks_its_arguments_before_it_touches_a_device():
    """No context: LSFM_ERR_ARG (-1) after the argument checks -- the binding's argument list fits the library's"""
    import ctypes as C
    pb = cr.problem("dense2")
    m, n = pb.m, 6 * pb.m
    z, dot, info = np.zeros(cr.NRHS * n), np.zeros(cr.NRHS), np.full(16, 7, np.int32)
    seg = np.zeros(m, np.int32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    val, r = np.ascontiguousarray(pb.val).reshape(-1), np.ascontiguousarray(pb.r).reshape(-1)

    def call(colidx, mode):
        return api.lib().lsfm_selftest_chol(None, m, p(pb.rowptr, C.c_int), p(colidx, C.c_int), p(val, C.c_double), None, None, p(seg, C.c_int), 1,
                                            p(r, C.c_double), cr.NRHS, mode, p(z, C.c_double), p(dot, C.c_double), None, None, None, None, None, None, 0,
                                            p(info, C.c_int))
    assert call(pb.colidx[::-1].copy(), 0) == -1 and np.all(info == 7)   # refused before anything is written
    assert call(pb.colidx, 4) == -1 and np.all(info == 7)
    assert call(pb.colidx, 0) == -1 and np.all(info == 0)                 # well-formed: refused for the missing context only
