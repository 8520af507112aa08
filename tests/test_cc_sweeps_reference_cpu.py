"""The host half of the direct tests of the side-by-side sweeps (tests/cc_sweeps_reference.py; the device half is
tests/test_gpu_cc_sweeps.py), no GPU needed: the reference and a numpy model of the side-by-side solve stay inside the bars on
their own, the bars tell a slightly wrong forward or backward half from a right one and from each other -- and the refinement of
the columns calls does NOT: behind it the same wrong sweep ends inside the columns tests' 1e-9, which is why those tests cannot see
the sweeps.  The printed figures (pytest -s) are the ones DESIGN.md, "Direct tests of the side-by-side sweeps", records."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cc_sweeps_reference as cs
import chol_reference as cr
from linearsfm_amd import api

MODEL_CASES = [("band40", False), ("dense20", False), ("five30", True)]
BAD = 1 + 1e-6


def test_entry_is_exported():
    assert "lsfm_selftest_cc_sweeps" in api.EXPORTS
    assert hasattr(api.Context, "selftest_cc_sweeps")


def test_entry_checks_its_arguments_before_it_touches_a_device():
    """No context: LSFM_ERR_ARG (-1) after the argument checks -- the binding's argument list fits the library's"""
    import ctypes as C
    sp = cs.sweep_problem("dense2")
    pb = sp.pb
    B = np.ascontiguousarray(sp.B[:, :6])
    val, info = np.ascontiguousarray(pb.val).reshape(-1), np.full(16, 7, np.int32)
    x, y = np.zeros_like(B), np.zeros_like(B)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None else None

    def call(colidx, R, X, yy):
        return api.lib().lsfm_selftest_cc_sweeps(None, pb.m, p(pb.rowptr, C.c_int), p(colidx, C.c_int), p(val, C.c_double), None, None, p(B, C.c_double), R,
                                                 p(X, C.c_double), p(x, C.c_double), None, None, None, p(yy, C.c_double), p(info, C.c_int))
    assert call(pb.colidx[::-1].copy(), 6, None, None) == -1 and np.all(info == 7)   # refused before anything is written
    assert call(pb.colidx, 0, None, None) == -1 and np.all(info == 7)
    assert call(pb.colidx, 193, None, None) == -1 and np.all(info == 7)
    assert call(pb.colidx, 6, B, None) == -1 and np.all(info == 7)                  # X without y
    assert call(pb.colidx, 6, None, y) == -1 and np.all(info == 7)                  # y without X
    assert call(pb.colidx, 6, B, y) == -1 and np.all(info == 0)                     # well-formed: refused for the missing context only


def test_dense270_is_inside_what_the_fp64_bar_assumes():
    """The FP64_BAR derivation assumes 6m <= 1800 and a Jacobi-scaled condition number of at most 1.7"""
    rowptr, colidx = cs.DENSE270.pattern
    _, _, A0, _ = cr.make_values(rowptr, colidx)
    w = np.linalg.eigvalsh(A0)
    print(f"dense270: 6m = {A0.shape[0]}, kappa(A0) {w[-1] / w[0]:.3f}")
    assert A0.shape[0] == 1620 <= 1800 and w[-1] / w[0] <= 1.7


def test_dense270_gives_the_structure_it_was_made_for():
    rowptr, colidx = cs.DENSE270.pattern
    r = api.symbolic_analyse(rowptr, colidx, None)
    info = r["info"]
    got = dict(leaf_tasks=int(info[4]), groups=int(info[2]), group_levels=int(info[3]))
    print("dense270", got)
    assert got == {k: cs.DENSE270.expect[k] for k in got}
    # a chain of groups on a full lower triangle: the first run is CHOL_GS wide and everything else lies below it
    assert np.all(np.diff(r["colptr"]) == np.arange(270, 0, -1))
    rows_below = 270 - cr.CHOL_GS
    assert rows_below == cs.DENSE270.expect["max_run_rows"] > 256 and (6 * rows_below + cs.CC_GK - 1) // cs.CC_GK == 33 > cs.CC_GY


@pytest.mark.parametrize("setting", list(cs.SWITCHES))
def test_switch_table_is_what_the_symbolic_analysis_gives(setting):
    """The switches are read once per process: the host analysis of the R_CASES in a child under each setting"""
    env_add, _, expect = cs.SWITCHES[setting]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, '.'); sys.path.insert(0, 'tests')\n"
            "import cc_sweeps_reference as cs\n"
            "from linearsfm_amd import api\n"
            "for name in cs.R_CASES:\n"
            "    info = api.symbolic_analyse(*cs.CASES[name].pattern, None)['info']\n"
            "    print('ANALYSED', name, int(info[4]), int(info[2]), int(info[3]))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, **env_add), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {ln.split()[1]: tuple(int(v) for v in ln.split()[2:]) for ln in r.stdout.splitlines() if ln.startswith("ANALYSED")}
    assert got == {name: (e["leaf_tasks"], e["groups"], e["group_levels"]) for name, e in expect.items()}


@pytest.mark.parametrize("name,with_fixed", MODEL_CASES)
def test_reference_and_host_model_are_inside_the_bars(name, with_fixed):
    sp = cs.sweep_problem(name, with_fixed)
    print(f"{name} fixed={with_fixed}: corrections {sp.corrections}, LAPACK fp64 worst column {np.max(sp.lapack_e):.2e}")
    assert np.all(sp.lapack_e <= cs.LAPACK_BAR)
    ds, L = cs.host_factor(sp)
    res = cs.host_sweeps(sp, cs.RMAX, ds, L)
    e = cs.check_solve(sp, res)
    ef = cs.check_forward(sp, res)
    # the forward reference itself: float64 against a long-double substitution with the same factor
    ref = cs.forward_reference(sp, res["perm"], ds)
    Ll, bl = L.astype(np.longdouble), (sp.B_in() * ds[:, None]).astype(np.longdouble)
    fl = np.zeros_like(bl)
    for i in range(sp.n):
        fl[i] = (bl[i] - Ll[i, :i] @ fl[:i]) / Ll[i, i]
    eref = np.asarray(np.max(np.abs(ref - fl), axis=0) / np.max(np.abs(fl), axis=0), np.float64)
    print(f"  host model: e {np.max(e):.2e}, forward {np.max(ef):.2e}; fwd_ref float64 against long double {np.max(eref):.2e}")
    assert np.all(e <= cs.LAPACK_BAR) and np.all(ef <= cs.LAPACK_BAR) and np.all(eref <= cs.LAPACK_BAR)
    if with_fixed:
        assert len(sp.fixed_rows) == 7 and np.all(sp.X[sp.fixed_rows] == 0.0)


@pytest.mark.parametrize("name,with_fixed", MODEL_CASES)
def test_bars_tell_a_wrong_half_and_which(name, with_fixed):
    """One strictly-lower block of the factor (the largest) times 1 + 1e-6 in one half of the solve only"""
    sp = cs.sweep_problem(name, with_fixed)
    ds, L = cs.host_factor(sp)
    i, j = cs.largest_lower_block(L)
    bwd = cs.host_sweeps(sp, cs.RMAX, ds, L, bad_bwd=(i, j, BAD))
    fwd = cs.host_sweeps(sp, cs.RMAX, ds, L, bad_fwd=(i, j, BAD))
    eb, ef = cs.solve_error(sp, bwd["x"]), cs.solve_error(sp, fwd["x"])
    fb, ff = cs.forward_error(sp, bwd), cs.forward_error(sp, fwd)
    print(f"{name} fixed={with_fixed}: block ({i}, {j}) off by 1e-6 relative -- backward half only: e {np.max(eb):.2e}, forward check {np.max(fb):.2e}; "
          f"forward half only: e {np.max(ef):.2e}, forward check {np.max(ff):.2e}")
    assert np.max(eb) > cs.FP64_BAR and np.max(ef) > cs.FP64_BAR
    for bad in (bwd, fwd):
        with pytest.raises(AssertionError):
            cs.check_solve(sp, bad)
    cs.check_forward(sp, bwd)
    with pytest.raises(AssertionError):
        cs.check_forward(sp, fwd)


def _sigma_metric(got, sigma):
    """max |dSigma_ij| / sqrt(Sigma_ii Sigma_jj) over the leading columns of Sigma = S^-1 that got holds (the columns tests' metric)"""
    v = np.diag(sigma)
    k = got.shape[1]
    return float(np.max(np.abs(got - sigma[:, :k]) / np.sqrt(v[:, None] * v[None, :k])))


@pytest.mark.parametrize("half", ["bad_bwd", "bad_fwd"])
def test_refinement_hides_the_wrong_sweep(half):
    """The blind spot: the perturbed sweep as the preconditioner of cc_solve_refine's rule, on unit columns as
    lsfm_map_covariance_columns solves them, ends inside the columns tests' flat 1e-9 -- it only takes more steps"""
    sp = cs.sweep_problem("band40")
    pb = sp.pb
    n = sp.n
    ds, L = cs.host_factor(sp)
    i, j = cs.largest_lower_block(L)
    yl, corr = cr.reference_scaled(pb.A0, np.eye(n), steps=2)
    assert corr[1] <= 1e-17
    Dl = pb.D.astype(np.longdouble)
    sigma = np.asarray(yl / Dl[:, None] / Dl[None, :], np.float64)
    E = np.eye(n)[:, :cs.RMAX]
    out = {}
    for label, kw in (("right", {}), ("wrong", {half: (i, j, BAD)})):
        sweep = lambda Y, kw=kw: cs.host_sweeps(sp, Y.shape[1], ds, L, B=Y, **kw)["x"]
        unrefined = _sigma_metric(sweep(E), sigma)
        X, steps, hist = cs.host_refine(sp, E, sweep)
        out[label] = (unrefined, _sigma_metric(X, sigma), steps, hist)
        print(f"band40, {half if kw else 'no block'} off by 1e-6: unrefined {unrefined:.2e}, refined {out[label][1]:.2e} after {steps} steps, corrections "
              + " ".join(f"{h:.1e}" for h in hist))
    assert out["wrong"][1] <= 1e-9 and out["right"][1] <= 1e-9
    assert out["wrong"][2] >= out["right"][2] >= 1


def test_residual_bar_holds_for_shuffled_sums_and_refuses_an_untransposed_block():
    sp = cs.sweep_problem("five30", True)
    pb = sp.pb
    m, R = pb.m, 12
    rng = np.random.default_rng(5)
    blocks = []   # both orientations of every block of the upper pattern: (target block row, source block row, 6 x 6)
    for p in range(m):
        for k in range(pb.rowptr[p], pb.rowptr[p + 1]):
            q = int(pb.colidx[k])
            blk = pb.val[k].reshape(6, 6)
            blocks.append((p, q, blk))
            if q != p:
                blocks.append((q, p, blk.T))

    def product(blocks):
        y = sp.B[:, :R].copy()
        for t in rng.permutation(len(blocks)):
            p, q, blk = blocks[t]
            y[6 * p:6 * p + 6] -= blk @ sp.X[6 * q:6 * q + 6, :R]
        y[sp.fixed_rows] = sp.B[sp.fixed_rows, :R]
        return y
    frac = cs.check_residual(sp, product(blocks))
    print(f"five30 +fixed: a float64 product with its sums in a shuffled order sits at {frac:.2f} of the bound")
    t = next(t for t, (p, q, _) in enumerate(blocks) if p > q)   # a lower-orientation entry, used as it is stored
    wrong = list(blocks)
    wrong[t] = (wrong[t][0], wrong[t][1], wrong[t][2].T)
    with pytest.raises(AssertionError):
        cs.check_residual(sp, product(wrong))
