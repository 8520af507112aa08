"""The side-by-side sweeps behind every columns call (linearsfm_amd/csrc/lsfm_covcols.hip: k_cc_fwd / k_cc_bwd, k_cc_fwd_panel /
k_cc_bwd_panel, both panel versions) and their residual product k_cc_resid seen directly, UNREFINED, through
lsfm_selftest_cc_sweeps, against a high-precision host reference (tests/cc_sweeps_reference.py has the right-hand sides, the
reference and the derivation of every bar).  Everywhere else in the suite the sweeps are the preconditioner of cc_solve_refine's
fp64 refinement against S itself: a wrong block of a panel kernel, a mishandled last k step, a missed tile or a lost atomic costs
refinement steps there and the result still lands inside the columns tests' flat 1e-9 (tests/test_cc_sweeps_reference_cpu.py shows
it on the host); lsfm_selftest_chol launches none of these kernels.

What each case reaches (every case asserts from the call's info that the schedule it was made for is the one that ran):
  dense1, dense2, dense7, chain12   a leaf task alone: k_cc_fwd<false> / k_cc_bwd<false>, no group launch, no panel launch
  band40, five30                    leaf tasks whose columns have rows outside the task: the atomic branch of the leaf kernel
  hubs300                           levels whose groups differ in rows below: work-groups of the panel kernels that leave at once
  dense20                           a narrow last group
  dense110                          no leaf task; 612 scalar rows below the first group = 39 tiles > 32 work-groups: the forward
                                    panel's strided loop takes a second round; 13 backward chunks
  hubs260                           111-row panels under many groups
  dense270 (this module's own)      1572 scalar rows below the first group = 33 chunks > 32 work-groups: the backward panel's
                                    strided loop takes a second round
Every case runs with the plain panel (1) and the MFMA panel (2) at R = 6 (6 of a tile's 16 columns; plain: 8 row slices) and R = 192
(full; plain: 4 slices); band40, hubs300 and dense110 also at R = 3 (one feature column group), 16 (exactly one tile), 17 (one
column in a second wave) and 102 (a partly filled last wave).  Odd run widths (a half-empty last MFMA k step, a last run tile of 2,
6, 10 or 14 live rows) need other switches than the default and so a process of their own.

Every test prints the device's worst e beside LAPACK's own on the same columns, the forward half's error, the residual as a fraction
of its bound and the info counts (pytest -s); DESIGN.md, "Direct tests of the side-by-side sweeps", keeps the record."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cc_sweeps_reference as cs
from linearsfm_amd import api

pytestmark = pytest.mark.gpu

RESID = set(cs.RESID_CASES)
RUNS = [(name, fx, R) for name, fx in cs.VARIANTS for R in (cs.R_ALL if name in cs.R_CASES and not fx else cs.R_BASE)]


@pytest.mark.parametrize("panel", list(cs.PANELS))
@pytest.mark.parametrize("name,with_fixed,R", RUNS)
def test_unrefined_sweeps(ctx, name, with_fixed, R, panel):
    try:
        ctx.set_covcols_panel(panel)
        line, _ = cs.device_case(ctx, name, with_fixed, panel, R, cs.CASES[name].expect, resid=(name, with_fixed) in RESID)
    finally:
        ctx.set_covcols_panel(0)
    print(line)


@pytest.mark.parametrize("setting", list(cs.SWITCHES))
def test_odd_run_widths_behind_switches(setting, tmp_path):
    """LSFM_TASK_X and LSFM_GS are read once per process: a fresh child per setting, one after another.  The references are the
    parent's (computed once for the whole module), handed over as files."""
    for name in cs.R_CASES:
        np.save(tmp_path / (name + ".npy"), cs.sweep_problem(name).y_ref)
    env = dict(os.environ, **cs.SWITCHES[setting][0])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, '.'); sys.path.insert(0, 'tests')\n"
            "import cc_sweeps_reference as cs\n"
            f"cs.child_main({setting!r}, {str(tmp_path)!r})\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "cc sweeps child ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_malformed_input_is_refused(ctx):
    sp = cs.sweep_problem("dense2")
    pb = sp.pb
    B = sp.B[:, :6]
    with pytest.raises(api.LsfmError):
        ctx.selftest_cc_sweeps(pb.rowptr, pb.colidx[::-1].copy(), pb.val, B)     # rows that do not start with their diagonal block
    with pytest.raises(api.LsfmError):
        ctx.selftest_cc_sweeps(pb.rowptr, pb.colidx, pb.val, np.zeros((12, 0)))  # R = 0
    with pytest.raises(api.LsfmError):
        ctx.selftest_cc_sweeps(pb.rowptr, pb.colidx, pb.val, np.zeros((12, 193)))  # more than a chunk's columns
    # X without y: the binding always hands y along with X, so through the library itself
    import ctypes as C
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    Bc, val, info = np.ascontiguousarray(B), np.ascontiguousarray(pb.val).reshape(-1), np.full(16, 7, np.int32)
    x = np.full_like(Bc, 7.0)
    rc = api.lib().lsfm_selftest_cc_sweeps(ctx._h, pb.m, p(pb.rowptr, C.c_int), p(pb.colidx, C.c_int), p(val, C.c_double), None, None, p(Bc, C.c_double), 6,
                                           p(Bc, C.c_double), p(x, C.c_double), None, None, None, None, p(info, C.c_int))
    assert rc == -1 and np.all(info == 7) and np.all(x == 7.0)   # refused before anything is written
    # and the context still works
    ctx.selftest_cc_sweeps(pb.rowptr, pb.colidx, pb.val, B)
