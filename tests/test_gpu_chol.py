"""The device Cholesky (linearsfm_amd/csrc/lsfm_chol.hip) seen directly: its factor and UNREFINED applications of it, through
lsfm_selftest_chol, against a high-precision host reference (tests/chol_reference.py has the generator, the reference and the
derivation of every bar).  Everywhere else in the suite the factor is the preconditioner of a refinement that tests the true residual
-- a missing update, a wrong block of a sweep or a stale work vector only costs steps there -- or is inverted by the covariance calls,
which never run chol_apply, the leaf-task and supernode-group sweeps, the fused first forward substitution or the fp32 sweeps.

The patterns are crafted so that every schedule is launched -- leaf tasks alone, leaf tasks with deferred updates into the columns
above (k_chol_update_outer), chains of supernode groups, the fused panel kernel and the panel + rank-update pair, several independent
systems -- and every case asserts from the call's info that the schedule it was made for is the one that ran.  Each case runs plain
(mode 0), with the first right-hand side's forward substitution riding on the factorisation as in a level solve (mode 1; the second
and third right-hand sides follow it and catch state left in the work vectors) and with the fp32 sweeps (mode 2).

Every test prints the device's e (worst right-hand side) beside LAPACK's own Cholesky on the same system, max|L L^T - S^| beside its
bar and r.z as a fraction of its bar (pytest -s); DESIGN.md, "Direct tests of the factor and of the sweeps", keeps the record."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chol_reference as cr
from linearsfm_amd import api

pytestmark = pytest.mark.gpu

VARIANTS = [(name, False) for name in cr.CASES] + [(name, True) for name, c in cr.CASES.items() if c.fixed_pose]


@pytest.mark.parametrize("mode", list(cr.MODES))
@pytest.mark.parametrize("name,with_fixed", VARIANTS)
def test_factor_and_unrefined_solves(ctx, name, with_fixed, mode):
    print(cr.device_case(ctx, name, with_fixed, mode, cr.CASES[name].expect))


@pytest.mark.parametrize("setting", list(cr.SWITCHES))
def test_schedules_behind_switches(setting):
    """LSFM_TASK_X, LSFM_GS and LSFM_SN_FUSE_MAX are read once per process: a fresh child per setting, one after another"""
    env = dict(os.environ, **cr.SWITCHES[setting][0])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, '.'); sys.path.insert(0, 'tests')\n"
            "import chol_reference as cr\n"
            f"cr.child_main({setting!r})\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "chol child ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_malformed_input_is_refused(ctx):
    pb = cr.problem("dense2")
    with pytest.raises(api.LsfmError):
        ctx.selftest_chol(pb.rowptr, pb.colidx[::-1].copy(), pb.val, pb.r)            # rows that do not start with their diagonal block
    with pytest.raises(api.LsfmError):
        ctx.selftest_chol(pb.rowptr, pb.colidx, pb.val, pb.r, pose_seg=np.array([0, 1], np.int32), nseg=1)  # a system that does not exist
    with pytest.raises(api.LsfmError):
        ctx.selftest_chol(pb.rowptr, pb.colidx, pb.val, pb.r, mode=4)
