"""Host side of the direct tests of the columns calls' side-by-side sweeps (tests/test_gpu_cc_sweeps.py,
tests/test_cc_sweeps_reference_cpu.py): the kernels k_cc_fwd / k_cc_bwd / k_cc_fwd_panel / k_cc_bwd_panel / k_cc_resid of
linearsfm_amd/csrc/lsfm_covcols.hip through lsfm_selftest_cc_sweeps, which runs them UNREFINED.  Built on tests/chol_reference.py: its
patterns, values, reference and error measure; one pattern of this module's own.  numpy + scipy.linalg only.

Right-hand sides.  B = D N(0,1), dense, seeded, 192 columns: every row of every column is non-zero in both halves of the solve
(a unit column's forward half is zero above its pose).  Columns 0 .. R-1 of the one 192-column reference serve every smaller R.

Reference.  chol_reference.reference_scaled on all columns at once (two refinement steps in long double; the second correction is
asserted below 1e-17 of the solution, so the state after the first was already that good).

Bars (derivations; nothing here is taken from what the device gives):
  solve     per column e_c = max|D (x_c - x_ref,c)| / max|D x_ref,c| <= FP64_BAR = 1e-11: chol_reference's derivation column by column
            -- the same factor, backward-stable sweeps; in which order the atomics arrive only permutes the terms of sums the
            bound already takes in the worst order.  It assumes 6m <= 1800 and kappa(A0) <= 1.7: dense270 (below) has 6m = 1620
            and kappa(A0) = 1.07 (tests/test_cc_sweeps_reference_cpu.py asserts it).
  forward   S^ = D^ P S_fixed P^T D^ from the device's perm and dscale (exact: powers of two), L_ref = LAPACK's Cholesky factor of
            S^ (the factor is unique: nothing of the device's L enters), fwd_ref = L_ref^-1 (D^ P B);
            max|fwd_c - fwd_ref,c| / max|fwd_ref,c| <= FP64_BAR per column, the same 3 n u kappa.  fwd_ref in float64 and by a
            long-double substitution agree below LAPACK_BAR (the CPU module asserts it), so the reference is nothing beside the bar.
  residual  y = B - S X with X = the reference solution rounded to double (0 in fixed rows), against the same in long double:
            |y_i - y_ref,i| <= (8 nb_i + 2) 2^-53 (|B_i| + sum_j |S_ij| |X_j|), nb_i = blocks in block row i of the full symmetric
            pattern: the rounding bound of 6 nb_i fused products and of the at most nb_i + 1 partial sums (a row's entries are
            split over work-groups of CC_EPW = 16, wherever the row begins) that atomics add to B_i, every term within the
            bracket.  A fixed row: y = B exactly.
"""
import functools
import hashlib
import os

import numpy as np
import scipy.linalg as sla

import chol_reference as cr
from chol_reference import FP64_BAR, LAPACK_BAR

RMAX = 192                      # 6 CC_KC: the columns of a full chunk
R_BASE = (6, 192)               # every case
R_ALL = (3, 6, 16, 17, 102, 192)
R_CASES = ("band40", "hubs300", "dense110")   # the cases every column count and every switch setting runs on
CC_GY = 32                      # lsfm_covcols.hip: most work-groups that share one group's panel
CC_GK = 6 * cr.CHOL_GS
PANELS = {1: "plain", 2: "MFMA"}

# 262 rows below the first group: 1572 scalar rows = 33 chunks of CC_GK > CC_GY, the only way to make k_cc_bwd_panel's strided loop
# over the chunks take a second round.  Not one of chol_reference.CASES: that module's parametrisation stays as it is.
DENSE270 = cr.Case("dense270", lambda: cr.dense_pattern(270), dict(leaf_tasks=0, groups=34, group_levels=34, max_run_rows=262))
CASES = dict(cr.CASES, dense270=DENSE270)
LEAF_ONLY = ("dense1", "dense2", "dense7", "chain12")
RESID_CASES = (("dense1", False), ("chain12", False), ("hubs260", False), ("five30", True))
VARIANTS = [(name, False) for name in CASES] + [(name, True) for name, c in CASES.items() if c.fixed_pose]

# Odd run widths (K = 6 s: the last MFMA k step half empty, the last 16-row tile of the run with 2, 6, 10 or 14 live rows) need other
# switches than the default LSFM_GS = 8; they are read once per process.  (environment, widest run = the odd width that must occur,
# what lsfm_symbolic_analyse makes of the R_CASES under it -- numbers from the host analysis, as chol_reference.SWITCHES')
SWITCHES = {
    "widths_1_to_3": (dict(LSFM_TASK_X="4", LSFM_GS="3"), 3, dict(
        band40=dict(leaf_tasks=2, groups=28, group_levels=7), hubs300=dict(leaf_tasks=0, groups=215, group_levels=21),
        dense110=dict(leaf_tasks=0, groups=37, group_levels=37))),
    "width_7": (dict(LSFM_GS="7"), 7, dict(
        band40=dict(leaf_tasks=3, groups=1, group_levels=1), hubs300=dict(leaf_tasks=34, groups=46, group_levels=10),
        dense110=dict(leaf_tasks=0, groups=16, group_levels=16))),
    "width_5": (dict(LSFM_GS="5"), 5, dict(
        band40=dict(leaf_tasks=3, groups=1, group_levels=1), hubs300=dict(leaf_tasks=34, groups=48, group_levels=12),
        dense110=dict(leaf_tasks=0, groups=22, group_levels=22))),
}
SWITCH_R = (17, 192)


# ---------------------------------------------------------------------------------------------------------------
# the problem: chol_reference's, with 192 dense right-hand sides and their reference
# ---------------------------------------------------------------------------------------------------------------
class SweepProblem:
    def __init__(self, pb, y_ref=None):
        self.pb = pb
        self.name = pb.case.name
        n = 6 * pb.m
        self.n = n
        rng = np.random.default_rng(11)
        self.c = rng.normal(size=(n, RMAX))
        self.B = pb.D[:, None] * self.c                     # [n, RMAX], the caller's numbering, unscaled
        self.fixed_rows = np.flatnonzero(pb.fixed) if pb.fixed is not None else np.zeros(0, np.int64)
        k = pb.keep
        self.A0k = pb.A0[np.ix_(k, k)]
        if y_ref is None:
            yl, self.corrections = cr.reference_scaled(self.A0k, self.c[k], steps=2)
            assert self.corrections[1] <= 1e-17, self.corrections
            y_ref = np.zeros((n, RMAX), np.longdouble)
            y_ref[k] = yl
        self.y_ref = y_ref                                   # D x_ref, long double, 0 in fixed rows
        self.X = np.asarray(self.y_ref / pb.D[:, None].astype(np.longdouble), np.float64)   # the reference solution rounded to double
        rp, ci = pb.rowptr, pb.colidx
        self.nb = np.diff(rp) + np.bincount(ci, minlength=pb.m) - 1   # blocks per block row of the full symmetric pattern

    @functools.cached_property
    def lapack_e(self):
        """LAPACK's own Cholesky on the same columns, per column"""
        y = np.zeros((self.n, RMAX))
        y[self.pb.keep] = cr.lapack_scaled(self.A0k, self.c[self.pb.keep])
        return cr.scaled_error(y, self.y_ref)

    @functools.cached_property
    def resid_ref(self):
        """(B - S X in long double, the bracket |B| + |S| |X| of the bound)"""
        pb = self.pb
        Xl = self.X.astype(np.longdouble)
        y = self.B.astype(np.longdouble) - pb.S.astype(np.longdouble) @ Xl
        mag = np.abs(self.B) + np.abs(pb.S) @ np.abs(self.X)
        return y, mag

    def B_in(self):
        """B as the sweeps see it: zero in fixed rows"""
        B = self.B.copy()
        B[self.fixed_rows] = 0.0
        return B


@functools.lru_cache(maxsize=None)
def sweep_problem(name, with_fixed=False):
    pb = cr.problem(name, with_fixed) if name in cr.CASES else cr.Problem(CASES[name], with_fixed)
    return SweepProblem(pb)


# ---------------------------------------------------------------------------------------------------------------
# checks of a result (the dict Context.selftest_cc_sweeps returns, or host_sweeps below)
# ---------------------------------------------------------------------------------------------------------------
def solve_error(sp, x):
    """e per column of x [n, R]"""
    R = x.shape[1]
    return cr.scaled_error(np.asarray(x) * sp.pb.D[:, None], sp.y_ref[:, :R])


def check_solve(sp, res):
    x = res["x"]
    assert np.all(x[sp.fixed_rows] == 0.0), "a fixed scalar did not come back as zero"
    e = solve_error(sp, x)
    assert np.all(e <= FP64_BAR), f"{sp.name}: e = {np.max(e):.3e} in column {int(np.argmax(e))} of {x.shape[1]}, above {FP64_BAR:.0e}"
    return e


_fwd_seen = {}


def scaled_system(sp, perm, ds):
    """(index of the new numbering into the old, S^ = D^ P S_fixed P^T D^)"""
    idx = (6 * np.asarray(perm)[:, None] + np.arange(6)[None, :]).reshape(-1)
    Sh = sp.pb.S_fixed()[np.ix_(idx, idx)] * ds[:, None] * ds[None, :]
    return idx, Sh


def forward_reference(sp, perm, ds):
    """fwd_ref [n, RMAX] for the device's perm and dscale; computed once per (problem, perm, dscale)"""
    key = hashlib.sha1(np.ascontiguousarray(perm).tobytes() + np.ascontiguousarray(ds).tobytes()
                       + sp.name.encode() + (b"f" if len(sp.fixed_rows) else b"-")).hexdigest()
    if key not in _fwd_seen:
        assert sorted(np.asarray(perm).tolist()) == list(range(sp.pb.m))
        assert np.all(np.log2(ds) == np.round(np.log2(ds))), "dscale is not made of powers of two"
        idx, Sh = scaled_system(sp, perm, ds)
        Lref = np.linalg.cholesky(Sh)
        _fwd_seen[key] = sla.solve_triangular(Lref, sp.B_in()[idx] * ds[:, None], lower=True)
    return _fwd_seen[key]


def forward_error(sp, res):
    R = res["fwd"].shape[1]
    ref = forward_reference(sp, res["perm"], res["dscale"])[:, :R]
    return np.max(np.abs(res["fwd"] - ref), axis=0) / np.max(np.abs(ref), axis=0)


def check_forward(sp, res):
    ef = forward_error(sp, res)
    assert np.all(ef <= FP64_BAR), f"{sp.name}: forward half off by {np.max(ef):.3e} in column {int(np.argmax(ef))}, above {FP64_BAR:.0e}"
    return ef


def check_residual(sp, y):
    """y [n, R] of the device against the long-double B - S X; returns the worst |y - y_ref| as a fraction of its bound"""
    R = y.shape[1]
    yref, mag = sp.resid_ref
    assert np.array_equal(y[sp.fixed_rows], sp.B[sp.fixed_rows, :R]), "a fixed row of y is not B's"
    bound = (np.repeat(8.0 * sp.nb + 2.0, 6) * 2.0 ** -53)[:, None] * mag[:, :R]
    d = np.asarray(np.abs(y.astype(np.longdouble) - yref[:, :R]), np.float64)
    live = np.ones(sp.n, bool)
    live[sp.fixed_rows] = False
    frac = d[live] / bound[live]
    i = np.unravel_index(int(np.argmax(frac)), frac.shape)
    assert np.all(d[live] <= bound[live]), f"{sp.name}: residual off by {frac[i]:.2f} of its bound at (live row {i[0]}, column {i[1]})"
    return float(frac[i])


def check_structure(name, info, expect, panel):
    """The schedule the device launched (info of lsfm_selftest_cc_sweeps) is the one the case was made for"""
    for k in ("leaf_tasks", "groups", "group_levels"):
        if k in expect:
            assert info[k] == expect[k], f"{name}: {k} = {info[k]}, made for {expect[k]}: {info}"
    assert info["d_err"] == 0 and info["floored"] == 0, info
    assert info["panel"] == panel, info
    assert info["fwd_task_launches"] == (1 if info["leaf_tasks"] else 0), info
    assert info["fwd_group_launches"] == info["group_levels"], info
    assert info["fwd_panel_launches"] == info["bwd_panel_launches"] <= info["group_levels"], info
    assert (info["width_mask"] == 0) == (info["groups"] == 0) and info["width_mask"] < (1 << cr.CHOL_GS), info
    if panel == 1 or name in LEAF_ONLY:
        assert info["fwd_panel_launches"] == 0, f"{name}: a panel kernel was launched: {info}"
    if name in LEAF_ONLY:
        assert info["groups"] == 0 and info["fwd_group_launches"] == 0, info
    if "max_run_rows" in expect:
        assert info["max_rows_below"] == expect["max_run_rows"], info
    if name == "dense110":
        # 39 tiles of 16 rows > CC_GY: the forward panel's strided loop over the tiles takes a second round
        assert info["max_rows_below"] >= 86 and (6 * info["max_rows_below"] + 15) // 16 > CC_GY, info
        if panel == 2:
            assert info["fwd_panel_launches"] == info["group_levels"] - 1, info   # (every group but the last has rows below it)
    if name == "dense270":
        assert info["max_rows_below"] > 256 and (6 * info["max_rows_below"] + CC_GK - 1) // CC_GK > CC_GY, info


def device_case(ctx, name, with_fixed, panel, R, expect, resid=False, sp=None):
    """One case on the device with one panel version and R columns under every assertion; returns (a line of the measured figures,
    the call's info).  The caller has set the panel version (Context.set_covcols_panel)."""
    case = CASES[name]
    sp = sp or sweep_problem(name, with_fixed)
    pb = sp.pb
    res = ctx.selftest_cc_sweeps(pb.rowptr, pb.colidx, pb.val, sp.B[:, :R], origin=case.origin, fixed=pb.fixed, X=sp.X[:, :R] if resid else None)
    info = res["info"]
    e, ef = solve_error(sp, res["x"]), forward_error(sp, res)
    line = (f"{name}{' +fixed' if with_fixed else ''} panel {panel} ({PANELS[panel]}) R {R}: e {np.max(e):.2e} (LAPACK {np.max(sp.lapack_e[:R]):.2e}), "
            f"forward {np.max(ef):.2e}")
    print(line, "|", info, flush=True)
    check_structure(name, info, expect, panel)
    check_solve(sp, res)
    check_forward(sp, res)
    if resid:
        line += f", residual at {check_residual(sp, res['y']):.2f} of its bound"
    return line + f", width mask {info['width_mask']:#x}, panel launches {info['fwd_panel_launches']}", info


def child_main(setting, ref_dir):
    """The R_CASES at SWITCH_R columns with both panel versions under the switches of SWITCHES[setting], which the parent has put in
    the environment; the parent's references are read from ref_dir"""
    from linearsfm_amd import api
    env, width, expect = SWITCHES[setting]
    assert all(os.environ.get(k) == v for k, v in env.items())
    ctx = api.Context(0)
    masks = {}
    try:
        for name in R_CASES:
            sp = SweepProblem(cr.problem(name), y_ref=np.load(os.path.join(ref_dir, name + ".npy")))
            for panel in PANELS:
                ctx.set_covcols_panel(panel)
                for R in SWITCH_R:
                    line, info = device_case(ctx, name, False, panel, R, expect[name], sp=sp)
                    print(line, flush=True)
                    masks[name] = info["width_mask"]
    finally:
        ctx.set_covcols_panel(0)
        ctx.close()
    print("width masks", {k: hex(v) for k, v in masks.items()})
    # no run wider than the setting allows, and the odd width itself occurred (dense110's chain of groups is cut into full runs)
    assert all(v < (1 << width) for v in masks.values()), masks
    assert masks["dense110"] & (1 << (width - 1)), masks
    print("cc sweeps child ok")


# ---------------------------------------------------------------------------------------------------------------
# host model (tests/test_cc_sweeps_reference_cpu.py): the side-by-side solve through LAPACK's factor
# ---------------------------------------------------------------------------------------------------------------
def host_factor(sp):
    """(dscale, LAPACK's factor of the power-of-four-scaled S_fixed) in the natural order, as chol_reference.host_result"""
    Sf = sp.pb.S_fixed()
    ds = 2.0 ** -((np.frexp(np.diag(Sf))[1] + 1) >> 1)
    return ds, np.linalg.cholesky(Sf * ds[:, None] * ds[None, :])


def largest_lower_block(L):
    """(i, j) of the strictly-lower 6 x 6 block of L with the largest norm"""
    m = L.shape[0] // 6
    nb = np.linalg.norm(L.reshape(m, 6, m, 6), axis=(1, 3))
    nb[np.triu_indices(m)] = 0.0
    i, j = np.unravel_index(int(np.argmax(nb)), nb.shape)
    return int(i), int(j)


def host_sweeps(sp, R, ds, L, bad_fwd=None, bad_bwd=None, B=None):
    """What Context.selftest_cc_sweeps returns, made on the host with the factor L of the scaled matrix in the natural order.
    bad_fwd / bad_bwd = (i, j, f): block (i, j) of the factor times f in that half of the solve only -- a sweep that is slightly
    wrong.  B: other right-hand sides than the problem's first R."""
    def factor(bad):
        if not bad:
            return L
        i, j, f = bad
        Lb = L.copy()
        Lb[6 * i:6 * i + 6, 6 * j:6 * j + 6] *= f
        return Lb
    B = sp.B[:, :R].copy() if B is None else B.copy()
    B[sp.fixed_rows] = 0.0
    fwd = sla.solve_triangular(factor(bad_fwd), B * ds[:, None], lower=True)
    x = sla.solve_triangular(factor(bad_bwd), fwd, lower=True, trans="T") * ds[:, None]
    x[sp.fixed_rows] = 0.0
    return dict(x=x, fwd=fwd, perm=np.arange(sp.pb.m, dtype=np.int32), dscale=ds, y=None, info=None)


def host_refine(sp, B, sweep, tol=1e-12, max_steps=50):
    """cc_solve_refine's rule on the host: X = sweep(B); always one step X += sweep(B - S X), further steps while the worst column's
    correction |delta|_inf / |x|_inf is above tol and still halving.  Returns (X, steps, the worst correction of every step)."""
    S = sp.pb.S_fixed()
    X = sweep(B)
    steps, prev, hist = 0, 0.0, []
    while True:
        d = sweep(B - S @ X)
        X = X + d
        steps += 1
        worst = float(np.max(np.max(np.abs(d), axis=0) / np.max(np.abs(X), axis=0)))
        hist.append(worst)
        if worst <= tol or steps >= max_steps:
            break
        if steps > 1 and not worst <= 0.5 * prev:
            break
        prev = worst
    return X, steps, hist
