"""Host side of the direct tests of the device Cholesky (tests/test_gpu_chol.py, tests/test_chol_reference_cpu.py): crafted block
patterns that force every schedule of linearsfm_amd/csrc/lsfm_chol.hip, well-conditioned values with a wide spread of scales on them,
a high-precision reference solution, and the checks of a factor and of unrefined solves against it.  numpy only.

Values.  Off-diagonal blocks are N(0,1); a diagonal block is a random symmetric block plus 2 x (absolute row sum) + 1e-3 on its
diagonal, so the matrix is strictly diagonally dominant; it is Jacobi-scaled to unit diagonal (A0: condition number 1.1 - 1.6 on the
cases of 40 poses and more, up to 2.1 on the tiny dense ones) and then spread out as S = D A0 D with D = 10^uniform(-3, 3) per scalar, which gives k_chol_scatter's power-of-four
scaling work to do.

Reference.  A0 y = D^-1 r by LAPACK, then three refinement steps with the residual in np.longdouble (the corrections fall to 1e-18,
1e-19 of the solution); z_ref = y / D.  Fixed scalars: their rows and columns leave the system, z_ref = 0 there (what k_perm_in /
k_perm_out_dot implement).  An LU of the unscaled S is NOT used: it sits 1e-10 away.

Error measure: the solution in the scaled variables, e = max|D (z - z_ref)| / max|D z_ref|.

Bars (derivations; nothing here is taken from what the device gives):
  factor   max|L L^T - S^| <= 6m 2^-52 with S^ = D^ P S P^T D^ built from the device's perm and dscale (an exact scaling, entries in
           (-1, 1)): the worst case of 6m rounded products per entry; max|Dinv_j L_jj - I| <= 1e-13; no floored pivot, no error word
  fp64     e <= 1e-11: the forward error of a backward-stable Cholesky is at most 3 n u kappa, n = 6m <= 1800, kappa <= 13 (the
           Jacobi-scaled 1.6 times the factor 8 that the power-of-four scaling leaves on the diagonal): 8e-12
  fp32     at most 20 x what LAPACK's factor of A0 rounded to fp32 gives on the same system, measured in the test: the device's factor
           is rounded after another scaling and applied in another order, each within a small multiple of fp32's unit roundoff
  dot      the per-system r . z the device returns is within 6m 2^-52 sum|r_i z_i| of the same sum over the device's own z in long
           double: the rounding bound of a sum of 6m products (against z_ref's the bound could not hold in fp32 mode, nor at m = 1)
"""
import functools
import hashlib

import numpy as np

from linearsfm_amd import synth

CHOL_GS = 8          # lsfm_symbolic.hpp: most block columns of a supernode group
SN_FUSE_MAX = 96     # lsfm_chol.hip chol_factor: tallest panel the fused kernel takes (LSFM_SN_FUSE_MAX)
FP64_BAR = 1e-11
FP32_FACTOR = 20.0
DINV_BAR = 1e-13
LAPACK_BAR = 5e-15   # LAPACK's own Cholesky against the reference (tests/test_chol_reference_cpu.py)


# ---------------------------------------------------------------------------------------------------------------
# patterns
# ---------------------------------------------------------------------------------------------------------------
def dense_pattern(m):
    rowptr = np.concatenate([[0], np.cumsum(np.arange(m, 0, -1))]).astype(np.int32)
    colidx = np.concatenate([np.arange(p, m) for p in range(m)]).astype(np.int32)
    return rowptr, colidx


def schur_pattern(m, band, hubs):
    rowptr, colidx, _ = synth.schur_like_matrix(m, band, hubs, seed=1)
    return np.asarray(rowptr, np.int32), np.asarray(colidx, np.int32)


def block_diag_pattern(k, m, band, hubs):
    """k independent schur_like_matrix(m, band, hubs) systems (seeds 0 .. k-1) on the diagonal of one block matrix"""
    rps, cis = [np.zeros(1, np.int64)], []
    for s in range(k):
        rp, ci, _ = synth.schur_like_matrix(m, band, hubs, seed=s)
        cis.append(np.asarray(ci, np.int64) + s * m)
        rps.append(np.asarray(rp[1:], np.int64) + rps[-1][-1])
    return np.concatenate(rps).astype(np.int32), np.concatenate(cis).astype(np.int32)


class Case:
    """A pattern and what the symbolic analysis makes of it under default switches.  expect: leaf_tasks, groups, group_levels
    (absent: not stated), max_col_rows = most blocks below the diagonal of a column of L, max_run_rows = most rows below a supernode
    group (what the device reports); split = some group level takes k_sn_panel<false> + k_sn_syrk (a run with more than SN_FUSE_MAX
    rows below it); outer = leaf columns have deferred updates into the columns above (k_chol_update_outer runs)."""

    def __init__(self, name, pattern, expect, origin=None, pose_seg=None, nseg=1, fixed_pose=None, symbolic_checked=True):
        self.name, self._pattern, self.expect = name, pattern, expect
        self.origin, self.pose_seg, self.nseg, self.fixed_pose, self.symbolic_checked = origin, pose_seg, nseg, fixed_pose, symbolic_checked

    @property
    def pattern(self):
        return self._pattern()

    def __repr__(self):
        return self.name


_five = np.repeat(np.arange(5), 30).astype(np.int32)
CASES = {c.name: c for c in [
    Case("dense1", lambda: dense_pattern(1), dict(leaf_tasks=1, groups=0, group_levels=0)),
    Case("dense2", lambda: dense_pattern(2), dict(leaf_tasks=1, groups=0, group_levels=0)),
    Case("dense7", lambda: dense_pattern(7), dict(leaf_tasks=1, groups=0, group_levels=0), fixed_pose=(3, 5)),
    Case("chain12", lambda: schur_pattern(12, 1, 0), dict(leaf_tasks=1, groups=0, group_levels=0)),
    Case("band40", lambda: schur_pattern(40, 2, 0), dict(leaf_tasks=3, groups=1, group_levels=1)),
    # one leaf task, then two groups in a chain, the last one narrower than CHOL_GS
    Case("dense20", lambda: dense_pattern(20), dict(leaf_tasks=1, groups=2, group_levels=2)),
    Case("hubs300", lambda: schur_pattern(300, 4, 12), dict(leaf_tasks=34, groups=46, group_levels=10, outer=True), fixed_pose=(17, 250)),
    # 111 rows below a column: above SN_FUSE_MAX, so k_sn_panel<false> + k_sn_syrk
    Case("hubs260", lambda: schur_pattern(260, 1, 110), dict(leaf_tasks=61, groups=85, group_levels=23, max_col_rows=111, split=True)),
    # no leaf task: a pure chain of groups whose first panel is 110 - CHOL_GS = 102 rows tall
    Case("dense110", lambda: dense_pattern(110), dict(leaf_tasks=0, groups=14, group_levels=14, max_col_rows=109, max_run_rows=102, split=True), symbolic_checked=False),
    Case("five30", lambda: block_diag_pattern(5, 30, 2, 2), dict(leaf_tasks=5, groups=34), origin=_five, pose_seg=_five, nseg=5, fixed_pose=(31, 149)),
]}
# the cases every switch setting of tests/test_gpu_chol.py runs again in a process of its own
SWITCH_CASES = ("band40", "hubs300", "hubs260", "five30")
NRHS = 3
# Schedules the default switches cannot reach (the switches are read once per process: one child process per setting), and what the
# symbolic analysis makes of the SWITCH_CASES under each -- the same numbers lsfm_symbolic_analyse gives without a device
SWITCHES = {
    "no_leaf_task": (dict(LSFM_TASK_X="1"), dict(
        band40=dict(leaf_tasks=0, groups=29, group_levels=7), hubs300=dict(leaf_tasks=0, groups=187, group_levels=15),
        hubs260=dict(leaf_tasks=0, groups=165, group_levels=23, split=True), five30=dict(leaf_tasks=0, groups=131, group_levels=27))),
    # the largest leaf tasks LDS admits; the five-system case is then leaf tasks alone
    "largest_leaf_tasks": (dict(LSFM_TASK_X="164"), dict(
        band40=dict(leaf_tasks=2, groups=1, group_levels=1), hubs300=dict(leaf_tasks=25, groups=30, group_levels=7, outer=True),
        hubs260=dict(leaf_tasks=77, groups=51, group_levels=22, split=True), five30=dict(leaf_tasks=5, groups=0, group_levels=0))),
    "narrow_groups": (dict(LSFM_TASK_X="4", LSFM_GS="3"), dict(
        band40=dict(leaf_tasks=2, groups=28, group_levels=7), hubs300=dict(leaf_tasks=0, groups=215, group_levels=21),
        hubs260=dict(leaf_tasks=1, groups=186, group_levels=45, split=True), five30=dict(leaf_tasks=1, groups=130, group_levels=26))),
    # the panel + rank-update pair on short panels
    "split_short_panels": (dict(LSFM_SN_FUSE_MAX="8"), dict(
        band40=dict(leaf_tasks=3, groups=1, group_levels=1), hubs300=dict(leaf_tasks=34, groups=46, group_levels=10, outer=True, split=True),
        hubs260=dict(leaf_tasks=61, groups=85, group_levels=23, split=True), five30=dict(leaf_tasks=5, groups=34, group_levels=9))),
}
MODES = {0: "plain", 1: "fused first forward substitution", 2: "fp32 sweeps"}


def fixed_mask(case):
    """The Mono gauge on one pose and one scalar elsewhere: 7 fixed scalars (all six of pose a, scalar 2 of pose b)"""
    a, b = case.fixed_pose
    fx = np.zeros(6 * (len(case.pattern[0]) - 1), np.uint8)
    fx[6 * a:6 * a + 6] = 1
    fx[6 * b + 2] = 1
    return fx


# ---------------------------------------------------------------------------------------------------------------
# values and reference
# ---------------------------------------------------------------------------------------------------------------
def make_values(rowptr, colidx, seed=3, spread=3.0):
    """(val [nnzb, 36] for the pattern, dense S, A0, D) as the module's docstring describes"""
    m = len(rowptr) - 1
    n = 6 * m
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n))
    for p in range(m):
        for k in range(rowptr[p] + 1, rowptr[p + 1]):
            q = colidx[k]
            B = rng.normal(size=(6, 6))
            A[6 * p:6 * p + 6, 6 * q:6 * q + 6] = B
            A[6 * q:6 * q + 6, 6 * p:6 * p + 6] = B.T
    for p in range(m):
        G = rng.normal(size=(6, 6))
        B = G @ G.T / 6
        A[6 * p:6 * p + 6, 6 * p:6 * p + 6] = B - np.diag(np.diag(B))
    A = A + np.diag(2.0 * np.abs(A).sum(1) + 1e-3)
    d = 1 / np.sqrt(np.diag(A))
    A0 = A * d[:, None] * d[None, :]
    A0 = (A0 + A0.T) / 2
    D = 10.0 ** rng.uniform(-spread, spread, size=n)
    S = A0 * D[:, None] * D[None, :]
    S = (S + S.T) / 2
    val = np.empty((len(colidx), 36))
    for p in range(m):
        for k in range(rowptr[p], rowptr[p + 1]):
            q = colidx[k]
            val[k] = S[6 * p:6 * p + 6, 6 * q:6 * q + 6].reshape(36)
    return val, S, A0, D


def reference_scaled(A0, c, steps=3):
    """y with A0 y = c (c: [n, k]) to far below double precision: LAPACK + refinement with the residual in long double.  Returns
    (y as long double, the relative size of every correction)."""
    y = np.linalg.solve(A0, c)
    yl, Al, cl = y.astype(np.longdouble), A0.astype(np.longdouble), c.astype(np.longdouble)
    corr = []
    for _ in range(steps):
        res = cl - Al @ yl
        dy = np.linalg.solve(A0, res.astype(np.float64))
        yl = yl + dy.astype(np.longdouble)
        corr.append(float(np.max(np.abs(dy)) / np.max(np.abs(y))))
    return yl, corr


def lapack_scaled(A0, c, fp32=False):
    """y = A0^-1 c through LAPACK's Cholesky factor of A0 (fp32: the factor rounded to float before it is applied)"""
    Lc = np.linalg.cholesky(A0)
    if fp32:
        Lc = Lc.astype(np.float32).astype(np.float64)
    return np.linalg.solve(Lc.T, np.linalg.solve(Lc, c))


def scaled_error(y, y_ref):
    """e per right-hand side (columns): max|y - y_ref| / max|y_ref| in the scaled variables y = D z"""
    y_ref = np.asarray(y_ref, np.longdouble)
    return np.asarray(np.max(np.abs(np.asarray(y, np.longdouble) - y_ref), axis=0) / np.max(np.abs(y_ref), axis=0), np.float64)


class Problem:
    """A case with values, right-hand sides and everything the host can say about the answer, computed once"""

    def __init__(self, case, with_fixed):
        self.case = case
        self.rowptr, self.colidx = case.pattern
        self.m = len(self.rowptr) - 1
        n = 6 * self.m
        self.val, self.S, self.A0, self.D = make_values(self.rowptr, self.colidx)
        self.fixed = fixed_mask(case) if with_fixed else None
        self.keep = np.flatnonzero(self.fixed == 0) if with_fixed else np.arange(n)
        rng = np.random.default_rng(9)
        self.r = (self.D[None, :] * rng.normal(size=(NRHS, n)))           # [NRHS, n]: distinct right-hand sides
        self.pose_seg = case.pose_seg if case.pose_seg is not None else np.zeros(self.m, np.int32)
        k = self.keep
        A0k = self.A0[np.ix_(k, k)]
        c = (self.r / self.D[None, :]).T[k]                                # [kept, NRHS]
        yl, self.corrections = reference_scaled(A0k, c)
        self.y_ref = np.zeros((n, NRHS), np.longdouble)
        self.y_ref[k] = yl
        self.z_ref = np.asarray(self.y_ref / self.D[:, None].astype(np.longdouble), np.float64).T   # [NRHS, n]
        y64 = np.zeros((n, NRHS)); y64[k] = lapack_scaled(A0k, c)
        y32 = np.zeros((n, NRHS)); y32[k] = lapack_scaled(A0k, c, fp32=True)
        self.lapack_e = scaled_error(y64, self.y_ref)   # LAPACK's Cholesky in fp64 against the reference
        self.lapack_e32 = scaled_error(y32, self.y_ref) # ... its factor rounded to fp32

    def error(self, z):
        """e of a device result z [NRHS, n]"""
        return scaled_error((np.asarray(z) * self.D[None, :]).T, self.y_ref)

    def S_fixed(self):
        """S with the rows and columns of the fixed scalars replaced by the identity's (what k_chol_scatter factors)"""
        if self.fixed is None:
            return self.S
        S = self.S.copy()
        f = np.flatnonzero(self.fixed)
        S[f, :] = 0.0
        S[:, f] = 0.0
        S[f, f] = 1.0
        return S


@functools.lru_cache(maxsize=None)
def problem(name, with_fixed=False):
    return Problem(CASES[name], with_fixed)


# ---------------------------------------------------------------------------------------------------------------
# checks of a device result (the dict Context.selftest_chol returns)
# ---------------------------------------------------------------------------------------------------------------
def dense_factor(res, m):
    """L of the device as a dense lower-triangular matrix in the new numbering"""
    n = 6 * m
    Ld = np.zeros((n, n))
    colptr, rowidx, Lb = res["colptr"], res["rowidx"], res["L"]
    for j in range(m):
        for e in range(colptr[j], colptr[j + 1]):
            i = rowidx[e]
            Ld[6 * i:6 * i + 6, 6 * j:6 * j + 6] = Lb[e]
    return Ld


def llt_minus(Ld, Sh):
    """max|L L^T - S^| with no rounding error of its own to speak of: L = L1 + Lr with L1 on the grid 2^-21 (|L| < 1: L1 L1^T is then
    a sum of at most 2^11 integers below 2^42 in units of 2^-42 -- exact in doubles in whatever order BLAS adds them -- and Lr = L -
    L1 is exact); the products with Lr are below 1e-5 and their rounding below 1e-18.  A plain double product would carry up to
    n u of its own, half the bar."""
    assert Ld.shape[0] <= 2048 and np.max(np.abs(Ld)) < 1.0
    L1 = np.round(Ld * 2.0 ** 21) * 2.0 ** -21
    Lr = Ld - L1
    P1r = L1 @ Lr.T
    R = (L1 @ L1.T).astype(np.longdouble) - Sh.astype(np.longdouble)
    R += (P1r + P1r.T).astype(np.longdouble)
    R += (Lr @ Lr.T).astype(np.longdouble)
    return float(np.max(np.abs(R)))


_factor_seen = {}


def check_factor(pb, res):
    """The factor the device returned against S itself.  Returns (max|L L^T - S^|, its bar, max|Dinv L_jj - I|); asserts the bars.
    (A factor whose every bit was checked before -- the factorisation is deterministic, the modes share it -- is not multiplied out
    again.)"""
    m = pb.m
    info = res["info"]
    assert info["d_err"] == 0 and info["floored"] == 0, info
    perm, ds = res["perm"], res["dscale"]
    assert sorted(perm.tolist()) == list(range(m))
    assert np.all(np.log2(ds) == np.round(np.log2(ds))), "dscale is not made of powers of two"
    key = hashlib.sha1(b"".join(np.ascontiguousarray(res[k]).tobytes() for k in ("perm", "colptr", "rowidx", "L", "Dinv", "dscale"))
                       + (pb.fixed.tobytes() if pb.fixed is not None else b"-") + pb.case.name.encode()).hexdigest()
    if key not in _factor_seen:
        idx = (6 * perm[:, None] + np.arange(6)[None, :]).reshape(-1)
        Sh = pb.S_fixed()[np.ix_(idx, idx)] * ds[:, None] * ds[None, :]   # exact: powers of two
        assert np.max(np.abs(Sh)) < 1.0 and np.all(np.diag(Sh) >= 0.125)
        Ld = dense_factor(res, m)
        assert np.all(np.triu(Ld, 1) == 0.0)
        llt = llt_minus(Ld, Sh)
        dinv = max(float(np.max(np.abs(res["Dinv"][j] @ Ld[6 * j:6 * j + 6, 6 * j:6 * j + 6] - np.eye(6)))) for j in range(m))
        _factor_seen[key] = (llt, dinv)
    llt, dinv = _factor_seen[key]
    bar = 6 * m * 2.0 ** -52
    assert llt <= bar, f"{pb.case.name}: max|L L^T - S^| = {llt:.3e} above {bar:.3e}"
    assert dinv <= DINV_BAR, f"{pb.case.name}: max|Dinv L_jj - I| = {dinv:.3e}"
    return llt, bar, dinv


def check_dot(pb, res, nseg):
    """per-system r . z of the device against the same sum over the device's own z in long double"""
    z, r = res["z"].astype(np.longdouble), pb.r.astype(np.longdouble)
    worst = 0.0
    for k in range(NRHS):
        for g in range(nseg):
            rows = np.repeat(pb.pose_seg == g, 6)
            ref = np.sum(r[k, rows] * z[k, rows])
            tol = 6 * pb.m * 2.0 ** -52 * float(np.sum(np.abs(r[k, rows] * z[k, rows])))
            d = abs(float(res["dot"][k, g] - ref))
            assert d <= tol, f"{pb.case.name}: r.z of right-hand side {k}, system {g}: off by {d:.3e}, allowed {tol:.3e}"
            worst = max(worst, d / tol if tol > 0 else 0.0)
    return worst


def check_solves(pb, res, fp32):
    """e of every right-hand side against the bar of the mode; returns (e [NRHS], bar)"""
    if pb.fixed is not None:
        assert np.all(res["z"][:, pb.fixed != 0] == 0.0), "a fixed scalar did not come back as zero"
    e = pb.error(res["z"])
    bar = FP32_FACTOR * pb.lapack_e32 if fp32 else np.full(NRHS, FP64_BAR)
    assert np.all(e <= bar), f"{pb.case.name}: e = {e} above {bar} (LAPACK: fp64 {pb.lapack_e}, fp32 factor {pb.lapack_e32})"
    return e, bar


def host_result(pb, scale_block=None):
    """What Context.selftest_chol returns, made on the host: LAPACK's factor of the power-of-four-scaled S in the natural order, and
    the solves with it.  scale_block = (i, j, f): block (i, j) of the factor times f first -- a factor that is slightly wrong."""
    m, n = pb.m, 6 * pb.m
    Sf = pb.S_fixed()
    ds = 2.0 ** -((np.frexp(np.diag(Sf))[1] + 1) >> 1)   # s with s^2 d in [1/8, 1)
    Ld = np.linalg.cholesky(Sf * ds[:, None] * ds[None, :])
    if scale_block:
        i, j, f = scale_block
        Ld[6 * i:6 * i + 6, 6 * j:6 * j + 6] *= f
    colptr = np.concatenate([[0], np.cumsum(np.arange(m, 0, -1))]).astype(np.int32)
    rowidx = np.concatenate([np.arange(j, m) for j in range(m)]).astype(np.int32)
    Lb = np.stack([Ld[6 * i:6 * i + 6, 6 * j:6 * j + 6] for j in range(m) for i in range(j, m)])
    Dinv = np.stack([np.linalg.inv(Ld[6 * j:6 * j + 6, 6 * j:6 * j + 6]) for j in range(m)])
    rr = pb.r.copy()
    if pb.fixed is not None:
        rr[:, pb.fixed != 0] = 0.0
    z = (np.linalg.solve(Ld.T, np.linalg.solve(Ld, (rr * ds[None, :]).T)) * ds[:, None]).T
    if pb.fixed is not None:
        z[:, pb.fixed != 0] = 0.0
    dot = np.array([[np.sum((pb.r[k] * z[k])[np.repeat(pb.pose_seg == g, 6)]) for g in range(pb.case.nseg)] for k in range(NRHS)])
    return dict(z=z, dot=dot, perm=np.arange(m, dtype=np.int32), colptr=colptr, rowidx=rowidx, L=Lb, Dinv=Dinv, dscale=ds,
                info=dict(d_err=0, floored=0))


def check_structure(name, info, expect, fuse_max=SN_FUSE_MAX):
    """The schedule the device launched (info of lsfm_selftest_chol) is the one the case was made for"""
    for k in ("leaf_tasks", "groups", "group_levels"):
        if k in expect:
            assert info[k] == expect[k], f"{name}: {k} = {info[k]}, made for {expect[k]}: {info}"
    assert (info["leaf_tasks"] == 0) == (info["leaf_columns"] == 0), info
    assert info["fused_levels"] + info["split_levels"] == info["group_levels"], info
    assert (info["max_rows_below"] > fuse_max) == (info["split_levels"] > 0), info
    if expect.get("split"):
        assert info["split_levels"] > 0, f"{name}: no group level took k_sn_panel<false> + k_sn_syrk: {info}"
    if expect.get("outer"):
        assert info["task0_outer"] > 0, f"{name}: k_chol_update_outer had nothing to do: {info}"
    if "max_run_rows" in expect:
        assert info["max_rows_below"] == expect["max_run_rows"], info


def device_case(ctx, name, with_fixed, mode, expect, fuse_max=SN_FUSE_MAX):
    """One case on the device in one mode (bit 0: fused first forward substitution, bit 1: fp32 sweeps) under every assertion;
    returns a line of the measured figures"""
    case = CASES[name]
    pb = problem(name, with_fixed)
    res = ctx.selftest_chol(pb.rowptr, pb.colidx, pb.val, pb.r, origin=case.origin, fixed=pb.fixed, pose_seg=pb.pose_seg, nseg=case.nseg, mode=mode)
    info = res["info"]
    fp32 = bool(mode & 2)
    e = pb.error(res["z"])
    line = (f"{name}{' +fixed' if with_fixed else ''} mode {mode}: e {np.max(e):.2e} (LAPACK {'fp32 factor' if fp32 else 'fp64'} "
            f"{np.max(pb.lapack_e32 if fp32 else pb.lapack_e):.2e})")
    print(line, "| per right-hand side", e, "|", info, flush=True)
    check_structure(name, info, expect, fuse_max)
    llt, bar, dinv = check_factor(pb, res)
    check_solves(pb, res, fp32)
    dot = check_dot(pb, res, case.nseg)
    return line + f", max|L L^T - S^| {llt:.2e} (bar {bar:.2e}), max|Dinv L_jj - I| {dinv:.2e}, r.z at {dot:.2f} of its bar"


def child_main(setting):
    """The SWITCH_CASES in every mode under the switches of SWITCHES[setting], which the parent has put in the environment"""
    import os

    from linearsfm_amd import api
    env, expect = SWITCHES[setting]
    assert all(os.environ.get(k) == v for k, v in env.items())
    fuse_max = int(env.get("LSFM_SN_FUSE_MAX", SN_FUSE_MAX))
    ctx = api.Context(0)
    try:
        for name in SWITCH_CASES:
            for mode in MODES:
                print(device_case(ctx, name, False, mode, expect[name], fuse_max), flush=True)
    finally:
        ctx.close()
    print("chol child ok")
