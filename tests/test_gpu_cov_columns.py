"""-m gpu: lsfm_map_covariance_columns (csrc/lsfm_covcols.hip) -- whole columns of Sigma = I^-1 for chosen poses, solved side by side
against the camera system's factor and refined in fp64.  No reference counterpart: the expected values come from host linear algebra
(a dense numpy inverse of the whole I on the small sets, scipy's sparse LU of the camera system with one refinement step on the larger
ones), from the library's own single right-hand-side solve, and from lsfm_map_covariance where the two overlap.

Metric: |dSigma_ij| / sqrt(Sigma_ii Sigma_jj), bar 1e-9 FLAT -- no u kappa allowance (test_gpu_covariance.py needs one on the same sets)."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

from linearsfm_amd import synth
from test_gpu_covariance import BAR, LARGE, SMALL, _fixed, _kappa, _norm_err, _small_set, _sparse_parts, _tree_map, dense_sigma, schur_sigma

pytestmark = pytest.mark.gpu
CHUNK = 32  # poses per chunk of the device code (lsfm_covcols.hip CC_KC)


def _err(got, exp, vr, vc):
    """max |got - exp| / sqrt(vr_i vc_j) for matrices [rows, cols] with the variances of their rows / columns (0: gauge)."""
    den = np.sqrt(np.maximum(vr[:, None] * vc[None, :], 1e-300))
    return float(np.max(np.abs(got - exp) / den)) if got.size else 0.0


def _pose_matrix(pose, a):
    """pose_cols [k, m, 6, 6] -> the [6 m, 6] column block of requested pose a."""
    return pose[a].reshape(-1, 6)


def _feat_matrix(feat, a):
    return feat[a].reshape(-1, 6)


# ---- 1. small sets against a dense inverse ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mono,n,kw", SMALL)
def test_small_sets_vs_dense_inverse(ctx, mono, n, kw):
    """Every block of Sigma_pp (off-pattern included) and of Sigma_fp with poses = all m, against a dense inverse of the whole I; the
    floor (dense vs host Schur route < 1e-10) first, as test_gpu_covariance.py.  joint: the dense Sigma_pp, exactly symmetric, with a
    Cholesky factor once the gauge rows are dropped."""
    G = _tree_map(ctx, _small_set(mono, n, kw), mono)
    m, nf = int(G["m"]), int(G["n"])
    Sig = dense_sigma(G, mono)
    Sp, Fs = schur_sigma(G, mono)
    var = np.diag(Sig)
    vP, vF = var[: 6 * m], var[6 * m:]
    P = np.stack([Sig[6 * p: 6 * p + 6, 6 * p: 6 * p + 6] for p in range(m)])
    F = np.stack([Sig[6 * m + 3 * f: 6 * m + 3 * f + 3, 6 * m + 3 * f: 6 * m + 3 * f + 3] for f in range(nf)])
    dP, dF = np.einsum("kii->ki", P), np.einsum("kii->ki", F)
    floor = max(_norm_err(np.stack([Sp[6 * p: 6 * p + 6, 6 * p: 6 * p + 6] for p in range(m)]), P, dP, dP), _norm_err(Fs, F, dF, dF))
    assert floor < 1e-10, floor
    out = ctx.covariance_columns(G, mono, np.arange(m), features=True, joint=True)
    assert out["pose"].shape == (m, m, 6, 6) and out["feature"].shape == (m, nf, 3, 6) and out["joint"].shape == (6 * m, 6 * m)
    worst_p = worst_f = 0.0
    for a in range(m):
        worst_p = max(worst_p, _err(_pose_matrix(out["pose"], a), Sig[: 6 * m, 6 * a: 6 * a + 6], vP, vP[6 * a: 6 * a + 6]))
        worst_f = max(worst_f, _err(_feat_matrix(out["feature"], a), Sig[6 * m:, 6 * a: 6 * a + 6], vF, vP[6 * a: 6 * a + 6]))
    print(f"small mono={mono} n={n}: floor {floor:.2e}, steps {out['steps']}, pose {worst_p:.2e}, feature {worst_f:.2e}, last_corr {out['last_corr'].max():.1e}")
    assert worst_p < BAR and worst_f < BAR
    J = out["joint"]
    assert _err(J, Sig[: 6 * m, : 6 * m], vP, vP) < BAR
    assert np.array_equal(J, J.T)
    free = ~_fixed(G, mono)
    assert not J[~free].any() and not J[:, ~free].any()
    np.linalg.cholesky(J[np.ix_(free, free)])


# ---- 2. larger sets against the refined sparse LU -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stereo512", "mono200", "nc3500"])
def test_larger_sets_vs_sparse_lu(ctx, name):
    """16 requested poses (fixed seed; Mono: a gauge pose among them) against scipy's sparse LU of S (gauge removed) with one step of
    iterative refinement.  Floor: two such LUs with different orderings agree < 1e-10 over all compared rows.  Variances: a dense inverse
    of S on the two smaller sets (a normaliser only); on nc3500 a fixed sample of 64 row poses whose variances come from reference solves.
    Feature rows: up to 8 features per requested pose and 200 random ones.  Prints floor, kappa, steps and errors, and -- not asserted --
    how far lsfm_map_covariance's pair blocks are from the same reference on the same columns."""
    mono, make = LARGE[name]
    G = _tree_map(ctx, make(), mono)
    m, nf = int(G["m"]), int(G["n"])
    Usp, Wsp, Vsp, IVsp, IV = _sparse_parts(G)
    fx = _fixed(G, mono)
    keep = ~fx
    kidx = np.nonzero(keep)[0]
    S = (Usp - Wsp @ IVsp @ Wsp.T).tocsc()[kidx][:, kidx].tocsc()
    lus = [spla.splu(S, permc_spec=spec) for spec in ("COLAMD", "MMD_AT_PLUS_A")]

    def solve(B, lu):
        X = np.zeros((6 * m, B.shape[1]))
        Bk = np.ascontiguousarray(B[kidx])
        x = lu.solve(Bk)
        x += lu.solve(Bk - S @ x)  # one step of iterative refinement
        X[kidx] = x
        return X

    def unit(poses):
        E = np.zeros((6 * m, 6 * len(poses)))
        for a, j in enumerate(poses):
            E[6 * j: 6 * j + 6, 6 * a: 6 * a + 6] = np.eye(6)
        E[fx] = 0
        return E

    rng = np.random.default_rng(17)
    req = rng.choice(m, size=16, replace=False)
    if mono:
        ids = -np.asarray(G["stno"])[: 6 * m: 6]
        pr = int(np.nonzero(ids == G["Ref"])[0][0])
        if pr not in req:
            req[0] = pr
    X, X2 = solve(unit(req), lus[0]), solve(unit(req), lus[1])
    # which pose rows are compared, and the variances of all pose scalars that takes
    if name == "nc3500":
        rows_p = np.unique(np.concatenate([req, rng.choice(m, size=64, replace=False)]))
        extra = np.setdiff1d(rows_p, req)
        Xe = solve(unit(extra), lus[0])
        vP = np.zeros(6 * m)
        for a, j in enumerate(req):
            vP[6 * j: 6 * j + 6] = np.diag(X[6 * j: 6 * j + 6, 6 * a: 6 * a + 6])
        for a, j in enumerate(extra):
            vP[6 * j: 6 * j + 6] = np.diag(Xe[6 * j: 6 * j + 6, 6 * a: 6 * a + 6])
    else:
        rows_p = np.arange(m)
        vP = np.zeros(6 * m)
        vP[kidx] = np.diag(np.linalg.inv(S.toarray()))
    srow = (6 * rows_p[:, None] + np.arange(6)[None]).ravel()
    vQ = np.concatenate([vP[6 * j: 6 * j + 6] for j in req])
    # feature rows: up to 8 features of every requested pose and 200 random ones
    ph, fe = np.asarray(G["photo"]), np.asarray(G["feature"])
    feats = np.unique(np.concatenate([np.unique(fe[ph == j])[:8] for j in req] + [rng.choice(nf, size=min(nf, 200), replace=False)]))
    frow = (3 * feats[:, None] + np.arange(3)[None]).ravel()
    Gm = (IVsp @ Wsp.T).tocsr()[frow]           # V^-1 W^T of the sampled features
    XF, XF2 = -(Gm @ X), -(Gm @ X2)             # Sigma_{f,Q}
    Z = solve(np.ascontiguousarray(Gm.T.toarray()), lus[0])
    vF = np.array([IV[f][i, i] for f in feats for i in range(3)]) + np.einsum("ij,ji->i", Gm.toarray(), Z)
    floor_p, floor_f = _err(X[srow], X2[srow], vP[srow], vQ), _err(XF, XF2, vF, vQ)
    assert max(floor_p, floor_f) < 1e-10, (floor_p, floor_f)
    kappa = _kappa(S, lus[0])
    out = ctx.covariance_columns(G, mono, req, features=True, joint=True)
    got_p = np.concatenate([_pose_matrix(out["pose"], a) for a in range(len(req))], axis=1)
    got_f = np.concatenate([_feat_matrix(out["feature"], a) for a in range(len(req))], axis=1)
    err_p, err_f = _err(got_p[srow], X[srow], vP[srow], vQ), _err(got_f[frow], XF, vF, vQ)
    # the selected inversion's pair blocks on the same columns, for the record
    cov = ctx.covariance(G, mono, pairs=True)
    rowptr, colidx, blocks = cov["pairs"]
    brow = np.repeat(np.arange(m), np.diff(rowptr))
    sel = 0.0
    for a, j in enumerate(req):
        for s_ in np.nonzero(colidx == j)[0]:
            p = brow[s_]
            sel = max(sel, _err(blocks[s_], X[6 * p: 6 * p + 6, 6 * a: 6 * a + 6], np.diag(cov["pose"][p]), vQ[6 * a: 6 * a + 6]))
    print(f"{name}: m {m}, n {nf}, kappa(S) {kappa:.2e}, floor pose {floor_p:.2e} feature {floor_f:.2e}, steps {out['steps']}, "
          f"last_corr {out['last_corr'].max():.1e}, columns error pose {err_p:.2e} feature {err_f:.2e} (bar {BAR:.0e}); "
          f"lsfm_map_covariance pair blocks on the same columns {sel:.2e}")
    assert err_p < BAR and err_f < BAR, (err_p, err_f, floor_p, floor_f, kappa)
    J = out["joint"]
    assert np.array_equal(J, J.T)
    if mono:
        a = int(np.nonzero(req == pr)[0][0])
        assert not out["pose"][a].any() and not out["feature"][a].any()


# ---- 3. against the parent's only route: one solve per scalar column ------------------------------------------------------------------
@pytest.mark.parametrize("mono", [False, True])
def test_against_single_solves(ctx, mono):
    """One pose's six columns from Context.solve with unit eP, eF = 0 (Mono: the same gauge) -- six uploads, reductions and
    factorisations -- against the columns call."""
    G = _tree_map(ctx, _small_set(mono, 40, dict(lap=12, home=4, revisit=0.5)), mono)
    m, nf = int(G["m"]), int(G["n"])
    fx = _fixed(G, mono)
    sa = None
    if mono:
        ids = -np.asarray(G["stno"])[: 6 * m: 6]
        pr, ps = int(np.nonzero(ids == G["Ref"])[0][0]), int(np.nonzero(ids == G["ScaP"])[0][0])
        sa = [pr, 6 * pr, 6 * ps + int(G["Fix"]), 0, 0]
    j = m // 2
    assert not fx[6 * j: 6 * j + 6].any()
    cols = np.zeros((6 * m + 3 * nf, 6))
    for c in range(6):
        eP = np.zeros(6 * m)
        eP[6 * j + c] = 1.0
        st, rc = ctx.solve(G, eP, np.zeros(3 * nf), mono, sa)
        assert rc == 0
        cols[:, c] = st
    out = ctx.covariance_columns(G, mono, [j], features=True)
    Sig = dense_sigma(G, mono)  # (the variances only)
    var = np.diag(Sig)
    vQ = var[6 * j: 6 * j + 6]
    ep = _err(_pose_matrix(out["pose"], 0), cols[: 6 * m], var[: 6 * m], vQ)
    ef = _err(_feat_matrix(out["feature"], 0), cols[6 * m:], var[6 * m:], vQ)
    print(f"single solves mono={mono}: pose {ep:.2e}, feature {ef:.2e}")
    assert ep < BAR and ef < BAR


# ---- 4. against lsfm_map_covariance where the two overlap ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stereo512(ctx):
    return _tree_map(ctx, LARGE["stereo512"][1](), False)


def test_against_selected_inversion(ctx, stereo512):
    """stereo512 (kappa 6e6): the diagonal blocks of pose_cols and every on-pattern pair block against Context.covariance(pairs=True)."""
    G = stereo512
    m = int(G["m"])
    cov = ctx.covariance(G, False, pairs=True)
    rowptr, colidx, blocks = cov["pairs"]
    brow = np.repeat(np.arange(m), np.diff(rowptr))
    dP = np.einsum("kii->ki", cov["pose"])
    worst = 0.0
    for c0 in range(0, m, 128):
        q = np.arange(c0, min(m, c0 + 128))
        out = ctx.covariance_columns(G, False, q)
        for s_ in np.nonzero((colidx >= q[0]) & (colidx <= q[-1]))[0]:
            p, j = brow[s_], colidx[s_]
            worst = max(worst, _err(out["pose"][j - c0, p], blocks[s_], dP[p], dP[j]))
    print(f"stereo512 vs selected inversion: {worst:.2e}")
    assert worst < BAR


# ---- 5. chunking -------------------------------------------------------------------------------------------------------------------
def test_chunking(ctx, stereo512):
    """3 chunks + 1 poses in one call against the same poses asked one at a time (no bit equality: the sweeps add by atomics)."""
    G = stereo512
    m = int(G["m"])
    k = 3 * CHUNK + 1
    q = np.random.default_rng(5).choice(m, size=k, replace=False)
    out = ctx.covariance_columns(G, False, q, features=True, joint=True)
    cov = ctx.covariance(G, False)
    vP, vF = np.einsum("kii->ki", cov["pose"]).ravel(), np.einsum("kii->ki", cov["feature"]).ravel()
    worst = 0.0
    for a in range(k):
        one = ctx.covariance_columns(G, False, [q[a]], features=True)
        vQ = vP[6 * q[a]: 6 * q[a] + 6]
        worst = max(worst, _err(_pose_matrix(out["pose"], a), _pose_matrix(one["pose"], 0), vP, vQ),
                    _err(_feat_matrix(out["feature"], a), _feat_matrix(one["feature"], 0), vF, vQ))
    print(f"chunking: {worst:.2e}")
    assert worst < BAR
    J = out["joint"]
    assert np.array_equal(J, J.T)
    for a in (0, CHUNK, k - 1):
        for b in (1, 2 * CHUNK + 3):
            if a < b:
                assert np.array_equal(J[6 * a: 6 * a + 6, 6 * b: 6 * b + 6], out["pose"][b, q[a]])


# ---- 6. the precision and small-system switches do not apply ----------------------------------------------------------------------
@pytest.mark.parametrize("which", ["nine_maps", "one_pose"])
def test_settings_do_not_apply(ctx, which):
    if which == "nine_maps":
        G = _tree_map(ctx, _small_set(False, 9, {}), False)
    else:
        G = synth.make_stereo_set(1, 10, 4, seed=8)[0].__dict__
    m = int(G["m"])
    q = np.arange(min(m, 3))
    a = ctx.covariance_columns(G, False, q, features=True)
    ctx.set_precision(True)
    ctx.set_small_solve(16)
    try:
        b = ctx.covariance_columns(G, False, q, features=True)
    finally:
        ctx.set_precision(False)
        ctx.set_small_solve(5)
    var = np.diag(dense_sigma(G, False))
    for i, j in enumerate(q):
        vQ = var[6 * j: 6 * j + 6]
        assert _err(_pose_matrix(a["pose"], i), _pose_matrix(b["pose"], i), var[: 6 * m], vQ) < BAR
        assert _err(_feat_matrix(a["feature"], i), _feat_matrix(b["feature"], i), var[6 * m:], vQ) < BAR


# ---- 7. arguments and statuses -----------------------------------------------------------------------------------------------------
def test_arguments_and_statuses(ctx):
    from linearsfm_amd import api
    import ctypes as C
    maps = synth.make_mono_set(9, 8, 4, seed=5)
    G = _tree_map(ctx, maps, True)
    m = int(G["m"])
    raw = ctx.covariance_columns_raw
    assert raw(G, True, [0, 1])[0] == 0
    assert raw(G, True, [])[0] == -1           # k < 1
    assert raw(G, True, [m])[0] == -1          # out of range
    assert raw(G, True, [-1])[0] == -1
    assert raw(G, True, [1, 2, 1])[0] == -1    # repeated
    # all outputs NULL
    h = api.HostMap(G)
    q = np.array([0], np.int32)
    rc = api.lib().lsfm_map_covariance_columns(ctx._h, C.byref(h.c), 1, q.ctypes.data_as(C.POINTER(C.c_int)), 1, None, None, None, None, None)
    assert rc == -1
    # what lsfm_map_covariance refuses
    bad = dict(G); bad["Ref"] = 10 ** 6
    assert raw(bad, True, [0])[0] == -1
    bad = dict(G)
    perm = np.arange(len(G["photo"]))[::-1]
    bad["W"] = np.asarray(G["W"])[perm]; bad["photo"] = np.asarray(G["photo"])[perm]; bad["feature"] = np.asarray(G["feature"])[perm]
    assert raw(bad, True, [0])[0] == -1
    # the Ref pose's column is all zero, and so are the gauge rows of every other column
    ids = -np.asarray(G["stno"])[: 6 * m: 6]
    pr = int(np.nonzero(ids == G["Ref"])[0][0])
    other = (pr + 1) % m
    out = ctx.covariance_columns(G, True, [pr, other], features=True, joint=True)
    assert not out["pose"][0].any() and not out["feature"][0].any() and out["last_corr"][0] == 0
    assert out["pose"][1].any() and not out["pose"][1, pr].any()
    assert not out["joint"][:6].any() and not out["joint"][:, :6].any()
    assert out["steps"] >= 1
    # a tree run on the same context afterwards
    G2 = _tree_map(ctx, maps, True)
    assert np.array_equal(G2["stno"], G["stno"])


def test_not_positive_definite(ctx):
    """The indefinite map of test_gpu_covariance.test_not_positive_definite: a numerical status, the outputs untouched."""
    G = _tree_map(ctx, synth.make_stereo_set(4, 8, 4, seed=5), False)
    m = int(G["m"])
    d = dict(G)
    d["m"] = m + 1
    d["stno"] = np.concatenate([np.asarray(G["stno"])[: 6 * m], np.full(6, -999, np.int32), np.asarray(G["stno"])[6 * m:]])
    d["stVal"] = np.concatenate([np.asarray(G["stVal"])[: 6 * m], np.zeros(6), np.asarray(G["stVal"])[6 * m:]])
    d["U"] = np.concatenate([np.asarray(G["U"]).reshape(-1, 36), np.zeros((1, 36))])
    d["Ui"] = np.concatenate([np.asarray(G["Ui"]), [m]]).astype(np.int32)
    d["Uj"] = np.concatenate([np.asarray(G["Uj"]), [m]]).astype(np.int32)
    d.pop("pose_origin", None)
    rc, pose, feat, jt, steps, corr, _ = ctx.covariance_columns_raw(d, False, [0, m], features=True, joint=True)
    assert rc == -7 and steps == 0, rc  # LSFM_ERR_NOT_SPD
    assert not pose.any() and not feat.any() and not jt.any()
