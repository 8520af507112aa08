"""-m gpu: lsfm_map_feature_pair_gate (csrc/lsfm_featcols.hip) -- Sigma_d = Var(x_f - x_g) with the cross-covariance, and the gate
d^2 = (x_f - x_g)^T Sigma_d^-1 (x_f - x_g), three columns per pair.  No reference counterpart: the expected values are read off a dense
numpy inverse of the whole I (route A of feature_cov_reference.py; the floor between the two host routes: test_feature_columns_cpu.py).

Bars: Sigma_d within 1e-9 normalised by diag(Sigma_ff + Sigma_gg); d^2 within 3 kappa_c rho 1e-9 relative, the first-order propagation
of that bar (feature_cov_reference.d2_bars), which may not exceed 1e-3 on any tested pair.  The error normalised by Sigma_d's own
diagonal is printed, not asserted."""
import numpy as np
import pytest

import feature_cov_reference as ref
from test_gpu_covariance import BAR, SMALL
from test_gpu_feature_columns import small

pytestmark = pytest.mark.gpu
CHUNK = 64  # pairs per chunk of the device code


def _check_gate(ctx, mono, G, Sig, pairs, what):
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    out = ctx.feature_pair_gate(G, mono, pairs)
    covA, marg = ref.route_a(Sig, G, pairs)
    dA = ref.d2_of(covA, ref.state_diff(G, pairs))
    bars = ref.d2_bars(covA, marg)
    e_marg = ref.cov_err(out["cov_diff"], covA, np.einsum("kii->ki", marg))
    e_own = ref.cov_err(out["cov_diff"], covA, np.einsum("kii->ki", covA))
    rel = np.abs(out["d2"] - dA) / dA
    print(f"gate {what}: {len(pairs)} pairs, steps {out['steps']}, Sigma_d error / marginals {e_marg:.2e}, / own diagonal {e_own:.2e}, "
          f"d2 rel {rel.max():.2e} (largest bar {bars.max():.2e}), last_corr {out['last_corr'].max():.1e}")
    assert out["converged"]
    assert bars.max() < ref.BAR_D2_CAP
    assert e_marg < BAR
    assert np.all(rel < bars), (rel / bars).max()
    assert np.array_equal(out["cov_diff"], np.transpose(out["cov_diff"], (0, 2, 1)))
    return out


# ---- 3. the gate against the dense inverse -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SMALL)))
def test_small_sets_vs_dense_inverse(ctx, i):
    """200 seeded pairs (all pairs where there are fewer); the 1-map Stereo set: runs of one block."""
    mono, G, Sig = small(ctx, i)
    _check_gate(ctx, mono, G, Sig, ref.seeded_pairs(int(G["n"])), f"small {SMALL[i][:2]}")


# ---- 4. the gate equals the joint of the two features' columns ---------------------------------------------------------------------------
@pytest.mark.parametrize("i", [2, 6])
def test_gate_equals_joint(ctx, i):
    mono, G, Sig = small(ctx, i)
    o = 6 * int(G["m"])
    worst = 0.0
    for f, g in ref.seeded_pairs(int(G["n"]))[:6]:
        J = ctx.covariance_feature_columns(G, mono, [f, g], joint=True)["joint"]
        cov = ctx.feature_pair_gate(G, mono, [[f, g]])["cov_diff"][0]
        marg = np.diag(Sig)[o + 3 * f: o + 3 * f + 3] + np.diag(Sig)[o + 3 * g: o + 3 * g + 3]
        worst = max(worst, ref.cov_err((J[:3, :3] + J[3:, 3:] - J[:3, 3:] - J[3:, :3])[None], cov[None], marg[None]))
    print(f"gate vs joint {SMALL[i][:2]}: {worst:.2e}")
    assert worst < BAR


# ---- 5. shapes that can go wrong -----------------------------------------------------------------------------------------------------------
def _designed_pairs(G, mono):
    """One feature in three pairs, a pair in both orders, the pair with the fewest and the pair with the most common poses (in these
    small worlds some pose sees every feature: no pair is without a common pose; the far pairs of a larger set: test_far_pairs_vs_sparse_lu);
    Mono: a feature the scale pose sees against one it does not, and two such features; the same for the reference pose."""
    n = int(G["n"])
    ph, fe = np.asarray(G["photo"]), np.asarray(G["feature"])
    seen = [set(ph[fe == f]) for f in range(n)]
    common = {(f, g): len(seen[f] & seen[g]) for f in range(n) for g in range(f + 1, n)}
    few, many = min(common, key=common.get), max(common, key=common.get)
    pairs = [few, many, (few[1], few[0]), (few[0], many[1]), (few[0], n - 1), (n - 1, few[0])]
    if mono:
        ids = -np.asarray(G["stno"])[: 6 * int(G["m"]): 6]
        ps = int(np.nonzero(ids == G["ScaP"])[0][0])
        sf = [f for f in range(n) if ps in seen[f]]
        far = [f for f in range(n) if ps not in seen[f]]
        assert len(sf) >= 2
        pairs += [(sf[0], sf[1]), (sf[1], sf[0])] + ([(sf[0], far[-1])] if far else [])
        # ... and the reference pose, all six of whose scalars are fixed: every row of its W blocks drops out of the right-hand side
        pr = int(np.nonzero(ids == G["Ref"])[0][0])
        rf = [f for f in range(n) if pr in seen[f]]
        nr = [f for f in range(n) if pr not in seen[f]]
        assert len(rf) >= 2
        pairs += [(rf[0], rf[-1]), (rf[-1], rf[0])] + ([(rf[0], nr[-1]), (nr[0], rf[-1])] if nr else [])
    return [p for p in pairs if p[0] != p[1]]


@pytest.mark.parametrize("i", [3, 7])
def test_designed_pairs(ctx, i):
    mono, G, Sig = small(ctx, i)
    pairs = _designed_pairs(G, mono)
    out = _check_gate(ctx, mono, G, Sig, pairs, f"designed {SMALL[i][:2]}")
    assert np.all(np.isfinite(out["d2"])) and np.all(out["d2"] > 0)


@pytest.mark.parametrize("K", [1, CHUNK, CHUNK + 1])
def test_chunk_edges(ctx, K):
    mono, G, Sig = small(ctx, 3)
    _check_gate(ctx, mono, G, Sig, ref.seeded_pairs(int(G["n"]))[:K], f"chunk edge K={K}")


@pytest.mark.parametrize("i", [2, 6])
def test_repeated_block(ctx, i):
    """A map whose chosen feature's W block to one pose is stored as two adjacent halves gives the unsplit map's columns and d^2."""
    mono, G, Sig = small(ctx, i)
    m, n = int(G["m"]), int(G["n"])
    f, g = n // 2, n // 3
    Gs = ref.split_block(G, f)
    assert len(Gs["photo"]) == len(G["photo"]) + 1
    _check_gate(ctx, mono, Gs, Sig, [(f, g), (g, f), (f, 0)], f"repeated block {SMALL[i][:2]}")
    a = ctx.covariance_feature_columns(G, mono, [f, g], features=True)
    b = ctx.covariance_feature_columns(Gs, mono, [f, g], features=True)
    var = np.diag(Sig)
    from test_gpu_cov_columns import _err
    for c, h in enumerate((f, g)):
        vQ = var[6 * m + 3 * h: 6 * m + 3 * h + 3]
        assert _err(a["pose"][c].reshape(-1, 3), b["pose"][c].reshape(-1, 3), var[: 6 * m], vQ) < BAR
        assert _err(a["feature"][c].reshape(-1, 3), b["feature"][c].reshape(-1, 3), var[6 * m:], vQ) < BAR


# ---- 7. arguments ---------------------------------------------------------------------------------------------------------------------------
def test_arguments(ctx):
    import ctypes as C
    from linearsfm_amd import api
    mono, G, _ = small(ctx, 6)
    n = int(G["n"])
    raw = ctx.feature_pair_gate_raw
    assert raw(G, mono, [[0, 1], [1, 0], [0, 2]])[0] == 0  # a feature may occur in several pairs
    for bad in ([], [[0, n]], [[-1, 0]], [[3, 3]]):  # K < 1, out of range, f == g
        rc, d2, cov, steps, _, _ = raw(G, mono, bad)
        assert rc == -1 and steps == 0, bad
        assert not d2.any() and not cov.any()
    h = api.HostMap(G)
    q = np.array([0, 1], np.int32)
    assert api.lib().lsfm_map_feature_pair_gate(ctx._h, C.byref(h.c), 1, q.ctypes.data_as(C.POINTER(C.c_int)), 1, None, None, None, None) == -1
    # d2 alone and cov_diff alone give what the two together give
    both = raw(G, mono, [[0, 1]])
    assert raw(G, mono, [[0, 1]], cov=False)[2] is None and raw(G, mono, [[0, 1]], d2=False)[1] is None
    assert np.allclose(raw(G, mono, [[0, 1]], cov=False)[1], both[1], rtol=1e-6) and np.allclose(raw(G, mono, [[0, 1]], d2=False)[2], both[2], rtol=1e-6)


def test_settings_do_not_apply(ctx):
    mono, G, Sig = small(ctx, 2)
    pairs = ref.seeded_pairs(int(G["n"]))[:8]
    a = ctx.feature_pair_gate(G, mono, pairs)
    ctx.set_precision(True)
    ctx.set_small_solve(16)
    try:
        b = ctx.feature_pair_gate(G, mono, pairs)
    finally:
        ctx.set_precision(False)
        ctx.set_small_solve(5)
    _, marg = ref.route_a(Sig, G, pairs)
    assert ref.cov_err(a["cov_diff"], b["cov_diff"], np.einsum("kii->ki", marg)) < BAR



# ---- 6. mid-size, against a reference that owes nothing to the dense inverse ---------------------------------------------------------------
def _far_pairs(ctx, G, count=64, lap=60):
    """Pairs of features of the 512-map Stereo set that are as far apart as that set allows.  Its root pose sees every feature, so no
    pair is without a common pose.  Chosen (photo / feature, lsfm_schur_pattern; 4000 seeded draws, the first `count` that qualify):
    the root pose is the ONLY common pose; every other pose of f is at least a lap (60 labels) from every other pose of g; and of the
    pose pairs (p in P(f), q in P(g)) beside the common pose at most 2 are on the pattern of S -- the other Sigma_pq the cross term needs
    are off-pattern blocks.  Returns the pairs and, for the record, the share of those pose pairs that is off the pattern."""
    import scipy.sparse as sp
    m, n = int(G["m"]), int(G["n"])
    ph, fe = np.asarray(G["photo"]), np.asarray(G["feature"])
    ids = -np.asarray(G["stno"])[: 6 * m: 6]
    rowptr, colidx = ctx.schur_pattern(G)
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    A = sp.csr_matrix((np.ones(len(colidx)), (rows, colidx)), shape=(m, m))
    A = (A + A.T).tocsr()
    fptr = np.searchsorted(fe, np.arange(n + 1))
    poses = lambda f: np.unique(ph[fptr[f]: fptr[f + 1]])
    rng = np.random.default_rng(6)
    pairs, on, total = [], 0, 0
    for _ in range(4000):
        f, g = rng.choice(n, size=2, replace=False)
        common = np.intersect1d(poses(f), poses(g))
        a, b = np.setdiff1d(poses(f), common), np.setdiff1d(poses(g), common)
        if len(common) != 1 or not len(a) or not len(b) or np.abs(ids[a][:, None] - ids[b][None, :]).min() < lap:
            continue
        links = A[a][:, b].nnz
        if links > 2:
            continue
        pairs.append((f, g)); on += links; total += len(a) * len(b)
        if len(pairs) == count:
            break
    assert len(pairs) == count, len(pairs)
    return np.array(pairs, np.int32), 1.0 - on / total


def test_far_pairs_vs_sparse_lu(ctx):
    """stereo512, 64 far pairs (_far_pairs) against scipy's sparse LU of S with one refinement step, as test_gpu_cov_columns.py.  Floor
    first: two such LUs with different orderings agree on Sigma_d < 1e-10 in both normalisations.  Then the bars of the small sets:
    Sigma_d within 1e-9 of the marginals' diagonal, d2 within its derived bar, no bar above 1e-3."""
    import scipy.sparse.linalg as spla
    from test_gpu_covariance import LARGE, _sparse_parts, _tree_map
    mono, make = LARGE["stereo512"]
    G = _tree_map(ctx, make(), mono)
    pairs, off_share = _far_pairs(ctx, G)
    Usp, Wsp, _, IVsp, IV = _sparse_parts(G)
    S = (Usp - Wsp @ IVsp @ Wsp.T).tocsc()
    WIV = (Wsp @ IVsp).tocsc()
    feats = np.unique(pairs)
    at = {int(f): i for i, f in enumerate(feats)}
    col = lambda f: WIV[:, 3 * f: 3 * f + 3].toarray()
    Bd = np.concatenate([-(col(f) - col(g)) for f, g in pairs], axis=1)   # the pairs' right-hand sides
    Bm = np.concatenate([-col(f) for f in feats], axis=1)                 # ... and the single features', for the marginals
    B = np.concatenate([Bd, Bm], axis=1)
    o = Bd.shape[1]
    sols = []
    for spec in ("COLAMD", "MMD_AT_PLUS_A"):
        lu = spla.splu(S, permc_spec=spec)
        X = lu.solve(B)
        X += lu.solve(B - S @ X)  # one step of iterative refinement
        cov = np.stack([IV[f] + IV[g] + Bd[:, 3 * a: 3 * a + 3].T @ X[:, 3 * a: 3 * a + 3] for a, (f, g) in enumerate(pairs)])
        mf = np.stack([IV[f] + Bm[:, 3 * i: 3 * i + 3].T @ X[:, o + 3 * i: o + 3 * i + 3] for i, f in enumerate(feats)])
        sols.append((0.5 * (cov + np.transpose(cov, (0, 2, 1))), mf))
    (cov, mf), (cov2, _) = sols
    marg = np.stack([mf[at[int(f)]] + mf[at[int(g)]] for f, g in pairs])
    dm, do = np.einsum("kii->ki", marg), np.einsum("kii->ki", cov)
    floor = max(ref.cov_err(cov2, cov, dm), ref.cov_err(cov2, cov, do))
    assert floor < 1e-10, floor
    out = ctx.feature_pair_gate(G, mono, pairs)
    dA = ref.d2_of(cov, ref.state_diff(G, pairs))
    bars = ref.d2_bars(cov, marg)
    e_marg, e_own = ref.cov_err(out["cov_diff"], cov, dm), ref.cov_err(out["cov_diff"], cov, do)
    rel = np.abs(out["d2"] - dA) / dA
    print(f"gate stereo512 far pairs: {100 * off_share:.1f} % of the pose pairs off the pattern, floor {floor:.2e}, steps {out['steps']}, "
          f"Sigma_d error / marginals {e_marg:.2e}, / own diagonal {e_own:.2e}, d2 rel {rel.max():.2e} (largest bar {bars.max():.2e}), "
          f"smallest diag(Sigma_d) / diag(marginals) {float((do / dm).min()):.2e}")
    assert out["converged"]
    assert bars.max() < ref.BAR_D2_CAP
    assert e_marg < BAR and np.all(rel < bars)
    # the columns of the same features: pose rows and the joint against the same solves
    k = min(len(feats), 70)  # a full chunk and a part of one
    fc = ctx.covariance_feature_columns(G, mono, feats[:k], joint=True)
    vP = np.einsum("kii->ki", ctx.covariance(G, mono)["pose"]).ravel()  # (normaliser only)
    from test_gpu_cov_columns import _err
    worst = max(_err(fc["pose"][i].reshape(-1, 3), X[:, o + 3 * i: o + 3 * i + 3], vP, np.diag(mf[i])) for i in range(k))
    Jd = np.stack([fc["joint"][3 * i: 3 * i + 3, 3 * i: 3 * i + 3] for i in range(k)])
    ej = ref.cov_err(Jd, mf[:k], np.einsum("kii->ki", mf[:k]))
    print(f"columns stereo512: {k} features, pose rows {worst:.2e}, own blocks of the joint {ej:.2e}")
    assert worst < BAR and ej < BAR
