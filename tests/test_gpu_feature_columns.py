"""-m gpu: lsfm_map_covariance_feature_columns (csrc/lsfm_featcols.hip) -- whole columns of Sigma = I^-1 for chosen features, three
columns per feature through the sweeps and the refinement of lsfm_map_covariance_columns.  No reference counterpart: the expected
values come from a dense numpy inverse of the whole I on the small sets, and from lsfm_map_covariance_columns where the two overlap.

Metric: |dSigma_ij| / sqrt(Sigma_ii Sigma_jj), bar 1e-9 flat."""
import ctypes as C

import numpy as np
import pytest

from linearsfm_amd import api, synth
from test_gpu_covariance import BAR, SMALL, _fixed, _small_set, _tree_map, dense_sigma
from test_gpu_cov_columns import _err

pytestmark = pytest.mark.gpu
CHUNK = 64  # features per chunk of the device code (lsfm_featcols.hip FC_KC)
_SETS = {}


def small(ctx, i):
    """The tree's map of SMALL[i] and its dense Sigma, computed once for every test of this module and of test_gpu_feature_gate.py."""
    if i not in _SETS:
        mono, n, kw = SMALL[i]
        G = _tree_map(ctx, _small_set(mono, n, kw), mono)
        _SETS[i] = (mono, G, dense_sigma(G, mono))
    return _SETS[i]


def _check_columns(out, feats, G, Sig, what):
    m, nf = int(G["m"]), int(G["n"])
    var = np.diag(Sig)
    vP, vF = var[: 6 * m], var[6 * m:]
    worst_p = worst_f = 0.0
    for a, f in enumerate(feats):
        cols = slice(6 * m + 3 * f, 6 * m + 3 * f + 3)
        worst_p = max(worst_p, _err(out["pose"][a].reshape(-1, 3), Sig[: 6 * m, cols], vP, vF[3 * f: 3 * f + 3]))
        worst_f = max(worst_f, _err(out["feature"][a].reshape(-1, 3), Sig[6 * m:, cols], vF, vF[3 * f: 3 * f + 3]))
    print(f"{what}: k {len(feats)}, steps {out['steps']}, pose rows {worst_p:.2e}, feature rows {worst_f:.2e}, last_corr {out['last_corr'].max():.1e}")
    assert worst_p < BAR and worst_f < BAR
    return vF


# ---- 1. columns against the dense inverse ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SMALL)))
def test_small_sets_vs_dense_inverse(ctx, i):
    """Every pose row and every feature row (the requested feature's own diagonal block included) of the columns of all features
    (n <= 130) or of a seeded sample of 130 = 64 + 64 + 2: two full chunks and a last chunk of 6 columns.  joint: Sigma_FF within the
    bar, exactly symmetric, with a Cholesky factor."""
    mono, G, Sig = small(ctx, i)
    m, nf = int(G["m"]), int(G["n"])
    feats = np.arange(nf) if nf <= 130 else np.sort(np.random.default_rng(1).choice(nf, size=130, replace=False))
    out = ctx.covariance_feature_columns(G, mono, feats, features=True, joint=True)
    k = len(feats)
    assert out["pose"].shape == (k, m, 6, 3) and out["feature"].shape == (k, nf, 3, 3) and out["joint"].shape == (3 * k, 3 * k)
    assert out["converged"]
    vF = _check_columns(out, feats, G, Sig, f"small {SMALL[i][:2]}")
    fx = _fixed(G, mono).reshape(-1, 6)
    assert not out["pose"][:, fx].any()  # the gauge rows are exactly zero
    frow = (6 * m + 3 * feats[:, None] + np.arange(3)[None]).ravel()
    J = out["joint"]
    vQ = vF[frow - 6 * m]
    assert _err(J, Sig[np.ix_(frow, frow)], vQ, vQ) < BAR
    assert np.array_equal(J, J.T)
    np.linalg.cholesky(J)


@pytest.mark.parametrize("k", [1, CHUNK, CHUNK + 1])
def test_chunk_edges(ctx, k):
    """One feature, exactly a chunk, a chunk and one: the 40-map Mono set."""
    mono, G, Sig = small(ctx, 7)
    feats = np.random.default_rng(k).choice(int(G["n"]), size=k, replace=False)
    out = ctx.covariance_feature_columns(G, mono, feats, features=True, joint=True)
    _check_columns(out, feats, G, Sig, f"chunk edge k={k}")
    assert np.array_equal(out["joint"], out["joint"].T)
    for a in range(k):  # a joint block off the diagonal is the feature row of the column it was taken from
        for b in range(a + 1, min(k, a + 3)):
            assert np.array_equal(out["joint"][3 * a: 3 * a + 3, 3 * b: 3 * b + 3], out["feature"][b, feats[a]])


# ---- 2. against lsfm_map_covariance_columns ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [3, 6])
def test_against_pose_columns(ctx, i):
    """Sigma_{p, f} from the feature's columns is the transpose of Sigma_{f, p} from the pose's columns."""
    mono, G, Sig = small(ctx, i)
    m, nf = int(G["m"]), int(G["n"])
    rng = np.random.default_rng(3)
    poses = np.sort(rng.choice(m, size=min(m, 12), replace=False))
    feats = rng.choice(nf, size=min(nf, 20), replace=False)
    pc = ctx.covariance_columns(G, mono, poses, features=True)["feature"]  # [kp, n, 3, 6]
    fc = ctx.covariance_feature_columns(G, mono, feats)["pose"]            # [kf, m, 6, 3]
    var = np.diag(Sig)
    worst = 0.0
    for a, f in enumerate(feats):
        for b, p in enumerate(poses):
            worst = max(worst, _err(fc[a, p], pc[b, f].T, var[6 * p: 6 * p + 6], var[6 * m + 3 * f: 6 * m + 3 * f + 3]))
    print(f"feature columns vs pose columns {SMALL[i][:2]}: {worst:.2e}")
    assert worst < BAR


# ---- 7. arguments and statuses ---------------------------------------------------------------------------------------------------------
def test_arguments(ctx):
    mono, G, _ = small(ctx, 6)
    nf = int(G["n"])
    raw = ctx.covariance_feature_columns_raw
    assert raw(G, mono, [0, 1])[0] == 0
    for bad in ([], [nf], [-1], [1, 2, 1]):  # k < 1, out of range, repeated
        rc, pose, feat, jt, steps, _, _ = raw(G, mono, bad, features=True, joint=True)
        assert rc == -1 and steps == 0, bad
        assert not pose.any() and not feat.any() and not jt.any()
    h = api.HostMap(G)
    q = np.array([0], np.int32)
    rc = api.lib().lsfm_map_covariance_feature_columns(ctx._h, C.byref(h.c), 1, q.ctypes.data_as(C.POINTER(C.c_int)), 1, None, None, None, None, None)
    assert rc == -1  # all outputs NULL
    bad = dict(G); bad["Ref"] = 10 ** 6
    assert raw(bad, mono, [0])[0] == -1  # what lsfm_map_covariance refuses
    # a tree run on the same context afterwards
    G2 = _tree_map(ctx, _small_set(*SMALL[6]), True)
    assert np.array_equal(G2["stno"], G["stno"])


def test_not_positive_definite(ctx):
    """The indefinite map of test_gpu_covariance.test_not_positive_definite: the same status, the outputs untouched."""
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
    ref_rc = ctx.covariance_columns_raw(d, False, [0])[0]
    rc, pose, feat, jt, steps, _, _ = ctx.covariance_feature_columns_raw(d, False, [0, 1], features=True, joint=True)
    assert rc == ref_rc == -7 and steps == 0, (rc, ref_rc)  # LSFM_ERR_NOT_SPD
    assert not pose.any() and not feat.any() and not jt.any()
    rc, d2, cov, steps, _, _ = ctx.feature_pair_gate_raw(d, False, [[0, 1]])
    assert rc == -7 and steps == 0 and not d2.any() and not cov.any()


def test_settings_do_not_apply(ctx):
    """lsfm_set_precision(1) and lsfm_set_small_solve(16) change the results by less than the bar."""
    mono, G, Sig = small(ctx, 2)
    m = int(G["m"])
    feats = [0, 5, 9]
    a = ctx.covariance_feature_columns(G, mono, feats, features=True)
    ctx.set_precision(True)
    ctx.set_small_solve(16)
    try:
        b = ctx.covariance_feature_columns(G, mono, feats, features=True)
    finally:
        ctx.set_precision(False)
        ctx.set_small_solve(5)
    var = np.diag(Sig)
    for i, f in enumerate(feats):
        vQ = var[6 * m + 3 * f: 6 * m + 3 * f + 3]
        assert _err(a["pose"][i].reshape(-1, 3), b["pose"][i].reshape(-1, 3), var[: 6 * m], vQ) < BAR
        assert _err(a["feature"][i].reshape(-1, 3), b["feature"][i].reshape(-1, 3), var[6 * m:], vQ) < BAR
