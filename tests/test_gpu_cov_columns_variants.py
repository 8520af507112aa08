"""-m gpu: the two versions of lsfm_map_covariance_columns' supernode-group panel product (lsfm_set_covcols_panel: lane per column, and
16x16 tiles on v_mfma_f64_16x16x4_f64) give the same columns, and the context's choice of CG product (lsfm_set_spmv_variant) does not
reach the call.

Both versions are refined in fp64 against S, so each is within the suite's flat bar of the true columns (test_gpu_cov_columns.py holds
the default to it against independent references); what is asked here is that they agree with each other to that bar,
|dSigma_ij| / sqrt(Sigma_ii Sigma_jj) < 1e-9.  Sets: stereo512 and mono200 -- the smallest generators of the suite whose factors have
supernode groups with panels below their runs (runs of 1..8 block columns: 6 s is a multiple of the MFMA's k step of 4 or not; panels
of any number of rows: the last 16-row tile is full or not).  k = 1 (6 columns: one partly filled 16-column tile), 5 (30: a full
and a partly filled tile) and 32 (192: the whole chunk, twelve waves)."""
import numpy as np
import pytest

from test_gpu_covariance import BAR, LARGE, _small_set, _tree_map
from test_gpu_cov_columns import _err, _feat_matrix, _pose_matrix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["stereo512", "mono200"])
def big(request, ctx):
    mono, make = LARGE[request.param]
    G = _tree_map(ctx, make(), mono)
    cov = ctx.covariance_raw(G, mono)  # (the variances only: a normaliser; floored pivots or not, its diagonal is good to 1e-6)
    return request.param, mono, G, np.einsum("kii->ki", cov[1]).ravel(), np.einsum("kii->ki", cov[2]).ravel()


@pytest.mark.parametrize("k", [1, 5, 32])
def test_panel_versions_agree(ctx, big, k):
    name, mono, G, vP, vF = big
    m = int(G["m"])
    q = np.random.default_rng(k).choice(m, size=k, replace=False)
    got = {}
    try:
        for v in (1, 2):
            ctx.set_covcols_panel(v)
            got[v] = ctx.covariance_columns(G, mono, q, features=True, joint=True)
    finally:
        ctx.set_covcols_panel(0)
    worst = 0.0
    for a in range(k):
        vQ = vP[6 * q[a]: 6 * q[a] + 6]
        worst = max(worst, _err(_pose_matrix(got[1]["pose"], a), _pose_matrix(got[2]["pose"], a), vP, vQ),
                    _err(_feat_matrix(got[1]["feature"], a), _feat_matrix(got[2]["feature"], a), vF, vQ))
    print(f"{name} k={k}: plain vs MFMA {worst:.2e}, steps {got[1]['steps']} / {got[2]['steps']}")
    assert got[1]["pose"].any()
    assert worst < BAR
    for v in (1, 2):
        assert got[v]["converged"] and np.array_equal(got[v]["joint"], got[v]["joint"].T)


def test_panel_setting_arguments(ctx):
    from linearsfm_amd import api
    assert api.lib().lsfm_set_covcols_panel(ctx._h, 3) == -1 and api.lib().lsfm_set_covcols_panel(ctx._h, -1) == -1
    assert api.lib().lsfm_set_covcols_panel(ctx._h, 0) == 0


@pytest.mark.parametrize("mono", [False, True])
def test_spmv_variant_does_not_apply(ctx, mono):
    """lsfm_set_spmv_variant(1) leaves the context's systems without the row-sorted list the residual reads: the call builds its own."""
    G = _tree_map(ctx, _small_set(mono, 40, dict(lap=12, home=4, revisit=0.5)), mono)
    m = int(G["m"])
    q = [m // 2, 1]
    a = ctx.covariance_columns(G, mono, q, features=True)
    ctx.set_spmv_variant(1)
    try:
        rc, pose, feat, _, steps, _, _ = ctx.covariance_columns_raw(G, mono, q, features=True)
    finally:
        ctx.set_spmv_variant(0)
    assert rc == 0 and steps >= 1
    cov = ctx.covariance(G, mono)
    vP, vF = np.einsum("kii->ki", cov["pose"]).ravel(), np.einsum("kii->ki", cov["feature"]).ravel()
    for i, j in enumerate(q):
        vQ = vP[6 * j: 6 * j + 6]
        assert _err(_pose_matrix(a["pose"], i), pose[i].reshape(-1, 6), vP, vQ) < BAR
        assert _err(_feat_matrix(a["feature"], i), feat[i].reshape(-1, 6), vF, vQ) < BAR
