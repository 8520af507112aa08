"""-m gpu: lsfm_gn_linearise_features (csrc/lsfm_gn.hip; kernels csrc/lsfm_gn_chi2.hip, csrc/lsfm_gn_assemble.hip) -- the joint map of the
local maps linearised at a state with given feature weights: H = sum_k w_k J_k^T I_k(w_k.) J_k, the matrix of one step of
lsfm_gn_polish_robust_features at fixed weights.  No reference counterpart (parity UNPINNED).  The expected H, b and obj are the oracle's on
the dicts robust_features_ref.reweight writes (tests/linearise_features_ref.py; test_linearise_features_cpu.py shows that reference to
hold 1e-14 on the host).  Unless a test says otherwise the weights are uniform in [0.1, 1] from a fixed seed, a tenth of them exactly 1.

Metric for H: |dH_ij| / sqrt(H_ii H_jj) <= 1e-9 (DESIGN.md section 13's bar); covariances: section 10's 1e-9."""
import numpy as np
import pytest

import linearise_features_ref as lf
import robust_features_ref as rf
from linearsfm_amd import api, synth
from refdump import dense_info
from test_gpu_linearise import IDS, _dense_sigma, _sigma_err

pytestmark = pytest.mark.gpu
BAR = 1e-9
CASES = list(range(len(IDS))) + [lf.CRAFTED]
CASE_IDS = IDS + [lf.CRAFTED]


def _states(oracle, i):
    """(state, the oracle's H of the re-weighted set there): the oracle's tree result and, on the six sets, the state two polish steps on"""
    c = lf.base(oracle, i)
    out = [(c["G"], lf.weighted_h(oracle, i))]
    if c["G2"] is not None:
        out.append((c["G2"], lf.weighted_h(oracle, i, True)))
    return out


@pytest.mark.parametrize("i", CASES, ids=CASE_IDS)
def test_h_against_the_oracle(ctx, oracle, i):
    """Tests 1 and 3 of the issue: dense_info(out) against the oracle's H on the re-weighted dicts.  The crafted set reaches slots
    without a U block of their own (210 pair slots of one feature seen by 20 poses in descending order), a diagonal slot beside an own
    block, a repeated (pose, feature) block, a 600-feature map in the global frame (nh = 0) and a map without features."""
    c = lf.base(oracle, i)
    for G, H in _states(oracle, i):
        out, F, b = ctx.gn_linearise(c["d"], c["mono"], G, feature_weight=c["fw"])
        e = lf.h_err(dense_info(out), H)
        print(f"{CASE_IDS[CASES.index(i)]}: H error with feature weights {e:.3e}")
        assert e <= BAR
        assert set(zip(out["Ui"].tolist(), out["Uj"].tolist())) == c["UX"] and out["nU"] == len(c["UX"])


@pytest.mark.parametrize("i", CASES, ids=CASE_IDS)
def test_b_and_obj(ctx, oracle, i):
    """b to 1e-7 max|b| and obj to 1e-9 of F against the oracle's gradient and objective on the same dicts; at the state after two
    polish steps b is held against the first state's size, as test_gpu_linearise.py::test_b_and_obj holds it."""
    c = lf.base(oracle, i)
    ds = lf.reweighted(c["d"], c["fw"])
    size = None
    for G, _ in _states(oracle, i):
        out, F, b = ctx.gn_linearise(c["d"], c["mono"], G, want_b=True, feature_weight=c["fw"])
        eF, eb = oracle.gn_objective(ds, c["mono"], G)
        size = np.max(np.abs(eb)) if size is None else size
        print(f"{CASE_IDS[CASES.index(i)]}: max|b| {np.max(np.abs(eb)):.3e}, b error {np.max(np.abs(b - eb)):.3e} (bound {1e-7 * size:.3e}), obj error {abs(F - eF) / eF:.3e}")
        assert np.max(np.abs(b - eb)) <= 1e-7 * size
        assert abs(F - eF) <= 1e-9 * eF


@pytest.mark.parametrize("i", CASES, ids=CASE_IDS)
def test_all_weights_one_is_the_plain_call(ctx, oracle, i):
    """Every weight 1: the values are the plain call's to 1e-13 (two assemblies differ by the order of their atomic sums), W and V index
    arrays bit for bit, a flat array is taken like a list per map, and a block that exists only because of the slots is exactly 0.0."""
    c = lf.base(oracle, i)
    d, mono, G = c["d"], c["mono"], c["G"]
    o0, F0, _ = ctx.gn_linearise(d, mono, G)
    o1, F1, _ = ctx.gn_linearise(d, mono, G, feature_weight=[np.ones(int(L["n"])) for L in d])
    o2, F2, _ = ctx.gn_linearise(d, mono, G, feature_weight=np.ones(sum(int(L["n"]) for L in d)))
    for o, F1 in ((o1, F1), (o2, F2)):
        assert lf.h_err(dense_info(o), dense_info(o0)) <= 1e-13
        for k in ("photo", "feature", "FBlock", "stno", "stVal", "pose_origin"):
            assert np.array_equal(o0[k], o[k]), k
        assert all(o0[k] == o[k] for k in ("m", "n", "nW", "Ref", "FRef", "ScaP", "Fix", "Sign", "FScaP", "FFix"))
        assert abs(F1 - F0) <= 1e-11 * F0
        pairs = list(zip(o["Ui"].tolist(), o["Uj"].tolist()))
        assert set(pairs) == c["UX"] and len(pairs) == len(c["UX"])
        only = np.array([p not in c["U"] for p in pairs])
        assert np.count_nonzero(only) == len(c["UX"]) - len(c["U"])
        assert np.all(o["U"][only] == 0.0)
        assert set(zip(o0["Ui"].tolist(), o0["Uj"].tolist())) == c["U"]  # (the plain call's pattern is what it was)
    if i == lf.CRAFTED:
        assert np.count_nonzero(only) == 170


def test_mono_three_pose_maps_hold_the_pair_block(ctx, oracle):
    """A Mono set whose maps hold m = 3 poses and nU = 2 diagonal blocks (no block couples local poses 1 and 2, which every feature
    sees): the result holds the block of that pair's global poses, for every map."""
    c = lf.base(oracle, 3)
    out, _, _ = ctx.gn_linearise(c["d"], True, c["G"], feature_weight=c["fw"])
    pairs = set(zip(out["Ui"].tolist(), out["Uj"].tolist()))
    pid = {int(-s): p for p, s in enumerate(np.asarray(c["G"]["stno"])[:6 * int(c["G"]["m"]):6])}
    for L in c["d"]:
        assert int(L["m"]) == 3 and len(L["Ui"]) == 2 and np.array_equal(L["Ui"], L["Uj"])
        assert set(np.asarray(L["photo"]).tolist()) == {1, 2}
        a, b = (pid[int(-L["stno"][6 * p])] for p in (1, 2))
        assert (min(a, b), max(a, b)) in pairs


@pytest.mark.parametrize("i", CASES, ids=CASE_IDS)
def test_map_and_feature_weights_together(ctx, oracle, i):
    """Random w_k in [0.1, 1] on top of the feature weights: the oracle on the dicts re-weighted and then scaled.  A w_k that missed
    the correction slots would leave map k's Schur correction at full size: an error of the size of H."""
    c = lf.base(oracle, i)
    d, mono, G = c["d"], c["mono"], c["G"]
    w = np.random.default_rng(900 + len(d)).uniform(0.1, 1.0, len(d))
    ds = lf.reweighted(d, c["fw"], w)
    out, F, b = ctx.gn_linearise(d, mono, G, weight=w, want_b=True, feature_weight=c["fw"])
    e = lf.h_err(dense_info(out), lf.dense_h(oracle, i, ds, G))
    eF, eb = oracle.gn_objective(ds, mono, G)
    print(f"{CASE_IDS[CASES.index(i)]}: H error with map and feature weights {e:.3e}, obj error {abs(F - eF) / eF:.3e}")
    assert e <= BAR
    assert np.max(np.abs(b - eb)) <= 1e-7 * np.max(np.abs(eb)) and abs(F - eF) <= 1e-9 * eF


@pytest.mark.parametrize("i", [1, 4], ids=[IDS[1], IDS[4]])
def test_weight_zero_is_marginalisation(ctx, oracle, i):
    """Two features of one map that other maps hold too, at weight 0 (every other weight 1): H is, to 1e-12 of sqrt(H_ii H_jj), the
    plain linearisation of the set in which lsfm_map_marginalise removed the two from that map -- the new path against a device call
    that existed before it."""
    c = lf.base(oracle, i)
    d, mono, G = c["d"], c["mono"], c["G"]
    labels = [set(np.asarray(L["stno"])[6 * int(L["m"])::3].tolist()) for L in d]
    k = len(d) // 2
    shared = [f for f, lab in enumerate(np.asarray(d[k]["stno"])[6 * int(d[k]["m"])::3].tolist()) if any(lab in s for j, s in enumerate(labels) if j != k)]
    assert len(shared) >= 2
    drop = np.zeros(int(d[k]["n"]), bool)
    drop[[shared[0], shared[-1]]] = True
    fw = [np.ones(int(L["n"])) for L in d]
    fw[k][drop] = 0.0
    out, _, _ = ctx.gn_linearise(d, mono, G, feature_weight=fw)
    red = dict(ctx.marginalise(d[k], drop))
    for key in ("Ref", "FRef", "ScaP", "Fix", "Sign", "FScaP", "FFix"):
        assert red[key] == d[k][key], key
    exp, _, _ = ctx.gn_linearise(d[:k] + [red] + d[k + 1:], mono, G)
    e = lf.h_err(dense_info(out), dense_info(exp))
    print(f"{IDS[i]}: weight 0 against lsfm_map_marginalise {e:.3e}")
    assert e <= 1e-12


def test_refusals(ctx, oracle):
    """A weight of -0.1, 1.5, NaN or inf: LSFM_ERR_ARG naming the map and the feature; a wrong length: LsfmError before the call; a V_f
    that is not positive definite: LSFM_ERR_NOT_SPD naming it.  After each the same context linearises the set to the bar."""
    c = lf.base(oracle, 1)
    d, mono, G = c["d"], c["mono"], c["G"]

    def fine():
        out, _, _ = ctx.gn_linearise(d, mono, G, feature_weight=c["fw"])
        assert lf.h_err(dense_info(out), lf.weighted_h(oracle, 1)) <= BAR

    n2 = int(d[2]["n"])
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        fw = [np.array(x, copy=True) for x in c["fw"]]
        fw[2][n2 - 1] = bad
        with pytest.raises(api.LsfmError) as e:
            ctx.gn_linearise(d, mono, G, feature_weight=fw)
        assert "rc=-1" in str(e.value) and f"feature {n2}" in str(e.value) and "local map 3" in str(e.value), str(e.value)
        fine()
    flat = np.concatenate(c["fw"])
    for wrong in (flat[:-1], np.concatenate([flat, [1.0]]), c["fw"][:-1], [x[:-1] for x in c["fw"]]):
        with pytest.raises(api.LsfmError) as e:
            ctx.gn_linearise(d, mono, G, feature_weight=wrong)
        assert "rc=" not in str(e.value)
    neg = [dict(m) for m in d]
    V = np.array(neg[1]["V"], np.float64, copy=True).reshape(-1, 9)
    V[2] = -V[2]
    neg[1]["V"] = V
    with pytest.raises(api.LsfmError) as e:
        ctx.gn_linearise(neg, mono, G, feature_weight=c["fw"])
    assert "rc=-7" in str(e.value) and "not positive definite" in str(e.value) and "feature 3" in str(e.value) and "local map 2" in str(e.value), str(e.value)
    fine()
    with pytest.raises(api.LsfmError):  # what lsfm_gn_linearise checks is checked here too: a map weight, a feature outside the state
        ctx.gn_linearise(d, mono, G, weight=-np.ones(len(d)), feature_weight=c["fw"])
    with pytest.raises(api.LsfmError):
        ctx.gn_linearise(d, mono, dict(G, n=G["n"] - 1, stno=G["stno"][:-3], stVal=G["stVal"][:-3]), feature_weight=c["fw"])
    fine()


@pytest.mark.parametrize("i", [0, 1, 3, 4], ids=[IDS[q] for q in (0, 1, 3, 4)])
def test_it_composes_with_the_covariances(ctx, oracle, i):
    """lsfm_map_covariance and lsfm_map_covariance_columns on the result against a dense inverse of the oracle's H (Mono: the gauge
    rows and columns removed), the 2- and 9-map sets."""
    c = lf.base(oracle, i)
    mono, G = c["mono"], c["G"]
    m, n = int(G["m"]), int(G["n"])
    out, _, _ = ctx.gn_linearise(c["d"], mono, G, feature_weight=c["fw"])
    S = _dense_sigma(lf.weighted_h(oracle, i), G, mono)
    var = np.diag(S)
    P = np.stack([S[6 * p:6 * p + 6, 6 * p:6 * p + 6] for p in range(m)])
    Fb = np.stack([S[6 * m + 3 * f:6 * m + 3 * f + 3, 6 * m + 3 * f:6 * m + 3 * f + 3] for f in range(n)])
    vp, vf = var[:6 * m].reshape(m, 6), var[6 * m:].reshape(n, 3)
    cov = ctx.covariance(out, mono)
    ep, ef = _sigma_err(cov["pose"], P, vp, vp), _sigma_err(cov["feature"], Fb, vf, vf)
    poses = sorted({0, m // 2, m - 1})
    cols = ctx.covariance_columns(out, mono, poses)
    exp = np.stack([np.stack([S[6 * p:6 * p + 6, 6 * q:6 * q + 6] for p in range(m)]) for q in poses])
    ec = _sigma_err(cols["pose"], exp, np.broadcast_to(vp, (len(poses), m, 6)), np.stack([np.broadcast_to(vp[q], (m, 6)) for q in poses]))
    print(f"{IDS[i]}: Sigma error poses {ep:.3e} features {ef:.3e} columns {ec:.3e}")
    assert ep <= BAR and ef <= BAR and ec <= BAR and cols["converged"]


@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
def test_covariances_follow_the_feature_weights(ctx, oracle, mono):
    """The reason the call exists.  The 40-map sets with features 2 and 5 of map 8 moved by 30 sigma, polished with Huber c = 1.5, 8
    steps.  At the polished state: (a) linearised with the weights the polish returned, (b) without them.  I_k(w) <= I_k in the
    positive semi-definite order, so Sigma_a >= Sigma_b: every marginal variance of (a) is at least (b)'s times (1 - 1e-9), and for
    the two corrupted features and the poses of map 8 it is strictly larger.  Printed, not asserted: both against the clean set
    linearised at the same state."""
    n, npf, vis, kw = (40, 8, 4, synth.SPIRAL) if mono else (40, 8, 5, dict(lap=12, home=4, revisit=0.5))
    maps = synth.make_mono_set(n, npf, vis, seed=9, **kw) if mono else synth.make_stereo_set(n, npf, vis, seed=9, **kw)
    dc = [oracle.localmap_to_dict(x) for x in maps]
    j, bad = 7, [2, 5]
    db = list(dc)
    db[j] = rf.corrupt_features(dc[j], bad, 30.0)
    Gb, _, rc = ctx.divide_conquer(db, mono)
    assert rc == 0
    rob, _, _, _, _, fw, rc = ctx.gn_polish_robust_features(db, mono, Gb, 8, "huber", 1.5)
    assert rc == 0
    assert np.all(fw[j][bad] < 0.5)
    Gr = dict(Gb, stVal=rob)
    Ha, _, _ = ctx.gn_linearise(db, mono, Gr, feature_weight=fw)
    Hb, _, _ = ctx.gn_linearise(db, mono, Gr)
    Hc, _, _ = ctx.gn_linearise(dc, mono, Gr)
    ca, cb, cc = (ctx.covariance(H, mono) for H in (Ha, Hb, Hc))
    va, vb, vc = (np.concatenate([np.einsum("kii->ki", c["pose"]).reshape(-1), np.einsum("kii->ki", c["feature"]).reshape(-1)]) for c in (ca, cb, cc))
    m = int(Gb["m"])
    stno = np.asarray(Gb["stno"])
    pid = {int(-stno[6 * p]): p for p in range(m)}
    fid = {int(stno[6 * m + 3 * f]): f for f in range(int(Gb["n"]))}
    L = db[j]
    poses = [pid[int(-L["stno"][6 * p])] for p in range(int(L["m"]))]
    feats = [fid[int(L["stno"][6 * int(L["m"]) + 3 * f])] for f in bad]
    touched = np.concatenate([np.arange(6 * p, 6 * p + 6) for p in poses] + [np.arange(6 * m + 3 * f, 6 * m + 3 * f + 3) for f in feats])
    free = vc[touched] > 0
    print(f"{'Mono' if mono else 'Stereo'}: w corrupted {fw[j][bad]}, {sum(int(np.sum(x < 1)) for x in fw)} weights below 1; variances of map 8's poses and the two "
          f"features: weighted / unweighted {np.min(va[touched] / np.where(free, vb[touched], 1)):.4f}..{np.max(va[touched] / np.where(free, vb[touched], 1)):.4f}, "
          f"weighted / clean {np.min(va[touched][free] / vc[touched][free]):.4f}..{np.max(va[touched][free] / vc[touched][free]):.4f}, "
          f"unweighted / clean {np.min(vb[touched][free] / vc[touched][free]):.4f}..{np.max(vb[touched][free] / vc[touched][free]):.4f}; "
          f"all variables: smallest weighted / unweighted {np.min(va[vb > 0] / vb[vb > 0]):.12f}")
    assert np.all(va >= vb * (1.0 - 1e-9))
    assert np.all(va[touched] > vb[touched])
