"""-m gpu: lsfm_map_feature_chi2 and lsfm_gn_polish_robust_features (csrc/lsfm_gn.hip, kernels: csrc/lsfm_gn_chi2.hip, slots: csrc/lsfm_gn_structure.cpp) -- the chi^2 c_kf of single features of single
local maps given their map's poses, and the Gauss-Newton polish that re-weights those conditional terms by an M-estimator on c_kf / 3
(IRLS on the maps I_k(w)).  No reference counterpart (parity UNPINNED).  The oracle checks both without a change of its own through
tests/robust_features_ref.py: `reweight` writes I_k(w) as a map dict, and F is linear in every map's information."""
import numpy as np
import pytest

import robust_features_ref as rf
from common import feat_param_err, pose_param_err
from linearsfm_amd import synth

pytestmark = pytest.mark.gpu

SETS = [(False, 2, 6, 4, {}), (False, 9, 8, 4, {}), (False, 40, 8, 5, dict(lap=12, home=4, revisit=0.5)),
        (True, 2, 6, 4, {}), (True, 9, 8, 4, {}), (True, 40, 8, 4, synth.SPIRAL)]


def _maps(mono, n, npf, vis, kw):
    return synth.make_mono_set(n, npf, vis, seed=9, **kw) if mono else synth.make_stereo_set(n, npf, vis, seed=9, **kw)


def _dicts(oracle, maps):
    return [oracle.localmap_to_dict(m) for m in maps]


def _lap(mono):
    return _maps(mono, 40, 8, 5 if not mono else 4, dict(lap=12, home=4, revisit=0.5) if not mono else synth.SPIRAL)


@pytest.mark.parametrize("mono,n,npf,vis,kw", SETS)
def test_feature_chi2_against_the_oracle(ctx, oracle, mono, n, npf, vis, kw):
    """At the oracle's tree result: c_kf is F(I_k(e_f)) - F(I_k(0)) of the oracle to 1e-10 chi2_k (the difference cancels: the bar is
    relative to the map's chi2), pose_chi2_k + sum_f c_kf is lsfm_map_chi2's chi2_k to 1e-10, every c_kf >= 0, two calls give the same
    bits."""
    d = _dicts(oracle, _maps(mono, n, npf, vis, kw))
    G, _, rc = oracle.divide_conquer(d, mono)
    assert rc == 0
    fchi2, pose = ctx.map_feature_chi2(d, mono, G)
    chi2, _ = ctx.map_chi2(d, mono, G)
    assert [len(c) for c in fchi2] == [int(m["n"]) for m in d]
    for k in range(n):
        exp, F0, chi2_k = rf.feature_chi2_by_oracle(oracle, d, mono, G, k)
        assert np.max(np.abs(fchi2[k] - exp)) <= 1e-10 * chi2_k, (k, np.max(np.abs(fchi2[k] - exp)), chi2_k)
        assert abs(pose[k] - F0) <= 1e-10 * chi2_k
        assert abs(pose[k] + fchi2[k].sum() - chi2[k]) <= 1e-10 * chi2[k]
        assert np.all(fchi2[k] >= 0.0)
    fchi2b, poseb = ctx.map_feature_chi2(d, mono, G)
    assert all(np.array_equal(a, b) for a, b in zip(fchi2, fchi2b)) and np.array_equal(pose, poseb)


@pytest.fixture(scope="module")
def crafted(oracle):
    """rf.crafted_set: a 22-map Stereo set plus the crafted maps A (the transposed run, 210 slots, a repeated (pose, feature) block), B (nh = 0, 600
    features) and C (no feature)."""
    return rf.crafted_set(oracle)


def test_crafted_maps_chi2(ctx, oracle, crafted):
    """The crafted maps' c_kf against the oracle (map B: every 7th feature and the identity over all of them)."""
    d, G = crafted
    fchi2, pose = ctx.map_feature_chi2(d, False, G)
    chi2, _ = ctx.map_chi2(d, False, G)
    assert len(fchi2[-1]) == 0
    for k in range(len(d)):
        assert abs(pose[k] + fchi2[k].sum() - chi2[k]) <= 1e-10 * chi2[k]
        assert np.all(fchi2[k] >= 0.0)
    kA, kB = len(d) - 3, len(d) - 2
    exp, F0, chi2_k = rf.feature_chi2_by_oracle(oracle, d, False, G, kA)
    assert np.max(np.abs(fchi2[kA] - exp)) <= 1e-10 * chi2_k and abs(pose[kA] - F0) <= 1e-10 * chi2_k
    n = int(d[kB]["n"])
    chi2_k = rf.map_objective(oracle, d, False, G, kB, d[kB])
    F0 = rf.map_objective(oracle, d, False, G, kB, rf.reweight(d[kB], np.zeros(n)))
    assert abs(pose[kB] - F0) <= 1e-10 * chi2_k
    for f in range(0, n, 7):
        e = np.zeros(n)
        e[f] = 1.0
        assert abs(fchi2[kB][f] - (rf.map_objective(oracle, d, False, G, kB, rf.reweight(d[kB], e)) - F0)) <= 1e-10 * chi2_k


@pytest.mark.parametrize("kind", [1, 2])
def test_crafted_maps_one_step(ctx, oracle, crafted, kind):
    """One IRLS step on the crafted set against the oracle's plain step on reweight(...) with the device's starting weights: the
    transposed slot, many contributors per slot, slots with and without a U block of their own, the repeated block, n = 0, nh = 0.
    c = the root of the median s_kf: half of the instances are down-weighted."""
    d, G = crafted
    fchi2, pose = ctx.map_feature_chi2(d, False, G)
    c = float(np.sqrt(np.median(np.concatenate(fchi2) / 3.0)))
    w = [rf.weights(kind, f / 3.0, c) for f in fchi2]
    assert min(np.min(x) for x in w if len(x)) < 0.9
    got, obj, gn, hv, _, _, rc = ctx.gn_polish_robust_features(d, False, G, 1, kind, c)
    exp, eobj, egn, ehv, erc = oracle.gn_polish([rf.reweight(m, x) for m, x in zip(d, w)], False, G, 1)
    assert rc == 0 and erc == 0
    assert abs(obj[0] - rf.objective(kind, c, fchi2, pose)) <= 1e-12 * obj[0]
    assert abs(gn[0] - egn[0]) <= 1e-7 * egn[0]
    assert hv[0] == 0 and ehv[0] == 0
    assert pose_param_err(got, exp, G["stno"]) < 1e-6 and feat_param_err(got, exp, G["stno"]) < 1e-6


@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("kind", [1, 2])
def test_one_irls_step_against_the_oracle(ctx, oracle, mono, kind):
    """One step from the oracle's tree result against the oracle's plain step on the maps re-weighted with the device's starting
    weights w_kf = rho'(c_kf / 3): 1e-6 on poses and features, G at the start against its numpy statement to 1e-12, the weighted
    gradient's size to 1e-7.  The 40-map Stereo lap and the 9-map Mono set: there both sides take the step whole.  c = 0.5 lies inside
    the spread of s_kf (median c_kf about 0.35), so weights differ from 1."""
    d = _dicts(oracle, _lap(False) if not mono else _maps(True, 9, 8, 4, {}))
    G, _, rc = oracle.divide_conquer(d, mono)
    assert rc == 0
    c = 0.5
    fchi2, pose = ctx.map_feature_chi2(d, mono, G)
    w = [rf.weights(kind, f / 3.0, c) for f in fchi2]
    assert min(np.min(x) for x in w) < 0.9
    got, obj, gn, hv, _, _, rc = ctx.gn_polish_robust_features(d, mono, G, 1, kind, c)
    exp, eobj, egn, ehv, erc = oracle.gn_polish([rf.reweight(m, x) for m, x in zip(d, w)], mono, G, 1)
    assert rc == 0 and erc == 0
    assert hv[0] == 0 and ehv[0] == 0
    assert pose_param_err(got, exp, G["stno"]) < 1e-6 and feat_param_err(got, exp, G["stno"]) < 1e-6
    assert abs(obj[0] - rf.objective(kind, c, fchi2, pose)) <= 1e-12 * obj[0]
    assert abs(gn[0] - egn[0]) <= 1e-7 * egn[0]


@pytest.mark.parametrize("mono", [False, True])
def test_weights_of_one_are_the_plain_polish(ctx, oracle, mono):
    """kind 0, and Huber with c above every s_kf (every weight exactly 1, every correction slot exactly 0), against lsfm_gn_polish with
    the bars of test_gpu_robust.py::test_kind_none_is_the_plain_polish (two plain calls already differ in the last bits: F to 1e-11,
    the state to 1e-9, equal halvings)."""
    d = _dicts(oracle, _lap(mono))
    G, _, rc = oracle.divide_conquer(d, mono)
    assert rc == 0
    st, obj, gn, hv, rc = ctx.gn_polish(d, mono, G, 3)
    assert rc == 0
    for kind, c in ((0, 1.0), (1, 1e3)):
        st0, obj0, gn0, hv0, fchi2, fw, rc0 = ctx.gn_polish_robust_features(d, mono, G, 3, kind, c)
        assert rc0 == 0
        assert np.max(np.abs(obj0 - obj) / obj) <= 1e-11
        assert np.array_equal(hv0, hv)
        assert np.max(np.abs(st0 - st)) <= 1e-9 * max(1.0, np.max(np.abs(st)))
        assert all(np.all(x == 1.0) for x in fw)
        assert max(np.max(f) for f in fchi2) / 3.0 < c * c or kind == 0
        exp, _ = ctx.map_feature_chi2(d, mono, dict(G, stVal=st0))
        assert all(np.array_equal(a, b) for a, b in zip(fchi2, exp))


@pytest.mark.parametrize("mono,kind,c,closer", [(False, 2, 2.0, 8.0), (False, 1, 1.5, 4.0), (True, 1, 1.5, 8.0)])
def test_outlier_features_are_found_and_down_weighted(ctx, oracle, mono, kind, c, closer):
    """Features 2 and 5 of map 8 (index 7) of the 40-map sets have their estimate moved by 30 sigma (1, -1, 1), sigma = sqrt(diag(V_f^-1)).
    Both polishes start from the device's tree result of the corrupted set; the clean set's plain polish is the right answer.

    The bars sit at about one third of what a CPU prototype of the same IRLS through the oracle gave (re-weight the dicts with
    `reweight`, one orc_gn_polish step, 8 times; the device's line search is on G, the prototype accepted the oracle's step on the
    weighted F), from the oracle's tree result: Stereo Cauchy c = 2: 25.8x closer to the clean polish than the plain polish, corrupted
    weights 4.5e-3, every other weight >= 0.65 (median 0.98); Stereo Huber c = 1.5: 11.9x, corrupted weights 0.05, every other 1; Mono
    Huber c = 1.5: 24.7x.  c_kf of the two at the tree result: Stereo 1196 and 1289 (largest other of the map 8.2, median of all 0.35),
    Mono 14169 and 1020 (855; 2.35).  Bars: >= 8x / 4x / 8x; Stereo Cauchy also corrupted weights < 0.02 and every other > 0.4.
    Mono uses Huber: with Cauchy a pulled global feature makes every instance of it large and a redescending weight may choose the
    wrong one -- the prototype with Cauchy c = 2 ended 2.3x closer only, one corrupted instance back at weight 0.9997 and a good
    instance at 0."""
    maps = _lap(mono)
    dc = _dicts(oracle, maps)
    j, bad = 7, [2, 5]
    db = list(dc)
    db[j] = rf.corrupt_features(dc[j], bad, 30.0)
    Gc, _, rc = ctx.divide_conquer(dc, mono)
    assert rc == 0
    Gb, _, rc = ctx.divide_conquer(db, mono)
    assert rc == 0
    assert np.array_equal(Gb["stno"], Gc["stno"])
    f0, _ = ctx.map_feature_chi2(db, mono, Gb)
    assert sorted(np.argsort(f0[j])[-2:].tolist()) == bad, f0[j]
    clean, _, _, _, rc = ctx.gn_polish(dc, mono, Gc, 6)
    assert rc == 0
    plain, _, _, _, rc = ctx.gn_polish(db, mono, Gb, 8)
    assert rc == 0
    rob, obj, _, hv, fchi2, fw, rc = ctx.gn_polish_robust_features(db, mono, Gb, 8, kind, c)
    assert rc == 0
    assert np.all(np.diff(obj) <= 1e-12 * obj[0])
    e_plain, e_rob = pose_param_err(plain, clean, Gb["stno"]), pose_param_err(rob, clean, Gb["stno"])
    others = np.concatenate([np.delete(fw[j], bad)] + [x for k, x in enumerate(fw) if k != j])
    print(f"{'Mono' if mono else 'Stereo'} kind {kind}: c_kf corrupted {f0[j][bad]}, largest other of the map {np.max(np.delete(f0[j], bad)):.2f}, "
          f"error plain {e_plain:.3e} robust {e_rob:.3e} ({e_plain / e_rob:.1f}x), w corrupted {fw[j][bad]}, others min {np.min(others):.3f} "
          f"median {np.median(others):.3f}, halvings {hv.tolist()}")
    assert e_rob * closer <= e_plain
    if not mono and kind == 2:
        assert np.all(fw[j][bad] < 0.02)
        assert np.all(others > 0.4)


@pytest.mark.parametrize("config,kind,c", [("rs90", 2, 2.0), ("nc3500-512", 1, 0.5)])
def test_returned_chi2_and_weights_on_the_named_sets(ctx, oracle, config, kind, c):
    """From the device's own tree result: G never rises, halvings <= 8, the returned c_kf is lsfm_map_feature_chi2 at the returned state
    bit for bit, and the returned weights are rho'(c_kf / 3) recomputed here to 1e-15."""
    if config == "rs90":
        typ, maps = synth.make_config("rs90")
        steps = 6
    else:
        typ, maps = synth.make_config("nc3500", 512)
        steps = 3
    mono = typ == "Monocular"
    d = _dicts(oracle, maps)
    G, _, rc = ctx.divide_conquer(d, mono)
    assert rc == 0
    st, obj, gn, hv, fchi2, fw, rc = ctx.gn_polish_robust_features(d, mono, G, steps, kind, c)
    assert rc == 0
    assert np.all(np.diff(obj) <= 1e-12 * obj[0]) and obj[-1] < obj[0]
    assert np.all(hv <= 8)
    exp, _ = ctx.map_feature_chi2(d, mono, dict(G, stVal=st))
    assert all(np.array_equal(a, b) for a, b in zip(fchi2, exp))
    cf, w = np.concatenate(fchi2), np.concatenate(fw)
    ew = rf.weights(kind, cf / 3.0, c)
    assert np.max(np.abs(w - ew) / ew) <= 1e-15
    print(f"{config}: G {obj[0]:.6f} -> {obj[-1]:.6f}, halvings {hv.tolist()}, weights {np.min(w):.3f}..{np.max(w):.3f}, {np.mean(w < 1):.3f} below 1")


def test_refusals(ctx, oracle):
    from linearsfm_amd import api
    d = _dicts(oracle, synth.make_stereo_set(5, 6, 4, seed=2))
    G, _, rc = ctx.divide_conquer(d, False)
    for kind, c in ((3, 1.0), (-1, 1.0), (1, 0.0), (2, -1.0), (1, float("nan")), (2, float("inf"))):
        with pytest.raises(api.LsfmError):
            ctx.gn_polish_robust_features(d, False, G, 1, kind, c)
    short = dict(G, n=G["n"] - 1, stno=G["stno"][:-3], stVal=G["stVal"][:-3])  # a local feature that is not in the global state
    with pytest.raises(api.LsfmError):
        ctx.map_feature_chi2(d, False, short)
    with pytest.raises(api.LsfmError):
        ctx.gn_polish_robust_features(d, False, short, 1, 1, 1.0)
    # V of feature 3 of map 2 negated: not positive definite, named in the message; the context stays usable
    neg = [dict(m) for m in d]
    V = np.array(neg[1]["V"], np.float64, copy=True).reshape(-1, 9)
    V[2] = -V[2]
    neg[1]["V"] = V
    for call in (lambda: ctx.map_feature_chi2(neg, False, G), lambda: ctx.gn_polish_robust_features(neg, False, G, 1, 1, 1.0)):
        with pytest.raises(api.LsfmError) as e:
            call()
        assert "not positive definite" in str(e.value) and "feature 3" in str(e.value) and "local map 2" in str(e.value), str(e.value)
    st, obj, gn, hv, fchi2, fw, rc = ctx.gn_polish_robust_features(d, False, G, 1, 2, 1.0)
    assert rc == 0 and obj[1] <= obj[0]
