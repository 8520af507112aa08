"""-m gpu: lsfm_map_merge_features (csrc/lsfm_merge.hip, structure csrc/lsfm_merge_structure.cpp) -- the map with pairs of features declared
equal and the joint compatibility D^2 of all pairs.  No reference counterpart: the expected state, D^2 and covariance come from the
constraint form on a dense numpy inverse of the device tree's map AS STORED (merge_reference.merged_dense; the floor between that
and the device's own formulation on the host: test_merge_cpu.py), the expected matrix from merge_reference.merged_blocks, bit for bit.

Bars (BAR = 1e-9, the project's):
  state   |y_i - y_ref,i| / (sigma_i max(1, sqrt(D^2_ref))) < BAR, sigma_i^2 = Sigma_ii of the UNMERGED map: Cauchy-Schwarz bounds the move
          of scalar i by sigma_i sqrt(D^2); gauge scalars are bit-equal to the input
  D^2     relative < BAR max(1, c), c = sum_g r_g^T V_g r_g / D^2_ref, the formula's own cancellation, from the reference; BAR c <= 1e-3
          is asserted first on every case
  Sigma'  lsfm_map_covariance of the merged map: within BAR of Sigma_c in units of the unmerged variances (merge_reference.sigma_err), and
          within BAR of a dense inverse of the merged map as stored in its own units (test_gpu_covariance's metric)"""
import ctypes as C

import numpy as np
import pytest

import feature_cov_reference as fref
import merge_reference as ref
from linearsfm_amd import api, synth
from test_gpu_covariance import BAR, SMALL, _diag, _feat_blocks, _norm_err, _pose_blocks, _small_set, _tree_map, dense_sigma
from test_gpu_feature_columns import small
from test_gpu_feature_gate import _designed_pairs

pytestmark = pytest.mark.gpu
SPLITS = [(1, 1), (2, 8), (3, 32), (5, 1), (6, 8), (7, 32)]  # (index into SMALL, features split): Stereo / Mono 2, 9, 40 maps
COV_SETS = (2, 3, 6, 7)
_SPLIT = {}


def _split(ctx, i, count):
    """The device tree's map of SMALL[i] with `count` features split (merge_reference.split_set), its dense Sigma and the split pairs;
    computed once."""
    if (i, count) not in _SPLIT:
        mono, n, kw = SMALL[i]
        dicts, chosen = ref.split_set([dict(vars(mp)) for mp in _small_set(mono, n, kw)], count)
        G = _tree_map(ctx, dicts, mono)
        _SPLIT[i, count] = (mono, G, dense_sigma(G, mono), ref.split_pairs(G, chosen))
    return _SPLIT[i, count]


def _check_matrix(out, G, pairs):
    """U / Ui / Uj and the head equal the input's; V', W', the index arrays, the labels and rep equal merged_blocks: bit for bit."""
    g = out["map"]
    exp, rep, _, _ = ref.merged_blocks(G, pairs)
    m = int(G["m"])
    for k in ("Ref", "FRef", "m", "ScaP", "Fix", "Sign", "FScaP", "FFix"):
        assert int(g[k]) == int(G.get(k, g[k])), k
    assert g["n"] == exp["n"] and g["nW"] == exp["nW"] and g["nU"] == len(np.asarray(G["Ui"]))
    for k in ("U", "Ui", "Uj"):
        assert np.array_equal(np.asarray(g[k]).ravel(), np.asarray(G[k]).ravel()), k
    for k in ("V", "W", "photo", "feature", "FBlock", "stno"):
        assert np.array_equal(np.asarray(g[k]).ravel(), np.asarray(exp[k]).ravel()), k
    if G.get("pose_origin") is not None:
        assert np.array_equal(g["pose_origin"], G["pose_origin"])
    assert np.array_equal(out["rep"], rep)
    assert np.array_equal(g["stno"][: 6 * m], np.asarray(G["stno"])[: 6 * m])
    return exp


def _check_merge(ctx, mono, G, Sig, pairs, what, cov=False):
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    m = int(G["m"])
    A = ref.merged_dense(G, mono, pairs, Sig)
    out = ctx.merge_features(G, mono, pairs)
    g = out["map"]
    _check_matrix(out, G, pairs)
    kept = ref.kept_scalars(m, A["members"])
    e_state = ref.state_err(g["stVal"], A["y"], Sig, kept, A["d2"])
    e_d2 = abs(out["d2"] - A["d2"]) / A["d2"]
    bar_d2 = BAR * max(1.0, A["c"])
    print(f"merge {what}: K {len(pairs)}, n {G['n']} -> {g['n']}, nW {len(G['photo'])} -> {g['nW']}, dof {out['dof']}, D2 {out['d2']:.6g} (ref {A['d2']:.6g}, "
          f"c {A['c']:.3g}), D2 rel {e_d2:.2e} (bar {bar_d2:.1e}), state {e_state:.2e}, steps {out['steps']}, last_corr {out['last_corr']:.1e}")
    assert BAR * A["c"] <= ref.CAP
    assert out["converged"] and out["steps"] >= 1
    assert out["dof"] == A["dof"] == 3 * (int(G["n"]) - int(g["n"]))
    fx = np.concatenate([ref._fixed(G, mono), np.zeros(3 * int(g["n"]), bool)])
    assert np.array_equal(g["stVal"][fx], np.asarray(G["stVal"])[kept][fx])
    assert e_state < BAR
    assert e_d2 < bar_d2
    if cov:
        no = int(g["n"])
        cv = ctx.covariance(g, mono)
        e_c = ref.sigma_err(cv["pose"], cv["feature"], A["Sigma_c"], Sig, kept, m, no)
        S1 = dense_sigma(g, mono)
        P1, F1 = _pose_blocks(S1, m), _feat_blocks(S1, m, no)
        e_own = max(_norm_err(cv["pose"], P1, _diag(P1), _diag(P1)), _norm_err(cv["feature"], F1, _diag(F1), _diag(F1)))
        print(f"      covariance of the merged map: against Sigma_c {e_c:.2e}, against its own dense inverse {e_own:.2e}")
        assert e_c < BAR and e_own < BAR
    return out, A


# ---- 1. split pairs: a class of two, a pose that sees both members ----------------------------------------------------------------------
@pytest.mark.parametrize("i,count", SPLITS)
def test_split_pairs(ctx, i, count):
    mono, G, Sig, pairs = _split(ctx, i, count)
    ph, fe = np.asarray(G["photo"]), np.asarray(G["feature"])
    assert all(set(ph[fe == f]) & set(ph[fe == g]) for f, g in pairs)  # every merge sums blocks
    out, _ = _check_merge(ctx, mono, G, Sig, pairs, f"split {SMALL[i][:2]} x{count}", cov=i in COV_SETS)
    assert out["map"]["nW"] < len(ph) and out["map"]["n"] == int(G["n"]) - count


# ---- 2. seeded pairs: large D^2, large c -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", COV_SETS)
def test_seeded_pairs(ctx, i):
    mono, G, Sig = small(ctx, i)
    _check_merge(ctx, mono, G, Sig, fref.seeded_pairs(int(G["n"]), 24), f"seeded {SMALL[i][:2]}", cov=True)


# ---- 3. designed pairs --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [3, 7])
def test_designed_pairs(ctx, i):
    mono, G, Sig = small(ctx, i)
    n = int(G["n"])
    out, A = _check_merge(ctx, mono, G, Sig, [(0, 1), (1, 2), (3, 2)], f"chain {SMALL[i][:2]}", cov=True)
    assert max(len(c) for c in A["members"]) == 4 and out["map"]["n"] == n - 3
    _check_merge(ctx, mono, G, Sig, [(0, n - 1)], f"(0, n-1) {SMALL[i][:2]}")
    # a pair in both orders and twice: the same arrays as the single pair, bit for bit in V', W' and the indices
    a, _ = _check_merge(ctx, mono, G, Sig, [(5, n - 2)], f"single {SMALL[i][:2]}")
    b, _ = _check_merge(ctx, mono, G, Sig, [(n - 2, 5), (5, n - 2), (n - 2, 5)], f"both orders, twice {SMALL[i][:2]}")
    for k in ("V", "W", "U", "photo", "feature", "FBlock", "stno", "Ui", "Uj"):
        assert np.array_equal(a["map"][k], b["map"][k]), k
    assert np.array_equal(a["rep"], b["rep"])
    if mono:
        # members seen by the Ref pose (all six scalars fixed) and by the ScaP pose (one fixed), as the gate's tests pick them
        _check_merge(ctx, mono, G, Sig, _designed_pairs(G, True)[len(_designed_pairs(G, False)):], f"Ref / ScaP members {SMALL[i][:2]}")


# ---- 4. every feature in one class -------------------------------------------------------------------------------------------------------------
def test_one_class(ctx):
    """n' = 1: one run coalesced from every block of W -- the longest source lists."""
    mono, G, Sig = small(ctx, 3)
    n = int(G["n"])
    out, _ = _check_merge(ctx, mono, G, Sig, [(f, f + 1) for f in range(n - 1)], "one class, Stereo 40")
    g = out["map"]
    assert g["n"] == 1 and g["nW"] == len(np.unique(G["photo"])) and np.all(np.diff(g["photo"]) > 0)


# ---- 5. a hand-made map: a pair without a common pose --------------------------------------------------------------------------------------------
def _hand_made():
    """Stereo, m = 3, n = 8, diagonally dominant, seeded: features 0-3 see pose 0 only, features 4-7 see poses 1 and 2 only."""
    rng = np.random.default_rng(11)
    m, n = 3, 8
    sym = lambda k: (lambda a: a + a.T)(rng.normal(size=(k, k)))
    Ui, Uj = [0, 0, 1, 1, 2], [0, 1, 1, 2, 2]
    U = np.stack([1e3 * np.eye(6) + sym(6) if a == b else rng.normal(size=(6, 6)) for a, b in zip(Ui, Uj)])
    photo = [0] * 4 + [1, 2] * 4
    feature = [0, 1, 2, 3] + [f for f in range(4, 8) for _ in range(2)]
    W = rng.normal(size=(len(photo), 18))
    V = np.stack([100.0 * np.eye(3) + sym(3) for _ in range(n)])
    stno = np.concatenate([np.repeat(-np.arange(1, m + 1), 6), np.repeat(np.arange(1, n + 1), 3)]).astype(np.int32)
    return dict(Ref=1, FRef=1, m=m, n=n, ScaP=0, Fix=0, Sign=1, FScaP=0, FFix=0, stno=stno, stVal=rng.normal(size=6 * m + 3 * n),
                U=U.reshape(-1, 36), Ui=np.array(Ui, np.int32), Uj=np.array(Uj, np.int32), W=W, photo=np.array(photo, np.int32),
                feature=np.array(feature, np.int32), V=V.reshape(-1, 9), FBlock=np.searchsorted(feature, np.arange(n)).astype(np.int32))


def test_hand_made_no_common_pose(ctx):
    """(0, 4) share NO pose -- the stand-in sets never give such a pair: their merged run is the two runs interleaved, no block is
    summed.  (1, 2) see pose 0 alone, both: their merged run is one summed block (with four features on one pose no pair among them
    could keep its blocks apart)."""
    G = _hand_made()
    Sig = dense_sigma(G, False)
    out, _ = _check_merge(ctx, False, G, Sig, [(0, 4), (1, 2)], "hand-made", cov=True)
    assert out["map"]["nW"] == len(G["photo"]) - 1 and out["map"]["n"] == 6
    assert out["map"]["photo"][:3].tolist() == [0, 1, 2]  # feature 0's block, then feature 4's two
    assert api.merge_structure(G, [(0, 4)])["info"]["summed_blocks"] == 0
    assert api.merge_structure(G, [(0, 4), (1, 2)])["info"]["summed_blocks"] == 1


# ---- 6. a member with a repeated block ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [2, 6])
def test_repeated_block(ctx, i):
    mono, G, Sig = small(ctx, i)
    n = int(G["n"])
    f = n // 2
    Gs = fref.split_block(G, f)
    un, _ = _check_merge(ctx, mono, Gs, Sig, [(0, 1)], f"repeated block untouched {SMALL[i][:2]}")
    c = int(un["rep"][f])
    o = int(un["map"]["FBlock"][c])
    assert un["map"]["photo"][o] == un["map"]["photo"][o + 1]  # both halves stay
    mg, _ = _check_merge(ctx, mono, Gs, Sig, [(f, n // 3)], f"repeated block merged {SMALL[i][:2]}")
    whole, _ = _check_merge(ctx, mono, G, Sig, [(f, n // 3)], f"the same pair, unsplit map {SMALL[i][:2]}")
    assert mg["map"]["nW"] == whole["map"]["nW"] and np.array_equal(mg["map"]["photo"], whole["map"]["photo"])
    den = np.sqrt(np.abs(np.diag(Sig)[ref.kept_scalars(int(G["m"]), ref.classes(n, [(f, n // 3)])[1])])) + 1e-300
    assert np.max(np.abs(mg["map"]["stVal"] - whole["map"]["stVal"]) / den) < BAR * max(1.0, np.sqrt(whole["d2"]))


# ---- 8. K = 1 is the gate's d^2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", COV_SETS)
def test_one_pair_equals_gate(ctx, i):
    mono, G, Sig = small(ctx, i)
    pairs = fref.seeded_pairs(int(G["n"]), 6)
    covA, marg = fref.route_a(Sig, G, pairs)
    bars = fref.d2_bars(covA, marg)
    gate = ctx.feature_pair_gate(G, mono, pairs)["d2"]
    assert bars.max() < fref.BAR_D2_CAP
    for a, (f, g) in enumerate(pairs):
        d2 = ctx.merge_features(G, mono, [(f, g)])["d2"]
        rel = abs(d2 - gate[a]) / gate[a]
        print(f"K = 1 {SMALL[i][:2]} ({f}, {g}): merge {d2:.9g}, gate {gate[a]:.9g}, rel {rel:.2e} (bar {bars[a]:.1e})")
        assert rel < bars[a]


# ---- 9. refusals, statuses, settings -------------------------------------------------------------------------------------------------------------
def test_arguments(ctx):
    mono, G, _ = small(ctx, 6)
    n = int(G["n"])
    raw = ctx.merge_features_raw
    for bad in ([], [[0, n]], [[-1, 0]], [[3, 3]]):
        rc, g, d2, dof, rep, steps, corr, _ = raw(G, mono, bad)
        assert rc == -1 and g is None and steps == 0 and d2 == 0.0 and dof == 0, bad
    fe = np.array(G["feature"], np.int32, copy=True)
    fe[0], fe[-1] = fe[-1], fe[0]
    assert raw(dict(G, feature=fe), mono, [[0, 1]])[:2] == (-1, None)
    assert raw(dict(G, Ref=10 ** 6), mono, [[0, 1]])[:2] == (-1, None)  # what lsfm_map_covariance refuses
    h = api.HostMap(G)
    q = np.array([0, 1], np.int32)
    assert api.lib().lsfm_map_merge_features(ctx._h, C.byref(h.c), 1, q.ctypes.data_as(C.POINTER(C.c_int)), 1, None, None, None, None, None, None) == -1
    # every optional output NULL but the map
    out = api.LsfmMap()
    assert api.lib().lsfm_map_merge_features(ctx._h, C.byref(h.c), 1, q.ctypes.data_as(C.POINTER(C.c_int)), 1, C.byref(out), None, None, None, None, None) == 0
    assert api.map_to_dict(out)["n"] == n - 1
    # a tree run on the same context afterwards
    G2 = _tree_map(ctx, _small_set(*SMALL[6]), True)
    assert np.array_equal(G2["stno"], G["stno"])


def test_not_positive_definite(ctx):
    """The indefinite map of test_gpu_covariance.test_not_positive_definite: the numerical status, no map."""
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
    rc, g, d2, dof, _, steps, _, _ = ctx.merge_features_raw(d, False, [[0, 1]])
    assert (rc == -7 or rc > 0) and g is None and steps == 0, rc


def test_settings_do_not_apply_and_resident_tree(ctx):
    mono, G, Sig, pairs = _split(ctx, 2, 8)
    maps = _small_set(*SMALL[2])
    t = ctx.tree_upload(maps, mono)
    try:
        _, rc = ctx.tree_run(t)
        assert rc == 0
        G0 = ctx.tree_download(t)
        a = ctx.merge_features(G, mono, pairs)
        ctx.set_precision(True)
        ctx.set_small_solve(16)
        try:
            b = ctx.merge_features(G, mono, pairs)
        finally:
            ctx.set_precision(False)
            ctx.set_small_solve(5)
        for k in ("V", "W", "U", "photo", "feature", "FBlock", "stno"):
            assert np.array_equal(a["map"][k], b["map"][k]), k
        A = ref.merged_dense(G, mono, pairs, Sig)
        kept = ref.kept_scalars(int(G["m"]), A["members"])
        assert ref.state_err(b["map"]["stVal"], A["y"], Sig, kept, A["d2"]) < BAR and abs(b["d2"] - A["d2"]) / A["d2"] < BAR * max(1.0, A["c"])
        # the resident inputs of the tree still run, to the same result
        _, rc = ctx.tree_run(t)
        assert rc == 0
        G2 = ctx.tree_download(t)
        assert np.array_equal(G2["stno"], G0["stno"])
        assert np.max(np.abs(G2["stVal"] - G0["stVal"]) / np.maximum(1.0, np.abs(G0["stVal"]))) < 1e-8
    finally:
        ctx.tree_free(t)


# ---- 10. printed, not asserted: the merged split set against the tree of the unsplit set ----------------------------------------------------------
@pytest.mark.parametrize("i,count", [(2, 8), (6, 8)])
def test_merged_split_vs_unsplit_tree(ctx, i, count):
    """The two differ by the joins' linearisation (the split set's tree linearises around two estimates of a split feature); the
    figure is printed for the record, only the labels are asserted."""
    mono, G, Sig, pairs = _split(ctx, i, count)
    _, G0, Sig0 = small(ctx, i)
    g = ctx.merge_features(G, mono, pairs)["map"]
    m = int(G["m"])
    assert np.array_equal(g["stno"][: 6 * m], G0["stno"][: 6 * m]) and sorted(ref.feature_ids(g)) == sorted(ref.feature_ids(G0))
    at = {int(l): f for f, l in enumerate(ref.feature_ids(G0))}
    idx = np.concatenate([np.arange(6 * m)] + [6 * m + 3 * at[int(l)] + np.arange(3) for l in ref.feature_ids(g)])
    sig = np.sqrt(np.diag(Sig0)[idx])
    on = sig > 0
    diff = np.abs(g["stVal"] - np.asarray(G0["stVal"])[idx])[on] / sig[on]
    print(f"merged split set vs unsplit tree {SMALL[i][:2]}: largest |dy| / sigma {diff.max():.3e}, median {np.median(diff):.3e}")
