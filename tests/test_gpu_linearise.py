"""-m gpu: lsfm_gn_linearise (csrc/lsfm_gn.hip, structure: csrc/lsfm_gn_structure.cpp) -- the joint map of the N local maps linearised at a given state: H = sum_k w_k J_k^T I_k J_k
as U / W / V with every block once, the matrix a step of lsfm_gn_polish[_robust] solves with.  No reference counterpart (parity UNPINNED).
The expected H is the oracle's (oracle/lsfm_gn.inc, orc_gn_hessian_times), made dense here; b and F are the oracle's gn_objective.

Metric for H: |dH_ij| / sqrt(H_ii H_jj) <= 1e-9, the bar the project pins assembled U / W / V at; for covariances
section 10's |dSigma_ij| / sqrt(Sigma_ii Sigma_jj) <= 1e-9."""
import copy
import functools

import numpy as np
import pytest

from common import feat_param_err, pose_param_err
from linearsfm_amd import api, synth
from refdump import dense_info

pytestmark = pytest.mark.gpu
BAR = 1e-9

SETS = [(False, 2, 6, 4, {}), (False, 9, 8, 4, {}), (False, 40, 8, 5, dict(lap=12, home=4, revisit=0.5)),
        (True, 2, 6, 4, {}), (True, 9, 8, 4, {}), (True, 40, 8, 4, synth.SPIRAL)]
IDS = ["stereo2", "stereo9", "stereo40", "mono2", "mono9", "mono40"]
COV_SETS = [0, 1, 2, 3, 4]  # the sets of <= 9 maps and Stereo 40 (the 40-map Mono spiral is too ill-conditioned a yardstick for Sigma)


def _scaled(dicts, w):
    """I_k enters H, b and F linearly: map k's U, W and V scaled by w_k turn the oracle's plain quantities into the weighted ones."""
    out = []
    for d, wk in zip(dicts, w):
        e = dict(d)
        e["U"], e["W"], e["V"] = d["U"] * wk, d["W"] * wk, d["V"] * wk
        out.append(e)
    return out


def label_structure(dicts, mono, G):
    """From the labels alone: the distinct (pose, feature) and (pose <= pose) pairs that the local maps and their hub roles (a map's Ref
    [, ScaP] pose against every variable of the map; none for a Stereo map in the global frame) produce, and the block counts of the
    working form, in which every map writes its own."""
    m = int(G["m"])
    stno = np.asarray(G["stno"])
    pid = {int(-stno[6 * i]): i for i in range(m)}
    fid = {int(stno[6 * m + 3 * i]): i for i in range(int(G["n"]))}
    W, U = set(), set()
    nWJ = nUJ = 0
    for L in dicts:
        lm, ln = int(L["m"]), int(L["n"])
        ls = np.asarray(L["stno"])
        gp = [pid[int(-ls[6 * i])] for i in range(lm)]
        gf = [fid[int(ls[6 * lm + 3 * i])] for i in range(ln)]
        hubs = [] if (not mono and int(L["Ref"]) == int(G["Ref"])) else [pid[int(L["Ref"])]] + ([pid[int(L["ScaP"])]] if mono else [])
        nh = len(hubs)
        nWJ += len(L["photo"]) + nh * ln
        nUJ += len(L["Ui"]) + nh * lm + nh * (nh + 1) // 2
        for p, f in zip(L["photo"], L["feature"]):
            W.add((gp[int(p)], gf[int(f)]))
        for s, h in enumerate(hubs):
            W.update((h, f) for f in gf)
            U.update((min(a, h), max(a, h)) for a in gp)
            U.update((min(h, h2), max(h, h2)) for h2 in hubs[s:])
        for a, b in zip(L["Ui"], L["Uj"]):
            ga, gb = gp[int(a)], gp[int(b)]
            U.add((min(ga, gb), max(ga, gb)))
    return W, U, nWJ, nUJ


def oracle_dense_h(oracle, dicts, mono, G, W, U):
    """The oracle's H, dense.  H v costs one assembly, so the unit vectors of block columns whose rows (known from the labels: W, U)
    do not meet go into one product; a product with a random vector then checks that nothing of H lies outside those rows."""
    m, n = int(G["m"]), int(G["n"])
    R = 6 * m + 3 * n
    start = [6 * i for i in range(m)] + [6 * m + 3 * i for i in range(n)]
    width = [6] * m + [3] * n
    adj = [{i} for i in range(m + n)]
    for a, b in U:
        adj[a].add(b); adj[b].add(a)
    for p, f in W:
        adj[p].add(m + f); adj[m + f].add(p)
    rows = [np.concatenate([np.arange(start[j], start[j] + width[j]) for j in sorted(a)]) for a in adj]
    H = np.zeros((R, R))
    for nodes, wd in ((range(m), 6), (range(m, m + n), 3)):
        groups = []  # [members, union of their rows]
        for i in nodes:
            for g in groups:
                if not (g[1] & adj[i]):
                    g[0].append(i); g[1] |= adj[i]
                    break
            else:
                groups.append([[i], set(adj[i])])
        for members, _ in groups:
            for c in range(wd):
                v = np.zeros(R)
                v[[start[i] + c for i in members]] = 1.0
                y = oracle.gn_hessian_times(dicts, mono, G, v)
                for i in members:
                    H[rows[i], start[i] + c] = y[rows[i]]
    v = np.random.default_rng(1).standard_normal(R)
    y = oracle.gn_hessian_times(dicts, mono, G, v)
    assert np.max(np.abs(H @ v - y)) <= 1e-12 * np.max(np.abs(y))
    return H


def h_err(got, exp):
    d = np.sqrt(np.diag(exp))
    return float(np.max(np.abs(got - exp) / np.outer(d, d)))


@functools.lru_cache(maxsize=None)
def _case(oracle, i):
    """Set i: the local maps as dicts, the oracle's tree result G, the state after two oracle polish steps, the label structure, and the
    oracle's dense H at both states.  Computed once and shared; nothing in it is changed by a test."""
    mono, n, npf, vis, kw = SETS[i]
    maps = synth.make_mono_set(n, npf, vis, seed=9, **kw) if mono else synth.make_stereo_set(n, npf, vis, seed=9, **kw)
    d = [oracle.localmap_to_dict(x) for x in maps]
    G, _, rc = oracle.divide_conquer(d, mono)
    assert rc == 0
    st2, _, _, _, rc = oracle.gn_polish(d, mono, G, 2)
    assert rc == 0
    G2 = dict(G, stVal=st2)
    W, U, nWJ, nUJ = label_structure(d, mono, G)
    return dict(mono=mono, d=d, G=G, G2=G2, W=W, U=U, nWJ=nWJ, nUJ=nUJ, H=oracle_dense_h(oracle, d, mono, G, W, U),
                H2=oracle_dense_h(oracle, d, mono, G2, W, U))


def _gauge_free(G, mono):
    m, n = int(G["m"]), int(G["n"])
    keep = np.ones(6 * m + 3 * n, bool)
    if mono:
        ids = -np.asarray(G["stno"])[:6 * m:6]
        pr, ps = int(np.nonzero(ids == G["Ref"])[0][0]), int(np.nonzero(ids == G["ScaP"])[0][0])
        keep[6 * pr:6 * pr + 6] = False
        keep[6 * ps + int(G["Fix"])] = False
    return keep


def _dense_sigma(H, G, mono):
    """Sigma = H^-1 with the Mono gauge rows / columns removed (0 there)."""
    keep = _gauge_free(G, mono)
    S = np.zeros_like(H)
    S[np.ix_(keep, keep)] = np.linalg.inv(H[np.ix_(keep, keep)])
    return S


def _sigma_err(got, exp, vr, vc):
    den = np.sqrt(np.maximum(vr[..., :, None] * vc[..., None, :], 1e-300))
    return float(np.max(np.abs(got - exp) / den))


@pytest.mark.parametrize("i", range(len(SETS)), ids=IDS)
def test_h_against_the_oracle(ctx, oracle, i):
    """dense_info(out) against the oracle's dense H, at the oracle's tree result and at the state after two oracle polish steps."""
    c = _case(oracle, i)
    for G, H in ((c["G"], c["H"]), (c["G2"], c["H2"])):
        out, F, b = ctx.gn_linearise(c["d"], c["mono"], G)
        e = h_err(dense_info(out), H)
        print(f"{IDS[i]}: H error {e:.3e}")
        assert e <= BAR


@pytest.mark.parametrize("i", range(len(SETS)), ids=IDS)
def test_canonical_form(ctx, oracle, i):
    c = _case(oracle, i)
    G = c["G"]
    out, _, _ = ctx.gn_linearise(c["d"], c["mono"], G)
    m, n = int(G["m"]), int(G["n"])
    assert out["m"] == m and out["n"] == n and out["nU"] == len(out["Ui"]) and out["nW"] == len(out["photo"])
    assert np.array_equal(out["stno"], G["stno"]) and np.array_equal(out["stVal"], G["stVal"])
    for k in ("Ref", "FRef", "ScaP", "Fix", "Sign", "FScaP", "FFix"):
        assert out[k] == G[k], k
    Ui, Uj = out["Ui"].astype(np.int64), out["Uj"].astype(np.int64)
    assert np.all(Ui <= Uj) and np.all(np.diff(Ui * m + Uj) > 0)
    fe, ph = out["feature"].astype(np.int64), out["photo"].astype(np.int64)
    assert np.all(np.diff(fe) >= 0) and np.all(np.diff(fe * m + ph) > 0)
    assert np.array_equal(out["FBlock"], np.searchsorted(fe, np.arange(n)))
    assert np.all(fe[out["FBlock"]] == np.arange(n))
    # exactly the pairs the labels give -- fewer than the working form holds: the set did coalesce
    assert set(zip(Ui.tolist(), Uj.tolist())) == c["U"] and out["nU"] == len(c["U"]) < c["nUJ"]
    assert set(zip(ph.tolist(), fe.tolist())) == c["W"] and out["nW"] == len(c["W"]) < c["nWJ"]
    print(f"{IDS[i]}: W {c['nWJ']} -> {out['nW']}, U {c['nUJ']} -> {out['nU']}")
    D = out["U"].reshape(-1, 6, 6)[Ui == Uj]
    assert len(D) == m
    assert np.max(np.abs(D - D.transpose(0, 2, 1))) <= 1e-14 * np.max(np.abs(D))
    assert len(out["pose_origin"]) == m and np.all((out["pose_origin"] >= 0) & (out["pose_origin"] < len(c["d"])))


def test_one_map_in_the_global_frame(ctx, oracle):
    """One Stereo local map, x = its own state and Ref: f is the identity, H = I_1 -- out has the input's pattern and its values."""
    L = _case(oracle, 0)["d"][0]
    x = dict(L, FRef=L["Ref"])
    out, F, b = ctx.gn_linearise([L], False, x, want_b=True)
    assert sorted(zip(out["Ui"].tolist(), out["Uj"].tolist())) == sorted(zip(np.minimum(L["Ui"], L["Uj"]).tolist(), np.maximum(L["Ui"], L["Uj"]).tolist()))
    assert sorted(zip(out["feature"].tolist(), out["photo"].tolist())) == sorted(zip(np.asarray(L["feature"]).tolist(), np.asarray(L["photo"]).tolist()))
    assert out["nU"] == len(L["Ui"]) and out["nW"] == len(L["photo"])
    assert h_err(dense_info(out), dense_info(L)) <= BAR
    assert abs(F) <= 1e-20 and np.max(np.abs(b)) <= 1e-9 * np.max(np.abs(out["U"]))


@pytest.mark.parametrize("i", range(len(SETS)), ids=IDS)
def test_b_and_obj(ctx, oracle, i):
    """b against the oracle's gradient at 1e-7 max|b|, F at 1e-9 relative, at the oracle's tree result.  At the state after two polish
    steps as well, where b has all but vanished (a small difference of terms of the first state's size): there it is held, as
    test_gpu_gn.py holds the gradient of a later iterate, against the first state's size."""
    c = _case(oracle, i)
    size = None
    for G in (c["G"], c["G2"]):
        out, F, b = ctx.gn_linearise(c["d"], c["mono"], G, want_b=True)
        eF, eb = oracle.gn_objective(c["d"], c["mono"], G)
        size = np.max(np.abs(eb)) if size is None else size
        print(f"{IDS[i]}: max|b| {np.max(np.abs(eb)):.3e}, b error {np.max(np.abs(b - eb)):.3e} (bound {1e-7 * size:.3e}), F error {abs(F - eF) / eF:.3e}")
        assert np.max(np.abs(b - eb)) <= 1e-7 * size
        assert abs(F - eF) <= 1e-9 * eF


@pytest.mark.parametrize("i", range(len(SETS)), ids=IDS)
def test_weights(ctx, oracle, i):
    c = _case(oracle, i)
    d, mono, G = c["d"], c["mono"], c["G"]
    w = np.random.default_rng(100 + i).uniform(0.1, 1.0, len(d))
    out, F, b = ctx.gn_linearise(d, mono, G, weight=w, want_b=True)
    ds = _scaled(d, w)
    e = h_err(dense_info(out), oracle_dense_h(oracle, ds, mono, G, c["W"], c["U"]))
    eF, eb = oracle.gn_objective(ds, mono, G)
    print(f"{IDS[i]}: weighted H error {e:.3e}")
    assert e <= BAR
    assert np.max(np.abs(b - eb)) <= 1e-7 * np.max(np.abs(eb)) and abs(F - eF) <= 1e-9 * eF
    # no weights = all ones: the same structure bit for bit, the same values to the rounding of the assembly's atomic sums
    o0, F0, _ = ctx.gn_linearise(d, mono, G)
    o1, F1, _ = ctx.gn_linearise(d, mono, G, weight=np.ones(len(d)))
    for k in ("Ui", "Uj", "photo", "feature", "FBlock", "stno", "stVal", "pose_origin"):
        assert np.array_equal(o0[k], o1[k]), k
    assert all(o0[k] == o1[k] for k in ("m", "n", "nU", "nW", "Ref", "FRef", "ScaP", "Fix", "Sign", "FScaP", "FFix"))
    assert h_err(dense_info(o1), dense_info(o0)) <= 1e-13


def test_bad_weights_are_refused(ctx, oracle):
    c = _case(oracle, 1)
    n = len(c["d"])
    for bad in (-0.5, float("nan"), float("inf")):
        w = np.ones(n)
        w[3] = bad
        with pytest.raises(api.LsfmError):
            ctx.gn_linearise(c["d"], c["mono"], c["G"], weight=w)
    with pytest.raises(api.LsfmError):  # a local feature that is not in the global state: lsfm_gn_polish's checks
        G = c["G"]
        ctx.gn_linearise(c["d"], c["mono"], dict(G, n=G["n"] - 1, stno=G["stno"][:-3], stVal=G["stVal"][:-3]))
    out, F, _ = ctx.gn_linearise(c["d"], c["mono"], c["G"], weight=np.zeros(n))  # (0 is allowed: the map drops out)
    assert F == 0.0 and not np.any(out["U"]) and not np.any(out["W"]) and not np.any(out["V"])
    assert h_err(dense_info(ctx.gn_linearise(c["d"], c["mono"], c["G"])[0]), c["H"]) <= BAR


@pytest.mark.parametrize("i", COV_SETS, ids=[IDS[i] for i in COV_SETS])
def test_it_composes_with_the_covariances(ctx, oracle, i):
    """lsfm_map_covariance and lsfm_map_covariance_columns on the result against a dense inverse of the oracle's H."""
    c = _case(oracle, i)
    mono, G = c["mono"], c["G"]
    m, n = int(G["m"]), int(G["n"])
    out, _, _ = ctx.gn_linearise(c["d"], mono, G)
    S = _dense_sigma(c["H"], G, mono)
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


@pytest.mark.parametrize("i", [0, 1, 2], ids=IDS[:3])
def test_one_step_of_the_polish(ctx, oracle, i):
    """H d = b solved on the host from the result (Stereo: no gauge) is the step lsfm_gn_polish takes from the same state."""
    c = _case(oracle, i)
    G = c["G"]
    out, _, b = ctx.gn_linearise(c["d"], False, G, want_b=True)
    st, obj, gn, hv, rc = ctx.gn_polish(c["d"], False, G, 1)
    assert rc == 0 and hv[0] == 0
    x = np.asarray(G["stVal"]) + np.linalg.solve(dense_info(out), b)
    assert pose_param_err(x, st, G["stno"]) < 1e-6 and feat_param_err(x, st, G["stno"]) < 1e-6


# ---- the reason the feature exists: the corrupted-duplicate scenario of test_gpu_robust.py ---------------------------------------------
def _corrupted_copy(m, ang=0.1, shift=0.5):
    """Map m with its whole state moved by a rigid transform of its own frame: x -> R x + t for the positions, R_pose -> R_pose R^T."""
    d = copy.deepcopy(m)
    Rd, td = synth.rot_ypr(ang, 0.0, 0.0), np.array([shift, 0.0, 0.0])
    st = d.stVal.copy()
    for i in range(d.m):
        p = st[6 * i:6 * i + 6].copy()
        st[6 * i:6 * i + 3] = Rd @ p[:3] + td
        st[6 * i + 3:6 * i + 6] = synth.ypr_from_rot(synth.rot_ypr(*p[3:]) @ Rd.T)
    X = st[6 * d.m:].reshape(-1, 3)
    st[6 * d.m:] = (X @ Rd.T + td).reshape(-1)
    d.stVal = st
    return d


def _first_copy_of_each_pose(G):
    """The tree keeps a pose that two maps hold as a variable twice (a duplicated map's poses): the first copy stays."""
    m, stno = int(G["m"]), np.asarray(G["stno"])
    _, first = np.unique(stno[:6 * m:6], return_index=True)
    keep = np.sort(first)
    idx = np.concatenate([(6 * keep[:, None] + np.arange(6)).reshape(-1), np.arange(6 * m, len(stno))])
    out = dict(G, m=len(keep), stno=stno[idx].copy(), stVal=np.asarray(G["stVal"])[idx].copy())
    if G.get("pose_origin") is not None:
        out["pose_origin"] = np.asarray(G["pose_origin"])[keep]
    return out


@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
def test_covariances_follow_the_robust_weights(ctx, oracle, mono):
    """A clean 40-map set plus a corrupted duplicate of map 8 (moved 0.1 rad / 0.5 m), polished with Cauchy c = 2, 8 steps.  At the
    polished state the variances of the duplicate's poses are larger from the relinearisation with the polish's weights than from the one
    without (which counts the corrupted map in full), within a factor 1.5 of the clean set's own relinearised variances, while the
    unweighted ones are below those: overconfident.  The clean set is linearised at the same state as the other two: H_unweighted =
    H_clean + J^T I J of the duplicate holds at a common state only, and only then is "below" a property of the weights and not of
    where each matrix was linearised (two states that differ move a variance by more than a barely observed scalar gains)."""
    mono_, n, npf, vis, kw = SETS[5] if mono else SETS[2]
    maps = synth.make_mono_set(n, npf, vis, seed=9, **kw) if mono else synth.make_stereo_set(n, npf, vis, seed=9, **kw)
    j = 7
    bad = maps[:j + 1] + [_corrupted_copy(maps[j])] + maps[j + 1:]
    dc, db = [oracle.localmap_to_dict(x) for x in maps], [oracle.localmap_to_dict(x) for x in bad]
    Gc, _, rc = ctx.divide_conquer(dc, mono)
    assert rc == 0
    Gb, _, rc = ctx.divide_conquer(db, mono)
    assert rc == 0
    Gb = _first_copy_of_each_pose(Gb)
    assert Gb["m"] == Gc["m"] and Gb["n"] == Gc["n"]
    rob, _, _, _, _, w, rc = ctx.gn_polish_robust(db, mono, Gb, 8, 2, 2.0)
    assert rc == 0
    Gr = dict(Gb, stVal=rob)
    Hw, _, _ = ctx.gn_linearise(db, mono, Gr, weight=w)
    H1, _, _ = ctx.gn_linearise(db, mono, Gr)
    Hc, _, _ = ctx.gn_linearise(dc, mono, {k: v for k, v in Gr.items() if k != "pose_origin"})  # (its origins count the duplicate)
    vw, v1, vc = (np.einsum("kii->ki", ctx.covariance(H, mono)["pose"]) for H in (Hw, H1, Hc))
    ids = [int(-x) for x in np.asarray(maps[j].stno)[:6 * maps[j].m:6]]
    rb = {int(-x): p for p, x in enumerate(np.asarray(Gb["stno"])[:6 * int(Gb["m"]):6])}
    vw, v1, vc = (v[[rb[q] for q in ids]] for v in (vw, v1, vc))
    free = vc > 0  # (Mono: a gauge scalar has variance 0 in all three)
    assert np.any(free)
    vw, v1, vc = vw[free], v1[free], vc[free]
    others = np.delete(w, j + 1)
    print(f"{'Mono' if mono else 'Stereo'}: w dup {w[j + 1]:.3e}, min other {np.min(others):.3f}; variances of the duplicate's poses: weighted / unweighted "
          f"{np.min(vw / v1):.3f}..{np.max(vw / v1):.3f}, weighted / clean {np.min(vw / vc):.3f}..{np.max(vw / vc):.3f}, "
          f"unweighted / clean {np.min(v1 / vc):.3f}..{np.max(v1 / vc):.3f}")
    assert np.all(vw > v1)
    assert np.all(vw <= 1.5 * vc) and np.all(vw * 1.5 >= vc)
    assert np.all(v1 < vc)
