"""-m gpu: lsfm_map_chi2 and lsfm_gn_polish_robust (csrc/lsfm_gn.hip, kernels: csrc/lsfm_gn_chi2.hip) -- the per-map chi^2 of the map-joining objective and the
Gauss-Newton polish that re-weights whole local maps by an M-estimator on chi2_k / dof_k (IRLS).  No reference counterpart (parity
UNPINNED).  The oracle checks both exactly without a change of its own: I_k enters F linearly, so scaling map k's U, W and V by w_k in
the map dicts turns the oracle's F into sum_k w_k chi2_k."""
import copy

import numpy as np
import pytest

from common import feat_param_err, pose_param_err
from linearsfm_amd import synth

pytestmark = pytest.mark.gpu

SETS = [(False, 2, 6, 4, {}), (False, 9, 8, 4, {}), (False, 40, 8, 5, dict(lap=12, home=4, revisit=0.5)),
        (True, 2, 6, 4, {}), (True, 9, 8, 4, {}), (True, 40, 8, 4, synth.SPIRAL)]


def _maps(mono, n, npf, vis, kw):
    return synth.make_mono_set(n, npf, vis, seed=9, **kw) if mono else synth.make_stereo_set(n, npf, vis, seed=9, **kw)


def _dicts(oracle, maps):
    return [oracle.localmap_to_dict(m) for m in maps]


def _scaled(dicts, w):
    out = []
    for d, wk in zip(dicts, w):
        e = dict(d)
        e["U"], e["W"], e["V"] = d["U"] * wk, d["W"] * wk, d["V"] * wk
        out.append(e)
    return out


def _weights(kind, s, c):
    """rho'(s) as include/lsfm.h states it, in the same operations as the device."""
    if kind == 1:
        return np.where(s <= c * c, 1.0, c / np.sqrt(s))
    return 1.0 / (1.0 + s / (c * c))


@pytest.mark.parametrize("mono,n,npf,vis,kw", SETS)
def test_chi2_against_the_oracle(ctx, oracle, mono, n, npf, vis, kw):
    """At the oracle's tree result: chi2_k is the oracle's F with every other map's information scaled by 0, the chi2 sum is F, dof is
    6 m_k + 3 n_k, and two calls give the same bits."""
    maps = _maps(mono, n, npf, vis, kw)
    d = _dicts(oracle, maps)
    G, _, rc = oracle.divide_conquer(d, mono)
    assert rc == 0
    chi2, dof = ctx.map_chi2(d, mono, G)
    assert np.array_equal(dof, [6 * m.m + 3 * m.n for m in maps])
    for k in range(n):
        w = np.zeros(n)
        w[k] = 1.0
        Fk, _ = oracle.gn_objective(_scaled(d, w), mono, G, False)
        assert abs(chi2[k] - Fk) <= 1e-10 * Fk, (k, chi2[k], Fk)
    F, _ = oracle.gn_objective(d, mono, G, False)
    assert abs(chi2.sum() - F) <= 1e-10 * F
    chi2b, dofb = ctx.map_chi2(d, mono, G)
    assert np.array_equal(chi2, chi2b) and np.array_equal(dof, dofb)


@pytest.mark.parametrize("mono", [False, True])
def test_kind_none_is_the_plain_polish(ctx, oracle, mono):
    """kind 0 runs lsfm_gn_polish's kernels with every weight 1.0 (x * 1.0 is exact).  The plain polish sums F and its system with
    atomics, so two plain calls already differ in the last bits (measured 1.2e-12 relative in F on the Mono spiral); the bars sit above
    that: F to 1e-11, the state to 1e-9, equal halvings, every weight exactly 1."""
    maps = _maps(mono, 40, 8, 5 if not mono else 4, dict(lap=12, home=4, revisit=0.5) if not mono else synth.SPIRAL)
    d = _dicts(oracle, maps)
    G, _, rc = oracle.divide_conquer(d, mono)
    assert rc == 0
    st, obj, gn, hv, rc = ctx.gn_polish(d, mono, G, 3)
    st0, obj0, gn0, hv0, chi2, w, rc0 = ctx.gn_polish_robust(d, mono, G, 3, 0, 1.0)
    assert rc == 0 and rc0 == 0
    assert np.max(np.abs(obj0 - obj) / obj) <= 1e-11
    assert np.array_equal(hv0, hv)
    assert np.max(np.abs(st0 - st)) <= 1e-9 * max(1.0, np.max(np.abs(st)))
    assert np.all(w == 1.0)
    exp, _ = ctx.map_chi2(d, mono, dict(G, stVal=st0))
    assert np.array_equal(chi2, exp)


@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("kind", [1, 2])
def test_one_irls_step_against_the_oracle(ctx, oracle, mono, kind):
    """One robust step from the oracle's tree result against the oracle's plain step on the map dicts scaled by the device's starting
    weights w = rho'(chi2 / dof).  c = 0.5 puts the threshold inside the spread of s_k on these sets, so the weights differ from 1.  Mono
    uses the 9-map set: on the 40-map spiral the oracle's weighted step already halves once, and one step is compared where both take it
    whole."""
    maps = _maps(False, 40, 8, 5, dict(lap=12, home=4, revisit=0.5)) if not mono else _maps(True, 9, 8, 4, {})
    d = _dicts(oracle, maps)
    G, _, rc = oracle.divide_conquer(d, mono)
    assert rc == 0
    c = 0.5
    chi2, dof = ctx.map_chi2(d, mono, G)
    w = _weights(kind, chi2 / dof, c)
    assert np.min(w) < 0.9
    got, obj, gn, hv, _, _, rc = ctx.gn_polish_robust(d, mono, G, 1, kind, c)
    exp, eobj, egn, ehv, erc = oracle.gn_polish(_scaled(d, w), mono, G, 1)
    assert rc == 0 and erc == 0
    assert hv[0] == 0 and ehv[0] == 0
    assert pose_param_err(got, exp, G["stno"]) < 1e-6 and feat_param_err(got, exp, G["stno"]) < 1e-6
    # G at the start is sum_k dof_k rho(s_k); the weighted gradient's size matches the oracle's on the scaled maps
    s = chi2 / dof
    rho = np.where(s <= c * c, s, 2 * c * np.sqrt(s) - c * c) if kind == 1 else c * c * np.log1p(s / (c * c))
    assert abs(obj[0] - np.sum(dof * rho)) <= 1e-12 * obj[0]
    assert abs(gn[0] - egn[0]) <= 1e-7 * egn[0]


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


def _in_order_of(st, G_from, G_to):
    """State st (labelled as G_from) in the variable order of G_to."""
    def blocks(G, v):
        m, stno = int(G["m"]), np.asarray(G["stno"])
        keys = [("p", int(x)) for x in stno[:6 * m:6]] + [("f", int(x)) for x in stno[6 * m::3]]
        vals = [v[6 * i:6 * i + 6] for i in range(m)] + [v[6 * m + 3 * i:6 * m + 3 * i + 3] for i in range(int(G["n"]))]
        return keys, vals
    kf, vf = blocks(G_from, st)
    kt, _ = blocks(G_to, G_to["stVal"])
    lut = dict(zip(kf, vf))
    return np.concatenate([lut[k] for k in kt])


@pytest.mark.parametrize("mono", [False, True])
def test_outlier_map_is_found_and_down_weighted(ctx, oracle, mono):
    """A clean set plus a corrupted duplicate of map 8 (its state moved by 0.1 rad and 0.5 m in its own frame).  Without the duplicate the
    set is the clean one, whose plain polish is the right answer.  Both polishes start from the device's tree result of the corrupted set.

    c and the bounds come from a CPU prototype of the same IRLS through the oracle (re-weight the dicts, one orc_gn_polish step, 8 times),
    Cauchy, c = 2: Stereo (40 maps, a lap): the duplicate's s = 365 at the tree result (the largest; the clean maps' median 0.29); after 8
    steps 118x closer to the clean answer than the plain polish, duplicate weight 4.7e-3, every other weight >= 0.84.  Mono (40 maps,
    spiral): s = 805 (median 0.63); 47x closer, duplicate weight 5.0e-3, every other >= 0.69.  Bars: >= 10x closer, duplicate weight
    < 0.02, every other > 0.5 (weights never exceed 1)."""
    maps = _maps(mono, 40, 8, 5 if not mono else 4, dict(lap=12, home=4, revisit=0.5) if not mono else synth.SPIRAL)
    j = 7
    bad = maps[:j + 1] + [_corrupted_copy(maps[j])] + maps[j + 1:]
    dc, db = _dicts(oracle, maps), _dicts(oracle, bad)
    Gc, _, rc = ctx.divide_conquer(dc, mono)
    assert rc == 0
    Gb, _, rc = ctx.divide_conquer(db, mono)
    assert rc == 0
    Gb = _first_copy_of_each_pose(Gb)
    assert Gb["m"] == Gc["m"]
    chi2, dof = ctx.map_chi2(db, mono, Gb)
    s = chi2 / dof
    assert int(np.argmax(s)) == j + 1, s
    clean, _, _, _, rc = ctx.gn_polish(dc, mono, Gc, 6)
    assert rc == 0
    clean = _in_order_of(clean, Gc, Gb)
    plain, _, _, _, rc = ctx.gn_polish(db, mono, Gb, 8)
    assert rc == 0
    rob, obj, _, hv, chi2r, w, rc = ctx.gn_polish_robust(db, mono, Gb, 8, 2, 2.0)
    assert rc == 0
    assert np.all(np.diff(obj) <= 1e-12 * obj[0])
    e_plain, e_rob = pose_param_err(plain, clean, Gb["stno"]), pose_param_err(rob, clean, Gb["stno"])
    print(f"{'Mono' if mono else 'Stereo'}: s dup {s[j + 1]:.3e}, error plain {e_plain:.3e} robust {e_rob:.3e} ({e_plain / e_rob:.1f}x), "
          f"w dup {w[j + 1]:.3e}, min other {np.min(np.delete(w, j + 1)):.3f}")
    assert e_rob * 10 <= e_plain
    assert w[j + 1] < 0.02
    assert np.all(np.delete(w, j + 1) > 0.5)


@pytest.mark.parametrize("config,kind,c", [("rs90", 2, 2.0), ("nc3500-512", 1, 0.3)])
def test_robust_properties_on_the_named_sets(ctx, oracle, config, kind, c):
    """From the device's own tree result: G never rises, halvings <= 8, the returned chi2 is lsfm_map_chi2 at the returned state bit
    for bit, and the returned weights are rho'(chi2 / dof) recomputed here."""
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
    st, obj, gn, hv, chi2, w, rc = ctx.gn_polish_robust(d, mono, G, steps, kind, c)
    assert rc == 0
    assert np.all(np.diff(obj) <= 1e-12 * obj[0]) and obj[-1] < obj[0]
    assert np.all(hv <= 8)
    exp, dof = ctx.map_chi2(d, mono, dict(G, stVal=st))
    assert np.array_equal(chi2, exp)
    ew = _weights(kind, chi2 / dof, c)
    assert np.max(np.abs(w - ew) / ew) <= 1e-15
    print(f"{config}: G {obj[0]:.6f} -> {obj[-1]:.6f}, halvings {hv.tolist()}, weights {np.min(w):.3f}..{np.max(w):.3f}")


def test_robust_refuses_bad_arguments(ctx, oracle):
    from linearsfm_amd import api
    maps = synth.make_stereo_set(5, 6, 4, seed=2)
    d = _dicts(oracle, maps)
    G, _, rc = ctx.divide_conquer(d, False)
    for kind, c in ((3, 1.0), (-1, 1.0), (1, 0.0), (2, -1.0), (1, float("nan")), (2, float("inf"))):
        with pytest.raises(api.LsfmError):
            ctx.gn_polish_robust(d, False, G, 1, kind, c)
    with pytest.raises(api.LsfmError):   # a local feature that is not in the global state
        ctx.map_chi2(d, False, dict(G, n=G["n"] - 1, stno=G["stno"][:-3], stVal=G["stVal"][:-3]))
    st, obj, gn, hv, chi2, w, rc = ctx.gn_polish_robust(d, False, G, 1, 2, 1.0)
    assert rc == 0 and obj[1] <= obj[0]
