"""-m gpu: lsfm_map_feature_pair_joint_gate (csrc/lsfm_jointgate.hip) on the device trees of the four split sets of test_gpu_merge.py -- the
joint matrix C = A Sigma A^T of the candidate pairs and the sequential selection among them.  No reference counterpart: the expected C
is read off a dense numpy inverse of the device tree's map AS STORED (test_gpu_covariance.dense_sigma), the expected selection is
joint_gate_reference.select (long double) on that C.

Bars (BAR = 1e-9, the project's):
  C       |C_ij - ref| / sqrt(u_i u_j) < BAR, u = diag(Sigma_ff + Sigma_gg) of the row's pair: section 17's metric, the marginal sums as units
  status  equal to the reference, after the assertion that no delta and no d2 lies within 1e-6 relative of tau
  delta   as section 17 derives its d^2 bar.  With D = diag(C_XX)^1/2 and C_s = D^-1 C_XX D^-1 over the rows X of a set of pairs, an error E with
          |E_ij| <= BAR sqrt(u_i u_j) is |D^-1 E D^-1|_ij <= BAR sqrt(rho_i rho_j), rho_i = u_i / C_ii, a matrix of 2-norm <= BAR sum_X rho_i; D2(X) =
          y^T C_s^-1 y then moves by at most r(X) = kappa_2(C_s) BAR sum_X rho_i relative.  delta_b = D2(Acc + b) - D2(Acc), so
              |delta_b - ref| <= 2 r(Acc + b) (D2_ref(Acc) + delta_ref,b),       |D2 - ref| <= r(Acc_final) D2_ref
          (kappa and the sum grow with the set, so r(Acc + b) covers both terms).  As section 18 caps its bar, no r used here exceeds
          merge_reference.CAP = 1e-3: every r, r(Acc_final) and each r(Acc + b), enters as min(r, CAP), so the bar can never go vacuous -- where the
          derivation gives more than CAP the test asks for MORE than the derivation (met with a wide margin: the measured errors are 1e-12).  On
          the lists of the split sets r(Acc_final) <= CAP is asserted as well.  The one list where it does not hold is the designed Mono list with
          the gauge poses' features at tau = inf, whose accepted C has kappa_s 5.6e3 and r = 1.2e-3; there the bar is CAP itself.  kappa_s and the
          uncapped r are measured here and printed."""
import ctypes as C

import numpy as np
import pytest

import feature_cov_reference as fref
import joint_gate_reference as jref
import merge_reference as mref
from linearsfm_amd import api, synth
from test_gpu_covariance import BAR, SMALL, _tree_map
from test_gpu_feature_columns import small
from test_gpu_feature_gate import _designed_pairs
from test_gpu_merge import _split

pytestmark = pytest.mark.gpu
SETS = [(2, 8), (3, 32), (6, 8), (7, 32)]  # (index into SMALL, features split): Stereo / Mono, 9 and 40 maps
TAU = jref.TAU


def _units(Sig, m, pairs):
    dg = np.diag(Sig)[6 * m:].reshape(-1, 3)
    return (dg[pairs[:, 0]] + dg[pairs[:, 1]]).ravel()


def _r(Cref, u, members):
    """r(X) of the module docstring for the pairs `members`, and kappa_s."""
    rows = np.concatenate([np.arange(3 * a, 3 * a + 3) for a in members])
    kap = jref.scaled_condition(Cref, members)
    return kap * BAR * float(np.sum(u[rows] / np.diag(Cref)[rows])), kap


def _check_joint(ctx, mono, G, Sig, pairs, tau, what, order=None, under_cap=True):
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    m, K = int(G["m"]), len(pairs)
    out = ctx.feature_pair_joint_gate(G, mono, pairs, tau=tau, order=order, want_C=True)
    Cref, d = jref.joint_matrix(Sig, m, pairs), jref.state_diff(G, pairs)
    u = _units(Sig, m, pairs)
    e_C = float(np.max(np.abs(out["C"] - Cref) / np.sqrt(np.outer(u, u))))
    # the individual d2: the gate's, within the gate's bars (section 17); the default order is a function of ITS bits alone, so where the caller
    # gives no order the expected selection runs in the order those bits give (a pair listed twice ties exactly in exact arithmetic)
    d2_ref = jref.individual_d2(Cref, d)
    bars = fref.d2_bars(np.stack([Cref[3 * b: 3 * b + 3, 3 * b: 3 * b + 3] for b in range(K)]), np.stack([np.diag(u[3 * b: 3 * b + 3]) for b in range(K)]))
    assert np.all(np.abs(out["d2"] - d2_ref) / d2_ref < bars)
    used = jref.default_order(out["d2"]) if order is None else order
    ref = jref.select(Cref, d, pairs, tau, order=used, dtype=np.longdouble)
    mar = jref.margins(ref, tau)
    r_raw, kap = _r(Cref, u, ref["accepted"]) if ref["accepted"] else (BAR, 1.0)
    r_fin = min(r_raw, mref.CAP)
    acc, run, worst, r_most = [], 0.0, 0.0, 0.0
    for b in (int(b) for b in ref["order"]):
        if ref["status"][b] == 2 or not np.isfinite(ref["delta"][b]):
            continue
        rb, _ = _r(Cref, u, acc + [b])
        r_most = max(r_most, rb)
        rb = min(rb, mref.CAP)
        worst = max(worst, abs(out["delta"][b] - ref["delta"][b]) / (2.0 * rb * (run + ref["delta"][b])))
        if ref["status"][b] == 1:
            acc.append(b)
            run += ref["delta"][b]
    e_D2 = abs(out["D2"] - ref["D2"]) / ref["D2"] if ref["D2"] > 0 else abs(out["D2"])
    print(f"joint gate {what}: K {K}, accepted {len(ref['accepted'])}, implied {ref['implied']}, steps {out['steps']}, C error {e_C:.2e}, margin {mar:.3g}, "
          f"kappa_s {kap:.3g}, r(accepted) {r_raw:.2e}, largest r(Acc + b) {r_most:.2e} (each capped at {mref.CAP:.0e}), delta err / bar {worst:.2e}, D2 {out['D2']:.9g} (ref {ref['D2']:.9g}), "
          f"D2 err {e_D2:.2e}, last_corr {out['last_corr'].max():.1e}")
    assert out["converged"] and out["steps"] >= 1
    assert mar > jref.REL
    if under_cap:
        assert r_raw <= mref.CAP
    assert e_C < BAR
    assert np.array_equal(out["C"], out["C"].T)
    assert np.array_equal(out["status"], ref["status"])
    assert out["accepted"] == len(ref["accepted"]) and out["implied"] == ref["implied"] and out["dof"] == 3 * out["accepted"]
    assert np.array_equal(np.isnan(out["delta"]), np.isnan(ref["delta"])) and np.all(out["delta"][ref["status"] == 2] == 0.0)
    assert worst <= 1.0 and e_D2 <= r_fin
    return out, ref, r_fin


def _merge_d2_agrees(ctx, mono, G, pairs, out, ref, r_fin, what):
    """merge_features' D^2 of exactly the accepted pairs against the selection's: each within its own bar of the reference."""
    accp = pairs[ref["accepted"]]
    mg = ctx.merge_features(G, mono, accp)
    _, members = mref.classes(int(G["n"]), accp)
    c = mref.quad_term(G, members) / ref["D2"]
    rel = abs(mg["d2"] - out["D2"]) / ref["D2"]
    print(f"      merge_features of the {len(accp)} accepted pairs {what}: D2 {mg['d2']:.9g}, dof {mg['dof']}, rel {rel:.2e} (bars {r_fin:.1e} + {BAR * max(1.0, c):.1e})")
    assert mg["dof"] == out["dof"]
    assert rel <= r_fin + BAR * max(1.0, c)


# ---- 1. the candidate lists of the four split sets ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,count", SETS)
def test_candidates_of_split_sets(ctx, i, count):
    mono, G, Sig, split = _split(ctx, i, count)
    pairs = jref.candidate_list(G, Sig, TAU)
    out, ref, r_fin = _check_joint(ctx, mono, G, Sig, pairs, TAU, f"{SMALL[i][:2]} x{count}")
    acc = {tuple(map(int, pairs[k])) for k in ref["accepted"]}
    assert {tuple(sorted(map(int, p))) for p in split} <= acc  # every true pair is kept
    _merge_d2_agrees(ctx, mono, G, pairs, out, ref, r_fin, f"{SMALL[i][:2]}")


# ---- 2. the lists at 10 tau: chunk edges 64 and 128 and the cross blocks between chunks ---------------------------------------------------------
@pytest.mark.parametrize("i,count,K", [(3, 32, 39), (7, 32, 167)])
def test_larger_lists(ctx, i, count, K):
    mono, G, Sig, split = _split(ctx, i, count)
    pairs = jref.candidate_list(G, Sig, 10.0 * TAU)
    assert len(pairs) == K
    small_ = jref.candidate_list(G, Sig, TAU)
    out, ref, _ = _check_joint(ctx, mono, G, Sig, pairs, TAU, f"{SMALL[i][:2]} x{count} at 10 tau")
    a = ctx.feature_pair_joint_gate(G, mono, small_)
    assert {tuple(pairs[k]) for k in np.nonzero(out["status"] == 1)[0]} == {tuple(small_[k]) for k in np.nonzero(a["status"] == 1)[0]}
    # a caller's order: the reverse of the default one is another selection, checked the same way
    _check_joint(ctx, mono, G, Sig, pairs, TAU, f"{SMALL[i][:2]} x{count} at 10 tau, reversed order", order=ref["order"][::-1])


# ---- 3. tau = inf on a cycle-free list: the merge's D^2 of the whole list -----------------------------------------------------------------------
@pytest.mark.parametrize("i,count", SETS)
def test_tau_inf_equals_merge(ctx, i, count):
    mono, G, Sig, split = _split(ctx, i, count)
    pairs = np.asarray(split, np.int32)  # disjoint pairs: cycle-free
    out, ref, r_fin = _check_joint(ctx, mono, G, Sig, pairs, np.inf, f"split pairs, tau = inf {SMALL[i][:2]}")
    assert out["accepted"] == count and out["implied"] == 0
    _merge_d2_agrees(ctx, mono, G, pairs, out, ref, r_fin, "(the whole list)")


# ---- 4. K = 1 is the gate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [2, 6])
def test_one_pair_is_the_gate(ctx, i):
    mono, G, Sig = small(ctx, i)
    for f, g in fref.seeded_pairs(int(G["n"]), 3):
        covA, marg = fref.route_a(Sig, G, np.array([[f, g]]))
        bar = fref.d2_bars(covA, marg)[0]
        gate = ctx.feature_pair_gate(G, mono, [[f, g]])
        out = ctx.feature_pair_joint_gate(G, mono, [[f, g]], tau=np.inf, want_C=True)
        assert out["status"].tolist() == [1] and out["accepted"] == 1
        assert abs(out["delta"][0] - out["d2"][0]) <= 1e-13 * out["d2"][0] and out["D2"] == out["delta"][0]
        assert abs(out["d2"][0] - gate["d2"][0]) / gate["d2"][0] < bar
        assert fref.cov_err(out["C"][None], gate["cov_diff"], np.einsum("kii->ki", marg)) < BAR
        rej = ctx.feature_pair_joint_gate(G, mono, [[f, g]], tau=0.5 * out["d2"][0])
        assert rej["status"].tolist() == [0] and rej["accepted"] == 0 and rej["D2"] == 0.0
        assert abs(rej["delta"][0] - out["delta"][0]) < 2.0 * bar * out["delta"][0]  # (two solves, each within the gate's bar)


# ---- 5. Mono lists with features of the gauge poses; pairs twice, reversed ------------------------------------------------------------------------
def test_gauge_pose_features_and_repeats(ctx):
    mono, G, Sig = small(ctx, 7)
    pairs = np.array(_designed_pairs(G, True), np.int32)
    out, ref, _ = _check_joint(ctx, mono, G, Sig, pairs, np.inf, "designed pairs Mono 40, tau = inf", under_cap=False)
    assert out["implied"] >= 3  # the reversed pairs of the list
    _check_joint(ctx, mono, G, Sig, pairs, TAU, "designed pairs Mono 40")


# ---- 6. refusals and statuses -----------------------------------------------------------------------------------------------------------------
def test_arguments(ctx):
    mono, G, _ = small(ctx, 6)
    n = int(G["n"])
    raw = ctx.feature_pair_joint_gate_raw
    good = [[0, 1], [1, 2], [2, 0]]
    rc, out, _ = raw(G, mono, good, tau=np.inf)
    assert rc == 0 and sorted(out["status"].tolist()) == [1, 1, 2]
    for bad in ([], [[0, n]], [[-1, 0]], [[3, 3]], np.zeros((api.JOINT_GATE_MAX + 1, 2), np.int32) + [0, 1]):  # K, index, f == g, the cap
        rc, out, _ = raw(G, mono, bad)
        assert rc == -1 and out["steps"] == 0 and not out["status"].any() and not out["delta"].any() and out["accepted"] == 0, len(bad)
    for order in ([0, 1, 1], [0, 1, 3], [-1, 0, 1]):
        assert raw(G, mono, good, order=order)[0] == -1, order
    for tau in (0.0, -2.0, float("nan")):
        assert raw(G, mono, good, tau=tau)[0] == -1, tau
    assert raw(dict(G, Ref=10 ** 6), mono, good)[0] == -1  # what lsfm_map_covariance refuses
    h = api.HostMap(G)
    q = np.array([0, 1], np.int32)
    st, dl = np.zeros(1, np.int32), np.zeros(1)
    acc, imp, D2 = C.c_int(0), C.c_int(0), C.c_double(0.0)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    call = lambda status, delta: api.lib().lsfm_map_feature_pair_joint_gate(ctx._h, C.byref(h.c), 1, q.ctypes.data_as(ip), 1, None, 1.0, status, delta, None,
                                                                             None, C.byref(acc), C.byref(imp), C.byref(D2), None, None)
    assert call(None, dl.ctypes.data_as(dp)) == -1 and call(st.ctypes.data_as(ip), None) == -1
    assert call(st.ctypes.data_as(ip), dl.ctypes.data_as(dp)) == 0  # every optional output NULL
    # the context is usable: the same call again, and a tree run
    rc, out2, t = raw(G, mono, good, tau=np.inf, times=True)
    assert rc == 0 and sorted(out2["status"].tolist()) == [1, 1, 2] and len(t) == 6 and np.all(t >= 0) and t[4] > 0
    from test_gpu_covariance import _small_set
    G2 = _tree_map(ctx, _small_set(*SMALL[6]), True)
    assert np.array_equal(G2["stno"], G["stno"])


def test_not_positive_definite(ctx):
    """The indefinite map of test_gpu_covariance.test_not_positive_definite: the numerical status, nothing written."""
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
    rc, out, _ = ctx.feature_pair_joint_gate_raw(d, False, [[0, 1], [2, 3]])
    assert (rc == -7 or rc > 0) and out["steps"] == 0 and not out["status"].any() and not out["delta"].any() and out["D2"] == 0.0, rc
    with pytest.raises(api.LsfmError):
        ctx.feature_pair_joint_gate(d, False, [[0, 1]])
