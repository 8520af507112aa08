"""-m gpu: the selection of lsfm_map_feature_pair_joint_gate alone (csrc/lsfm_jointgate.hip: k_jc_permute, k_jc_panel, k_jc_solve,
k_jc_update) through lsfm_selftest_pair_select on crafted matrices -- panel edges without solving anything.  C = A Sigma A^T from a
random SPD Sigma on a few dozen points, d = A x for a draw x ~ N(0, Sigma), scaled so that the decisions have the margins asserted here.

Expected: joint_gate_reference.select(route="conditional", dtype=np.longdouble).  Status is compared exactly, after the assertion that no
delta and no d2 lies within 1e-6 relative of tau; every case is run twice and the two calls must agree bit for bit.  Bar on delta and D^2: delta_b = D2(Acc + b) - D2(Acc), each of the two a quadratic
form through a Cholesky factor of at most n = 3K rows, whose relative rounding error is bounded to first order by n u kappa_s (u =
2^-53, kappa_s the 2-norm condition number of the accepted C scaled to unit diagonal, taken from the reference).  So
    |delta_b - ref| <= 8 n u kappa_s (D2_ref(Acc before b) + delta_ref,b),      |D2 - ref| <= 8 n u kappa_s D2_ref
with 8 for the constants the first-order statement drops; 8 n u kappa_s <= 1e-9 is asserted on every case so the bar cannot go vacuous."""
import ctypes as C

import numpy as np
import pytest

import joint_gate_reference as jref
from linearsfm_amd import api

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
PANEL = 16  # pairs of a panel of the device code
_WORLD = {}


def _world(points, seed=0):
    if (points, seed) not in _WORLD:
        _WORLD[points, seed] = jref.crafted_world(points, seed)
    return _WORLD[points, seed]


def _check(ctx, Cm, d, ends, tau, order=None, what=""):
    ref = jref.select(Cm, d, ends, tau, order=order, dtype=np.longdouble)
    mar = jref.margins(ref, tau)
    out = ctx.selftest_pair_select(Cm, d, ends, tau, order=order)
    n = len(d)
    kap = jref.scaled_condition(Cm, ref["accepted"]) if ref["accepted"] else 1.0
    rel = 8.0 * n * U * kap
    run, worst = 0.0, 0.0
    for b in ref["order"]:
        if ref["status"][b] == 2 or not np.isfinite(ref["delta"][b]):
            continue
        scale = run + ref["delta"][b]
        worst = max(worst, abs(out["delta"][b] - ref["delta"][b]) / scale)
        if ref["status"][b] == 1:
            run = scale
    e_D2 = abs(out["D2"] - ref["D2"]) / ref["D2"] if ref["D2"] > 0 else abs(out["D2"])
    print(f"pair select {what}: K {len(ends)}, accepted {len(ref['accepted'])}, implied {ref['implied']}, margin {mar:.3g}, kappa_s {kap:.3g}, "
          f"delta err {worst:.2e}, D2 err {e_D2:.2e} (bar {rel:.2e})")
    assert mar > jref.REL
    assert rel <= 1e-9
    assert np.array_equal(out["status"], ref["status"])
    assert out["accepted"] == len(ref["accepted"]) and out["implied"] == ref["implied"]
    nan = np.isnan(ref["delta"])
    assert np.array_equal(np.isnan(out["delta"]), nan)
    assert np.all(out["delta"][ref["status"] == 2] == 0.0)
    assert worst <= rel and e_D2 <= rel
    # a second call gives the same bits: the union-find's parent array, the panels' skip flags and every sum are rebuilt the same way
    again = ctx.selftest_pair_select(Cm, d, ends, tau, order=order)
    assert np.array_equal(out["status"], again["status"]) and np.array_equal(out["delta"], again["delta"], equal_nan=True) and out["D2"] == again["D2"]
    return out, ref


@pytest.mark.parametrize("K", [1, 15, 16, 17, 49])
def test_sizes_default_order(ctx, K):
    """Every size around a panel edge, the default order (ascending d2), tau = chi^2_3 at 0.99: a mixture of decisions."""
    Sig, x = _world(60)
    ends = jref.crafted_tree(60, K)
    Cm, d = jref.crafted_problem(Sig, x, ends, scale=1.6)
    out, ref = _check(ctx, Cm, d, ends, jref.TAU, what=f"K={K}")
    assert K < 15 or 0 < len(ref["accepted"]) < K  # both decisions occur: what the margins are for
    # the default order handed in explicitly: the same bits as with none given
    expl = ctx.selftest_pair_select(Cm, d, ends, jref.TAU, order=ref["order"])
    assert np.array_equal(out["delta"], expl["delta"], equal_nan=True) and np.array_equal(out["status"], expl["status"]) and out["D2"] == expl["D2"]


def test_rejections_across_a_panel_edge(ctx):
    """Identity order; the last pair of panel 0 and the first of panel 1 are pushed far out and rejected, everything else is accepted: the
    zero columns sit on both sides of the edge, and panel 1 and the later panels are conditioned on 15 pairs of panel 0."""
    Sig, x = _world(60)
    K = 49
    ends = jref.crafted_tree(60, K)
    Cm, d = jref.crafted_problem(Sig, x, ends, scale=0.3)
    for b in (PANEL - 1, PANEL):
        d[3 * b: 3 * b + 3] += 40.0 * np.sqrt(np.diag(Cm)[3 * b: 3 * b + 3])
    out, ref = _check(ctx, Cm, d, ends, jref.TAU, order=np.arange(K), what="rejections at 15, 16")
    exp = np.ones(K, np.int64)
    exp[[PANEL - 1, PANEL]] = 0
    assert np.array_equal(ref["status"], exp)


def test_implied_pairs_from_an_earlier_panel(ctx):
    """Identity order, tau = inf.  Pair 40 is pair 3 reversed, pair 41 is pair 3 again, pair 42 closes a triangle over pairs 0 and its
    neighbour in the tree -- partners in panel 0, the implied pairs in panel 2."""
    Sig, x = _world(60)
    K = 49
    ends = jref.crafted_tree(60, K)
    a, b = ends[0]
    k1 = next(k for k in range(1, PANEL) if set(ends[k]) & {a, b})
    other = [v for v in ends[k1] if v not in (a, b)][0]
    far = b if a in ends[k1] else a
    ends[40] = ends[3][::-1]
    ends[41] = ends[3]
    ends[42] = (far, other)
    Cm, d = jref.crafted_problem(Sig, x, ends)
    out, ref = _check(ctx, Cm, d, ends, np.inf, order=np.arange(K), what="implied")
    exp = np.ones(K, np.int64)
    exp[[40, 41, 42]] = 2
    assert np.array_equal(ref["status"], exp) and out["implied"] == 3


def test_everything_rejected_and_everything_accepted(ctx):
    Sig, x = _world(60)
    K = 49
    ends = jref.crafted_tree(60, K)
    Cm, d = jref.crafted_problem(Sig, x, ends)
    out, _ = _check(ctx, Cm, d, ends, 1e-9, what="all rejected")
    assert out["accepted"] == 0 and out["D2"] == 0.0 and not out["status"].any()
    out, ref = _check(ctx, Cm, d, ends, np.inf, what="all accepted")
    assert out["accepted"] == K
    # all accepted: D^2 is the quadratic form of the whole list, whatever the order
    full = float(d @ np.linalg.solve(Cm, d))
    assert abs(out["D2"] - full) <= 1e-9 * full


def test_callers_order_against_default(ctx):
    """The reverse of the default order is another selection (checked against the reference in that order); with everything accepted the
    two orders give the same D^2 and different deltas."""
    Sig, x = _world(60)
    K = 49
    ends = jref.crafted_tree(60, K)
    Cm, d = jref.crafted_problem(Sig, x, ends, scale=1.6)
    dflt, ref = _check(ctx, Cm, d, ends, jref.TAU, what="default order")
    rev, _ = _check(ctx, Cm, d, ends, jref.TAU, order=ref["order"][::-1], what="reversed order")
    assert not np.array_equal(dflt["delta"], rev["delta"], equal_nan=True)
    a, _ = _check(ctx, Cm, d, ends, np.inf, what="default order, tau = inf")
    b, _ = _check(ctx, Cm, d, ends, np.inf, order=ref["order"][::-1], what="reversed order, tau = inf")
    assert abs(a["D2"] - b["D2"]) <= 1e-9 * a["D2"] and not np.array_equal(a["delta"], b["delta"])


def test_nan_individual_distance(ctx):
    """A pair whose own block is not positive definite has d2 = NaN: status 0, delta NaN, last in the default order, the rest unaffected."""
    Sig, x = _world(60)
    K = 17
    ends = jref.crafted_tree(60, K)
    Cm, d = jref.crafted_problem(Sig, x, ends, scale=0.3)
    Cm[15, 15] = -1.0
    out, ref = _check(ctx, Cm, d, ends, jref.TAU, what="NaN d2")
    assert ref["status"][5] == 0 and np.isnan(out["delta"][5]) and ref["order"][-1] == 5


def test_cap_and_refusals(ctx):
    """K = 2048 once (tau = inf on a tree: every pair accepted, the expected deltas are the squared blocks of L^-1 d of one float64 Cholesky
    of the whole C, so the bar is doubled for the reference's own rounding); K = 2049 and the other bad arguments are refused."""
    import scipy.linalg as sla
    K = api.JOINT_GATE_MAX
    # Sigma = I / 2 + U U^T on 2 K points, the pairs a perfect matching (2 b, 2 b + 1): C = I + (A U)(A U)^T without a dense Sigma -- well
    # conditioned by construction (a tree of 2048 edges is not: its edge Laplacian alone has a condition number in the thousands)
    rng = np.random.default_rng(5)
    Um = 0.02 * rng.normal(size=(2 * K, 3, 24))
    x = Um @ rng.normal(size=24) + np.sqrt(0.5) * rng.normal(size=(2 * K, 3))
    B = (Um[0::2] - Um[1::2]).reshape(3 * K, 24)
    Cm = B @ B.T + np.eye(3 * K)
    Cm = np.triu(Cm) + np.triu(Cm, 1).T
    d = (x[0::2] - x[1::2]).ravel()
    ends = np.arange(2 * K).reshape(K, 2)
    L = np.linalg.cholesky(Cm)
    y = sla.solve_triangular(L, d, lower=True)
    exp = (y.reshape(-1, 3) ** 2).sum(axis=1)
    # kappa_s from above without a 6144 x 6144 decomposition: C_s = D^-2 + (D^-1 B)(D^-1 B)^T with D^2 = diag(C), so its eigenvalues lie in
    # [1 / max C_ii, 1 / min C_ii + lambda_max((D^-1 B)^T (D^-1 B))], a 24 x 24 problem
    dg = np.diag(Cm)
    Bs = B / np.sqrt(dg)[:, None]
    kap = float((1.0 / dg.min() + np.linalg.eigvalsh(Bs.T @ Bs)[-1]) * dg.max())
    rel = 2.0 * 8.0 * 3 * K * U * kap
    out = ctx.selftest_pair_select(Cm, d, ends, np.inf, order=np.arange(K))
    run = np.cumsum(exp)
    worst = float(np.max(np.abs(out["delta"] - exp) / run))
    e_D2 = abs(out["D2"] - run[-1]) / run[-1]
    print(f"pair select K={K}: kappa_s <= {kap:.3g}, delta err {worst:.2e}, D2 err {e_D2:.2e} (bar {rel:.2e})")
    assert rel <= 1e-9
    assert np.all(out["status"] == 1) and out["accepted"] == K and out["implied"] == 0
    assert worst <= rel and e_D2 <= rel
    again = ctx.selftest_pair_select(Cm, d, ends, np.inf, order=np.arange(K))
    assert np.array_equal(out["delta"], again["delta"]) and out["D2"] == again["D2"]  # 128 panels, 381 tile rows: the same bits
    # refusals: nothing is read before the checks, so small buffers do
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    buf, ibuf = np.zeros(64), np.arange(64, dtype=np.int32)
    acc, imp, D2 = C.c_int(0), C.c_int(0), C.c_double(0.0)

    def raw(K, order, tau):
        return api.lib().lsfm_selftest_pair_select(ctx._h, K, buf.ctypes.data_as(dp), buf.ctypes.data_as(dp), ibuf.ctypes.data_as(ip),
                                                   order.ctypes.data_as(ip) if order is not None else None, tau, ibuf.ctypes.data_as(ip),
                                                   buf.ctypes.data_as(dp), C.byref(D2), C.byref(acc), C.byref(imp))
    assert raw(K + 1, None, 1.0) == -1 and raw(0, None, 1.0) == -1
    for tau in (0.0, -1.0, float("nan")):
        assert raw(2, None, tau) == -1
    for bad in ([0, 0], [0, 2], [-1, 0]):
        assert raw(2, np.array(bad, np.int32), 1.0) == -1
    small, ends2 = np.eye(6), np.array([[0, 1], [2, 2]])
    assert ctx.selftest_pair_select(small, np.ones(6), ends2, 1.0, raw=True)[0] == -1  # a pair that names one endpoint twice
    ok = ctx.selftest_pair_select(small, np.ones(6), [[0, 1], [1, 2]], np.inf)  # the context is still usable
    assert ok["accepted"] == 2 and ok["D2"] == 6.0
