"""-m gpu: the one-launch dense path for camera systems of at most 16 poses (csrc/lsfm_small.hip, k_small_solve) on systems and batches
built to order (crafted_small.py), so that the run-pointer chunks, the super-passes, the W rows parked in LDS, the strip masks, the
four instances of the kernel and the layout of a batch are chosen, not met by chance.

Single systems: lsfm_solve_stereo / lsfm_solve_mono with set_small_solve(16) -- the production route solve_batch ->
solve_level_dense -- against common.dense_reference_solve, max |d| / max(1, |x|) over poses and over features, at test_gpu_parity.py's
DENSE_TOL = 1e-10; the same call twice gives the same bits.
Batches: lsfm_selftest_small (host plumbing only: G systems back to back in a batch's numbering, one small_solve_launch, the outputs
prefilled by the caller so that what the kernel did not write shows).  Every segment against its own exact solution at DENSE_TOL; a
segment in a batch against the same system alone at the same instance, bit for bit.
test_crafted_small_cpu.py shows on the CPU that every case reaches the branch named here and that the yardstick's own floor is below
1e-13.

Which branch a case reaches (m poses, n features):
  p1 (1, 17)  p2a (2, 16)  p2b (2, 257)     the 1-strip instance; a second pass of one feature; exactly one pass; a second chunk of
                                            run pointers and a super-pass of ONE feature
  p3 (3, 65)  p5a (5, 64)  p5b (5, 321)     the 2-strip instance at both edges; a super-pass + 1; exactly one; 256 + 64 + 1
  p6 (6, 15)  p8a (8, 256)  p8b (8, 513)    the 3-strip instance at both edges; a short pass; exactly one chunk (entry 256 read, no
                                            reload); two reloads (a buffer reused), super-passes of up to 389 blocks
  p9 (9, 63)  p16a (16, 1)  p16b (16, 600)  the 6-strip instance at both edges; one feature seen by all; tiles of features seen by 2-6
              p16c (16, 192)                poses (passes with two, three, four, six strips; 0.7 of the (pass, tile) pairs off; poses 2,
                                            5, 10, 13, whose rows lie in two strips, alone in theirs); every feature by every pose:
                                            > 1100 blocks a super-pass, ~90 repeats behind the LDS part each
  w170 (8, 34)  w171 (8, 57)                one super-pass of exactly 170 blocks (all parked) / 171 (block 170: pose parked, rows not)
  u16 (16, 200)                             poses 8-10 seen by nothing: strip 3 is never on, its rows of S are U's
  du5 (5, 100)                              every U block stored as two addends
  g3 (3, 80)  g9 (9, 150)                   Mono gauge: a seen pose's block and a scalar of another seen pose fixed
  v8 (8, 100)                               one V_f with an eigenvalue of -1e-3 of its largest
  a8, a9, a16 (crafted_system.CASES)        the K9 cases of this size, which only the pipeline had seen
Repeated (pose, feature) blocks are in every case but w170 / w171, one observation in ten.

Measured on an MI355X (information, not the bar):
  solve, poses / features:  p1 1.7e-16 / 8.7e-16  p2a 1.7e-16 / 3.3e-16  p2b 1.7e-16 / 1.4e-15  p3 2.2e-16 / 1.0e-15  p5a 5.6e-16 / 1.1e-15
                       p5b 5.6e-17 / 1.3e-15  p6 7.8e-16 / 5.6e-16  p8a 1.1e-16 / 2.1e-15  p8b 2.8e-17 / 5.3e-16  p9 4.0e-16 / 1.1e-15
                       p16a 2.4e-15 / 3.3e-16  p16b 3.2e-16 / 2.9e-15  p16c 5.6e-17 / 2.1e-17  w170 1.6e-16 / 1.1e-16  w171 2.2e-16 / 2.2e-16
                       u16 2.0e-16 / 9.4e-16  du5 2.2e-16 / 7.8e-16  g3 (Mono gauge) 3.3e-16 / 7.4e-16  g9 (Mono gauge) 5.6e-17 / 4.9e-16
                       a8 5.6e-17 / 1.9e-15  a9 2.2e-16 / 6.2e-16  a16 5.6e-17 / 2.2e-16;  every second run: the same bits
  v8 alone: refused with the not-positive-definite error; as segment 6 of the mixed batch: status [0, 7]
  batches: every segment of the mixed batch, at every instance, beside the bad segments, in the gauge batch and behind the segment
                       without features has the figures of its system above (it is the same bits); max_rel 1.2e-16; the segment
                       without features 1.6e-16; 2048 segments, worst poses / features: p1 1.1e-15 / 3.1e-15  p2a 8.3e-16 / 1.1e-15
                       p3 5.0e-16 / 1.4e-15  p6 1.7e-15 / 1.7e-15
  No case exposed a fault of k_small_solve or of its launch plumbing.  That the tests can fail was shown once on scratch builds with one
  arithmetic change each: the W rows read from memory behind the parked ones scaled by 1 + 1e-6 -> p5b, p8b, p16c, w171, g9, a8, a9, a16
  and the batches that hold one of them; the second strip of a straddling pose left out of the mask -> p3, p6, p16b, g3, a8, a9 and
  every batch with one of them.
"""
import numpy as np
import pytest

import crafted_small as sm
import crafted_system as cs
from common import dense_reference_solve
from linearsfm_amd import api
from test_gpu_parity import DENSE_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture()
def dense(ctx):
    """the dense path for every system it can hold (16 poses); leaves the default (5) behind, as test_gpu_small.py does"""
    try:
        ctx.set_small_solve(16)
        yield ctx
    finally:
        ctx.set_small_solve(5)


def _case(name):
    """(J, ea, eb, expected, mono, sa) of a case of crafted_small or of crafted_system"""
    if name in sm.CASES:
        return (sm.system(name),) + sm.rhs(name) + sm.expected_x(name)
    return (cs.system(name, 1),) + cs.rhs(name, 1) + cs.expected_x(name, 1)


# ---- single systems through lsfm_solve_* ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sm.GOOD + ["a8", "a9", "a16"])
def test_solve_against_the_exact_solution(dense, name):
    J, ea, eb, x, mono, sa = _case(name)
    assert J["m"] <= 16
    st, rc = dense.solve(J, ea, eb, mono, sa)
    assert rc == 0
    ep, ef = cs.state_metric(st, x, J["m"])
    print(f"{name} m {J['m']} n {J['n']}{' Mono gauge ' + str(sa) if mono else ''}: poses {ep:.3e} features {ef:.3e}")
    assert ep < DENSE_TOL and ef < DENSE_TOL
    if mono:
        assert st[sa[2]] == sa[3] and np.all(st[6 * sa[0]:6 * sa[0] + 6] == 0.0)
    again, rc = dense.solve(J, ea, eb, mono, sa)
    assert rc == 0 and np.array_equal(st, again)  # (no sum crosses work-groups: the same bits in every run)


def test_a_feature_without_a_factor(dense):
    """Refused with the not-positive-definite error, or reported as not converged, or within the bar -- never a clean return outside it."""
    J, ea, eb, x, _, _ = _case("v8")
    try:
        st, rc = dense.solve(J, ea, eb, False, None)
    except api.LsfmError as err:
        assert "not positive definite" in str(err)
        print(f"v8: refused ({err})")
        return
    ep, ef = cs.state_metric(st, x, J["m"]) if np.all(np.isfinite(st)) else (float("nan"),) * 2
    print(f"v8: rc {rc} poses {ep:.3e} features {ef:.3e}")
    assert rc != 0 or (ep < DENSE_TOL and ef < DENSE_TOL)


# ---- batches through lsfm_selftest_small ---------------------------------------------------------------------------------------------------
_ALONE = {}


def _alone(ctx, name, strips):
    """a case alone through the entry at the instance of `strips` strips: (state, status, max_rel).  Shared, never changed."""
    if (name, strips) not in _ALONE:
        B = sm.named_batch([name])
        xp, xf, st, mr = ctx.selftest_small(B, strips=strips)
        x = sm.segment(B, 0, xp, xf)
        x.setflags(write=False)
        _ALONE[name, strips] = (x, st.tolist(), mr)
    return _ALONE[name, strips]


def _expected(name):
    """the exact solution as the kernel leaves it: a fixed scalar is 0 (lsfm_solve_mono sets Sign afterwards)"""
    x, mono, sa = sm.expected_x(name)
    if mono:
        x = x.copy()
        x[sa[2]] = 0.0
    return x


def _within(B, g, xp, xf, x, what):
    m = int(B["pose_off"][g + 1] - B["pose_off"][g])
    got = sm.segment(B, g, xp, xf)
    assert np.all(np.isfinite(got)), what
    ep, ef = cs.state_metric(got, x, m) if len(x) > 6 * m else (float(np.max(np.abs(got - x) / np.maximum(1.0, np.abs(x)))), 0.0)
    print(f"{what}: poses {ep:.3e} features {ef:.3e}")
    assert ep < DENSE_TOL and ef < DENSE_TOL, what


def _prefill(B, seed=11):
    rng = np.random.default_rng(seed)
    return 7.0 + rng.random(6 * B["pose_off"][-1]), 7.0 + rng.random(3 * B["feat_off"][-1])


@pytest.fixture(scope="module")
def mixed(ctx):
    """the mixed batch in one launch (the 6-strip instance for all), prefilled: (B, prefill, x_pose, x_feat).  Shared, never changed."""
    B = sm.named_batch(sm.MIXED)
    pre = _prefill(B)
    xp, xf, st, mr = ctx.selftest_small(B, prefill=pre)
    assert st.tolist() == [0, 0] and 0.0 <= mr < 1e-8, (st, mr)
    print(f"mixed batch: max_rel {mr:.2e}")
    for a in pre + (xp, xf):
        a.setflags(write=False)
    return B, pre, xp, xf


def test_mixed_sizes_in_one_launch(ctx, mixed):
    B, _, xp, xf = mixed
    for g, k in enumerate(sm.MIXED):
        _within(B, g, xp, xf, _expected(k), f"mixed[{g}] {k}")
        one, st, mr = _alone(ctx, k, 6)
        assert st == [0, 0] and 0.0 <= mr < 1e-8
        assert np.array_equal(sm.segment(B, g, xp, xf), one), k  # nothing crosses segments: alone = in the batch, bit for bit


@pytest.mark.parametrize("name,strips", [("p2b", 1), ("p2b", 2), ("p2b", 3), ("p2b", 6), ("p5a", 2), ("p5a", 3), ("p5a", 6)])
def test_every_instance(ctx, name, strips):
    x, st, mr = _alone(ctx, name, strips)
    assert st == [0, 0] and 0.0 <= mr < 1e-8
    ep, ef = cs.state_metric(x, _expected(name), sm.system(name)["m"])
    print(f"{name} at {strips} strips: poses {ep:.3e} features {ef:.3e}")
    assert ep < DENSE_TOL and ef < DENSE_TOL


@pytest.mark.parametrize("with_x0", [True, False])
def test_carried_segments(ctx, mixed, with_x0):
    B, pre, full_p, full_f = mixed
    G = len(sm.MIXED)
    active = np.ones(G, bool)
    active[[1, 4, 7]] = False
    x0 = np.random.default_rng(5).standard_normal(6 * B["pose_off"][-1]) if with_x0 else None
    xp, xf, st, mr = ctx.selftest_small(B, active=active, x0=x0, prefill=pre)
    assert st.tolist() == [0, 0] and 0.0 <= mr < 1e-8
    for g in range(G):
        p, f = slice(6 * B["pose_off"][g], 6 * B["pose_off"][g + 1]), slice(3 * B["feat_off"][g], 3 * B["feat_off"][g + 1])
        if active[g]:
            assert np.array_equal(xp[p], full_p[p]) and np.array_equal(xf[f], full_f[f]), g
        else:
            assert np.array_equal(xp[p], x0[p] if with_x0 else np.zeros(p.stop - p.start)), g  # x0 bit for bit, or exactly 0
            assert np.array_equal(xf[f], pre[1][f]), g                                         # the features are not touched


def test_one_system_that_is_not_positive_definite_beside_good_ones(ctx, mixed):
    B, pre, _, _ = mixed
    Bb = dict(B)
    U = B["U"].reshape(-1, 36).copy()
    U[B["u_off"][3]:B["u_off"][4]] *= -1.0
    Bb["U"] = U.reshape(-1)
    xp, xf, st, mr = ctx.selftest_small(Bb, prefill=pre)
    assert st[1] == 4, st
    for g, k in enumerate(sm.MIXED):
        if g != 3:
            _within(B, g, xp, xf, _expected(k), f"beside a bad system: [{g}] {k}")
    assert np.array_equal(sm.segment(B, 3, xp, xf), sm.segment(B, 3, *pre))  # (it returns early: nothing of it is written)


def test_one_bad_v_beside_good_ones(ctx):
    names = list(sm.MIXED)
    names[6] = "v8"
    B = sm.named_batch(names)
    xp, xf, st, mr = ctx.selftest_small(B)
    print(f"v8 as segment 6: status {st.tolist()} max_rel {mr:.2e}")
    assert st[0] >= 1 or st[1] == 7, st
    for g, k in enumerate(names):
        if g != 6:
            _within(B, g, xp, xf, _expected(k), f"beside a bad V: [{g}] {k}")


def test_gauge_in_a_batch(ctx):
    names = ("g3", "p5a", "g9")
    B = sm.named_batch(names)
    fixed = np.concatenate([sm.gauge_mask(sm.system(k), sm.gauge(sm.system(k))) if k in sm.MONO else np.zeros(6 * sm.system(k)["m"], bool) for k in names])
    xp, xf, st, mr = ctx.selftest_small(B, fixed=fixed)
    assert st.tolist() == [0, 0] and 0.0 <= mr < 1e-8 and fixed.sum() == 14
    assert np.all(xp[fixed] == 0.0)
    for g, k in enumerate(names):
        _within(B, g, xp, xf, _expected(k), f"gauge batch [{g}] {k}")


def test_a_segment_without_features(ctx):
    K = sm.without_features(sm.system("p6"))
    ea6 = sm.rhs("p6")[0]
    B = sm.batch([(sm.system("p3"),) + sm.rhs("p3"), (K, ea6, np.zeros(0)), (sm.system("p5a"),) + sm.rhs("p5a")])
    xp, xf, st, mr = ctx.selftest_small(B)
    assert st.tolist() == [0, 0] and 0.0 <= mr < 1e-8 and B["feat_off"][1] == B["feat_off"][2]
    _within(B, 0, xp, xf, _expected("p3"), "before the segment without features: p3")
    _within(B, 1, xp, xf, dense_reference_solve(K, ea6, np.zeros(0), False), "without features (U x = ea): p6's poses")
    _within(B, 2, xp, xf, _expected("p5a"), "behind the segment without features: p5a")


def test_more_segments_than_are_resident(ctx):
    """2048 work-groups of the 3-strip instance (~70 KB of LDS each: the device holds a quarter of them at once): four systems in turn, every segment with right-hand sides of
    its own, every segment against the exact solution of its system"""
    G, each = 2048, 2048 // len(sm.MANY)
    rng = np.random.default_rng(2048)
    rhs, exact = {}, {}
    for k in sm.MANY:
        J = sm.system(k)
        EA = np.sqrt(np.diag(cs.dense_u(J))) * rng.standard_normal((each, 6 * J["m"]))
        EB = rng.standard_normal((each, 3 * J["n"]))
        rhs[k], exact[k] = (EA, EB), sm.solve_many(J, EA, EB)
    order = [(sm.MANY[g % len(sm.MANY)], g // len(sm.MANY)) for g in range(G)]
    B = sm.batch([(sm.system(k), rhs[k][0][i], rhs[k][1][i]) for k, i in order])
    xp, xf, st, mr = ctx.selftest_small(B)
    assert st.tolist() == [0, 0] and 0.0 <= mr < 1e-8
    assert np.all(np.isfinite(xp)) and np.all(np.isfinite(xf))
    worst = {k: [0.0, 0.0] for k in sm.MANY}
    for g, (k, i) in enumerate(order):
        ep, ef = cs.state_metric(sm.segment(B, g, xp, xf), exact[k][i], sm.system(k)["m"])
        worst[k] = [max(worst[k][0], ep), max(worst[k][1], ef)]
    print(f"{G} segments, the 3-strip instance: worst poses / features " + "  ".join(f"{k} {v[0]:.2e} / {v[1]:.2e}" for k, v in worst.items()))
    assert all(v[0] < DENSE_TOL and v[1] < DENSE_TOL for v in worst.values())


def test_u_blocks_as_two_addends(ctx, mixed):
    x, st, mr = _alone(ctx, "du5", 0)
    assert st == [0, 0] and 0.0 <= mr < 1e-8
    m = sm.system("du5")["m"]
    ep, ef = cs.state_metric(x, _expected("du5"), m)
    print(f"du5 alone: poses {ep:.3e} features {ef:.3e}")
    assert ep < DENSE_TOL and ef < DENSE_TOL
    names = sm.MIXED + ("du5",)
    B = sm.named_batch(names)
    xp, xf, st, mr = ctx.selftest_small(B)
    assert st.tolist() == [0, 0] and 0.0 <= mr < 1e-8
    _within(B, len(names) - 1, xp, xf, _expected("du5"), "du5 behind the mixed batch")
    # (two addends commute: the systems in front of it are the mixed batch's, bit for bit)
    assert np.array_equal(xp[:len(mixed[2])], mixed[2]) and np.array_equal(xf[:len(mixed[3])], mixed[3])


def test_launches_that_would_not_fit_are_refused(ctx):
    """strips outside { 0, 1, 2, 3, 6 }, a panel with fewer rows than a system has scalars, more than 16 poses, a block of another
    system's pose: LSFM_ERR_ARG before anything is enqueued; the context works afterwards."""
    B = sm.named_batch(["p5a"])
    for strips in (4, 5, 7, -1):
        with pytest.raises(api.LsfmError):
            ctx.selftest_small(B, strips=strips)
    with pytest.raises(api.LsfmError, match="does not fit"):
        ctx.selftest_small(B, strips=1)  # 30 scalars, 16 rows
    with pytest.raises(api.LsfmError, match="does not fit"):
        ctx.selftest_small(sm.named_batch(["p2a", "p6", "p1"]), strips=2)  # 36 scalars, 32 rows
    wide = cs.system("b16", 1)
    assert wide["m"] == 19
    with pytest.raises(api.LsfmError, match="holds 16"):
        ctx.selftest_small(sm.batch([(wide,) + cs.rhs("b16", 1)]))
    two = sm.named_batch(["p3", "p5a"])
    bad = dict(two, photo=two["photo"].copy())
    bad["photo"][0] = two["pose_off"][1]  # the first feature of p3 seen by a pose of p5a
    with pytest.raises(api.LsfmError, match="another system"):
        ctx.selftest_small(bad)
    bad = dict(two, pose_off=two["pose_off"].copy())
    bad["pose_off"][0] = 1
    with pytest.raises(api.LsfmError):
        ctx.selftest_small(bad)
    xp, xf, st, mr = ctx.selftest_small(B)
    assert st.tolist() == [0, 0]
    _within(B, 0, xp, xf, _expected("p5a"), "p5a behind the refusals")
