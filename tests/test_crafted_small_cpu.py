"""The crafted systems and batches of test_gpu_small_crafted.py (crafted_small.py), checked without a GPU: describe() finds on the
index arrays of every case the branch of k_small_solve it was built for -- against the constants of csrc/lsfm_small.hip, which are read
from the source here, so that a changed constant names the case that no longer reaches its branch --, every system is positive
definite (but the one that is meant not to be), and the yardstick agrees with itself: a plain fp64 Schur solve lies within 1e-13
(test_crafted_cpu.py's floor) of the expected state the GPU tests use.  A case that misses one of these is reshaped; the bars of the
GPU tests are not widened."""
import os
import re

import numpy as np
import pytest

import crafted_small as sm
import crafted_system as cs
from test_crafted_cpu import FLOOR, _has_factor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, S, C, PARKED = sm.SM_PASS, sm.SM_SUPER, sm.SM_CHUNK, sm.PARKED


def test_the_entry_point_is_bound():
    from linearsfm_amd import api
    assert "lsfm_selftest_small" in api.EXPORTS and hasattr(api.Context, "selftest_small")
    assert FLOOR == 1e-13 and sm.DECADES == 1


def test_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "linearsfm_amd", "csrc", "lsfm_small.hip")).read()
    for name, v in (("SM_PASS", P), ("SM_SUPER", S), ("SM_CHUNK", C), ("SM_WROWS", sm.SM_WROWS)):
        assert int(re.search(rf"#define {name} (\d+)", src).group(1)) == v, name
    body = src[src.index("static int small_solve_strips("):]
    body = body[:body.index("}")]
    assert tuple((int(a), int(b)) for a, b in re.findall(r"if \(most_poses <= (\d+)\) return (\d+);", body)) == sm.STRIPS
    assert [16 * s // 6 for _, s in sm.STRIPS] == [cap for cap, _ in sm.STRIPS]  # MCAP = R / 6: the panel has rows for exactly these
    assert all(f"case {s}: launch_small<{s}>" in src for _, s in sm.STRIPS[:-1]) and f"default: launch_small<{sm.STRIPS[-1][1]}>" in src
    assert "const int ph = 6 * e < SM_WROWS ? sh.sph[e]" in src and "if (6 * e + 5 < SM_WROWS)" in src  # block 170: its pose parked, its rows not
    assert S == 4 * P and C == 4 * S and PARKED == 170
    assert [sm.strips_of(m) for m in (1, 2, 3, 5, 6, 8, 9, 16)] == [1, 1, 2, 2, 3, 3, 6, 6]


@pytest.mark.parametrize("name", list(sm.CASES))
def test_every_system_is_valid(name):
    J = sm.system(name)
    m, tiles, kw = sm.CASES[name]
    assert J["m"] == m and J["n"] == sum(t.get("n", cs.TILE) for t in tiles) and 6 * m + 3 * J["n"] < cs.DENSE_LIMIT
    fe, ph = np.asarray(J["feature"]), np.asarray(J["photo"])
    assert np.all(np.diff(fe) >= 0) and np.array_equal(np.unique(fe), np.arange(J["n"])) and ph.min() >= 0 and ph.max() < m
    assert np.all(J["Ui"] <= J["Uj"]) and J["Ui"].min() >= 0 and J["Uj"].max() < m
    pairs = J["Ui"].astype(np.int64) * m + J["Uj"]
    nu = m + (m - 1 if kw.get("offdiag") and m > 1 else 0)
    assert len(np.unique(pairs)) == nu and len(pairs) == (2 * nu if name == "du5" else nu)  # one U block per pose pair, du5: two
    key = fe.astype(np.int64) * m + ph
    assert (len(np.unique(key)) < len(key)) == (kw.get("dup", 0.1) > 0)  # repeated (pose, feature) blocks, but where dup = 0


def _d(name, strips=None):
    return sm.describe(sm.system(name), strips)


def test_what_the_cases_are_for():
    """The conditions of the branches, counted on the index arrays as the kernel walks them."""
    D = {k: _d(k) for k in sm.CASES}
    n = {k: sm.system(k)["n"] for k in sm.CASES}
    feats = lambda k: [s["feats"] for s in D[k]["supers"]]
    pfeats = lambda k: [p["feats"] for p in D[k]["passes"]]
    blocks = lambda k: [s["blocks"] for s in D[k]["supers"]]
    # the four instances and their edges: m = 1, 2 | 3, 5 | 6, 8 | 9, 16
    assert {k: (sm.system(k)["m"], D[k]["instance"]) for k in ("p1", "p2a", "p2b", "p3", "p5a", "p5b", "p6", "p8a", "p8b", "p9", "p16a", "p16b", "p16c")} == {
        "p1": (1, 1), "p2a": (2, 1), "p2b": (2, 1), "p3": (3, 2), "p5a": (5, 2), "p5b": (5, 2), "p6": (6, 3), "p8a": (8, 3), "p8b": (8, 3),
        "p9": (9, 6), "p16a": (16, 6), "p16b": (16, 6), "p16c": (16, 6)}
    # passes and super-passes: 1, 15, 16, 17, 63, 64, 65 features
    assert (n["p16a"], n["p6"], n["p2a"], n["p1"], n["p9"], n["p5a"], n["p3"]) == (1, P - 1, P, P + 1, S - 1, S, S + 1)
    assert pfeats("p1") == [P, 1] and pfeats("p2a") == [P] and pfeats("p6") == [P - 1] and pfeats("p9") == [P, P, P, P - 1]
    assert feats("p5a") == [S] and feats("p3") == [S, 1] and feats("p9") == [S - 1]
    # run-pointer chunks: exactly one (entry 256 is read, no reload); 257 (a chunk and a super-pass of one feature); 256 + 64 + 1;
    # 513: two reloads, the second into the buffer of the first chunk
    assert n["p8a"] == C and D["p8a"]["loads"] == [0] and D["p8a"]["last_entry"] == C
    assert n["p2b"] == C + 1 and D["p2b"]["loads"] == [0, C] and feats("p2b") == [S, S, S, S, 1]
    assert n["p5b"] == C + S + 1 and D["p5b"]["loads"] == [0, C] and feats("p5b") == [S] * 5 + [1]
    assert n["p8b"] == 2 * C + 1 and D["p8b"]["loads"] == [0, C, 2 * C] and max(blocks("p8b")) > 2 * PARKED
    assert n["p16b"] > 2 * C and len(D["p16b"]["loads"]) == 3
    assert all(D[k]["loads"] == [0] for k in sm.CASES if n[k] <= C)
    # the W rows in LDS: all parked; exactly 170; exactly 171 (block 170: pose parked, rows from memory); more than 1000
    assert blocks("w170") == [PARKED] and blocks("w171") == [PARKED + 1] and min(blocks("p16c")) > 1100
    assert all(max(blocks(k)) < PARKED for k in ("p1", "p2a", "p2b", "p3", "p5a", "p6", "p8a", "p9", "p16a", "p16b", "u16", "du5", "g3", "v8"))
    assert sm.CASES["w170"][2]["dup"] == sm.CASES["w171"][2]["dup"] == 0.0 and set(D["w170"]["runs"]) == {5} and set(D["w171"]["runs"]) == {3}
    # repeated blocks inside the parked rows (every case with repeats) and behind them
    for k in sm.CASES:
        if k not in ("w170", "w171"):
            assert sum(s["rep_in"] for s in D[k]["supers"]) >= 1, k
    assert all(s["rep_behind"] > 50 for s in D["p16c"]["supers"]) and sum(s["rep_behind"] for s in D["p8b"]["supers"]) > 50
    assert all(s["rep_behind"] == 0 for k in sm.CASES for s in D[k]["supers"] if s["blocks"] <= PARKED)
    # every feature seen by every pose
    for k in ("p16a", "p16c"):
        J = sm.system(k)
        first = np.unique(J["feature"].astype(np.int64) * 16 + J["photo"])
        assert len(first) == 16 * J["n"], k
    # strip masks: p16b has passes with two, three, four and all six strips on, and tiles off.  Poses 2, 5, 10, 13 straddle two strips
    # (7 does not: rows 42-47); in the passes seen by (5, 10) and by (2, 13) alone each one's second strip is on through it alone
    masks = [p["mask"] for p in D["p16b"]["passes"]]
    assert sm.STRADDLE == [2, 5, 10, 13]
    assert {0b000011, 0b011110, 0b111000, 0b110011, 0b111111} <= set(masks) and D["p16b"]["tiles"] == 21
    assert masks.count(0b011110) >= 6 and masks.count(0b110011) >= 6 and max(p["off"] for p in D["p16b"]["passes"]) == 18
    off = sum(p["off"] for p in D["p16b"]["passes"]) / (21 * len(masks))
    print(f"p16b: {len(masks)} passes, {off:.2f} of the (pass, tile) pairs off")
    assert 0.5 < off < 0.9
    # (a straddling pose as the last of its system: its second strip has no other pose -- p3's pose 2, p6's pose 5)
    assert all(p["mask"] == 0b11 for p in D["p3"]["passes"][:4]) and D["p6"]["passes"][0]["mask"] == 0b111
    # a small system in a larger instance (the batch's mixed launch): its padding strips are off in every pass
    assert all(p["mask"] == 0b1 and p["off"] == 20 for p in _d("p2a", 6)["passes"]) and all(p["mask"] == 0b11 for p in _d("p5b", 6)["passes"])
    # poses no feature sees: a whole strip (rows 48-63 are poses 8, 9 and four rows of 10)
    assert D["u16"]["unseen"] == [8, 9, 10] and all(p["mask"] & 0b001000 == 0 for p in D["u16"]["passes"]) and sm.CASES["u16"][2]["offdiag"]
    assert all(D[k]["unseen"] == [] for k in sm.CASES if k != "u16")
    # the gauges: the fixed pose and the pose of the fixed scalar are seen by features
    for k in sm.MONO:
        J = sm.system(k)
        sa = sm.gauge(J)
        assert sa[1] == 6 * sa[0] and sa[2] // 6 == sa[4] != sa[0] and {sa[0], sa[4]} <= set(J["photo"].tolist()) and sm.gauge_mask(J, sa).sum() == 7
    assert sm.CASES["v8"][2]["bad_v"][0] == 50
    # the batches
    assert [D[k]["instance"] for k in sm.MIXED] == [1, 6, 1, 2, 6, 2, 3, 3] and [D[k]["instance"] for k in sm.MANY] == [1, 1, 2, 3]


@pytest.mark.parametrize("name", sm.GOOD)
def test_positive_definite(name):
    """[[U, W], [W^T, V]] is positive definite exactly when every V_f and the Schur complement are"""
    J = sm.system(name)
    np.linalg.cholesky(np.asarray(J["V"]).reshape(-1, 3, 3))
    Sl = np.asarray(cs.schur_by_feature(J, np.longdouble), np.float64)
    assert _has_factor(Sl)
    print(f"{name}: cond(S) {np.linalg.cond(Sl):.1e}")


def test_the_one_system_that_is_not_positive_definite():
    J = sm.system("v8")
    V = np.asarray(J["V"]).reshape(-1, 3, 3)
    f = sm.CASES["v8"][2]["bad_v"][0]
    w = np.linalg.eigvalsh(V)
    assert np.all(w[np.arange(len(V)) != f] > 0) and w[f, 0] < 0 < w[f, 1] and not _has_factor(V[f])


@pytest.mark.parametrize("name", list(sm.CASES))
def test_floor_of_the_solve(name):
    J = sm.system(name)
    ea, eb = sm.rhs(name)
    x, mono, sa = sm.expected_x(name)
    ep, ef = cs.state_metric(cs.plain_schur_solve(J, ea, eb, mono, sa), x, J["m"])
    print(f"{name}: plain fp64 Schur solve against the expected state: poses {ep:.2e} features {ef:.2e}")
    assert ep <= FLOOR and ef <= FLOOR


def test_two_addends_are_the_same_system():
    """du5: the addends of every U block sum to a symmetric matrix with the chain's pattern; split_u changes nothing else"""
    m, tiles, kw = sm.CASES["du5"]
    J = sm.system("du5")
    K = cs.craft(m, tiles, 50000 + sorted(sm.CASES).index("du5"), decades=sm.DECADES, offdiag=True)
    nu = len(K["Ui"])
    assert np.array_equal(J["Ui"], np.r_[K["Ui"], K["Ui"]]) and np.array_equal(J["W"], K["W"]) and np.array_equal(J["V"], K["V"])
    assert not np.array_equal(J["U"][:nu], K["U"]) and np.max(np.abs(J["U"][:nu] + J["U"][nu:] - K["U"]) / np.abs(K["U"]).max()) < 1e-15
    Ud = J["U"][:m].reshape(m, 6, 6)
    assert np.array_equal(Ud, Ud.transpose(0, 2, 1))


def test_batches_and_the_many_right_hand_sides():
    """batch() shifts every index into its system's range; solve_many is dense_reference_solve for several right-hand sides"""
    B = sm.named_batch(sm.MIXED)
    G = len(sm.MIXED)
    assert len(B["pose_off"]) == G + 1 and B["pose_off"][-1] == sum(sm.system(k)["m"] for k in sm.MIXED)
    fptr = np.searchsorted(B["feature"], np.arange(B["feat_off"][-1] + 1))
    for g, k in enumerate(sm.MIXED):
        p0, p1 = B["pose_off"][g:g + 2]
        u = slice(B["u_off"][g], B["u_off"][g + 1])
        w = slice(fptr[B["feat_off"][g]], fptr[B["feat_off"][g + 1]])
        assert B["Ui"][u].min() >= p0 and B["Uj"][u].max() < p1 and B["photo"][w].min() >= p0 and B["photo"][w].max() < p1
        assert np.array_equal(B["photo"][w] - p0, sm.system(k)["photo"]) and np.array_equal(B["W"].reshape(-1, 18)[w], sm.system(k)["W"])
    assert np.all(np.diff(B["feature"]) >= 0)
    for k in sm.MANY:
        J = sm.system(k)
        ea, eb = sm.rhs(k)
        rng = np.random.default_rng(1)
        EA, EB = np.stack([ea, ea * rng.standard_normal(len(ea))]), np.stack([eb, rng.standard_normal(len(eb))])
        X = sm.solve_many(J, EA, EB)
        x = sm.expected_x(k)[0]
        assert max(cs.state_metric(X[0], x, J["m"])) <= 1e-15
        y = sm.dense_reference_solve(J, EA[1], EB[1], False)
        assert max(cs.state_metric(X[1], y, J["m"])) <= 1e-15
    K = sm.without_features(sm.system("p3"))
    ea, _ = sm.rhs("p3")
    x = sm.dense_reference_solve(K, ea, np.zeros(0), False)
    assert np.max(np.abs(cs.dense_u(K) @ x - ea) / np.abs(ea).max()) < 1e-14
    B = sm.batch([(sm.system("p1"),) + sm.rhs("p1"), (K, ea, np.zeros(0)), (sm.system("p2a"),) + sm.rhs("p2a")])
    assert B["feat_off"].tolist() == [0, 17, 17, 33] and B["pose_off"].tolist() == [0, 1, 4, 6] and B["feature"].max() == 32
    assert B["Ui"].dtype == B["photo"].dtype == B["feature"].dtype == np.int32 and len(B["eb"]) == 3 * 33
