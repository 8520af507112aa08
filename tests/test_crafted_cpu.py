"""The crafted systems of test_gpu_schur_crafted.py (crafted_system.py), checked without a GPU: every system reaches the tile pose
counts -- and with them the panel variant, the list and its split -- it was built for, it is positive definite, and the yardsticks
the GPU tests hold K9 to agree with themselves to 1e-13: S evaluated feature by feature in fp64 against long double, and a plain fp64
Schur solve against the expected state (dense_reference_solve / schur_reference_solve).  A case that misses one of these is
reshaped; the bars of the GPU tests are not widened."""
import numpy as np
import pytest

import crafted_system as cs
from common import PANEL_RANGE, tile_pose_counts

FLOOR = 1e-13
E_COUNTS = [47, 52, 28, 39]  # tiles of d2's dropped features once every second feature is dropped
MAXE, MAXE_64, BF, SCHUR_CAP, SCHUR_ECAP, HASH = 3584, 2560, 352, 256, 64, 64  # lsfm_schur_panel.hip, lsfm_solve.hip


@pytest.mark.parametrize("decades", [3, 1])
@pytest.mark.parametrize("name", list(cs.CASES))
def test_tiles_are_the_intended_ones(name, decades):
    J = cs.system(name, decades)
    tiles = cs.CASES[name][1]
    assert tile_pose_counts(J["photo"], J["feature"], J["n"]) == [len(t["poses"]) for t in tiles] == J["counts"]
    assert J["n"] == sum(t.get("n", cs.TILE) for t in tiles)
    fe = np.asarray(J["feature"])
    assert np.all(np.diff(fe) >= 0) and np.array_equal(np.unique(fe), np.arange(J["n"]))  # sorted by feature, none without a block
    key = fe.astype(np.int64) * J["m"] + J["photo"]
    assert len(np.unique(key)) < len(key)  # repeated (pose, feature) blocks
    for k, t in enumerate(tiles):  # a tile's poses are the described ones
        sel = (fe >= k * cs.TILE) & (fe < (k + 1) * cs.TILE)
        assert np.array_equal(np.unique(J["photo"][sel]), np.sort(t["poses"]))


def test_what_the_cases_are_for():
    """The conditions of the branches, counted on the index arrays."""
    counts = lambda name: cs.system(name, 3)["counts"]
    assert counts("a8") == [8, 5, 8] and cs.system("a8", 3)["n"] == 2 * 128 + 37 and counts("a9")[0] == 9 and counts("a16") == [16]
    assert tuple(counts(f"b{c}")[0] for c in cs.B_COUNTS) == cs.B_COUNTS == (16, 17, 32, 33, 48, 49, 62, 63, 64, 65, 100)
    assert PANEL_RANGE[48] == (33, 48) and PANEL_RANGE[64] == (49, 63)
    for c in cs.B_COUNTS:  # m = count + 3: poses nothing sees
        J = cs.system(f"b{c}", 3)
        assert J["m"] == c + 3 and len(np.unique(J["photo"])) == c
    # b100: more pose pairs and more poses than k_schur_w's LDS tables hold, more poses than the slot kernel's hash table
    J = cs.system("b100", 3)
    ph, fe = np.asarray(J["photo"], np.int64), np.asarray(J["feature"])
    pairs = set()
    for f in range(J["n"]):
        p = np.unique(ph[fe == f])
        pairs.update((p[:, None] * 1000 + p[None, :])[np.triu_indices(len(p))].tolist())
    assert len(pairs) > SCHUR_CAP and counts("b100")[0] > max(SCHUR_ECAP, HASH) and np.bincount(fe).mean() > 65
    # c: blocks behind the LDS slot list, repeats among them, a pass of 16 features with more blocks than the block -> feature table
    for name, maxe in (("c32", MAXE), ("c48", MAXE), ("c63", MAXE_64)):
        J = cs.system(name, 3)
        ph, fe = np.asarray(J["photo"], np.int64), np.asarray(J["feature"], np.int64)
        assert len(ph) > MAXE
        key = fe * 1000 + ph
        first = np.unique(key, return_index=True)[1]
        rep = np.setdiff1d(np.arange(len(key)), first)
        assert np.sum(rep >= maxe) > 50, name
        if name != "c63":  # every feature seen by every pose
            assert np.all(np.bincount(fe[first]) == J["m"])
        assert max(np.sum((fe >= p0) & (fe < p0 + 16)) for p0 in range(0, 128, 16)) > BF
    assert np.bincount(cs.system("c63", 3)["feature"]).min() >= 30
    # d: the lists of the 32- / 48- / 64-slot variants and how k9_kernel cuts them (256 CUs; any count >= 17 gives the same)
    assert [cs.list_lengths(counts(k)) for k in cs.LIST_CASES] == [[4, 1, 2], [5, 3, 0], [0, 2, 4]]
    for v in range(3):
        got = {cs.parts_of_list(cs.list_lengths(counts(k))[v], len(counts(k)), 256) for k in cs.LIST_CASES}
        got.add(cs.parts_of_list(cs.list_lengths(E_COUNTS)[v], len(E_COUNTS), 256))
        assert got - {0}, v
    allparts = {cs.parts_of_list(n, len(counts(k)), 256) for k in cs.LIST_CASES for n in cs.list_lengths(counts(k))}
    assert {8, 4, 2, 1} <= allparts
    # (the ragged last tile of d1 / d3 is a wide tile of a split list; d1's ends before the last parts begin: those are empty)
    for name, lo, some_empty in (("d1", 33, True), ("d3", 49, False)):
        t = cs.CASES[name][1][-1]
        n_last, c = t["n"], len(t["poses"])
        v = cs.list_lengths([c]).index(1)
        parts = cs.parts_of_list(cs.list_lengths(counts(name))[v], len(counts(name)), 256)
        assert c >= lo and parts > 1 and n_last < 128 and (-(-n_last // (128 // parts)) < parts) == some_empty
    assert any(c > 63 for c in counts("d3")) and any(c <= 16 for c in counts("d3"))  # k_schur_w and the 16-slot variant beside the lists
    # e: the compacted input
    for dec in (3, 1):
        _, K = cs.half_dropped("d2", dec)
        assert tile_pose_counts(K["photo"], K["feature"], K["n"]) == E_COUNTS
    # f: the fixed pose and the pose of the fixed scalar are seen by features
    J = cs.system("f33", 1)
    sa = cs.gauge(J)
    assert counts("f33") == [33] and sa[1] == 6 * sa[0] and sa[2] // 6 == sa[4] != sa[0] and {sa[0], sa[4]} <= set(J["photo"].tolist())
    assert counts("g20") == [20]


def _has_factor(M):
    try:
        np.linalg.cholesky(M)
        return True
    except np.linalg.LinAlgError:
        return False


@pytest.mark.parametrize("decades", [3, 1])
@pytest.mark.parametrize("name", cs.S_CASES)
def test_positive_definite_and_the_floor_of_s(name, decades):
    """Every V_f has a Cholesky factor, and so has the whole matrix: [[U, W], [W^T, V]] is positive definite exactly when V and the
    Schur complement S = U - W V^-1 W^T are (S is taken from the long-double evaluation: the dense matrix of the largest case would
    have 6864 rows).  S in fp64 and in long double agree to 1e-13 in the GPU test's metric."""
    J = cs.system(name, decades)
    V = np.asarray(J["V"]).reshape(-1, 3, 3)
    np.linalg.cholesky(V)
    Sl = cs.expected_s(name, decades)
    assert _has_factor(np.asarray(Sl, np.float64))
    if 6 * J["m"] + 3 * J["n"] <= 1500:
        from refdump import dense_info
        assert _has_factor(dense_info(J))
    e = cs.info_metric(cs.schur_by_feature(J, np.float64), Sl, np.diag(cs.dense_u(J)))
    print(f"{name} decades {decades}: S fp64 against long double {e:.2e}")
    assert e <= FLOOR


def test_the_one_system_that_is_not_positive_definite():
    J = cs.system("g20", 3)
    V = np.asarray(J["V"]).reshape(-1, 3, 3)
    f = cs.CASES["g20"][2]["bad_v"][0]
    w = np.linalg.eigvalsh(V)
    assert np.all(w[np.arange(len(V)) != f] > 0) and w[f, 0] < 0 < w[f, 1] and abs(w[f, 0]) < 2e-3 * w[f, 2]
    assert not _has_factor(V[f])


@pytest.mark.parametrize("name", cs.SOLVE_CASES)
def test_floor_of_the_solve(name):
    J = cs.system(name, 1)
    ea, eb = cs.rhs(name, 1)
    x, mono, sa = cs.expected_x(name, 1)
    ep, ef = cs.state_metric(cs.plain_schur_solve(J, ea, eb, mono, sa), x, J["m"])
    print(f"{name}: plain fp64 Schur solve against the expected state: poses {ep:.2e} features {ef:.2e}")
    assert ep <= FLOOR and ef <= FLOOR


def test_floor_of_the_compacted_case():
    """expected_info (fp64, numpy's 3x3 inverses) on the case with every second feature dropped, against the long-double sum"""
    from refdump import dense_info
    from test_gpu_marginalise import expected_info
    J = cs.system("d2", 3)
    drop, _ = cs.half_dropped("d2", 3)
    m, n = J["m"], J["n"]
    E = expected_info(dense_info(J), m, n, drop)
    e = cs.info_metric(E[:6 * m, :6 * m], cs.schur_by_feature(J, np.longdouble, drop=drop), np.diag(cs.dense_u(J)))
    print(f"d2, every second feature dropped: expected_info against long double {e:.2e}")
    assert e <= FLOOR
