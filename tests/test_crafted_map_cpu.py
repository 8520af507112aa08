"""The crafted maps and batches of test_gpu_transform_crafted.py (crafted_map.py), checked without a GPU: every case is a valid map,
describe() finds on its index arrays the path it was built for -- against the constants of csrc/lsfm_transform.hip, which are read
from the source here, so that a changed constant names the case that no longer reaches its path --, and the yardstick agrees with
itself: the oracle's transform of a map and of the same map with its features reordered, mapped back, differ by the reference
arithmetic's own re-association, in the per-block metric of the GPU test.  That distance must be at least 1000 x below STAGE_TOL;
a case that misses it is reshaped, the bound of the GPU test stays."""
import os
import re

import numpy as np
import pytest

import crafted_map as cm

FLOOR = 1e-9 / 1000  # STAGE_TOL (test_gpu_parity.py) / 1000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_bound():
    from linearsfm_amd import api
    assert "lsfm_selftest_transform" in api.EXPORTS and hasattr(api.Context, "selftest_transform")
    from test_gpu_parity import STAGE_TOL
    assert FLOOR == STAGE_TOL / 1000


def test_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "linearsfm_amd", "csrc", "lsfm_transform.hip")).read()
    assert int(re.search(r"#define TRE_TILE (\d+)", src).group(1)) == cm.TRE_TILE
    assert int(re.search(r"#define TRE_ROUND (\d+)", src).group(1)) == cm.TRE_ROUND
    s, mo = re.search(r"constexpr int GCAP = NH == 1 \? (\d+) : (\d+)", src).groups()
    assert (int(s), int(mo)) == (cm.GCAP[False], cm.GCAP[True])
    ub = src[src.index("k_tr_ublocks(int NU"):]
    assert int(re.search(r"constexpr int GCAP = (\d+);", ub).group(1)) == cm.UCAP
    assert re.search(r"__launch_bounds__\(128, 1\)\s*k_tr_ublocks", src) and "dim3((in.NU + 127) / 128), dim3(128)" in src
    assert "dim3((M + 127) / 128), dim3(128), 0, su, M, d_tm" in src and "k_tr_feat_post<NH>, dim3((in.NF + 255) / 256), dim3(256)" in src
    assert (cm.UGROUP, cm.POSE_GROUP, cm.POST_GROUP) == (128, 128, 256)


@pytest.mark.parametrize("name,mono", cm.CASES)
def test_every_map_is_valid(name, mono):
    maps, targets = cm.case(name, mono)
    assert len(maps) == len(targets)
    for d, t in zip(maps, targets):
        m, n = d["m"], d["n"]
        fe, ph = np.asarray(d["feature"]), np.asarray(d["photo"])
        assert np.all(np.diff(fe) >= 0) and np.array_equal(np.unique(fe), np.arange(n)) and ph.min() >= 0 and ph.max() < m
        assert np.array_equal(d["FBlock"], np.searchsorted(fe, np.arange(n)))
        assert len(d["stno"]) == len(d["stVal"]) == 6 * m + 3 * n and np.all(d["stno"][:6 * m] < 0) and np.all(d["stno"][6 * m:] > 0)
        V = d["V"].reshape(-1, 3, 3)
        U = d["U"].reshape(-1, 6, 6)
        assert np.array_equal(V, V.transpose(0, 2, 1)) and np.array_equal(U[:m], U[:m].transpose(0, 2, 1))
        assert np.array_equal(d["Ui"][:m], np.arange(m)) and np.array_equal(d["Uj"][:m], np.arange(m))
        assert np.array_equal(d["Ui"][m:], np.arange(m - 1)) and np.array_equal(d["Uj"][m:], np.arange(1, m))
        pose = d["stVal"][:6 * m].reshape(m, 6)
        ids = -d["stno"][:6 * m:6]
        assert len(np.unique(ids)) == m and np.abs(pose[:, 3:]).max() <= 0.6 and np.abs(pose[:, :3]).max() <= 1.5
        assert np.all(d["stVal"][6 * m:].reshape(n, 3)[:, 2] >= 3.0)
        if not mono:
            assert d["Ref"] not in ids
            continue
        if m == 1:
            assert not cm.is_active(d, t, mono)  # (a Mono map of one pose is only ever passed through)
            continue
        h0, h1 = int(np.flatnonzero(ids == d["Ref"])[0]), int(np.flatnonzero(ids == d["ScaP"])[0])
        assert (h0, h1) == d["hubs"] and np.all(pose[h0] == 0.0) and pose[h1, d["Fix"]] == d["Sign"] and abs(d["Sign"]) == 1
        if cm.is_active(d, t, mono):
            r, s = int(np.flatnonzero(ids == t[0])[0]), int(np.flatnonzero(ids == t[1])[0])
            ts = cm._rot(*pose[r, 3:]) @ (pose[s, :3] - pose[r, :3])
            assert r != s and 0.5 <= abs(ts[t[2]]) <= 3.0
            if name[0] != "d":
                assert t[2] == int(np.argmax(np.abs(ts)))


def test_permute_features_and_back():
    (d,), _ = cm.case("c", True)
    perm = np.random.default_rng(3).permutation(d["n"])
    p = cm.permute_features(d, perm)
    assert not np.array_equal(p["photo"], d["photo"]) and np.array_equal(p["stno"][6 * d["m"]::3], d["stno"][6 * d["m"]::3][perm])
    f = 5
    assert np.array_equal(p["W"][p["feature"] == f], d["W"][d["feature"] == perm[f]]) and np.array_equal(p["V"][f], d["V"][perm[f]])
    cm.assert_identical(cm.permute_features(p, np.argsort(perm)), d, True)


def _hub_positions(d, f, hub):
    """positions within feature f's run of its blocks to pose `hub`"""
    return np.flatnonzero(np.asarray(d["photo"])[np.asarray(d["feature"]) == f] == hub)


@pytest.mark.parametrize("name,mono", cm.CASES)
def test_what_the_case_reaches(name, mono):
    maps, targets = cm.case(name, mono)
    D = cm.describe(maps, targets, mono)
    G, R, T = cm.GCAP[mono], cm.TRE_ROUND, cm.TRE_TILE
    nh = 2 if mono else 1
    if name == "a":
        assert len(D["run"]) == T + 1 and len(D["tiles"]) == 2 and D["tiles"][0]["poses"] <= G  # (no overflow of the pose table here)
        assert [D["run"][f] for f in (0, 2, 3, 4, 5, 60, 62, T - 1)] == [2 * R + 1, R - 1, R, R - 1, 2, R + 4, R + 1, 300]
        assert [D["chunks"][f] for f in (0, 3, 60, 62, T - 1)] == [3, 1, 2, 2, 2] and D["chunks"].max() == 3
        chunked = np.flatnonzero(D["chunks"] > 1)
        assert chunked[0] == 0 and chunked[-1] == T - 1 and any(0 < f < T - 1 for f in chunked)  # first, middle, last of the tile
        rs = D["rounds"][0]
        assert [r[2] for r in rs] == [2 * R + 1, R, R, R - 1, 56, R + 4, 1, R + 1, 64, 300]
        assert rs[1][:2] == (1, 2) and rs[2][:2] == (3, 1)          # a round that ends at exactly 256, then a run of exactly 256
        assert rs[3][:2] == (4, 1) and rs[4][0] == 5                # 255, and the feature with 2 blocks starts the next round
        assert np.all(D["run"][6:60] == 1) and np.all(D["run"][63:T - 1] == 1)
        kinds = set()
        for f in chunked:
            for h in D["hubs"][0]:
                pos = _hub_positions(maps[0], f, h)
                if len(pos):
                    assert pos.min() >= R, (f, pos)  # hub blocks only behind the first chunk
                    kinds.add((D["hubs"][0].index(h), min(len(pos), 2)))
        assert kinds >= {(s, k) for s in range(nh) for k in (1, 2)}  # single and repeated, to every hub
    elif name == "b1":
        assert [t["poses"] for t in D["tiles"]] == [G, G + 1]
    elif name == "b2":
        big = cm.B2_POSES[mono]
        assert [t["poses"] for t in D["tiles"]][:2] == [big, big] and big > 2 * G and len(D["tiles"]) == 3 and len(D["run"]) == 2 * T + 5
        ph, fe = np.asarray(maps[0]["photo"]), np.asarray(maps[0]["feature"])
        first = [set(ph[(fe >= t0) & (fe < t0 + 64)].tolist()) for t0 in (0, T)]
        assert np.all(D["run"][:2 * T] == 4) and len(first[0]) == len(first[1]) == G  # a first round of 256 blocks that fills the table ...
        assert len(first[0] & first[1]) == 0                                          # ... with other poses in the second tile
    elif name == "c":
        hb = D["hub_blocks"][:T]
        assert set(hb[:, 0].tolist()) == set(cm.C_COUNTS[0]) and D["run"][17] == hb[17].sum() >= 1
        if mono:
            assert {(min(a, 2), min(b, 2)) for a, b in hb.tolist()} == {(a, b) for a in range(3) for b in range(3)}
            assert set(hb[:, 1].tolist()) == set(cm.C_COUNTS[1])
    elif name[0] == "d":
        d, t = maps[0], targets[0]
        assert d["m"] == 12 and (t[1] == d["Ref"], t[0] == d["ScaP"], t[2]) == (bool(int(name[1])), bool(int(name[2])), int(name[4]))
        assert D["active"] == [True] and D["hub_blocks"].min() == 0 and D["hub_blocks"].max() >= 1
    elif name[0] == "e":
        pattern = name[2:]
        assert D["active"] == [c == "A" for c in pattern] and tuple(d["n"] for d in maps) == cm.E_N
        assert [t["maps"] for t in D["tiles"]] == [[0, 1], [1, 2], [2, 3, 4], [4]]  # every tile boundary inside a map; one tile holds three
        assert (any(d["m"] == 1 for d in maps) or (mono and pattern[3] == "A")) and D["chunks"][T - 1] == 2 and D["run"][T - 1] == 300
        assert [t is not None and not a for t, a in zip(targets, D["active"])] == [c == "F" for c in pattern]
        if pattern == "AAAAA":
            assert D["tiles"][0]["poses"] == cm.E_M[0] + cm.E_M[1] and (cm.E_M[0] + cm.E_M[1] > cm.GCAP[False]) and max(cm.E_M[:2]) <= 22
            assert D["waves_poses"][0] == [0, 1, 2] and D["waves_feats"][1] == [0, 1] and D["hub_blocks"].max() >= 2
        if pattern[0] == "A" and pattern[2] == "A":
            assert len(D["pose_groups"][0]) >= 2 and len(D["post_groups"][0]) >= 2  # one work-group holds two transformed maps
        if pattern == "NFNFN":
            assert not any(D["active"]) and all(t["poses"] == 0 for t in D["tiles"])
    elif name == "f":
        d = maps[0]
        assert d["m"] == 300 and D["ugroups"][0] == cm.UGROUP > cm.UCAP and min(D["ugroups"][:-1]) > cm.UCAP
        for h in D["hubs"][0]:
            assert 100 <= h <= 200
            assert len({int(i) // cm.UGROUP for i in np.flatnonzero((d["Ui"] == h) | (d["Uj"] == h))}) >= 2
    else:
        raise AssertionError(name)


@pytest.mark.parametrize("name,mono", cm.CASES)
def test_floor_of_the_reference(oracle, name, mono):
    """How far two evaluations of the reference's own arithmetic lie apart: the oracle on the map, and on the map with its features
    reordered, mapped back."""
    maps, targets = cm.case(name, mono)
    worst = {}
    for b, (d, t) in enumerate(zip(maps, targets)):
        if not cm.is_active(d, t, mono):
            if t is not None:
                cm.assert_identical(oracle.transform(d, mono, *(t if mono else (t,))), d, mono)  # in that frame already: a copy
            continue
        tt = t if mono else (t,)
        exp = oracle.transform(d, mono, *tt)
        for k in ("U", "W", "V", "stVal"):
            assert np.all(np.isfinite(exp[k])), (name, b, k)
        perm = np.random.default_rng(7 + b).permutation(d["n"])
        back = cm.permute_features(oracle.transform(cm.permute_features(d, perm), mono, *tt), np.argsort(perm))
        for k, (e, _) in cm.compare(back, exp, mono).items():
            worst[k] = max(worst.get(k, 0.0), e)
    print(f"{name} {'Mono' if mono else 'Stereo'}: floor " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= FLOOR, (name, k, v)
