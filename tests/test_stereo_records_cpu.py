"""No GPU: the batches of crafted_stereo_records.py are valid map sets and reach what test_gpu_transform_stereo_records.py says they
reach -- counted on the index arrays with crafted_map.describe, against the capacity of k_tr_entries' LDS table of map records as the
source states it."""
import os
import re

import numpy as np
import pytest

import crafted_map as cm
import crafted_stereo_records as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _capacity():
    src = open(os.path.join(ROOT, "linearsfm_amd", "csrc", "lsfm_transform.hip")).read()
    cap = int(re.search(r"#define TRE_MAPS (\d+)", src).group(1))
    assert re.search(r"__shared__ double sMap\[NH == 1 \? TRE_MAPS \* TR_REC : 1\]", src)
    return cap


@pytest.mark.parametrize("name", sr.CASES)
def test_every_batch_is_a_valid_map_set(name):
    maps, targets = sr.case(name)
    assert len(maps) == len(targets)
    refs = set()
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
        assert d["Ref"] not in ids and d["Ref"] not in refs
        refs.add(d["Ref"])
        if cm.is_active(d, t, False):
            assert t in ids  # (the target is a pose of the map: the transform finds it)
            h = int(np.flatnonzero(ids == t)[0])
            assert np.abs(pose[h, 3:]).min() > 0.0  # a rotation of its own, about every axis


def test_the_batches_reach_what_they_claim():
    cap = _capacity()
    # more maps in a tile than the table holds, all transformed
    maps, targets = sr.case("many")
    D = cm.describe(maps, targets, False)
    assert all(D["active"]) and len({d["target"] for d in maps}) == len(maps)
    assert all(3 <= d["m"] <= 4 and 18 <= d["n"] <= 22 for d in maps)
    wide = max(D["tiles"], key=lambda t: len(t["maps"]))
    assert len(wide["maps"]) > cap and wide["maps"] == list(range(wide["maps"][0], wide["maps"][-1] + 1))
    # the same tile with every second map passed through: transformed maps on both sides of the table's end
    maps, targets = sr.case("alternate")
    D = cm.describe(maps, targets, False)
    assert D["active"] == [b % 2 == 0 for b in range(len(maps))]
    assert any(t is None for t in targets) and any(t is not None and not cm.is_active(d, t, False) for d, t in zip(maps, targets))
    wide = max(D["tiles"], key=lambda t: len(t["maps"]))
    first = wide["maps"][0]
    act = [b for b in wide["maps"] if D["active"][b]]
    assert any(b - first < cap for b in act) and any(b - first >= cap for b in act)
    # a map boundary on a tile boundary: the second tile is the second map's one feature
    maps, targets = sr.case("boundary")
    D = cm.describe(maps, targets, False)
    assert all(D["active"]) and [d["n"] for d in maps] == [cm.TRE_TILE, 1]
    assert [t["maps"] for t in D["tiles"]] == [[0], [1]]
    # old blocks to the hub pose occur in every batch (the epilogue's hub-block path runs with the new C_f too)
    assert D["hub_blocks"].max() >= 1
