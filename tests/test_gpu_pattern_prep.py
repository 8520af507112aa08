"""The block pattern of S as the device prepares it (lsfm_pattern.hip): pose pairs of features spread over the lanes of a work-group,
sent through the work-group's own LDS set of the pairs it has sent already, so that the global hash table sees each distinct pair
about once; a compaction with one atomic per work-group; one sort of packed keys.

The first test holds lsfm_schur_pattern against the pattern worked out in numpy from the same index arrays -- the only check here
whose expected value is not made by the device as well.  The second runs whole analysing trees with LSFM_CHECK_EARLY_PATTERN=1, which
makes every level compare the pattern it built ahead (early: from the level's inputs; prefetched: one level ahead, with the cross
pairs of the matched features) with the joint map's, block for block."""
import numpy as np
import pytest

from common import pose_param_err
from linearsfm_amd import synth

pytestmark = pytest.mark.gpu

TREE_TOL = 1e-6      # BASELINE.json's bar on pose parameters (as tests/test_gpu_configs.py)
PAT_RUN = 32         # lsfm_pattern.hip: features a work-group takes at a time
PAT_WG = 256         # ... and its lanes
PAIRSET_SLOTS = 2048  # lsfm_solve.hpp: slots of the work-group's LDS set, emptied for every run of features


def numpy_pattern(j):
    """upper block CSR of: pose pairs sharing a feature + U's pairs + the diagonal"""
    m, n = int(j["m"]), int(j["n"])
    mask = np.eye(m, dtype=bool)
    mask[np.asarray(j["Ui"]), np.asarray(j["Uj"])] = True
    photo, feature = np.asarray(j["photo"]), np.asarray(j["feature"])
    fptr = np.searchsorted(feature, np.arange(n + 1))
    for f in range(n):
        p = photo[fptr[f]:fptr[f + 1]]
        mask[np.ix_(p, p)] = True
    mask = np.triu(mask | mask.T)
    rowptr = np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int32)
    colidx = np.nonzero(mask)[1].astype(np.int32)
    return rowptr, colidx


def index_map(m, n, track, seed, window=None):
    """index arrays of a joint map: n features, feature f seen by `track` distinct poses drawn from a window of the m poses that
    moves along with f (neighbouring features are seen by much the same poses), U = the pose chain"""
    rng = np.random.default_rng(seed)
    window = min(m, window or 2 * track)
    photo, feature = [], []
    for f in range(n):
        lo = (f * max(1, m - window)) // max(1, n - 1) if n > 1 else 0
        p = np.sort(lo + rng.choice(window, size=min(track, window), replace=False))
        photo.append(p)
        feature.append(np.full(len(p), f))
    Ui = np.concatenate([np.arange(m), np.arange(m - 1)]).astype(np.int32)
    Uj = np.concatenate([np.arange(m), np.arange(1, m)]).astype(np.int32)
    return dict(m=m, n=n, Ui=Ui, Uj=Uj, photo=np.concatenate(photo).astype(np.int32), feature=np.concatenate(feature).astype(np.int32))


def distinct_pairs_per_run(j):
    """distinct pose pairs each run of PAT_RUN consecutive features forms (what one filling of the LDS set is asked to hold)"""
    photo, feature = np.asarray(j["photo"]), np.asarray(j["feature"])
    fptr = np.searchsorted(feature, np.arange(int(j["n"]) + 1))
    out = []
    for r0 in range(0, int(j["n"]), PAT_RUN):
        keys = set()
        for f in range(r0, min(r0 + PAT_RUN, int(j["n"]))):
            p = photo[fptr[f]:fptr[f + 1]].astype(np.int64)
            a, b = np.meshgrid(p, p)
            keys.update((np.minimum(a, b) * (1 << 32) + np.maximum(a, b))[a != b].tolist())
        out.append(len(keys))
    return out


def first_table_capacity(nU, m):
    """pattern_capacity of lsfm_pattern.hip"""
    cap = 1024
    while cap < 4 * (nU + 8 * m + 64):
        cap <<= 1
    return cap


def _long_track_joint_map(oracle):
    # (c) tracks of 80 frames over 100 poses: the features of one run are seen by ~85 poses and form ~3800 distinct pairs, more
    # than the PAIRSET_SLOTS = 2048 the set holds, so part of them finds no slot and goes to the global table directly
    maps = synth.make_stereo_set(100, new_per_frame=4, vis=80, seed=12)
    J, _, rc = oracle.divide_conquer([oracle.localmap_to_dict(mp) for mp in maps], False)
    assert rc == 0
    return J


CASES = {
    "a_handful": lambda oracle: index_map(7, 5, 3, seed=1),
    "b_one_more_than_a_run": lambda oracle: index_map(40, 3 * PAT_RUN + 1, 6, seed=2),
    "b_one_more_than_a_work_group": lambda oracle: index_map(60, 2 * PAT_WG + 1, 9, seed=3),
    "b_one_short_of_a_run": lambda oracle: index_map(40, 2 * PAT_RUN - 1, 2, seed=4),
    "c_long_tracks_spill": _long_track_joint_map,
    "c_spill_index_only": lambda oracle: index_map(300, 5 * PAT_RUN + 3, 90, seed=5, window=120),
    "d_first_table_overflows": lambda oracle: index_map(120, 400, 12, seed=6, window=120),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_schur_pattern_equals_numpy(ctx, oracle, case):
    """lsfm_schur_pattern (U's pairs + the diagonal + all pose pairs of every feature's W run through the work-group's set, compaction,
    packed sort, block CSR) against numpy_pattern: equality of (rowptr, colidx)."""
    J = CASES[case](oracle)
    exp_rowptr, exp_colidx = numpy_pattern(J)
    if case.startswith("c_"):
        most = max(distinct_pairs_per_run(J))
        print(f"{case}: most distinct pairs of one run of {PAT_RUN} features {most}, the set holds {PAIRSET_SLOTS}")
        assert most > PAIRSET_SLOTS, most  # the spill path runs
    if case.startswith("d_"):
        cap = first_table_capacity(len(J["Ui"]), J["m"])
        print(f"{case}: {len(exp_colidx)} blocks, first table {cap} slots")
        assert 2 * len(exp_colidx) > cap  # more than half full: the table is built again, four times as large
    rowptr, colidx = ctx.schur_pattern(J)
    assert np.array_equal(rowptr, exp_rowptr), case
    assert np.array_equal(colidx, exp_colidx), case


def _same_structure(got, exp):
    assert np.array_equal(got["stno"], exp["stno"])
    assert got["Ref"] == exp["Ref"] and got["FRef"] == exp["FRef"]
    for k in ("photo", "feature", "Ui", "Uj", "FBlock"):
        assert np.array_equal(got[k], exp[k]), k


@pytest.mark.parametrize("N,npf,vis,seed,lap", [
    (33, 6, 2, 5, 0),       # vis = 2: neighbouring maps share a pose and NO feature -- the cross pairs get zero matched features; a carry
    (37, 6, 5, 4, 0),       # an unpaired carry at three levels
    (40, 4, 40, 8, 0),      # tracks as long as the set: many poses per matched feature
    (150, 10, 5, 3, 30),    # loop closures: features matched across distant poses
    (300, 12, 5, 10, 50),   # loop closures and carries
])
def test_patterns_made_ahead_equal_the_joint_maps(ctx, oracle, monkeypatch, N, npf, vis, seed, lap):
    maps = synth.make_stereo_set(N, new_per_frame=npf, vis=vis, seed=seed, lap=lap)
    dicts = [oracle.localmap_to_dict(m) for m in maps]
    if vis == 2:
        ids = [set(np.asarray(m.stno)[np.asarray(m.stno) > 0].tolist()) for m in maps]
        assert all(not (ids[k] & ids[k + 1]) for k in range(N - 1))
    monkeypatch.setenv("LSFM_CHECK_EARLY_PATTERN", "1")
    got, stats, rc = ctx.divide_conquer(dicts, False)
    monkeypatch.delenv("LSFM_CHECK_EARLY_PATTERN")
    assert rc == 0, stats
    exp, _, orc = oracle.divide_conquer(dicts, False)
    assert orc == 0
    _same_structure(got, exp)
    err = pose_param_err(got["stVal"], exp["stVal"], exp["stno"])
    print(f"{N} maps, vis {vis}, lap {lap}: pose parameter max rel err vs oracle {err:.2e}")
    assert err < TREE_TOL, err
