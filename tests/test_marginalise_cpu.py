"""No device: the C ABI of the marginalisation is there, a map without features survives the file formats, and -- with the oracle and
numpy alone -- the property the feature rests on: sub-tree roots whose private features were marginalised out join to the state the
full roots join to.  The figures printed here are the floor against which the bars of tests/test_gpu_marginalise.py are read."""
import os
import re

import numpy as np
import pytest

from common import feat_param_err, pose_param_err
from linearsfm_amd import api, synth
from refdump import dense_info

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["lsfm_map_marginalise", "lsfm_tree_export_reduced_size", "lsfm_tree_export_reduced_dev"]
STEREO40 = (40, 8, 5, dict(lap=12, home=4, revisit=0.5))  # the 40-map sets of test_gpu_linearise.py, seed 9
MONO40 = (40, 8, 4, synth.SPIRAL)


def test_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "lsfm.h")).read()
    for name in SYMBOLS:
        assert getattr(api.lib(), name) is not None
        assert name in api.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name


def test_a_map_without_features_survives_the_file_format(tmp_path):
    """Dropping every feature leaves the pose graph, n = 0 and nW = 0: lsfm_write_localmap / lsfm_read_localmap keep it."""
    m = 3
    rng = np.random.default_rng(0)
    U = rng.standard_normal((4, 36))
    g = dict(Ref=0, FRef=0, m=m, n=0, stno=np.repeat(-(np.arange(m) + 1), 6).astype(np.int32), stVal=rng.standard_normal(6 * m), U=U,
             Ui=np.array([0, 0, 1, 2], np.int32), Uj=np.array([0, 1, 1, 2], np.int32), W=np.zeros((0, 18)), photo=np.zeros(0, np.int32),
             feature=np.zeros(0, np.int32), V=np.zeros((0, 9)), FBlock=np.zeros(0, np.int32))
    path = str(tmp_path / "graph.txt")
    api.write_localmap(path, g, False)
    back = api.read_localmap(path, False)
    assert back["m"] == m and back["n"] == 0 and back["nW"] == 0 and len(back["photo"]) == 0
    for k in ("stno", "stVal", "Ui", "Uj"):
        assert np.array_equal(back[k], g[k]), k
    assert np.array_equal(back["U"], U)


def numpy_marginalise(d, drop):
    """The map dict d with the flagged features marginalised out, by numpy on the dense matrix (feature by feature, 3x3 inverses), in
    the canonical form of lsfm_map_marginalise."""
    m, n = int(d["m"]), int(d["n"])
    drop = np.asarray(drop, bool)
    I = dense_info(d)
    P = I[:6 * m, :6 * m].copy()
    ph, fe = np.asarray(d["photo"]), np.asarray(d["feature"])
    pairs = {(p, p) for p in range(m)} | {(int(min(a, b)), int(max(a, b))) for a, b in zip(d["Ui"], d["Uj"])}
    for f in np.nonzero(drop)[0]:
        r = slice(6 * m + 3 * f, 6 * m + 3 * f + 3)
        P -= I[:6 * m, r] @ np.linalg.inv(I[r, r]) @ I[r, :6 * m]
        ps = np.unique(ph[fe == f])
        pairs.update((int(a), int(b)) for k, a in enumerate(ps) for b in ps[k:])
    pairs = sorted(pairs)
    keep = np.nonzero(~drop)[0]
    wk = ~drop[fe]
    new = np.cumsum(~drop) - 1
    stno, st = np.asarray(d["stno"]), np.asarray(d["stVal"])
    idx = np.concatenate([np.arange(6 * m), (6 * m + 3 * keep[:, None] + np.arange(3)).reshape(-1)]).astype(np.int64)
    out = dict(d, n=len(keep), stno=stno[idx], stVal=st[idx], Ui=np.array([p[0] for p in pairs], np.int32), Uj=np.array([p[1] for p in pairs], np.int32),
               U=np.stack([P[6 * a:6 * a + 6, 6 * b:6 * b + 6].reshape(36) for a, b in pairs]), W=np.asarray(d["W"])[wk], photo=ph[wk],
               feature=new[fe[wk]].astype(np.int32), V=np.asarray(d["V"])[keep])
    out["FBlock"] = np.searchsorted(out["feature"], np.arange(len(keep))).astype(np.int32)
    out["nU"], out["nW"] = len(pairs), int(np.sum(wk))
    return out


@pytest.mark.parametrize("mono,N,blk", [(False, 8, 4), (False, 32, 8), (True, 8, 4), (True, 32, 8)], ids=["stereo8", "stereo32", "mono8", "mono32"])
def test_reduced_roots_join_to_the_state_of_the_full_roots(oracle, mono, N, blk):
    """Blocks of consecutive maps joined to roots by the oracle, every feature that only one root holds marginalised out by numpy, the
    roots joined by the oracle: the kept variables against the tree over the full roots at the project's bar on the state, 1e-6.  The
    arithmetic allows far more: measured here 2e-13 .. 4e-10 (the oracle's two-stage tree over full roots is its one-stage tree bit for
    bit: blocks of 2^k maps are sub-trees of the same binary tree).  The information matrix of the reduced result against the marginal of
    the full result, in |d_ij| / sqrt(I_ii I_jj): a join's matrix is formed at the state its transforms linearise at, so it is pinned
    no tighter than that state is -- the same 1e-6; measured 3e-14 .. 9e-10."""
    n40, npf, vis, kw = MONO40 if mono else STEREO40
    maps = (synth.make_mono_set(n40, npf, vis, seed=9, **kw) if mono else synth.make_stereo_set(n40, npf, vis, seed=9, **kw))[:N]
    dicts = [oracle.localmap_to_dict(x) for x in maps]
    bounds = [(lo, lo + blk) for lo in range(0, N, blk)]
    roots = []
    for r, (lo, hi) in enumerate(bounds):
        root, _, rc = oracle.divide_conquer(dicts[lo:hi], mono, final_reanchor=(r % 2 == 1))
        assert rc == 0
        roots.append(root)
    ids = [np.asarray(g["stno"])[6 * int(g["m"])::3] for g in roots]
    allids, cnt = np.unique(np.concatenate(ids), return_counts=True)
    keep_ids = allids[cnt >= 2]
    reduced = [numpy_marginalise(g, ~np.isin(i, keep_ids)) for g, i in zip(roots, ids)]
    full, _, rc = oracle.divide_conquer(roots, mono)
    assert rc == 0
    red, _, rc = oracle.divide_conquer(reduced, mono)
    assert rc == 0
    one, _, rc = oracle.divide_conquer(dicts, mono)
    assert rc == 0
    m, nf = int(full["m"]), int(full["n"])
    assert int(red["m"]) == m and np.array_equal(np.asarray(red["stno"])[:6 * m], np.asarray(full["stno"])[:6 * m])
    fid = np.asarray(full["stno"])[6 * m::3]
    kept = np.isin(fid, keep_ids)
    assert np.array_equal(np.asarray(red["stno"])[6 * m::3], fid[kept])
    idx = np.concatenate([np.arange(6 * m), (6 * m + 3 * np.nonzero(kept)[0][:, None] + np.arange(3)).reshape(-1)]).astype(np.int64)
    ep, ef = pose_param_err(red["stVal"], np.asarray(full["stVal"])[idx], red["stno"]), feat_param_err(red["stVal"], np.asarray(full["stVal"])[idx], red["stno"])
    assert np.array_equal(np.asarray(one["stno"]), np.asarray(full["stno"]))
    e1 = max(pose_param_err(red["stVal"], np.asarray(one["stVal"])[idx], red["stno"]), feat_param_err(red["stVal"], np.asarray(one["stVal"])[idx], red["stno"]))
    e2 = max(pose_param_err(full["stVal"], one["stVal"], one["stno"]), feat_param_err(full["stVal"], one["stVal"], one["stno"]))
    I = dense_info(full)
    E = dense_info(numpy_marginalise(full, ~kept))
    d = np.sqrt(np.where(np.diag(I)[idx] == 0, 1.0, np.diag(I)[idx]))
    ei = float(np.max(np.abs(dense_info(red) - E) / np.outer(d, d)))
    dropped = sum(int(np.sum(~np.isin(i, keep_ids))) for i in ids)
    print(f"{'Mono' if mono else 'Stereo'} {N} maps in blocks of {blk}: {dropped} of {sum(len(i) for i in ids)} features dropped; kept variables against the tree "
          f"over full roots: poses {ep:.2e} features {ef:.2e}; against the one-stage tree {e1:.2e} (full roots against it: {e2:.2e}); information matrix {ei:.2e}")
    assert ep <= 1e-6 and ef <= 1e-6
    assert ei <= 1e-6
