"""No GPU: lsfm_map_merge_features is built, declared and bound; the -mergeout file round-trips (lsfm_save_merge_report /
lsfm_read_merge_report, host code); the structure (csrc/lsfm_merge_structure.cpp, lsfm_merge_structure) equals merge_reference.merged_blocks'
index arrays on the oracle's trees of the eight small sets; every refusal names its reason; and the two host statements of the merge
that the GPU tests measure against (merge_reference.py) agree with each other -- the floor under the GPU tests' bars."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from linearsfm_amd import api
import feature_cov_reference as fref
import merge_reference as ref
from test_gpu_covariance import SMALL, _pose_blocks, _small_set, dense_sigma, schur_sigma

NAMES = ("lsfm_map_merge_features", "lsfm_map_merge_features_timed", "lsfm_merge_structure", "lsfm_save_merge_report", "lsfm_read_merge_report")


def test_symbols_exported_declared_and_bound():
    L = C.CDLL(api.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "lsfm.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in api.EXPORTS
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert getattr(api.lib(), name).argtypes is not None
    for meth in ("merge_features", "merge_features_raw"):
        assert callable(getattr(api.Context, meth, None)), meth
    for fn in ("merge_structure", "save_merge_report", "read_merge_report"):
        assert callable(getattr(api, fn, None)), fn


# ---- the report file ----------------------------------------------------------------------------------------------------------------------
def test_report_round_trip(tmp_path):
    ids = np.array([[9, 100009, 9], [30, 5, 5], [2, 9, 2]])
    for d2 in (0.1 + 0.2, 1e300, -0.0):
        path = str(tmp_path / "m.txt")
        api.save_merge_report(path, ids, 2, 6, d2)
        r = api.read_merge_report(path)
        assert (r["K"], r["removed"], r["dof"]) == (3, 2, 6)
        assert r["d2"] == d2 and np.signbit(r["d2"]) == np.signbit(d2)
        assert np.array_equal(r["ids"], ids)
        lines = open(path).read().splitlines()
        assert len(lines) == 4 and len(lines[0].split()) == 4 and all(len(l.split()) == 3 for l in lines[1:])
        assert not os.path.exists(path + ".tmp")


def test_report_hand_written(tmp_path):
    p = tmp_path / "m.txt"
    p.write_text("2 2 6 12.5\n17 100017 17\n3 4 3\n")
    r = api.read_merge_report(str(p))
    assert r["K"] == 2 and r["removed"] == 2 and r["dof"] == 6 and r["d2"] == 12.5
    assert r["ids"].tolist() == [[17, 100017, 17], [3, 4, 3]]


def test_report_truncated_line_is_refused(tmp_path):
    p = tmp_path / "cut.txt"
    for text in ("2 2 6 12.5\n17 100017 17\n3 4\n", "2 2 6 12.5\n17 100017 17\n", "2 2 6\n", "1 1 3 0.5\n1 2 1\n4 5 4\n", ""):
        p.write_text(text)
        with pytest.raises(api.LsfmError):
            api.read_merge_report(str(p))
    with pytest.raises(api.LsfmError):
        api.save_merge_report(str(tmp_path / "x.txt"), [[1, 2]], 1, 3, 0.5)


# ---- the structure ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tree(oracle, i):
    """The oracle's tree of SMALL[i], its local map dicts; computed once, changed by no test."""
    mono, n, kw = SMALL[i]
    dicts = [oracle.localmap_to_dict(mp) for mp in _small_set(mono, n, kw)]
    G, _, rc = oracle.divide_conquer(dicts, mono)
    assert rc == 0
    return mono, dicts, G


def _check_structure(G, pairs, what):
    exp, rep, sptr, sidx = ref.merged_blocks(G, pairs)
    got = api.merge_structure(G, pairs)
    for k, e in (("rep", rep), ("photo", exp["photo"]), ("feature", exp["feature"]), ("FBlock", exp["FBlock"]), ("sptr", sptr), ("sidx", sidx)):
        assert np.array_equal(got[k], e), (what, k)
    n = int(G["n"])
    _, members = ref.classes(n, pairs)
    v = got["info"]
    assert v["n"] == len(members) and v["nW"] == len(exp["photo"]) and v["removed"] == n - len(members)
    assert v["classes"] == sum(len(c) > 1 for c in members) and v["summed_blocks"] == int(np.sum(np.diff(sptr) > 1))
    return got


@pytest.mark.parametrize("i", range(len(SMALL)))
def test_structure_vs_reference(oracle, i):
    _, _, G = _tree(oracle, i)
    n = int(G["n"])
    assert n >= 4
    one = _check_structure(G, [(1, 0)], "K=1")
    assert one["info"]["n"] == n - 1 and one["rep"][0] == 0 and one["rep"][1] == 0
    chain = _check_structure(G, [(0, 1), (1, 2), (3, 2)], "chain")
    assert chain["info"]["n"] == n - 3 and chain["info"]["classes"] == 1 and not chain["rep"][:4].any()
    _check_structure(G, [(0, n - 1)], "(0, n-1)")
    a = _check_structure(G, [(2, n - 2)], "single")
    b = _check_structure(G, [(2, n - 2), (n - 2, 2), (2, n - 2)], "twice and reversed")
    assert all(np.array_equal(a[k], b[k]) for k in ("rep", "photo", "feature", "FBlock", "sptr", "sidx"))
    every = _check_structure(G, [(f, f + 1) for f in range(n - 1)], "one class")
    assert every["info"]["n"] == 1 and len(np.unique(every["photo"])) == len(every["photo"]) and every["sptr"][-1] == len(G["photo"])
    _check_structure(G, [(0, 1), (1, 2), (2, 0), (3, 1)], "a cycle")


@pytest.mark.parametrize("i", [2, 6])
def test_structure_repeated_block(oracle, i):
    """A member whose W block to one pose is stored as two halves: untouched it keeps both, merged they are summed into one block."""
    _, _, G = _tree(oracle, i)
    n = int(G["n"])
    f = n // 2
    Gs = fref.split_block(G, f)
    w = int(np.nonzero(np.asarray(Gs["feature"]) == f)[0][0])
    un = _check_structure(Gs, [(0, 1)], "untouched")
    o = int(un["FBlock"][un["rep"][f]])
    assert un["photo"][o] == un["photo"][o + 1] and np.array_equal(un["sidx"][un["sptr"][o]: un["sptr"][o + 2]], [w, w + 1])
    mg = _check_structure(Gs, [(f, n // 3)], "merged")
    c = int(mg["rep"][f])
    run = mg["photo"][mg["FBlock"][c]: (mg["FBlock"][c + 1] if c + 1 < len(mg["FBlock"]) else len(mg["photo"]))]
    assert len(np.unique(run)) == len(run) and np.all(np.diff(run) > 0)
    assert mg["info"]["summed_blocks"] >= 1


def test_structure_refusals(oracle):
    _, _, G = _tree(oracle, 2)
    n = int(G["n"])
    for bad, word in (([], "K < 1"), ([(0, n)], "not one of"), ([(-1, 0)], "not one of"), ([(3, 3)], "twice")):
        with pytest.raises(api.LsfmError, match=word):
            api.merge_structure(G, bad)
    d = dict(G)
    fe = np.array(G["feature"], np.int32, copy=True)
    fe[0], fe[-1] = fe[-1], fe[0]
    d["feature"] = fe
    with pytest.raises(api.LsfmError, match="sorted by feature"):
        api.merge_structure(d, [(0, 1)])
    # a cap that is too small
    h = api.HostMap(G)
    q = np.array([0, 1], np.int32)
    small = np.zeros(4, np.int32)
    why = C.create_string_buffer(256)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    rc = api.lib().lsfm_merge_structure(C.byref(h.c), p(q), 1, None, p(small), None, None, None, None, 3, None, why, len(why))
    assert rc == -1 and b"cap_w" in why.value
    rc = api.lib().lsfm_merge_structure(C.byref(h.c), p(q), 1, None, None, None, None, None, None, 0, None, why, len(why))
    assert rc == 0 and why.value == b""


# ---- the floor: routes A and B on the oracle's trees ----------------------------------------------------------------------------------------
def _floor_cases(oracle, i):
    """(what, map, pairs): split pairs (count 1, and 32 where the set has that many features held by two maps -- the 2-map sets have 16
    --, through the oracle's tree of the split set) where the set has >= 2 maps, and 24 seeded pairs on the tree of the set itself; every map with its diagonal blocks made exactly symmetric (feature_cov_reference)."""
    mono, dicts, G = _tree(oracle, i)
    out = []
    if len(dicts) >= 2:
        for count in (1, 32):
            if len(ref.split_candidates(dicts)[0]) < count:
                continue
            sd, chosen = ref.split_set(dicts, count)
            Gs, _, rc = oracle.divide_conquer(sd, mono)
            assert rc == 0
            pairs = ref.split_pairs(Gs, chosen)
            seen = [set(np.asarray(Gs["photo"])[np.asarray(Gs["feature"]) == f]) for f in pairs.ravel()]
            assert all(seen[2 * a] & seen[2 * a + 1] for a in range(len(pairs)))  # a pose sees both halves: every merge sums blocks
            out.append((f"split {count}", fref.symmetric_blocks(Gs), pairs))
    out.append(("seeded 24", fref.symmetric_blocks(G), fref.seeded_pairs(int(G["n"]), 24)))
    return mono, out


@pytest.mark.parametrize("i", range(len(SMALL)))
def test_host_routes_agree(oracle, i):
    """The floor: the constraint form on the dense inverse and the merged Schur system agree below 1e-10 on the state (metric of
    merge_reference.state_err), on D^2 relative, and on the pose and feature blocks of Sigma' against Sigma_c (merge_reference.sigma_err:
    normalised by the UNMERGED variances, the scale of the two terms whose difference Sigma_c is); BAR c <= 1e-3 on every case.
    Measured with exactly these definitions (worst over the cases of a group): Stereo sets D^2 2.3e-15, state 7.8e-14, Sigma' 8.9e-13;
    Mono sets D^2 1.6e-11, state 3.9e-11, Sigma' 4.4e-11; c <= 5.1 on split pairs, <= 1.2e4 on the seeded pairs of the 40-map Mono set.
    This test compares two numpy routes of merge_reference.py: it calls nothing of the library and passes without it.  It is the
    floor under the GPU tests' bars, not coverage of lsfm_map_merge_features."""
    mono, cases = _floor_cases(oracle, i)
    for what, G, pairs in cases:
        m = int(G["m"])
        Sig = dense_sigma(G, mono)
        A = ref.merged_dense(G, mono, pairs, Sig)
        Gm, yB, d2B = ref.route_b(G, mono, pairs)
        no = int(Gm["n"])
        kept = ref.kept_scalars(m, A["members"])
        e_state = ref.state_err(yB, A["y"], Sig, kept, A["d2"])
        e_d2 = abs(d2B - A["d2"]) / A["d2"]
        Sp, F = schur_sigma(Gm, mono)
        e_sig = ref.sigma_err(_pose_blocks(Sp, m), F, A["Sigma_c"], Sig, kept, m, no)
        # the merged matrix itself: T^T I T is the merged map's own I
        import scipy.sparse as sp
        U1, W1, V1, _, _ = ref._sparse_parts(Gm)
        I1 = sp.bmat([[U1, W1], [W1.T, V1]]).toarray()
        e_I = float(np.max(np.abs(I1 - A["I1"]) / np.sqrt(np.maximum(np.outer(np.diag(I1), np.diag(I1)), 1e-300))))
        print(f"host routes {SMALL[i][:2]} {what}: K {len(pairs)}, dof {A['dof']}, D2 {A['d2']:.3g}, c {A['c']:.3g}, D2 rel {e_d2:.2e}, "
              f"state {e_state:.2e}, Sigma' {e_sig:.2e}, I' {e_I:.1e}")
        assert ref.BAR * A["c"] <= ref.CAP
        assert e_I < 1e-14
        assert e_state < 1e-10 and e_d2 < 1e-10 and e_sig < 1e-10
