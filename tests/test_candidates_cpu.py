"""No GPU: lsfm_map_feature_pair_candidates is built, declared and bound; the pair-list file (lsfm_save_pair_list / lsfm_read_pair_list, host
code) round-trips and is what -gate reads; and the bound the candidate search rests on,
    q_fg = 1/2 d^T (Sigma_ff + Sigma_gg)^-1 d  <=  d^2_fg = d^T Var(x_f - x_g)^-1 d,
holds on the oracle's trees of the four split sets of tests/test_gpu_merge.py against a dense inverse, with the counts DESIGN.md
section 19 records.  The last group compares numpy with numpy: it is the ground under the GPU tests, not coverage of the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from linearsfm_amd import api
import candidates_reference as cref
import merge_reference as ref
from test_gpu_covariance import SMALL, _small_set, dense_sigma

NAMES = ("lsfm_map_feature_pair_candidates", "lsfm_map_feature_pair_candidates_timed", "lsfm_save_pair_list", "lsfm_read_pair_list")


def test_symbols_exported_declared_and_bound():
    L = C.CDLL(api.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "lsfm.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in api.EXPORTS
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert getattr(api.lib(), name).argtypes is not None
    for meth in ("feature_pair_candidates", "feature_pair_candidates_raw"):
        assert callable(getattr(api.Context, meth, None)), meth
    for fn in ("save_pair_list", "read_pair_list"):
        assert callable(getattr(api, fn, None)), fn


# ---- the pair-list file ------------------------------------------------------------------------------------------------------------------
def _gate_reader(path):
    """The reader -gate documents (csrc/lsfm_cli.cpp): whitespace-separated feature ids, two per candidate."""
    ids = [int(t) for t in open(path).read().split()]
    assert len(ids) % 2 == 0
    return np.array(ids, np.int64).reshape(-1, 2)


def test_pair_list_round_trip(tmp_path):
    path = str(tmp_path / "pairs.txt")
    for ids in ([[9, 100009], [5, 30], [2, 2147483647]], [[1, 2]], np.zeros((0, 2), np.int32)):
        api.save_pair_list(path, ids)
        got = api.read_pair_list(path)
        assert got.dtype == np.int32 and got.shape == (len(ids), 2)
        assert np.array_equal(got, np.asarray(ids, np.int32).reshape(-1, 2))
        lines = open(path).read().splitlines()
        assert len(lines) == len(ids) and all(len(l.split()) == 2 for l in lines)
        assert np.array_equal(_gate_reader(path), np.asarray(ids, np.int64).reshape(-1, 2))
        assert not os.path.exists(path + ".tmp")
    with pytest.raises(api.LsfmError):
        api.save_pair_list(path, [1, 2, 3])


def test_pair_list_hand_written(tmp_path):
    p = tmp_path / "h.txt"
    p.write_text("17 100017\n\n  3\t4  \n5 6")
    assert api.read_pair_list(str(p)).tolist() == [[17, 100017], [3, 4], [5, 6]]
    # a cap that is too small: LSFM_ERR_ARG, the count still set
    ids = np.zeros((2, 2), np.int32)
    cnt = C.c_longlong(-1)
    rc = api.lib().lsfm_read_pair_list(str(p).encode(), ids.ctypes.data_as(C.POINTER(C.c_int)), 2, C.byref(cnt))
    assert rc == -1 and cnt.value == 3 and ids.tolist() == [[17, 100017], [3, 4]]
    with pytest.raises(api.LsfmError):
        api.read_pair_list(str(p), cap=2)


def test_pair_list_odd_count_and_truncated_line_are_refused(tmp_path):
    p = tmp_path / "cut.txt"
    for text in ("17 100017\n3\n", "17 100017\n3 4\n5", "17 100017\n3 x\n", "17 100017\n3 4 1.5\n", "1 2 3\n"):
        p.write_text(text)
        cnt = C.c_longlong(0)
        ids = np.zeros((8, 2), np.int32)
        rc = api.lib().lsfm_read_pair_list(str(p).encode(), ids.ctypes.data_as(C.POINTER(C.c_int)), 8, C.byref(cnt))
        assert rc == -6, text  # LSFM_ERR_IO
        with pytest.raises(api.LsfmError):
            api.read_pair_list(str(p))
    with pytest.raises(api.LsfmError):
        api.read_pair_list(str(tmp_path / "missing.txt"))


# ---- the bound, on the oracle's trees of the four split sets -------------------------------------------------------------------------------
# (index into SMALL, features split): gate accepts, candidates, feature pairs -- the table of DESIGN.md section 19
TABLE = {(2, 8): (8, 8, 4560), (3, 32): (32, 33, 67528), (6, 8): (8, 10, 3828), (7, 32): (36, 40, 64620)}


def _all_d2(Sig, m, x):
    """(f, g, d2) of the exact gate over ALL feature pairs of a dense Sigma."""
    n = len(x)
    o = 6 * m
    B = Sig[o:, o:].reshape(n, 3, n, 3).transpose(0, 2, 1, 3)
    f, g = np.triu_indices(n, 1)
    Sd = B[f, f] + B[g, g] - B[f, g] - B[g, f]
    d = x[f] - x[g]
    return f, g, np.einsum("ki,ki->k", d, np.linalg.solve(Sd, d[:, :, None])[:, :, 0])


@pytest.mark.parametrize("i,count", sorted(TABLE))
def test_bound_on_split_sets(oracle, i, count):
    mono, n, kw = SMALL[i]
    dicts = [oracle.localmap_to_dict(mp) for mp in _small_set(mono, n, kw)]
    sd, chosen = ref.split_set(dicts, count)
    G, _, rc = oracle.divide_conquer(sd, mono)
    assert rc == 0
    m, nf = int(G["m"]), int(G["n"])
    x = cref.features_of(G)
    Sig = dense_sigma(G, mono)
    f, g, d2 = _all_d2(Sig, m, x)
    o = 6 * m
    fcov = np.stack([Sig[o + 3 * a: o + 3 * a + 3, o + 3 * a: o + 3 * a + 3] for a in range(nf)])
    f2, g2, q, bad = cref.all_q(x, fcov)
    assert np.array_equal(f, f2) and np.array_equal(g, g2) and not bad.any()
    tau = cref.TAU
    accept, cand = d2 <= tau, q <= tau
    split = {tuple(sorted(map(int, p))) for p in ref.split_pairs(G, chosen)}
    cset = {(int(a), int(b)) for a, b in zip(f[cand], g[cand])}
    ratio = float(np.max(q / d2))
    print(f"bound {SMALL[i][:2]} x{count}: pairs {len(f)}, gate accepts {int(accept.sum())}, candidates {int(cand.sum())}, split among them "
          f"{len(split & cset)} / {len(split)}, max q / d2 {ratio:.4f}")
    # nothing sits on the threshold: the counts below do not hang on a rounding
    assert not np.any(np.abs(d2 - tau) <= 1e-6 * tau) and not np.any(np.abs(q - tau) <= 1e-6 * tau)
    assert np.all(q <= d2 * (1 + 1e-9))          # the bound itself, every pair
    assert not np.any(accept & ~cand)            # no accepted pair is lost
    assert split <= cset and len(split) == count  # every split pair is a candidate
    assert cand.sum() <= 0.01 * len(f)
    assert (int(accept.sum()), int(cand.sum()), len(f)) == TABLE[i, count]
    # the helper's brute force says the same
    r = cref.candidates(x, 2.0 * float(np.max(np.ptp(x, axis=0))), fcov, tau)
    assert {tuple(p) for p in r["pairs"].tolist()} == cset
