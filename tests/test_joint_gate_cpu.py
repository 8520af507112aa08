"""No GPU: lsfm_map_feature_pair_joint_gate is built, declared and bound; the report file (lsfm_save_joint_gate / lsfm_read_joint_gate, host
code) round-trips and refuses what it must; and the ground under the GPU tests: the two numpy routes of joint_gate_reference.select agree
on the oracle's trees of the four split sets of tests/test_gpu_merge.py, with the counts DESIGN.md section 20 records.  The last groups
compare numpy with numpy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from linearsfm_amd import api
import joint_gate_reference as jref
import merge_reference as ref
from test_gpu_covariance import SMALL, _small_set, dense_sigma

NAMES = ("lsfm_map_feature_pair_joint_gate", "lsfm_map_feature_pair_joint_gate_timed", "lsfm_selftest_pair_select", "lsfm_save_joint_gate",
         "lsfm_read_joint_gate")


def test_symbols_exported_declared_and_bound():
    L = C.CDLL(api.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "lsfm.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in api.EXPORTS
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert getattr(api.lib(), name).argtypes is not None
    for meth in ("feature_pair_joint_gate", "feature_pair_joint_gate_raw", "selftest_pair_select"):
        assert callable(getattr(api.Context, meth, None)), meth
    for fn in ("save_joint_gate", "read_joint_gate"):
        assert callable(getattr(api, fn, None)), fn
    assert int(re.search(r"#define\s+LSFM_JOINT_GATE_MAX\s+(\d+)", hdr).group(1)) == api.JOINT_GATE_MAX == 2048
    assert api.JOINT_GATE_TAU == jref.TAU


# ---- the report file -----------------------------------------------------------------------------------------------------------------------
def _report():
    ids = np.array([[9, 100009], [5, 30], [2, 2147483647], [5, 9]], np.int32)
    status = np.array([1, 0, 1, 2], np.int32)
    d2 = np.array([0.1, 1.0 / 3.0, 1e-300, np.nan])
    delta = np.array([0.1, np.nan, 7.123456789012345e10, 0.0])
    return ids, status, d2, delta, float(delta[0] + delta[2])


def test_report_round_trip(tmp_path):
    path = str(tmp_path / "jgate.txt")
    ids, status, d2, delta, D2 = _report()
    api.save_joint_gate(path, ids, status, d2, delta, D2)
    assert not os.path.exists(path + ".tmp")
    lines = open(path).read().splitlines()
    assert len(lines) == 5 and lines[0].split()[:4] == ["4", "2", "1", "6"] and float(lines[0].split()[4]) == D2
    assert all(len(l.split()) == 5 for l in lines[1:])
    r = api.read_joint_gate(path)
    assert (r["K"], r["accepted"], r["implied"], r["dof"]) == (4, 2, 1, 6) and r["D2"] == D2
    assert np.array_equal(r["ids"], ids) and np.array_equal(r["status"], status)
    assert np.array_equal(r["d2"], d2, equal_nan=True) and np.array_equal(r["delta"], delta, equal_nan=True)  # %.17g: bit for bit
    # a cap that is too small: LSFM_ERR_ARG with the head set
    head, D = np.zeros(4, np.int32), C.c_double(0.0)
    rc = api.lib().lsfm_read_joint_gate(path.encode(), None, None, None, None, 0, head.ctypes.data_as(C.POINTER(C.c_int)), C.byref(D))
    assert rc == -1 and head.tolist() == [4, 2, 1, 6] and D.value == D2
    with pytest.raises(api.LsfmError):
        api.save_joint_gate(path, ids[:3], status, d2, delta, D2)
    with pytest.raises(api.LsfmError):
        api.save_joint_gate(str(tmp_path / "no_such_dir" / "x.txt"), ids, status, d2, delta, D2)


def test_report_refusals(tmp_path):
    path = str(tmp_path / "jgate.txt")
    ids, status, d2, delta, D2 = _report()
    api.save_joint_gate(path, ids, status, d2, delta, D2)
    good = open(path).read().splitlines()
    p = tmp_path / "bad.txt"
    cases = {"a line cut short": good[:-1] + [" ".join(good[-1].split()[:4])], "a line missing": good[:-1], "a line too many": good + [good[-1]],
             "a status of 3": good[:2] + [good[2].replace(" 0 ", " 3 ", 1)] + good[3:], "accepted in the head": ["4 3 1 9 " + good[0].split()[4]] + good[1:],
             "dof in the head": ["4 2 1 5 " + good[0].split()[4]] + good[1:], "not a number": good[:1] + ["x " + good[1]] + good[2:], "empty": []}
    for what, lines in cases.items():
        p.write_text("\n".join(lines) + "\n")
        with pytest.raises(api.LsfmError):
            api.read_joint_gate(str(p), cap=16)
        head, D = np.zeros(4, np.int32), C.c_double(0.0)
        buf_i, buf_s, buf_d = np.zeros(32, np.int32), np.zeros(16, np.int32), np.zeros(16)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        rc = api.lib().lsfm_read_joint_gate(str(p).encode(), buf_i.ctypes.data_as(ip), buf_s.ctypes.data_as(ip), buf_d.ctypes.data_as(dp),
                                            buf_d.ctypes.data_as(dp), 16, head.ctypes.data_as(ip), C.byref(D))
        assert rc == -6, what  # LSFM_ERR_IO
    with pytest.raises(api.LsfmError):
        api.read_joint_gate(str(tmp_path / "missing.txt"), cap=4)


# ---- implied pairs: a hand-made list ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["conditional", "differences"])
def test_implied_pairs_hand_made(route):
    """Identity order, tau = inf: (0,1) (1,2) (3,4) | (1,0) reversed, (3,4) twice, (0,2) the triangle's third side, (2,3) independent,
    (0,4) implied through it."""
    Sig, x = jref.crafted_world(6, seed=3)
    ends = [(0, 1), (1, 2), (3, 4), (1, 0), (3, 4), (0, 2), (2, 3), (0, 4)]
    Cm, d = jref.crafted_problem(Sig, x, ends)
    s = jref.select(Cm, d, ends, np.inf, order=np.arange(len(ends)), route=route)
    assert s["status"].tolist() == [1, 1, 1, 2, 2, 2, 1, 2] and s["implied"] == 4
    assert np.all(s["delta"][s["status"] == 2] == 0.0)
    rows = np.concatenate([np.arange(3 * a, 3 * a + 3) for a in s["accepted"]])
    full = float(d[rows] @ np.linalg.solve(Cm[np.ix_(rows, rows)], d[rows]))
    assert abs(s["D2"] - full) <= 1e-12 * full
    # the whole C is singular exactly because of the implied rows
    assert np.linalg.matrix_rank(Cm) == 3 * len(s["accepted"])


# ---- the two routes and the table, on the oracle's trees of the four split sets ------------------------------------------------------------------
# (index into SMALL, features split): candidates K, gate accepts alone, sequential accepts, split pairs among the accepted, K at 10 tau
TABLE = {(2, 8): (8, 8, 8, 8, 8), (3, 32): (33, 32, 32, 32, 39), (6, 8): (10, 8, 8, 8, 48), (7, 32): (40, 36, 33, 32, 167)}
SUM_DELTA = {(2, 8): 7.79294, (3, 32): 18.1749, (6, 8): 12.5678, (7, 32): 83.065}  # six digits, as recorded
_TREE = {}


def split_tree(oracle, i, count):
    if (i, count) not in _TREE:
        mono, n, kw = SMALL[i]
        dicts = [oracle.localmap_to_dict(mp) for mp in _small_set(mono, n, kw)]
        sd, chosen = ref.split_set(dicts, count)
        G, _, rc = oracle.divide_conquer(sd, mono)
        assert rc == 0
        _TREE[i, count] = (mono, G, dense_sigma(G, mono), {tuple(sorted(map(int, p))) for p in ref.split_pairs(G, chosen)})
    return _TREE[i, count]


def _both_routes(G, Sig, pairs, tau, what):
    m = int(G["m"])
    Cm, d = jref.joint_matrix(Sig, m, pairs), jref.state_diff(G, pairs)
    a = jref.select(Cm, d, pairs, tau)
    b = jref.select(Cm, d, pairs, tau, route="differences")
    mar = jref.margins(a, tau)
    fin = np.isfinite(a["delta"])
    floor = float(np.max(np.abs(a["delta"][fin] - b["delta"][fin]) / np.maximum(1.0, a["delta"][fin])))
    fD = abs(a["D2"] - b["D2"]) / a["D2"]
    print(f"joint gate reference {what}: K {len(pairs)}, gate accepts {int(np.sum(a['d2'] <= tau))}, sequential accepts {len(a['accepted'])}, implied "
          f"{a['implied']}, D2 {a['D2']:.9g}, nearest |x / tau - 1| {mar:.3g}, kappa_s {jref.scaled_condition(Cm, a['accepted']):.3g}, host floor: "
          f"delta {floor:.2e}, D2 {fD:.2e}")
    assert mar > jref.REL  # nothing sits on the threshold: the counts do not hang on a rounding
    assert np.array_equal(a["status"], b["status"])
    assert floor < 1e-11 and fD < 1e-11
    return a


@pytest.mark.parametrize("i,count", sorted(TABLE))
def test_table_on_split_sets(oracle, i, count):
    mono, G, Sig, split = split_tree(oracle, i, count)
    pairs = jref.candidate_list(G, Sig, jref.TAU)
    a = _both_routes(G, Sig, pairs, jref.TAU, f"{SMALL[i][:2]} x{count}")
    acc = {tuple(map(int, pairs[k])) for k in a["accepted"]}
    got = (len(pairs), int(np.sum(a["d2"] <= jref.TAU)), len(a["accepted"]), len(split & acc))
    assert got == TABLE[i, count][:4] and len(split) == count
    assert abs(a["D2"] - SUM_DELTA[i, count]) <= 1e-5 * SUM_DELTA[i, count]
    # the larger list at 10 tau: the same accepted set
    big = jref.candidate_list(G, Sig, 10.0 * jref.TAU)
    assert len(big) == TABLE[i, count][4]
    b = _both_routes(G, Sig, big, jref.TAU, f"{SMALL[i][:2]} x{count}, candidates at 10 tau")
    assert {tuple(map(int, big[k])) for k in b["accepted"]} == acc
    assert abs(b["D2"] - a["D2"]) <= 1e-11 * a["D2"]
