"""What the tests of lsfm_gn_linearise_features share (test_linearise_features_cpu.py, test_gpu_linearise_features.py,
test_gpu_cli_relinf.py): the weight distribution, the pattern of the result stated from the labels, the maps I_k(w) as dicts by two host
routes, and the oracle's dense H of re-weighted sets, computed once per set.

The expected H is the oracle's on the dicts tests/robust_features_ref.py::reweight writes (I_k(w) as a map: appended U blocks, W and V
scaled); map weights scale a re-weighted dict's U, W and V (H, b and F are linear in every map's information)."""
import functools

import numpy as np

import robust_features_ref as rf
from test_gpu_linearise import _case, label_structure, oracle_dense_h

CRAFTED = "crafted"


def feature_weights(dicts, seed):
    """Per map an array over its features: uniform in [0.1, 1] from `seed`, a tenth of the instances (rounded up) set to exactly 1."""
    rng = np.random.default_rng(seed)
    ns = [int(d["n"]) for d in dicts]
    w = rng.uniform(0.1, 1.0, sum(ns))
    if len(w):
        w[rng.choice(len(w), (len(w) + 9) // 10, replace=False)] = 1.0
    return np.split(w, np.cumsum(ns)[:-1])


def co_observation_pairs(dicts, G):
    """The joint image of every co-observation pair: (min, max) of the global poses of every two poses (or one pose, twice) of a local
    map that see a common feature of it."""
    m = int(G["m"])
    stno = np.asarray(G["stno"])
    pid = {int(-stno[6 * i]): i for i in range(m)}
    out = set()
    for L in dicts:
        ls = np.asarray(L["stno"])
        gp = [pid[int(-ls[6 * i])] for i in range(int(L["m"]))]
        seen = {}
        for p, f in zip(np.asarray(L["photo"]).tolist(), np.asarray(L["feature"]).tolist()):
            seen.setdefault(f, set()).add(gp[p])
        for ps in seen.values():
            out.update((min(a, b), max(a, b)) for a in ps for b in ps)
    return out


def scaled(dicts, w):
    out = []
    for d, wk in zip(dicts, w):
        e = dict(d)
        e["U"], e["W"], e["V"] = np.asarray(d["U"]) * wk, np.asarray(d["W"]) * wk, np.asarray(d["V"]) * wk
        out.append(e)
    return out


def reweighted(dicts, fw, w=None):
    """The set with map k replaced by I_k(fw_k) (rf.reweight), times w_k where map weights are given."""
    out = [rf.reweight(d, x) for d, x in zip(dicts, fw)]
    return out if w is None else scaled(out, w)


def dict_from_dense(d, H):
    """A map dict with d's labels and estimate whose information is the dense matrix H (6m + 3n, block diagonal over the features): one
    U block per pose pair a <= b, d's W pattern (a repeated (pose, feature) pair: the block once, zeros in the repeats), V."""
    m, n = int(d["m"]), int(d["n"])
    e = dict(d)
    ij = [(a, b) for a in range(m) for b in range(a, m)]
    e["Ui"], e["Uj"] = np.array([a for a, _ in ij], np.int32), np.array([b for _, b in ij], np.int32)
    e["U"] = np.stack([H[6 * a:6 * a + 6, 6 * b:6 * b + 6] for a, b in ij]).reshape(-1, 36)
    W, done = [], set()
    for a, f in zip(np.asarray(d["photo"]).tolist(), np.asarray(d["feature"]).tolist()):
        W.append(np.zeros((6, 3)) if (a, f) in done else H[6 * a:6 * a + 6, 6 * m + 3 * f:6 * m + 3 * f + 3])
        done.add((a, f))
    e["W"] = np.array(W).reshape(-1, 18)
    e["V"] = np.array([H[6 * m + 3 * f:6 * m + 3 * f + 3, 6 * m + 3 * f:6 * m + 3 * f + 3] for f in range(n)]).reshape(-1, 9)
    return e


def oracle_dense_h_by_pose_columns(oracle, dicts, mono, G):
    """The oracle's H, dense, from 6 m + 3 products H v: every pose column by a unit vector of its own (U and, H being symmetric, W from
    the feature rows), then all features at once per coordinate (no two features share a block of H: the rows of feature f hold V_f e_c).
    test_gpu_linearise.oracle_dense_h probes every feature column by itself -- 1800 products where one map holds 600 features.  A
    product with a random vector checks the whole of it, as there."""
    m, n = int(G["m"]), int(G["n"])
    R = 6 * m + 3 * n
    H = np.zeros((R, R))
    for c in range(6 * m):
        v = np.zeros(R)
        v[c] = 1.0
        H[:, c] = oracle.gn_hessian_times(dicts, mono, G, v)
    H[:6 * m, 6 * m:] = H[6 * m:, :6 * m].T
    for c in range(3):
        v = np.zeros(R)
        v[6 * m + c::3] = 1.0
        y = oracle.gn_hessian_times(dicts, mono, G, v)
        # (the pose columns hold W^T already: what is left in the feature rows is V)
        for f in range(n):
            H[6 * m + 3 * f:6 * m + 3 * f + 3, 6 * m + 3 * f + c] = y[6 * m + 3 * f:6 * m + 3 * f + 3]
    v = np.random.default_rng(1).standard_normal(R)
    y = oracle.gn_hessian_times(dicts, mono, G, v)
    assert np.max(np.abs(H @ v - y)) <= 1e-12 * np.max(np.abs(y))
    return H


def h_err(got, exp):
    """max |dH_ij| / sqrt(H_ii H_jj)"""
    d = np.sqrt(np.diag(exp))
    return float(np.max(np.abs(got - exp) / np.outer(d, d)))


@functools.lru_cache(maxsize=None)
def base(oracle, i):
    """Set i of test_gpu_linearise.SETS or CRAFTED (rf.crafted_set): dicts, mono, the oracle's tree result G, the state after two oracle
    polish steps G2 (the crafted set: G alone), the pairs of the plain pattern (W, U) and U united with the co-observation pairs (UX)."""
    if i == CRAFTED:
        d, G = rf.crafted_set(oracle)
        W, U, _, _ = label_structure(d, False, G)
        c = dict(mono=False, d=d, G=G, G2=None, W=W, U=U)
    else:
        c = dict(_case(oracle, i))
    c["UX"] = c["U"] | co_observation_pairs(c["d"], c["G"])
    c["fw"] = feature_weights(c["d"], 500 + (len(c["d"]) if i == CRAFTED else i))
    return c


@functools.lru_cache(maxsize=None)
def weighted_h(oracle, i, polished=False):
    """The oracle's dense H of set i re-weighted with base(i)["fw"], at G or (polished) G2.  Shared; changed by no test."""
    c = base(oracle, i)
    return dense_h(oracle, i, reweighted(c["d"], c["fw"]), c["G2"] if polished else c["G"])


def dense_h(oracle, i, dicts, G):
    """The oracle's dense H of `dicts` (set i with other information matrices: the pattern is base(i)'s W and UX) at G."""
    c = base(oracle, i)
    if i == CRAFTED:
        return oracle_dense_h_by_pose_columns(oracle, dicts, c["mono"], G)
    return oracle_dense_h(oracle, dicts, c["mono"], G, c["W"], c["UX"])
