"""lsfm_map_covariance on the final map of a named stand-in set: the HIP-event time of its parts (Schur reduction + symbolic analysis,
numeric factorisation, selected inversion + gather onto the pattern, feature part) beside t_pcg_ms of the same set's tree run.
usage: python tools/cov_bench.py <config> [maps] [reps]  -> one JSON object on stdout (profiles/cov_bench_<config>.json).

  --columns K[,K...]   instead: lsfm_map_covariance_columns_timed for K requested poses each (pose columns only, then with the feature
                       rows), warm, medians of `reps` calls (profiles/cov_columns_<config>.json); with --panel V the supernode-group
                       panel product is set first (lsfm_set_covcols_panel: 1 lane per column, 2 MFMA; default 0 = the library's choice)
  --parent-route       instead: the wall time of six Context.solve calls with unit right-hand sides -- one pose's six columns by the
                       only route the library had before lsfm_map_covariance_columns (existing API only: runs on older commits too)
  --feature-columns K[,K...]   instead: lsfm_map_covariance_feature_columns_timed for K requested features each (pose rows only, then
                       with the feature rows), warm, medians of `reps` calls
  --gate K[,K...]      instead: lsfm_map_feature_pair_gate_timed for K seeded pairs each: HIP-event ms of the sweeps and of the gate
                       kernel, and the call's wall time (profiles/feature_gate_<config>.json)
  --gate-parent-route K[,K...]   instead: Sigma_d of the same pairs through covariance_columns(joint=True) of the union of the pairs' poses
                       and the host formula -- the only route before the gate (existing API only: runs on older commits too)
  --merge K[,K...]     instead: lsfm_map_merge_features_timed on the tree of the set with K features split in two (the rule of
                       tests/merge_reference.split_set, seed 3) for the K split pairs: HIP-event ms of the five parts, the call's wall
                       time, nW -> nW' and the bytes the W' pass moves; and two cross-checks of D^2 and the state on the same map: the
                       residual form (x^ - T y)^T I (x^ - T y) in long double, and the columns route below (profiles/merge_<config>.json)
  --merge-parent-route K[,K...]   instead: the same merged state and D^2 by the only route before lsfm_map_merge_features --
                       covariance_feature_columns(the 2K features, poses, features, joint) and the host formula x^ - Sigma A^T C^-1 d,
                       D^2 = d^T C^-1 d (existing API only: runs on older commits too; profiles/merge_parent_<config>.json)
  --candidates R[,R...] [--tau t] [--split K]   instead: lsfm_map_feature_pair_candidates_timed at every radius R on the tree of the set with
                       K features split in two (default 32; --merge's rule), with --tau on lsfm_map_covariance's feature blocks: HIP-event ms
                       of the four parts, info, pair tests per second of the counting pass, how many of the K split pairs are among the
                       candidates, and the wall time of the sizing + filling calls beside the only route without the entry point --
                       scipy.spatial.cKDTree.query_pairs(R) on the host and the q filter in numpy; the two lists are compared
                       (profiles/candidates_<config>.json)
  --joint-gate K[,K...] [--split S] [--radius R]   instead: lsfm_map_feature_pair_joint_gate_timed on the tree of the set with S features split in
                       two (default 32) for a list of K pairs -- the --candidates list of that tree (radius R, default 0.5; tau = chi^2_3 at 0.99
                       on lsfm_map_covariance's blocks), the split pairs first, then by ascending q, cut or padded with seeded pairs
                       (default_rng(1)) to K: HIP-event ms of
                       the six parts, the call's wall time, the selection kernels' GFLOP/s on (3K)^3 / 3 (profiles/joint_gate_<config>.json)
  --joint-gate-parent-route K[,K...]   instead: the same selection by the only route before the entry point -- covariance_feature_columns(
                       joint=True) of the distinct endpoints (6 columns per pair where no endpoint repeats), C = A J A^T and the sequential
                       selection in numpy / LAPACK on the host, whose share is reported separately (existing API only: runs on a build of
                       an older commit too; profiles/joint_gate_parent_<config>.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from linearsfm_amd import api, synth  # noqa: E402

args = sys.argv[1:]
columns, parent_route = None, False
if "--columns" in args:
    i = args.index("--columns")
    columns = [int(v) for v in args[i + 1].split(",")]
    del args[i: i + 2]
panel = 0
if "--panel" in args:
    i = args.index("--panel")
    panel = int(args[i + 1])
    del args[i: i + 2]
if "--parent-route" in args:
    parent_route = True
    args.remove("--parent-route")
modes = {}
for flag in ("--feature-columns", "--gate", "--gate-parent-route", "--merge", "--merge-parent-route", "--joint-gate", "--joint-gate-parent-route"):
    if flag in args:
        i = args.index(flag)
        modes[flag] = [int(v) for v in args[i + 1].split(",")]
        del args[i: i + 2]
cand_radii, cand_tau, cand_split = None, None, 32
if "--candidates" in args:
    i = args.index("--candidates")
    cand_radii = [float(v) for v in args[i + 1].split(",")]
    del args[i: i + 2]
if "--tau" in args:
    i = args.index("--tau")
    cand_tau = float(args[i + 1])
    del args[i: i + 2]
if "--split" in args:
    i = args.index("--split")
    cand_split = int(args[i + 1])
    del args[i: i + 2]
jg_radius = 0.5
if "--radius" in args:
    i = args.index("--radius")
    jg_radius = float(args[i + 1])
    del args[i: i + 2]
cfg = args[0]
nmaps = int(args[1]) if len(args) > 1 and int(args[1]) > 0 else None
reps = int(args[2]) if len(args) > 2 else 3
typ, maps = synth.make_config(cfg, nmaps)
mono = typ == "Monocular"
d = [m.__dict__ for m in maps]
ctx = api.Context(0)

SPLIT_OFFSET = 100000


def split_tree(K, seed=3):
    """The tree's map of the set with K features split in two and the K split pairs: candidates are the features held by >= 2 local
    maps, sorted by id; default_rng(seed).choice picks K without replacement; from the middle holder on a chosen feature carries the
    label id + SPLIT_OFFSET (the rule of tests/merge_reference.split_set, stated here so that the tool runs on older commits)."""
    holders = {}
    for k, lm in enumerate(d):
        for i in np.asarray(lm["stno"])[6 * int(lm["m"])::3]:
            holders.setdefault(int(i), []).append(k)
    cands = sorted(i for i, hs in holders.items() if len(hs) >= 2)
    chosen = sorted(int(i) for i in np.random.default_rng(seed).choice(cands, size=K, replace=False))
    sd = [dict(lm, stno=np.array(lm["stno"], np.int32, copy=True)) for lm in d]
    for i in chosen:
        hs = holders[i]
        for k in hs[len(hs) // 2:]:
            st, mk = sd[k]["stno"], int(sd[k]["m"])
            st[6 * mk:][st[6 * mk:] == i] = i + SPLIT_OFFSET
    Gs, _, src = ctx.divide_conquer(sd, mono)
    if src != 0:
        sys.exit(f"the tree of the split set ended with status {src}")
    at = {int(l): f for f, l in enumerate(np.asarray(Gs["stno"])[6 * int(Gs["m"])::3])}
    return Gs, np.array([(at[i], at[i + SPLIT_OFFSET]) for i in chosen], np.int32)


def residual_form(Gs, Ty):
    """(x^ - T y)^T I (x^ - T y) in long double, block by block: a statement of D^2 that owes nothing to either route.  D^2 is the
    MINIMUM of this form over y, so an error of y enters in second order only, and the form's own cancellation (1e3 .. 1e6 of the
    terms on the Mono sets) is far inside the 64-bit mantissa."""
    ld = np.longdouble
    ms = int(Gs["m"])
    e = np.asarray(Gs["stVal"], np.float64).astype(ld) - np.asarray(Ty, np.float64).astype(ld)
    ep, ef = e[: 6 * ms].reshape(-1, 6), e[6 * ms:].reshape(-1, 3)
    U = np.asarray(Gs["U"], np.float64).reshape(-1, 6, 6).astype(ld)
    Ui, Uj = np.asarray(Gs["Ui"]), np.asarray(Gs["Uj"])
    qu = np.einsum("bi,bij,bj->b", ep[Ui], U, ep[Uj])
    tot = (qu * np.where(Ui == Uj, 1, 2)).sum()
    ph, fe = np.asarray(Gs["photo"]), np.asarray(Gs["feature"])
    for lo in range(0, len(ph), 1 << 20):  # (in slices: the long-double copy of W is 16 bytes a number)
        hi = min(lo + (1 << 20), len(ph))
        W = np.asarray(Gs["W"], np.float64).reshape(-1, 6, 3)[lo:hi].astype(ld)
        tot += 2 * np.einsum("bi,bij,bj->b", ep[ph[lo:hi]], W, ef[fe[lo:hi]]).sum()
    V = np.asarray(Gs["V"], np.float64).reshape(-1, 3, 3).astype(ld)
    tot += np.einsum("bi,bij,bj->b", ef, V, ef).sum()
    return float(tot)


def columns_route(Gs, pairs):
    """The merged state and D^2 without lsfm_map_merge_features: covariance_feature_columns(poses, features, joint) of the 2K features
    and the host formula y = x - Sigma A^T C^-1 d, D^2 = d^T C^-1 d.  Returns (y in x's numbering, D^2, C, the call's dict, the time
    the call returned)."""
    K = len(pairs)
    ms, ns = int(Gs["m"]), int(Gs["n"])
    x = np.asarray(Gs["stVal"], np.float64)
    feats = pairs.reshape(-1)  # f0 g0 f1 g1 ...: distinct, every split feature is in one pair
    fc = ctx.covariance_feature_columns(Gs, mono, feats, poses=True, features=True, joint=True)
    t1 = time.perf_counter()
    cols = np.concatenate([fc["pose"].reshape(2 * K, 6 * ms, 3), fc["feature"].reshape(2 * K, 3 * ns, 3)], axis=1)  # Sigma_{., feature}
    SA = np.concatenate([cols[2 * a + 1] - cols[2 * a] for a in range(K)], axis=1)                                   # Sigma A^T, A x = x_g - x_f
    Am = np.zeros((3 * K, 6 * K))
    for a in range(K):
        Am[3 * a: 3 * a + 3, 6 * a + 3: 6 * a + 6] = np.eye(3)
        Am[3 * a: 3 * a + 3, 6 * a: 6 * a + 3] = -np.eye(3)
    Cm = Am @ fc["joint"] @ Am.T
    xf = x[6 * ms:].reshape(-1, 3)
    dv = (xf[pairs[:, 1]] - xf[pairs[:, 0]]).reshape(-1)
    sol = np.linalg.solve(Cm, dv)
    return x - SA @ sol, float(dv @ sol), Cm, fc, t1


def host_candidates(x, R, fcov, tau):
    """The route without the entry point: a k-d tree on the host for the radius, then q = 1/2 d^T (Sigma_ff + Sigma_gg)^-1 d in numpy.  Returns
    (pairs sorted by (f, g), seconds of the tree + query, seconds of the filter + sort)."""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    pr = cKDTree(x).query_pairs(R, output_type="ndarray")
    t1 = time.perf_counter()
    if fcov is not None and len(pr):
        dv = x[pr[:, 0]] - x[pr[:, 1]]
        M = fcov[pr[:, 0]] + fcov[pr[:, 1]]
        with np.errstate(all="ignore"):
            qv = 0.5 * np.einsum("ki,ki->k", dv, np.linalg.solve(M, dv[:, :, None])[:, :, 0])
        pr = pr[~(qv > tau)]
    pr = pr[np.lexsort((pr[:, 1], pr[:, 0]))] if len(pr) else pr.reshape(0, 2)
    return pr.astype(np.int32), t1 - t0, time.perf_counter() - t1


if cand_radii is not None:
    Gs, split = split_tree(cand_split)
    ms, ns = int(Gs["m"]), int(Gs["n"])
    x = np.ascontiguousarray(np.asarray(Gs["stVal"], np.float64)[6 * ms:].reshape(-1, 3))
    fcov = np.ascontiguousarray(ctx.covariance(Gs, mono)["feature"]) if cand_tau is not None else None
    splitset = {tuple(sorted(map(int, p))) for p in split}
    legs = []
    for R in cand_radii:
        walls, parts = [], []
        try:
            for rep in range(reps + 1):  # (the first round is a warm-up)
                t0 = time.perf_counter()
                out = ctx.feature_pair_candidates(Gs, R, fcov, cand_tau)
                wall = 1e3 * (time.perf_counter() - t0)
                if rep:
                    walls.append(wall)
        except api.LsfmError as e:  # (a refusal -- too many cells, too many candidates, no room -- is a row too)
            legs.append({"leg": "candidates", "radius": R, "tau": cand_tau, "refused": str(e)})
            continue
        for rep in range(reps):  # the parts, from filling calls of their own
            crc, count, pr, _, _, t, info = ctx.feature_pair_candidates_raw(Gs, R, fcov, cand_tau, cap=len(out["pairs"]), times=True)
            if crc != 0:
                sys.exit(f"lsfm_map_feature_pair_candidates: {api.lib().lsfm_last_error(ctx._h).decode()}")
            parts.append(t.tolist())
        med = np.median(np.array(parts), axis=0)
        hw, hq, hf = [], [], []
        for rep in range(max(1, min(reps, 2))):
            t0 = time.perf_counter()
            hp, tq, tf = host_candidates(x, R, fcov, cand_tau)
            hw.append(1e3 * (time.perf_counter() - t0)); hq.append(1e3 * tq); hf.append(1e3 * tf)
        have = {tuple(p) for p in out["pairs"].tolist()} if len(out["pairs"]) <= 5_000_000 else None
        legs.append({"leg": "candidates", "radius": R, "tau": cand_tau, "split_pairs": len(splitset),
                     "split_pairs_among_candidates": len(splitset & have) if have is not None else None,
                     "info": {"cells": int(info[0]), "fullest_cell": int(info[1]), "pair_tests": int(info[2]), "candidates": int(info[3])},
                     "ms_median": {"upload_keys": med[0], "sort_cell_table": med[1], "count_scan": med[2], "fill_sort_download": med[3]},
                     "pair_tests_per_s_count_pass": float(info[2]) / (med[2] * 1e-3) if med[2] > 0 else None,
                     "call_wall_ms_median": float(np.median(walls)), "call_wall_ms": walls,
                     "host_route_wall_ms_median": float(np.median(hw)), "host_route_wall_ms": hw, "host_kdtree_ms_median": float(np.median(hq)),
                     "host_filter_sort_ms_median": float(np.median(hf)), "host_route_pairs": int(len(hp)),
                     "same_pairs_as_host_route": bool(np.array_equal(hp, out["pairs"]))})
    print(json.dumps({"config": cfg, "type": typ, "maps": len(maps), "poses": ms, "features": ns, "split": cand_split, "legs": legs,
                      "note": "HIP events on the context's stream; call wall: Context.feature_pair_candidates, the sizing and the filling call with the "
                              "upload of the estimates (and blocks) and the downloads, the covariance call not included on either route; host route: "
                              "scipy.spatial.cKDTree(x).query_pairs(R) and the q filter in numpy on the same arrays; split pairs by default_rng(3)"}, indent=1))
    ctx.close()
    sys.exit(0)
JG_TAU = 11.344866730144373  # chi^2_3 at 0.99


def joint_gate_list(Gs, split, K):
    """K pairs for the joint gate: the candidates of the split tree at --radius (default 0.5, the first radius of profiles/candidates_*.json)
    and tau -- the split pairs among them first, then the others by ascending bound q --, cut to K, or padded with seeded pairs that are
    not yet in the list."""
    ms, ns = int(Gs["m"]), int(Gs["n"])
    radius = jg_radius
    fcov = np.ascontiguousarray(ctx.covariance(Gs, mono)["feature"])
    out = ctx.feature_pair_candidates(Gs, radius, fcov, JG_TAU)
    cand = out["pairs"]
    true = {tuple(sorted(map(int, p))) for p in split}
    is_split = np.array([tuple(p) in true for p in cand.tolist()], bool) if len(cand) <= 5_000_000 else np.zeros(len(cand), bool)
    rank = np.lexsort((np.nan_to_num(out["q"], nan=np.inf), ~is_split))
    pairs = [tuple(p) for p in cand[rank[:K]].tolist()]
    have = {tuple(sorted(p)) for p in pairs}
    rng = np.random.default_rng(1)
    while len(pairs) < K:
        f, g = (int(v) for v in rng.choice(ns, size=2, replace=False))
        if tuple(sorted((f, g))) not in have:
            have.add(tuple(sorted((f, g))))
            pairs.append((f, g))
    return np.array(pairs, np.int32), len(cand), radius


def host_select(Cm, dv, ends, tau):
    """The sequential selection of lsfm_map_feature_pair_joint_gate on the host, float64: ascending individual d2, a growing Cholesky factor of
    the accepted block, union-find for the implied pairs.  Returns (status, delta, D2)."""
    import scipy.linalg as sla
    K = len(ends)
    blk = lambda a, b: Cm[3 * a: 3 * a + 3, 3 * b: 3 * b + 3]
    d2 = np.full(K, np.nan)
    for b in range(K):
        try:
            y = sla.solve_triangular(np.linalg.cholesky(blk(b, b)), dv[3 * b: 3 * b + 3], lower=True)
            d2[b] = y @ y
        except np.linalg.LinAlgError:
            pass
    order = sorted(range(K), key=lambda b: (bool(np.isnan(d2[b])), 0.0 if np.isnan(d2[b]) else d2[b], b))
    parent = {}

    def find(v):
        parent.setdefault(v, v)
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    status, delta = np.zeros(K, np.int32), np.full(K, np.nan)
    L, yv, rows, n = np.zeros((3 * K, 3 * K)), np.zeros(3 * K), np.zeros(3 * K, np.int64), 0
    for b in order:
        if np.isnan(d2[b]):
            continue
        f, g = find(int(ends[b, 0])), find(int(ends[b, 1]))
        if f == g:
            status[b], delta[b] = 2, 0.0
            continue
        cb = np.arange(3 * b, 3 * b + 3)
        Wt = sla.solve_triangular(L[:n, :n], Cm[np.ix_(rows[:n], cb)], lower=True, check_finite=False) if n else np.zeros((0, 3))
        S = blk(b, b) - Wt.T @ Wt
        e = dv[cb] - Wt.T @ yv[:n]
        try:
            L3 = np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            continue
        y3 = sla.solve_triangular(L3, e, lower=True)
        delta[b] = y3 @ y3
        if delta[b] <= tau:
            status[b] = 1
            parent[max(f, g)] = min(f, g)
            L[n: n + 3, :n], L[n: n + 3, n: n + 3], yv[n: n + 3], rows[n: n + 3] = Wt.T, L3, y3, cb
            n += 3
    return status, delta, float(np.sum(delta[status == 1]))


if "--joint-gate" in modes or "--joint-gate-parent-route" in modes:
    parent_leg = "--joint-gate-parent-route" in modes
    Gs, split = split_tree(cand_split)
    ms, ns = int(Gs["m"]), int(Gs["n"])
    splitset = {tuple(sorted(map(int, p))) for p in split}
    legs = []
    for K in modes["--joint-gate-parent-route" if parent_leg else "--joint-gate"]:
        pairs, ncand, radius = joint_gate_list(Gs, split, K)
        row = {"K": K, "candidates": ncand, "radius": radius, "distinct_endpoints": int(len(np.unique(pairs)))}
        walls, parts, hosts = [], [], []
        for rep in range(reps + 1):  # (the first call is a warm-up)
            t0 = time.perf_counter()
            if parent_leg:
                feats = np.unique(pairs)
                fc = ctx.covariance_feature_columns(Gs, mono, feats, poses=False, features=False, joint=True)
                t1 = time.perf_counter()
                at = np.searchsorted(feats, pairs)
                idx = lambda col: (3 * at[:, col][:, None] + np.arange(3)[None, :]).ravel()
                R = fc["joint"][idx(0), :] - fc["joint"][idx(1), :]
                Cm = R[:, idx(0)] - R[:, idx(1)]
                xf = np.asarray(Gs["stVal"], np.float64)[6 * ms:].reshape(-1, 3)
                status, delta, D2 = host_select(Cm, (xf[pairs[:, 0]] - xf[pairs[:, 1]]).ravel(), pairs, JG_TAU)
                t2 = time.perf_counter()
                steps = fc["steps"]
                if rep:
                    hosts.append(1e3 * (t2 - t1))
            else:
                jrc, out, t = ctx.feature_pair_joint_gate_raw(Gs, mono, pairs, times=True)
                if jrc < 0 or (jrc > 0 and out["steps"] == 0):
                    sys.exit(f"lsfm_map_feature_pair_joint_gate: status {jrc}: {api.lib().lsfm_last_error(ctx._h).decode()}")
                status, delta, D2, steps = out["status"], out["delta"], out["D2"], out["steps"]
                if rep:
                    parts.append(t.tolist())
            if rep:
                walls.append(1e3 * (time.perf_counter() - t0))
            if parent_leg and K >= 1024 and rep:
                break  # (one warm call at this size: the host loop takes seconds)
        acc = {tuple(sorted(map(int, pairs[b]))) for b in np.nonzero(status == 1)[0]}
        row.update({"accepted": int(np.sum(status == 1)), "implied": int(np.sum(status == 2)), "split_pairs_among_accepted": len(splitset & acc),
                    "split_pairs_in_list": len(splitset & {tuple(sorted(map(int, p))) for p in pairs}), "D2": D2, "steps": int(steps),
                    "call_wall_ms_median": float(np.median(walls)), "call_wall_ms": walls, "calls_measured": len(walls), "warm_up_calls": 1})
        if parent_leg:
            row.update({"leg": "joint_gate_parent_route", "columns_solved": 3 * int(len(np.unique(pairs))), "host_ms_median": float(np.median(hosts)),
                        "columns_call_ms_median": float(np.median(walls) - np.median(hosts))})
        else:
            med = np.median(np.array(parts), axis=0)
            row.update({"leg": "joint_gate", "columns_solved": 3 * K,
                        "ms_median": {"reduce_analyse": med[0], "factor": med[1], "sweeps_refine": med[2], "C_blocks": med[3], "selection_kernels": med[4], "downloads_host_prep_alloc": med[5]},
                        "selection_gflops": (3.0 * K) ** 3 / 3.0 / (med[4] * 1e-3) / 1e9 if med[4] > 0 else None})
        legs.append(row)
    print(json.dumps({"config": cfg, "type": typ, "maps": len(maps), "poses": ms, "features": ns, "split": cand_split, "tau": JG_TAU, "legs": legs,
                      "note": "HIP events on the context's stream; call wall: the upload of the map and every download included, the candidate search and "
                              "its covariance call not included on either route; selection_kernels: events around k_jc_permute .. the last panel alone; "
                              "downloads_host_prep_alloc: d2 / status / delta down, the order and endpoint numbering on the host, the selection's "
                              "hipMallocs and uploads; parent route: host = C = A J A^T and the numpy / LAPACK selection loop"}, indent=1))
    ctx.close()
    sys.exit(0)
if "--merge" in modes:
    legs = []
    for K in modes["--merge"]:
        Gs, pairs = split_tree(K)
        walls, parts = [], []
        for rep in range(reps + 1):  # (the first call is a warm-up)
            t0 = time.perf_counter()
            mrc, g, d2, dof, rp, steps, corr, t = ctx.merge_features_raw(Gs, mono, pairs, times=True)
            wall = 1e3 * (time.perf_counter() - t0)
            if mrc < 0 or g is None:
                sys.exit(f"lsfm_map_merge_features: status {mrc}: {api.lib().lsfm_last_error(ctx._h).decode()}")
            if rep:
                walls.append(wall)
                parts.append(t.tolist())
        med = np.median(np.array(parts), axis=0)
        nW, nWo = len(Gs["photo"]), int(g["nW"])
        ms_ = int(Gs["m"])
        yv = np.asarray(g["stVal"], np.float64)
        d2_res = residual_form(Gs, np.concatenate([yv[: 6 * ms_], yv[6 * ms_:].reshape(-1, 3)[rp].reshape(-1)]))
        yc, d2_cols, _, _, _ = columns_route(Gs, pairs)  # the other route on the SAME map (a tree is not bit-reproducible from process to process)
        sig = np.sqrt(np.concatenate([np.einsum("kii->ki", v).reshape(-1) for v in (lambda c: (c["pose"], c["feature"]))(ctx.covariance(Gs, mono))]))
        kept = np.concatenate([np.arange(6 * ms_), (6 * ms_ + 3 * np.unique(rp, return_index=True)[1][:, None] + np.arange(3)).reshape(-1)])
        on = sig[kept] > 0
        dy = float(np.max(np.abs(yv - yc[kept])[on] / (sig[kept][on] * max(1.0, np.sqrt(d2_cols)))))
        ws = {f"mode{md}_ms": ctx.wstream_bench(nW, md, 20) for md in (0, 2)} if hasattr(ctx, "wstream_bench") else {}
        legs.append({"leg": "merge", "K": K, "status": mrc, "steps": steps, "last_corr": corr, "d2": d2, "d2_residual_form_long_double": d2_res, "d2_rel_diff": abs(d2 - d2_res) / d2_res,
                     "d2_columns_route_same_map": d2_cols, "d2_rel_diff_columns_route": abs(d2 - d2_cols) / d2_cols, "state_diff_columns_route": dy, "dof": dof, "poses": int(Gs["m"]), "features": int(Gs["n"]),
                     "nW": nW, "nW_merged": nWo, "w_pass_bytes": (nW + nWo) * 144,
                     "ms_median": {"upload_merge_passes": med[0], "reduce_analyse_factor": med[1], "rhs_sweeps_refinement": med[2], "backsub_d2": med[3], "download": med[4]},
                     "call_wall_ms_median": float(np.median(walls)), "call_wall_ms": walls, "wstream_same_blocks": ws})
    print(json.dumps({"config": cfg, "type": typ, "maps": len(maps), "legs": legs,
                      "note": "HIP events on the context's stream; upload_merge_passes covers the upload of W / V, the W' and V' passes and the merged map's "
                              "download (the W' pass alone is not bracketed: its bytes are given, beside lsfm_wstream_bench on as many blocks); "
                              "reduce_analyse_factor includes cov_front's upload of the merged map; split pairs by default_rng(3); d2_rel_diff: against the long-double "
                              "residual form at the call's own state; *_columns_route: against covariance_feature_columns + the host formula on the same map, "
                              "the state in units of sigma_i max(1, sqrt(D2))"}, indent=1))
    ctx.close()
    sys.exit(0)
if "--merge-parent-route" in modes:
    legs = []
    for K in modes["--merge-parent-route"]:
        Gs, pairs = split_tree(K)
        ms = int(Gs["m"])
        walls, hosts = [], []
        for rep in range(reps + 1):  # (the first round is a warm-up)
            t0 = time.perf_counter()
            y, d2, Cm, fc, t1 = columns_route(Gs, pairs)
            t2 = time.perf_counter()
            if rep:
                walls.append(1e3 * (t2 - t0))
                hosts.append(1e3 * (t2 - t1))
        Ty = y.copy()  # the route's state with both halves of a pair at the first one's value: T y
        Ty[6 * ms:].reshape(-1, 3)[pairs[:, 1]] = Ty[6 * ms:].reshape(-1, 3)[pairs[:, 0]]
        d2_res = residual_form(Gs, Ty)
        legs.append({"leg": "merge-parent-route", "K": K, "columns": 6 * K, "d2": d2, "d2_residual_form_long_double": d2_res, "d2_rel_diff": abs(d2 - d2_res) / d2_res,
                     "cond_C": float(np.linalg.cond(Cm)), "steps": fc["steps"], "wall_ms": walls,
                     "wall_ms_median": float(np.median(walls)), "host_formula_ms_median": float(np.median(hosts))})
    print(json.dumps({"config": cfg, "type": typ, "maps": len(maps), "legs": legs,
                      "note": "wall time of the merged state and D^2 of the same split pairs through covariance_feature_columns(poses, features, joint) of "
                              "the 2K features and the host formula y = x - Sigma A^T C^-1 d, D^2 = d^T C^-1 d; host_formula_ms: the part outside that call"}, indent=1))
    ctx.close()
    sys.exit(0)
G, stats, rc = ctx.divide_conquer(d, mono)
m_, n_ = int(G["m"]), int(G["n"])


def seeded_pairs(K):
    rng = np.random.default_rng(1)
    return np.stack([rng.choice(n_, size=2, replace=False) for _ in range(K)]).astype(np.int32)


def timed(call, name):
    """medians over `reps` warm calls of (rc, ..., steps, last_corr, times[4]) -> wall ms, parts, steps, last_corr"""
    walls, parts = [], []
    for rep in range(reps + 1):  # (the first call is a warm-up)
        t0 = time.perf_counter()
        out = call()
        wall = 1e3 * (time.perf_counter() - t0)
        if out[0] < 0:
            sys.exit(f"{name}: {api.lib().lsfm_last_error(ctx._h).decode()}")
        if rep:
            walls.append(wall)
            parts.append(out[-1].tolist())
    return walls, np.median(np.array(parts), axis=0), out


if "--feature-columns" in modes or "--gate" in modes:
    legs = []
    for K in modes.get("--feature-columns", []):
        q = np.random.default_rng(1).choice(n_, size=min(K, n_), replace=False)
        for feats in (False, True):
            walls, med, out = timed(lambda: ctx.covariance_feature_columns_raw(G, mono, q, features=feats, times=True), "lsfm_map_covariance_feature_columns")
            legs.append({"leg": "feature-columns", "K": int(len(q)), "features": feats, "status": out[0], "steps": out[4], "last_corr_max": float(out[5].max()),
                         "ms_median": {"reduce_analyse": med[0], "factor": med[1], "sweeps_products": med[2], "features": med[3]},
                         "call_wall_ms_median": float(np.median(walls)), "call_wall_ms": walls})
    for K in modes.get("--gate", []):
        pairs = seeded_pairs(K)
        walls, med, out = timed(lambda: ctx.feature_pair_gate_raw(G, mono, pairs, times=True), "lsfm_map_feature_pair_gate")
        legs.append({"leg": "gate", "K": K, "status": out[0], "steps": out[3], "last_corr_max": float(out[4].max()),
                     "ms_median": {"reduce_analyse": med[0], "factor": med[1], "sweeps_products": med[2], "gate_kernel": med[3]},
                     "call_wall_ms_median": float(np.median(walls)), "call_wall_ms": walls})
    print(json.dumps({"config": cfg, "type": typ, "maps": len(maps), "poses": m_, "features": n_, "tree_t_total_ms": stats["t_total_ms"], "legs": legs,
                      "note": "HIP events on the context's stream; sweeps_products covers the right-hand sides, the unrefined solve and every "
                              "refinement step; call wall includes the upload of the map and the download of the results; pairs from default_rng(1)"}, indent=1))
    ctx.close()
    sys.exit(0)
if "--gate-parent-route" in modes:
    ph, fe = np.asarray(G["photo"]), np.asarray(G["feature"])
    W = np.asarray(G["W"], np.float64).reshape(-1, 6, 3)
    V = np.asarray(G["V"], np.float64).reshape(-1, 3, 3)
    fptr = np.searchsorted(fe, np.arange(n_ + 1))  # (W is sorted by feature: a feature's run, no scan per feature)
    legs = []
    for K in modes["--gate-parent-route"]:
        pairs = seeded_pairs(K)
        walls, hosts = [], []
        for rep in range(reps + 1):  # (the first round is a warm-up)
            t0 = time.perf_counter()
            runs = {int(h): np.arange(fptr[h], fptr[h + 1]) for h in np.unique(pairs)}
            P = np.unique(np.concatenate([ph[b] for b in runs.values()]))
            t1 = time.perf_counter()
            J = ctx.covariance_columns(G, mono, P, joint=True)["joint"]
            t2 = time.perf_counter()
            at = np.full(m_, -1)
            at[P] = np.arange(len(P))
            GT = {h: np.einsum("ij,wkj->wik", np.linalg.inv(V[h]), W[b]) for h, b in runs.items()}  # V_h^-1 W_w^T of every block, [run, 3, 6]
            cov = np.zeros((K, 3, 3))
            for a, (f, g) in enumerate(pairs):
                L = np.zeros((3, len(P), 6))  # V_f^-1 W_f^T - V_g^-1 W_g^T on the union's columns
                for h, s in ((int(f), 1.0), (int(g), -1.0)):
                    np.add.at(L, (slice(None), at[ph[runs[h]]]), s * np.transpose(GT[h], (1, 0, 2)))
                L = L.reshape(3, -1)
                cov[a] = np.linalg.inv(V[f]) + np.linalg.inv(V[g]) + L @ J @ L.T
            t3 = time.perf_counter()
            if rep:
                walls.append(1e3 * (t3 - t0))
                hosts.append(1e3 * ((t1 - t0) + (t3 - t2)))
        legs.append({"leg": "gate-parent-route", "K": K, "union_poses": int(len(P)), "columns": int(6 * len(P)), "wall_ms": walls,
                     "wall_ms_median": float(np.median(walls)), "host_formula_ms_median": float(np.median(hosts))})
    print(json.dumps({"config": cfg, "type": typ, "maps": len(maps), "poses": m_, "features": n_, "legs": legs,
                      "note": "wall time of Sigma_d for the same seeded pairs through covariance_columns(joint=True) of the union of the pairs' poses "
                              "and the host formula V_f^-1 + V_g^-1 + L Sigma_PP L^T; host_formula_ms: the part outside the covariance_columns call"}, indent=1))
    ctx.close()
    sys.exit(0)
if parent_route:
    # one pose's six columns as six whole solves: six uploads, Schur reductions and factorisations
    j = m_ // 2
    sa = None
    if mono:
        ids = -np.asarray(G["stno"])[: 6 * m_: 6]
        pr, ps = int(np.nonzero(ids == G["Ref"])[0][0]), int(np.nonzero(ids == G["ScaP"])[0][0])
        sa = [pr, 6 * pr, 6 * ps + int(G["Fix"]), 0, 0]
        j = j if j != pr else (j + 1) % m_
    walls = []
    for rep in range(reps + 1):  # (the first round is a warm-up)
        t0 = time.perf_counter()
        for c in range(6):
            eP = np.zeros(6 * m_)
            eP[6 * j + c] = 1.0
            ctx.solve(G, eP, np.zeros(3 * n_), mono, sa)
        if rep:
            walls.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps({"config": cfg, "type": typ, "maps": len(maps), "poses": m_, "features": n_, "leg": "parent-route", "pose": j,
                      "six_solves_wall_ms": walls, "six_solves_wall_ms_median": float(np.median(walls)),
                      "sixteen_poses_scaled_ms": 16 * float(np.median(walls)),
                      "note": "wall time of six Context.solve calls (unit right-hand sides of one pose, eF = 0), each with its own upload, Schur "
                              "reduction and factorisation; 16 poses = 96 such calls"}, indent=1))
    ctx.close()
    sys.exit(0)
if columns:
    ctx.set_covcols_panel(panel)
    rng = np.random.default_rng(1)
    legs = []
    for K in columns:
        q = rng.choice(m_, size=min(K, m_), replace=False)
        for feats in (False, True):
            walls, parts, steps = [], [], 0
            for rep in range(reps + 1):  # (the first call is a warm-up)
                t0 = time.perf_counter()
                crc, pose, feat, _, steps, corr, t = ctx.covariance_columns_raw(G, mono, q, features=feats, times=True)
                wall = 1e3 * (time.perf_counter() - t0)
                if crc < 0:
                    sys.exit(f"lsfm_map_covariance_columns: {api.lib().lsfm_last_error(ctx._h).decode()}")
                if rep:
                    walls.append(wall)
                    parts.append(t.tolist())
            med = np.median(np.array(parts), axis=0)
            sweeps = 2 * (1 + steps)  # forward + backward of the unrefined solve and of every refinement step
            legs.append({"K": int(len(q)), "features": feats, "status": crc, "steps": steps, "last_corr_max": float(corr.max()),
                         "ms_median": {"reduce_analyse": med[0], "factor": med[1], "sweeps_products": med[2], "features": med[3]},
                         "sweeps_products_ms_per_column": med[2] / (6 * len(q)), "ms_per_sweep_per_chunk": med[2] / sweeps / -(-len(q) // 32),
                         "call_wall_ms_median": float(np.median(walls)), "call_wall_ms": walls,
                         "feature_out_GBps": (18 * len(q) * n_ * 8 / (med[3] * 1e-3) / 1e9) if feats and med[3] > 0 else None})
    print(json.dumps({"config": cfg, "type": typ, "maps": len(maps), "poses": m_, "features": n_, "leg": "columns", "panel": panel, "tree_t_total_ms": stats["t_total_ms"],
                      "legs": legs,
                      "note": "HIP events on the context's stream; sweeps_products covers the unrefined solve, every refinement step (product with S, "
                              "both sweeps, update and its norms read back) and the gather into the caller's layout; call wall includes the upload "
                              "of the map and the download of the columns"}, indent=1))
    ctx.close()
    sys.exit(0)
calls, parts = [], []
first = None
status = 0
for rep in range(reps + 1):  # (the first call is a warm-up)
    t0 = time.perf_counter()
    crc, pose, feat, _, nnzb, t = ctx.covariance_raw(G, mono, times=True)
    wall = 1e3 * (time.perf_counter() - t0)
    if crc != 0:
        # a numerical status (LSFM_ERR_NOT_SPD, floored pivots): recorded with the times of the parts that ran
        status = crc
        err = api.lib().lsfm_last_error(ctx._h).decode() if crc < 0 else f"{crc} pivot(s) floored"
    elif first is None:
        first = (pose, feat)
    elif not (np.array_equal(first[0], pose) and np.array_equal(first[1], feat)):
        sys.exit("two calls gave different bits")
    if rep:
        calls.append(wall)
        parts.append(t.tolist())
med = np.median(np.array(parts), axis=0)
print(json.dumps({"config": cfg, "type": typ, "maps": len(maps), "poses": int(G["m"]), "features": int(G["n"]), "pattern_blocks": nnzb,
                  "tree_rc": rc, "cov_status": status, "cov_error": err if status else None, "tree_t_total_ms": stats["t_total_ms"], "tree_t_pcg_ms": stats["t_pcg_ms"],
                  "cov_ms_median": {"reduce_analyse": med[0], "factor": med[1], "selinv_gather": med[2], "features": med[3]},
                  "selinv_over_factor": med[2] / med[1] if med[1] > 0 else None,
                  "cov_parts_ms_each_call": parts, "cov_call_wall_ms": calls, "same_bits_every_call": status == 0,
                  "note": "HIP events on the context's stream; reduce_analyse includes the host's symbolic analysis and the read-backs it waits "
                          "for; call wall includes the upload of the map and the download of the results"}, indent=1))
ctx.close()
