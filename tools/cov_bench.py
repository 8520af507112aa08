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
                       and the host formula -- the only route before the gate (existing API only: runs on older commits too)"""
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
for flag in ("--feature-columns", "--gate", "--gate-parent-route"):
    if flag in args:
        i = args.index(flag)
        modes[flag] = [int(v) for v in args[i + 1].split(",")]
        del args[i: i + 2]
cfg = args[0]
nmaps = int(args[1]) if len(args) > 1 and int(args[1]) > 0 else None
reps = int(args[2]) if len(args) > 2 else 3
typ, maps = synth.make_config(cfg, nmaps)
mono = typ == "Monocular"
d = [m.__dict__ for m in maps]
ctx = api.Context(0)
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
