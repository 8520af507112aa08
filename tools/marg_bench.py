"""Reduced hand-off of sub-tree roots on a named stand-in set: the set is cut into B blocks of consecutive maps, the B sub-trees run, every
root is exported full (lsfm_tree_export_dev) and reduced to the features that two or more roots hold (lsfm_tree_export_reduced_dev), and
the top tree runs over each kind of pack.
usage: python tools/marg_bench.py <config> --blocks B [--maps N] [--reps R]  -> one JSON object on stdout (profiles/marginalise_<config>.json)

Reported: HIP-event ms of the three parts of lsfm_map_marginalise on every downloaded root and of the five parts of the resident reduction;
GB/s of the partition pass over W against NW * 2 * 144 bytes, beside lsfm_wstream_bench modes 0 (lane per block) and 2 (stream copy) at
the same block count in the same process; features and W blocks before and after; t_total_ms of the top tree over full against reduced
packs (first run: analysing; then the median of R planned runs).

usage: python tools/marg_bench.py <config> --keep-poses every:K [--maps N] [--reps R]  -> profiles/marginalise_poses_<config>.json
The whole set is joined, then the result is cut to every K-th pose (and the gauge poses) by lsfm_map_marginalise_poses.  Reported: the
median HIP-event ms of its five parts and info[8]; GFLOP/s of k_pm_syrk against 2 * 36 * 6 |D| flops per output block over the last
part's time (which also holds k_pm_emit and the download of U': a lower bound); the wall time of the call beside the only route the
parent commit has to the information matrix of these poses at the same K: covariance_columns(joint=True) + numpy.linalg.inv (which
loses every kept feature)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.init()
from linearsfm_amd import api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("config")
ap.add_argument("--blocks", type=int, default=0)
ap.add_argument("--keep-poses", default="")
ap.add_argument("--maps", type=int, default=0)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
typ, maps = synth.make_config(a.config, a.maps or None)
mono = typ == "Monocular"
dicts = [dict(m.__dict__) for m in maps]
if a.keep_poses:
    import time

    if not a.keep_poses.startswith("every:") or int(a.keep_poses[6:]) < 1:
        sys.exit("--keep-poses every:K, K >= 1")
    K = int(a.keep_poses[6:])
    ctx = api.Context(0)
    G, stats, rc = ctx.divide_conquer(dicts, mono)
    if rc < 0:
        sys.exit(f"tree: rc {rc}")
    m = int(G["m"])
    ids = -np.asarray(G["stno"])[:6 * m:6]
    keep = np.zeros(m, bool)
    keep[::K] = True
    keep[np.isin(ids, [int(G["Ref"])] + ([int(G["ScaP"])] if mono else []))] = True
    ctx.marginalise_poses(G, mono, keep)  # (warm-up)
    runs, wall = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        red, t, info = ctx.marginalise_poses(G, mono, keep, times=True, info=True)
        wall.append((time.perf_counter() - t0) * 1e3)
        runs.append(t)
    med = {k: float(np.median([x[k] for x in runs])) for k in runs[0]}
    flops = 2.0 * 36 * 6 * info["dropped"] * info["blocks"]
    kept = np.nonzero(keep)[0]
    ctx.covariance_columns(G, mono, kept[:1], joint=True)  # (warm-up)
    parent = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        J = ctx.covariance_columns(G, mono, kept, joint=True)["joint"]
        free = np.diag(J) != 0  # (a Mono map's gauge scalars: rows and columns of zeros)
        np.linalg.inv(J[np.ix_(free, free)])
        parent.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"config": a.config, "type": typ, "maps": len(dicts), "poses": m, "features": int(G["n"]), "keep_poses": a.keep_poses, "poses_kept": int(red["m"]),
                      "features_kept": int(red["n"]), "nU": int(G["nU"]), "nU_reduced": int(red["nU"]), "info": info, "times_ms_median": med,
                      "wall_ms_median": float(np.median(wall)), "syrk_flops": flops,
                      "syrk_GFLOPs_lower_bound": flops / (med["syrk_emit_ms"] * 1e-3) / 1e9 if med["syrk_emit_ms"] > 0 else None,
                      "parent_route_wall_ms_median": float(np.median(parent)),
                      "note": "HIP events on the context's stream: stage A through the host | structure + uploads | factor of U1_DD | right-hand sides + forward "
                              "sweeps | k_pm_syrk + k_pm_emit + download of U'; the parent route is covariance_columns(joint=True) of the kept poses + "
                              "numpy.linalg.inv on the host, which gives the poses' information matrix alone"}, indent=1))
    ctx.close()
    sys.exit(0)
if a.blocks < 1:
    sys.exit("give --blocks B or --keep-poses every:K")
N, B = len(dicts), a.blocks
size = -(-N // B)
bounds = [(lo, min(N, lo + size)) for lo in range(0, N, size)]
held = [np.unique(np.concatenate([np.asarray(d["stno"])[6 * int(d["m"])::3] for d in dicts[lo:hi]])) for lo, hi in bounds]
ids, cnt = np.unique(np.concatenate(held), return_counts=True)
keep_ids = ids[cnt >= 2].astype(np.int32)

ctx = api.Context(0)
full_bufs, red_bufs, roots = [], [], []
for r, (lo, hi) in enumerate(bounds):
    part = [dict(d, pose_origin=np.full(int(d["m"]), lo + k, np.int32)) for k, d in enumerate(dicts[lo:hi])]
    t = ctx.tree_upload(part, mono)
    ctx.tree_set_final_reanchor(t, r % 2 == 1)
    stats, rc = ctx.tree_run(t)
    if rc < 0:
        sys.exit(f"sub-tree {r}: rc {rc}")
    nb = ctx.tree_export_size(t)
    fb = torch.empty(nb, dtype=torch.uint8, device="cuda:0")
    ctx.tree_export_dev(t, fb.data_ptr(), nb)
    nr = ctx.tree_export_reduced_size(t, keep_ids)
    rb = torch.empty(nr, dtype=torch.uint8, device="cuda:0")
    ctx.tree_export_reduced_dev(t, keep_ids, rb.data_ptr(), nr)  # (warm-up)
    res = [ctx.tree_export_reduced_dev(t, keep_ids, rb.data_ptr(), nr, times=True) for _ in range(a.reps)]
    root = ctx.tree_download(t)
    ctx.tree_free(t)
    fid = np.asarray(root["stno"])[6 * int(root["m"])::3]
    drop = ~np.isin(fid, keep_ids)
    ctx.marginalise(root, drop)  # (warm-up)
    host = [ctx.marginalise(root, drop, times=True) for _ in range(a.reps)]
    red, _ = host[-1]
    med = {k: float(np.median([x[k] for x in res])) for k in res[0]}
    hmed = {k: float(np.median([x[1][k] for x in host])) for k in host[0][1]}
    nw = int(root["nW"])
    roots.append({"root": r, "maps": hi - lo, "poses": int(root["m"]), "features": int(root["n"]), "features_kept": int(red["n"]), "nW": nw, "nW_kept": int(red["nW"]),
                  "nU": int(root["nU"]), "nU_reduced": int(red["nU"]), "pack_bytes": nb, "reduced_pack_bytes": nr, "subtree_t_total_ms": stats["t_total_ms"],
                  "resident_ms_median": med, "resident_total_ms": float(sum(med.values())),
                  "partition_GBps": (nw * 2 * 144 / (med["partition_ms"] * 1e-3) / 1e9) if med["partition_ms"] > 0 else None,
                  "partition_share_of_reduction": med["partition_ms"] / sum(med.values()), "host_entry_ms_median": hmed})
    full_bufs.append(fb)
    red_bufs.append(rb)
torch.cuda.synchronize()


def top(bufs):
    t = ctx.tree_upload_dev([b.data_ptr() for b in bufs], mono)
    first, rc = ctx.tree_run(t)
    warm = [ctx.tree_run(t)[0] for _ in range(a.reps)]
    out = ctx.tree_download(t)
    ctx.tree_free(t)
    keys = ("t_total_ms", "t_transform_ms", "t_join_ms", "t_schur_ms", "t_pcg_ms", "t_backsub_ms")
    return out, {"rc": rc, "first_run": {k: first[k] for k in keys}, "planned_median": {k: float(np.median([w[k] for w in warm])) for k in keys},
                 "poses": int(out["m"]), "features": int(out["n"]), "nW": int(out["nW"]), "nU": int(out["nU"])}


full, tf = top(full_bufs)
red, tr = top(red_bufs)
# the kept variables of the two results
m = int(full["m"])
assert int(red["m"]) == m and np.array_equal(np.asarray(red["stno"])[:6 * m], np.asarray(full["stno"])[:6 * m])
pos = {int(v): k for k, v in enumerate(np.asarray(full["stno"])[6 * m::3])}
fidx = np.array([pos[int(v)] for v in np.asarray(red["stno"])[6 * m::3]], np.int64)
idx = np.concatenate([np.arange(6 * m), (6 * m + 3 * fidx[:, None] + np.arange(3)).reshape(-1)])
fs, rs = np.asarray(full["stVal"])[idx], np.asarray(red["stVal"])
diff = float(np.max(np.abs(rs - fs) / np.maximum(1.0, np.abs(fs))))
nwmax = max(x["nW"] for x in roots)
ws = {f"mode{m}": ctx.wstream_bench(nwmax, m, 10) for m in (0, 2)}
print(json.dumps({"config": a.config, "type": typ, "maps": N, "blocks": len(bounds), "features_in_roots": int(sum(len(h) for h in held)),
                  "features_kept_ids": int(len(keep_ids)), "roots": roots, "top_tree_full_packs": tf, "top_tree_reduced_packs": tr,
                  "top_tree_speedup_planned": tf["planned_median"]["t_total_ms"] / tr["planned_median"]["t_total_ms"],
                  "kept_state_max_rel_diff_reduced_vs_full": diff,
                  "wstream": {"nblocks": nwmax, "ms": ws, "GBps": {k: nwmax * 2 * 144 / (v * 1e-3) / 1e9 for k, v in ws.items()}},
                  "note": "HIP events on the context's stream; resident parts: structure (flags, scans, pattern of U' with its read-backs), partition "
                          "pass over W, gather + V^-1, K9 values, emission; host entry parts: flags + partition + V^-1 + pattern, K9 values, emission "
                          "+ download; the full-pack route is the one the parent commit has"}, indent=1))
ctx.close()
