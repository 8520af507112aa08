"""lsfm_map_covariance on the final map of a named stand-in set: the HIP-event time of its parts (Schur reduction + symbolic analysis,
numeric factorisation, selected inversion + gather onto the pattern, feature part) beside t_pcg_ms of the same set's tree run.
usage: python tools/cov_bench.py <config> [maps] [reps]  -> one JSON object on stdout (profiles/cov_bench_<config>.json)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from linearsfm_amd import api, synth  # noqa: E402

cfg = sys.argv[1]
nmaps = int(sys.argv[2]) if len(sys.argv) > 2 and int(sys.argv[2]) > 0 else None
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
typ, maps = synth.make_config(cfg, nmaps)
mono = typ == "Monocular"
d = [m.__dict__ for m in maps]
ctx = api.Context(0)
G, stats, rc = ctx.divide_conquer(d, mono)
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
