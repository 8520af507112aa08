"""lsfm_gn_polish on a named stand-in set, from the device's own tree result: the objective / gradient trace and the wall clock of the
call's parts (LSFM_GN_TIMING=1: structure + upload, per assembly (with the chi2 + weights kernels' HIP-event time when robust), per
solve).  usage: python tools/gn_bench.py <config> [steps] [maps] [--robust huber|cauchy --c <c>] [--robust-features huber|cauchy --c <c>] [--linearise]
-> one JSON object per call on stdout (profiles/r06_gn_polish_<config>.json).  --robust: lsfm_gn_polish_robust instead, and the same
steps of the plain polish beside it (wall clock per step of each, the chi2 kernel's share of an assembly).  --linearise: after the
polish, lsfm_gn_linearise at the polished state (profiles/gn_linearise_<config>.json), one warm-up and the medians of 3 calls: HIP-event ms
of the assembly and of the two coalescing launches, the block counts of the working form and of the map, the GB/s of k_gn_coalesce<18>
against (NWJ + nW') * 144 bytes, the call's wall ms with the library's own split (structure + upload, device, download), and the wall ms
of lsfm_map_covariance on the result beside the same call on the tree's own map.  --robust-features huber|cauchy --c <c>:
lsfm_gn_polish_robust_features beside the plain and the map-robust polish (same kind and c), two calls of each and the warm one read
(profiles/gn_robust_features_<config>.json): per assembly the HIP-event ms of the feature chi2 pass (k_gn_chi2<true> + the objective
kernel) with its GB/s on the bytes it must read (every U, W and V block and feature estimate of the local maps once), beside
k_gn_chi2<false> (+ weights kernel) on the same arrays, the HIP-event ms of the U correction kernel, and the wall ms per assembly and step.
--linearise --robust-features huber|cauchy --c <c>: after `steps` of lsfm_gn_polish_robust_features, at its state, in one session and as
medians of 3 calls after a warm-up each: plain lsfm_gn_linearise beside lsfm_gn_linearise_features with the polish's weights -- HIP-event
ms per part (the chi2 pass + slot fill, the rest of the assembly, the two coalescing launches), NUJ -> nU' and NWJ -> nW' of each, and the
library's wall split of each call (written to profiles/gn_linearise_features_<config>.json as well as printed)."""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if len(sys.argv) > 1 and sys.argv[1] != "--child":
    # the library's timing line goes to stderr of the process: run the work in a child and pick it up
    env = dict(os.environ, LSFM_GN_TIMING="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], env=env, capture_output=True, text=True)
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    tim = [l for l in p.stderr.splitlines() if l.startswith("lsfm_gn:")]
    if not line:
        sys.exit(p.stdout + p.stderr)
    d = json.loads(line[0])
    d["library_timing"] = tim
    lin = [l for l in p.stderr.splitlines() if l.startswith("lsfm_gn_linearise:")]
    if lin and "linearise" in d:
        # the library's own split of the calls after the warm-up: medians
        pat = r"structure \+ upload ([0-9.]+) ms, assembly \+ coalescing ([0-9.]+) ms, download ([0-9.]+) ms, call ([0-9.]+) ms"
        rows = sorted(tuple(float(v) for v in re.search(pat, l).groups()) for l in lin[1:])
        up, dev, down, call = (sorted(r[i] for r in rows)[len(rows) // 2] for i in range(4))
        d["linearise"]["library_wall_ms"] = {"structure_upload": up, "device": dev, "download": down, "call": call,
                                             "upload_download_share": (up + down) / call}
    if "linearise_features" in d:
        pat = r"structure \+ upload ([0-9.]+) ms, assembly \+ coalescing ([0-9.]+) ms, download ([0-9.]+) ms, call ([0-9.]+) ms"
        for key, head in (("plain", "lsfm_gn_linearise:"), ("feature_weighted", "lsfm_gn_linearise_features:")):
            rows = [tuple(float(v) for v in re.search(pat, l).groups()) for l in p.stderr.splitlines() if l.startswith(head)][1:]
            up, dev, down, call = (sorted(r[i] for r in rows)[len(rows) // 2] for i in range(4))
            d["linearise_features"][key]["library_wall_ms"] = {"structure_upload": up, "device": dev, "download": down, "call": call}
        out = os.path.join(ROOT, "profiles", "gn_linearise_features_%s.json" % d["config"])
        with open(out, "w") as f:
            json.dump(d, f, indent=1)
            f.write("\n")
        print(json.dumps(d, indent=1))
        sys.exit(0)
    if "robust_features" in d and len(tim) >= 6:
        def parse(t):
            g = lambda pat: float(re.search(pat, t).group(1))
            o = {"assembly_ms": g(r"assemblies ([0-9.]+) ms each"), "solve_ms": g(r"solves ([0-9.]+) ms each"), "n_asm": int(re.search(r"(\d+) assemblies", t).group(1)),
                 "n_solve": int(re.search(r"(\d+) solves", t).group(1)), "call_ms": g(r"call ([0-9.]+) ms"), "structure_upload_ms": g(r"structure \+ upload ([0-9.]+) ms"),
                 "chi2_weights_ms": g(r"chi2 \+ weights ([0-9.]+) ms each")}
            m = re.search(r"U correction ([0-9.]+) ms each: (\d+) slots, (\d+) contributors", t)
            if m:
                o.update(u_correction_ms=float(m.group(1)), slots=int(m.group(2)), contributors=int(m.group(3)))
            o["step_ms"] = (o["n_asm"] * o["assembly_ms"] + o["n_solve"] * o["solve_ms"]) / max(o["n_solve"], 1)
            return o
        p_, r_, f_ = parse(tim[1]), parse(tim[3]), parse(tim[5])
        d["plain_warm"], d["map_robust_warm"], d["feature_robust_warm"] = p_, r_, f_
        B = d["chi2_pass_bytes"]
        d["feature_chi2_GBps"] = B / (f_["chi2_weights_ms"] * 1e6) if f_["chi2_weights_ms"] > 0 else None
        d["map_chi2_GBps"] = B / (r_["chi2_weights_ms"] * 1e6) if r_["chi2_weights_ms"] > 0 else None
        d["feature_chi2_over_map_chi2"] = f_["chi2_weights_ms"] / r_["chi2_weights_ms"] if r_["chi2_weights_ms"] > 0 else None
        d["u_correction_share_of_assembly"] = f_["u_correction_ms"] / f_["assembly_ms"]
        d["feature_robust_over_plain_step"] = f_["step_ms"] / p_["step_ms"]
    if "robust" in d and len(tim) >= 4:
        # per step = one solve + the assemblies of the line search; from the warm call of each kind
        def parse(t):
            g = lambda pat: float(re.search(pat, t).group(1))
            return {"assembly_ms": g(r"assemblies ([0-9.]+) ms each"), "chi2_weights_ms": g(r"chi2 \+ weights ([0-9.]+) ms each"),
                    "solve_ms": g(r"solves ([0-9.]+) ms each"), "n_asm": int(re.search(r"(\d+) assemblies", t).group(1)),
                    "n_solve": int(re.search(r"(\d+) solves", t).group(1)), "call_ms": g(r"call ([0-9.]+) ms")}
        p_, r_ = parse(tim[1]), parse(tim[3])
        for k, v in (("plain_warm", p_), ("robust_warm", r_)):
            v["step_ms"] = (v["n_asm"] * v["assembly_ms"] + v["n_solve"] * v["solve_ms"]) / max(v["n_solve"], 1)
            d[k] = v
        d["chi2_share_of_robust_assembly"] = r_["chi2_weights_ms"] / r_["assembly_ms"]
        d["robust_over_plain_step"] = r_["step_ms"] / p_["step_ms"]
    print(json.dumps(d, indent=1))
    sys.exit(0)

import argparse  # noqa: E402

import numpy as np  # noqa: E402
from linearsfm_amd import api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("config")
ap.add_argument("steps", nargs="?", type=int, default=3)
ap.add_argument("maps", nargs="?", type=int, default=0)
ap.add_argument("--robust", choices=["huber", "cauchy"])
ap.add_argument("--c", type=float, default=1.0)
ap.add_argument("--robust-features", choices=["huber", "cauchy"])
ap.add_argument("--linearise", action="store_true")
a = ap.parse_args(sys.argv[2:])
cfg, steps, nmaps = a.config, a.steps, a.maps
typ, maps = synth.make_config(cfg, nmaps or None)
mono = typ == "Monocular"
d = [m.__dict__ for m in maps]
ctx = api.Context(0)
G, stats, rc = ctx.divide_conquer(d, mono)
calls = []
for rep in range(2):
    t0 = time.perf_counter()
    st, obj, gn, hv, rc2 = ctx.gn_polish(d, mono, G, steps)
    calls.append(1e3 * (time.perf_counter() - t0))
if a.robust_features and a.linearise:
    med = lambda v: float(np.median(v))
    rst, robj, _, rhv, _, fw, rrc = ctx.gn_polish_robust_features(d, mono, G, steps, a.robust_features, a.c)
    Gp = dict(G, stVal=rst)
    res = {}
    for name, kw in (("plain", {}), ("feature_weighted", {"feature_weight": fw})):
        rows, walls = [], []
        for rep in range(4):
            t0 = time.perf_counter()
            H, F, _, tm, cnt = ctx.gn_linearise(d, mono, Gp, timed=True, **kw)
            walls.append(1e3 * (time.perf_counter() - t0))
            rows.append(tm)
        ev = {k: med([r[k] for r in rows[1:]]) for k in rows[0]}
        res[name] = {"events_ms": ev, "device_ms": sum(ev.values()), "blocks": cnt, "python_call_wall_ms": med(walls[1:]), "objective": F}
    w = np.concatenate(fw)
    sys.stdout.flush()
    print(json.dumps({"config": cfg, "type": typ, "maps": len(maps), "poses": int(G["m"]), "features": int(G["n"]), "steps": steps,
                      "robust_features": a.robust_features, "c": a.c, "polish_rc": rrc, "weights_below_1": float(np.mean(w < 1.0)), "weight_min": float(np.min(w)),
                      "linearise_features": dict(res, extra_device_ms=res["feature_weighted"]["device_ms"] - res["plain"]["device_ms"]),
                      "note": "at the state lsfm_gn_polish_robust_features ended at; plain = lsfm_gn_linearise, feature_weighted = "
                              "lsfm_gn_linearise_features with the polish's weights, one session, medians of 3 calls after one warm-up of each; events_ms: "
                              "HIP events (chi2_fill_ms: k_gn_chi2<true, true> + k_gn_given_objective + k_gn_feature_ufill); blocks: NWJ -> nW, NUJ -> nU; "
                              "python_call_wall_ms includes building the lsfm_map views and copying the result; library_wall_ms: the library's own clocks"}))
    sys.exit(0)
if a.robust_features:
    runs = {}
    for name, call in (("map_robust_run", lambda: ctx.gn_polish_robust(d, mono, G, steps, a.robust_features, a.c)),
                       ("feature_robust_run", lambda: ctx.gn_polish_robust_features(d, mono, G, steps, a.robust_features, a.c))):
        walls = []
        for rep in range(2):
            t0 = time.perf_counter()
            rst, robj, rgn, rhv, _, w, rrc = call()
            walls.append(1e3 * (time.perf_counter() - t0))
        w = np.concatenate(w) if isinstance(w, list) else w
        runs[name] = {"objective": robj.tolist(), "halvings": rhv.tolist(), "call_wall_ms": walls, "rc": rrc, "weight_min": float(np.min(w)),
                      "weight_median": float(np.median(w)), "weights_below_1": float(np.mean(w < 1.0))}
    nW, nF, nU = sum(m.nW for m in maps), sum(m.n for m in maps), sum(m.nU for m in maps)
    sys.stdout.flush()
    print(json.dumps({"config": cfg, "type": typ, "maps": len(maps), "poses": int(G["m"]), "features": int(G["n"]), "steps": steps,
                      "robust_features": a.robust_features, "c": a.c, "local_W_blocks": nW, "local_features": nF, "local_U_blocks": nU,
                      "chi2_pass_bytes": 144 * nW + (72 + 24) * nF + 288 * nU,
                      "plain": {"objective": obj.tolist(), "halvings": hv.tolist(), "call_wall_ms": calls}, **runs,
                      "note": "plain = lsfm_gn_polish, map_robust_run = lsfm_gn_polish_robust, feature_robust_run = lsfm_gn_polish_robust_features, same "
                              "kind, c and steps from the device's tree result; library_timing: the library's own clocks, in call order plain, plain, "
                              "map-robust x 2, feature-robust x 2 (the second of each warm); chi2_weights_ms: HIP events around k_gn_chi2<false> + "
                              "k_gn_robust_weights resp. k_gn_chi2<true> + k_gn_feature_objective; chi2_pass_bytes: every local U, W and V block "
                              "and feature estimate once, the least either pass reads"}))
    sys.exit(0)
if a.robust:
    rcalls = []
    for rep in range(2):
        t0 = time.perf_counter()
        rst, robj, rgn, rhv, chi2, w, rrc = ctx.gn_polish_robust(d, mono, G, steps, a.robust, a.c)
        rcalls.append(1e3 * (time.perf_counter() - t0))
    sys.stdout.flush()
    print(json.dumps({"config": cfg, "type": typ, "maps": len(maps), "poses": int(G["m"]), "features": int(G["n"]), "steps": steps,
                      "robust": a.robust, "c": a.c, "plain": {"objective": obj.tolist(), "halvings": hv.tolist(), "call_wall_ms": calls},
                      "robust_run": {"objective": robj.tolist(), "halvings": rhv.tolist(), "call_wall_ms": rcalls, "rc": rrc,
                                     "weight_min": float(np.min(w)), "weight_median": float(np.median(w))},
                      "note": "plain = lsfm_gn_polish, robust_run = lsfm_gn_polish_robust, same steps from the device's tree result; library_timing: "
                              "the library's own clocks, in call order plain, plain, robust, robust (the second of each warm)"}))
    sys.exit(0)
lin = None
if a.linearise:
    med = lambda v: float(np.median(v))
    Gp = dict(G, stVal=st)
    rows, walls = [], []
    for rep in range(4):
        t0 = time.perf_counter()
        H, F, _, tm, cnt = ctx.gn_linearise(d, mono, Gp, timed=True)
        walls.append(1e3 * (time.perf_counter() - t0))
        rows.append(tm)
    ev = {k: med([r[k] for r in rows[1:]]) for k in rows[0]}
    cov = {}
    for name, mp in (("linearised", H), ("tree", G)):
        t = []
        for rep in range(4):
            t0 = time.perf_counter()
            crc = ctx.covariance_raw(mp, mono)[0]
            t.append(1e3 * (time.perf_counter() - t0))
        cov[name] = {"wall_ms": med(t[1:]), "rc": crc, "U_blocks": int(mp["nU"]), "W_blocks": int(mp["nW"])}
    lin = {"events_ms": ev, "coalescing_over_assembly": (ev["coalesce_w_ms"] + ev["coalesce_u_ms"]) / ev["assembly_ms"], "blocks": cnt,
           "coalesce_w_GBps": (cnt["NWJ"] + cnt["nW"]) * 144 / (ev["coalesce_w_ms"] * 1e6) if ev["coalesce_w_ms"] > 0 else None,
           "python_call_wall_ms": med(walls[1:]), "objective": F, "map_covariance": cov,
           "note": "at the polished state; medians of 3 calls after one warm-up; python_call_wall_ms includes building the lsfm_map views and copying "
                   "the result into numpy arrays; library_wall_ms: the library's own clocks"}
print(json.dumps({"config": cfg, "type": typ, "maps": len(maps), "poses": int(G["m"]), "features": int(G["n"]), "steps": steps, "tree_ms": stats["t_total_ms"], "tree_rc": rc,
                  **({"linearise": lin} if lin else {}),
                  "gn_rc": rc2, "objective": obj.tolist(), "gradient_max": gn.tolist(), "halvings": hv.tolist(), "call_wall_ms": calls,
                  "max_state_change": float(np.max(np.abs(st - G["stVal"]))),
                  "note": "lsfm_gn_polish from the device's own tree result; call_wall_ms includes building the lsfm_map views in Python, the upload of the "
                          "local maps and the host's structure pass; library_timing = the library's own clocks (second call warm)"}))
