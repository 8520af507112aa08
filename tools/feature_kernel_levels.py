"""Per tree level, the time of the transform's per-feature kernels and of k_vinv with the number of features (poses) they ran over, from
a rocprofv3 kernel trace of `bench.py --steps 5 --warmup 2 --cpu-baseline 0 --extras 0`: the median over the last TREES trees of the
trace.  A level starts at its k_tr_find on the main queue (the busiest); a kernel belongs to the level its start falls into, whatever
queue it ran on (k_tr_poseslots runs on the side stream).  Elements = the launch's grid size: the count rounded up to the work-group.
    python tools/feature_kernel_levels.py <kernel_trace.csv[.gz]> [levels per tree = 13] [trees = 5]"""
import csv
import gzip
import statistics
import sys
from collections import defaultdict

KERNELS = ("k_tr_feat_pre", "k_tr_feat_post", "k_vinv", "k_tr_poseslots")

path = sys.argv[1]
per_tree = int(sys.argv[2]) if len(sys.argv) > 2 else 13
trees = int(sys.argv[3]) if len(sys.argv) > 3 else 5
op = gzip.open if path.endswith(".gz") else open
rows = []
with op(path, "rt") as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r["Queue_Id"], int(r.get("Grid_Size_X", 0) or 0)))
rows.sort()
byq = defaultdict(list)
for r in rows:
    byq[r[3]].append(r)
main = max(byq.values(), key=len)
starts = [r[0] for r in main if "k_tr_find" in r[2]]
assert len(starts) >= per_tree * trees, (len(starts), per_tree, trees)
starts = starts[len(starts) - per_tree * trees:] + [rows[-1][1] + 1]

# [tree][level][kernel] = (ns, elements)
acc = [[defaultdict(lambda: [0, 0]) for _ in range(per_tree)] for _ in range(trees)]
tree_ns = [starts[(t + 1) * per_tree] - starts[t * per_tree] for t in range(trees - 1)]
w = 0
for s, e, nm, _, grid in rows:
    if s < starts[0]:
        continue
    while s >= starts[w + 1]:
        w += 1
    for k in KERNELS:
        if k in nm:
            a = acc[w // per_tree][w % per_tree][k]
            a[0] += e - s
            a[1] = max(a[1], grid)

print(f"median over the last {trees} trees of the trace, {per_tree} transforms per tree (the last one returns the root to its first frame); "
      f"tree to tree under the profiler: {statistics.median(tree_ns) / 1e6:.2f} ms" if tree_ns else "")
print("level |  features |  feat_pre us  ns/feat | feat_post us  ns/feat |   k_vinv us  ns/feat (features) |  poses | poseslots us")
tot = defaultdict(float)
for lv in range(per_tree):
    med = {k: statistics.median(acc[t][lv][k][0] for t in range(trees)) / 1e3 for k in KERNELS}
    n = {k: acc[trees - 1][lv][k][1] for k in KERNELS}
    for k in KERNELS:
        tot[k] += med[k]
    per = lambda k: (1e3 * med[k] / n[k]) if n[k] else 0.0
    print(f"{lv:5d} | {n['k_tr_feat_post']:9d} | {med['k_tr_feat_pre']:11.1f} {per('k_tr_feat_pre'):8.3f} | {med['k_tr_feat_post']:11.1f} {per('k_tr_feat_post'):8.3f} | "
          f"{med['k_vinv']:11.1f} {per('k_vinv'):8.3f} ({n['k_vinv']:9d}) | {n['k_tr_poseslots']:6d} | {med['k_tr_poseslots']:11.1f}")
print("per tree, us: " + ", ".join(f"{k} {tot[k]:.0f}" for k in KERNELS))
