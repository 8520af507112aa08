"""Batches of Stereo maps for the direct tests of what k_tr_entries<1> / k_tr_feat_post<1> make a feature's Jacobians from: the record
(R, dRA, dRB, dRG, t) of the feature's map and its new value x' (csrc/lsfm_transform.hip, stereo_tf).  k_tr_entries keeps the records of
a tile's first TRE_MAPS maps in LDS; a lane whose map comes later in the tile reads global memory.  crafted_map.py's cases never put
more than four maps into a tile, so that path needs batches of its own (test_stereo_records_cpu.py counts, on the index arrays, that
these reach it; test_gpu_transform_stereo_records.py runs them).  Plain numpy, built with crafted_map.craft."""
import functools

import crafted_map as cm

# eight maps of about 20 features and 3 or 4 poses: the first tile of 128 features holds maps 0 .. 6, the second maps 6 and 7
MANY_N = (20, 19, 21, 20, 18, 22, 20, 20)
MANY_M = (3, 4, 3, 4, 4, 3, 4, 3)
# A transformed, N passed through (no target), F passed through (in that frame already)
PATTERNS = {"many": "AAAAAAAA", "alternate": "ANAFANAF"}
BOUNDARY_N = (cm.TRE_TILE, 1)
CASES = ("many", "alternate", "boundary")


def _maps(ns, ms, seed):
    maps = []
    for b, (n, m) in enumerate(zip(ns, ms)):
        runs = [cm._cyc(list(range(m)), 5 * f + b, 2 + (f + b) % 3) for f in range(n)]  # (the hub pose among them: old blocks to it)
        maps.append(cm.craft(m, runs, ((b + 1) % m,), False, seed + b, id_base=1000 * b))
    return maps


@functools.lru_cache(maxsize=None)
def case(name):
    """(maps, targets); every map has its own reference pose, hub and state, so a record taken from another map shows in every block.
    The arrays are shared between the tests: nobody writes to them"""
    if name == "boundary":
        maps = _maps(BOUNDARY_N, (5, 3), 140)
        return maps, [d["target"] for d in maps]
    maps = _maps(MANY_N, MANY_M, 130)
    return maps, [{"A": d["target"], "N": None, "F": cm.own_frame(d, False)}[c] for d, c in zip(maps, PATTERNS[name])]
