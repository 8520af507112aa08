"""Maps and batches built to order for the direct tests of the batched coordinate transform, csrc/lsfm_transform.hip
(test_crafted_map_cpu.py, test_gpu_transform_crafted.py): plain numpy, no GPU, nothing of the reference.  Which code of the transform
runs hangs on the index arrays alone -- the lengths of the features' runs of W blocks, the poses that see each tile of 128 consecutive
features of the batch, the old blocks to the hub pose(s), which maps of a batch are transformed -- so craft() takes exactly that as its
description, and describe() counts on the index arrays what a case is claimed to reach.

The state is a valid one (angles within +-0.6 rad, positions of O(1), features a few units in front; Stereo: the reference pose is not in
the state; Mono: the reference pose is in the state at zero, the Fix component of the scale pose is at Sign, and the new scale baseline
is of O(1)).  The information blocks are standard normal numbers, V and the diagonal U blocks symmetrised: the transform is a congruence
I' = J^T I J, it needs no positive definiteness."""
import functools

import numpy as np

# restated from csrc/lsfm_transform.hip (test_crafted_map_cpu.py::test_constants_are_the_kernels reads them there)
TRE_TILE = 128                    # features per work-group of k_tr_entries
TRE_ROUND = 256                   # W blocks per round = threads
GCAP = {False: 32, True: 64}      # entries of k_tr_entries' LDS pose table, by mono
UGROUP, UCAP = 128, 64            # k_tr_ublocks: U blocks per work-group, entries of its LDS table
POSE_GROUP, POST_GROUP = 128, 256  # lanes per work-group of k_tr_poseslots / k_tr_feat_post (one per pose / feature)
B2_POSES = {False: 70, True: 140}  # case b2: more than 2 GCAP poses on a tile


def _rot(a, b, g):
    """R = Rx(g) Ry(b) Rz(a) (yaw, pitch, roll)"""
    ca, sa, cb, sb, cg, sg = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(g), np.sin(g)
    return np.array([[cb * ca, cb * sa, -sb],
                     [sg * sb * ca - cg * sa, sg * sb * sa + cg * ca, sg * cb],
                     [cg * sb * ca + sg * sa, cg * sb * sa - sg * ca, cg * cb]])


def craft(m, runs, hubs, mono, seed, target=None, fix=None, old_fix=0, old_sign=1, id_base=0):
    """m poses; runs: per feature the poses (0 .. m - 1) of its W blocks, in order (repeats allowed, a join leaves them); hubs: the
    poses whose row the transform fills -- Stereo (h,): the pose that becomes the reference; Mono (h0, h1): the map's reference and
    scale pose.  Mono, target = (r, s): the poses that become the reference and the scale pose; fix: the fixed component of the new
    scale (None: the largest).  Pose p has the id id_base + 1 + p, feature f the id id_base + 1 + f (Stereo: Ref = id_base).
    Returns the map dict; d["target"] is what transforms it (Ref, or (Ref, ScaP, Fix)), d["hubs"] the hubs as given."""
    rng = np.random.default_rng(seed)
    n = len(runs)
    ids = id_base + 1 + np.arange(m)
    for _ in range(1000):  # (Mono: until the new scale baseline is of O(1) in the fixed component)
        pose = np.concatenate([rng.uniform(-1.5, 1.5, (m, 3)), rng.uniform(-0.6, 0.6, (m, 3))], axis=1)
        if not mono:
            break
        h0, h1 = hubs
        pose[h1, :3] = rng.uniform(-0.8, 0.8, 3)
        pose[h1, old_fix] = old_sign
        pose[h0] = 0.0
        if target is None or m == 1:
            break
        r, s = target
        ts = _rot(*pose[r, 3:]) @ (pose[s, :3] - pose[r, :3])
        f = int(np.argmax(np.abs(ts))) if fix is None else int(fix)
        if 0.5 <= abs(ts[f]) <= 3.0:
            break
    else:
        raise ValueError("no state with a scale baseline of O(1)")
    feat = np.concatenate([rng.uniform(-2.0, 2.0, (n, 2)), rng.uniform(3.0, 8.0, (n, 1))], axis=1)
    lens = np.array([len(r_) for r_ in runs], np.int64)
    assert n == 0 or lens.min() >= 1, "every feature needs a W block"
    photo = np.concatenate([np.asarray(r_, np.int64) for r_ in runs]) if n else np.zeros(0, np.int64)
    assert photo.size == 0 or (photo.min() >= 0 and photo.max() < m)
    W = rng.standard_normal((len(photo), 18))
    V = rng.standard_normal((n, 3, 3))
    V = 0.5 * (V + V.transpose(0, 2, 1))
    Ud = rng.standard_normal((m, 6, 6))
    Ud = 0.5 * (Ud + Ud.transpose(0, 2, 1))
    Uo = rng.standard_normal((max(m - 1, 0), 6, 6))
    d = dict(m=int(m), n=int(n), U=np.concatenate([Ud, Uo]).reshape(-1, 36),
             Ui=np.concatenate([np.arange(m), np.arange(m - 1)]).astype(np.int32),
             Uj=np.concatenate([np.arange(m), np.arange(1, m)]).astype(np.int32),
             W=W, photo=photo.astype(np.int32), feature=np.repeat(np.arange(n), lens).astype(np.int32), V=V.reshape(-1, 9),
             FBlock=(np.cumsum(lens) - lens).astype(np.int32),
             stno=np.concatenate([np.repeat(-ids, 6), np.repeat(id_base + 1 + np.arange(n), 3)]).astype(np.int32),
             stVal=np.concatenate([pose.reshape(-1), feat.reshape(-1)]), hubs=tuple(int(h) for h in hubs))
    if mono:
        d.update(Ref=int(ids[hubs[0]]), ScaP=int(ids[hubs[1]]), Fix=int(old_fix), Sign=int(old_sign))
        d["target"] = (int(ids[target[0]]), int(ids[target[1]]), f) if target is not None and m > 1 else None
    else:
        d.update(Ref=int(id_base), ScaP=0, Fix=0, Sign=1, target=int(ids[hubs[0]]))
    d.update(FRef=d["Ref"], FScaP=d["ScaP"], FFix=d["Fix"], nU=len(d["Ui"]), nW=len(photo))
    return d


def own_frame(d, mono):
    """the target that names the frame the map is in already (the transform passes such a map through, map_in_frame)"""
    return (d["Ref"], d["ScaP"], d["Fix"]) if mono else d["Ref"]


def permute_features(d, perm):
    """The same map with whole features reordered: feature i of the result is feature perm[i] of d -- runs, V, state and ids"""
    perm = np.asarray(perm, np.int64)
    m, n = int(d["m"]), int(d["n"])
    assert np.array_equal(np.sort(perm), np.arange(n))
    fe = np.asarray(d["feature"], np.int64)
    start = np.searchsorted(fe, np.arange(n))
    lens = np.searchsorted(fe, np.arange(n), side="right") - start
    idx = np.concatenate([np.arange(start[p], start[p] + lens[p]) for p in perm]) if n else np.zeros(0, np.int64)
    out = dict(d)
    out["W"] = np.asarray(d["W"]).reshape(-1, 18)[idx]
    out["photo"] = np.asarray(d["photo"])[idx]
    out["feature"] = np.repeat(np.arange(n), lens[perm]).astype(np.int32)
    out["FBlock"] = (np.cumsum(lens[perm]) - lens[perm]).astype(np.int32)
    out["V"] = np.asarray(d["V"]).reshape(-1, 9)[perm]
    for k in ("stno", "stVal"):
        a = np.asarray(d[k])
        out[k] = np.concatenate([a[:6 * m], a[6 * m:].reshape(n, 3)[perm].reshape(-1)])
    return out


def is_active(d, target, mono):
    if target is None or (not isinstance(target, tuple) and target < 0):
        return False
    return tuple(target)[:2] != (d["Ref"], d["ScaP"]) if mono else target != d["Ref"]


def describe(maps, targets, mono):
    """What the batch reaches, from the indices alone (poses and features numbered through the batch, as the device does):
    active[b]; hubs[b] (global pose indices of a transformed map's hub(s)); tiles: per tile of TRE_TILE consecutive features the
    number of distinct poses of its transformed maps' blocks (`poses`: what asks for a slot of the LDS table) and the maps it holds;
    run / chunks / hub_blocks per feature; rounds: per tile the (first feature, features, blocks) of every round as k_tr_entries
    forms them; ugroups: per UGROUP U blocks the distinct poses of transformed maps' blocks; pose_groups / post_groups: the
    transformed maps in each work-group of k_tr_poseslots / k_tr_feat_post."""
    nh = 2 if mono else 1
    active = [is_active(d, t, mono) for d, t in zip(maps, targets)]
    P0 = np.concatenate([[0], np.cumsum([d["m"] for d in maps])])
    F0 = np.concatenate([[0], np.cumsum([d["n"] for d in maps])])
    hubs = []
    for b, d in enumerate(maps):
        ids = -np.asarray(d["stno"])[:6 * d["m"]:6]
        want = (d["Ref"], d["ScaP"]) if mono else (targets[b],)
        hubs.append([int(P0[b] + np.flatnonzero(ids == w)[0]) for w in want] if active[b] else [])
    photo = np.concatenate([np.asarray(d["photo"], np.int64) + P0[b] for b, d in enumerate(maps)])
    wmap = np.concatenate([np.full(len(d["photo"]), b) for b, d in enumerate(maps)])
    fmap = np.concatenate([np.full(d["n"], b) for b, d in enumerate(maps)])
    run = np.concatenate([np.bincount(np.asarray(d["feature"]), minlength=d["n"]) for d in maps]).astype(np.int64)
    fptr = np.concatenate([[0], np.cumsum(run)])
    NF = len(run)
    wact = np.array(active)[wmap]
    hub_blocks = np.zeros((NF, nh), np.int64)
    for f in range(NF):
        for s, h in enumerate(hubs[fmap[f]]):
            hub_blocks[f, s] = np.sum(photo[fptr[f]:fptr[f + 1]] == h)
    tiles, rounds = [], []
    for f0 in range(0, NF, TRE_TILE):
        f1 = min(f0 + TRE_TILE, NF)
        sel = slice(fptr[f0], fptr[f1])
        tiles.append(dict(poses=len(np.unique(photo[sel][wact[sel]])), maps=sorted(set(fmap[f0:f1].tolist()))))
        rs, la = [], f0
        while la < f1:
            lb = la + 1
            while lb < f1 and fptr[lb + 1] - fptr[la] <= TRE_ROUND:
                lb += 1
            rs.append((la, lb - la, int(fptr[lb] - fptr[la])))
            la = lb
        rounds.append(rs)
    Ui = np.concatenate([np.asarray(d["Ui"], np.int64) + P0[b] for b, d in enumerate(maps)])
    Uj = np.concatenate([np.asarray(d["Uj"], np.int64) + P0[b] for b, d in enumerate(maps)])
    uact = np.concatenate([np.full(len(d["Ui"]), active[b]) for b, d in enumerate(maps)])
    ugroups = [len(np.unique(np.concatenate([Ui[i:i + UGROUP][uact[i:i + UGROUP]], Uj[i:i + UGROUP][uact[i:i + UGROUP]]])))
               for i in range(0, len(Ui), UGROUP)]
    pmap = np.concatenate([np.full(d["m"], b) for b, d in enumerate(maps)])
    groups = lambda seg, size: [sorted({int(b) for b in seg[i:i + size] if active[b]}) for i in range(0, len(seg), size)]
    return dict(active=active, hubs=hubs, tiles=tiles, run=run, chunks=-(-run // TRE_ROUND), hub_blocks=hub_blocks, rounds=rounds, ugroups=ugroups,
                pose_groups=groups(pmap, POSE_GROUP), post_groups=groups(fmap, POST_GROUP), waves_poses=groups(pmap, 64), waves_feats=groups(fmap, 64))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def _cyc(L, start, k):
    return [L[(start + i) % len(L)] for i in range(k)]


def _case_a(mono):
    """rounds and chunks: one tile and a ragged second one (n = 129).  Runs of 513 (three chunks; the tile's first feature), 260 (a middle
    one), 257 and 300 (its last feature); 1 + 255 = a round of exactly 256, then a run of exactly 256; 255 followed by 2: the feature with 2
    blocks starts a round; 1-block features between.  The chunked features have their hub blocks, single and repeated, behind the first chunk"""
    m = 24
    hubs = (5, 11) if mono else (5,)
    h0, h1 = hubs[0], hubs[-1]
    others = [p for p in range(m) if p not in hubs]
    lens = {0: 513, 1: 1, 2: 255, 3: 256, 4: 255, 5: 2, 60: 260, 62: 257, 127: 300, 128: 3}
    hub_at = {0: {300: h0, 512: h0, 400: h1}, 3: {100: h0}, 10: {0: h0}, 60: {256: h0, 257: h1, 259: h1}, 127: {260: h0, 261: h0, 262: h0, 263: h0, 264: h0, 290: h1}, 62: {256: h0},
              128: {1: h1}}
    runs = []
    for f in range(129):
        r = _cyc(others, 7 * f, lens.get(f, 1))
        for pos, h in hub_at.get(f, {}).items():
            r[pos] = h
        runs.append(r)
    return [craft(m, runs, hubs, mono, 101, target=(2, 17))]


def _case_b1(mono):
    """pose table: a tile seen by exactly GCAP poses, then one seen by GCAP + 1 (the hubs among both)"""
    G = GCAP[mono]
    hubs = (3, 9) if mono else (3,)
    A = list(range(G))
    B = list(hubs) + list(range(G, 2 * G + 1 - len(hubs)))
    runs = [_cyc(A, 4 * i, 4) for i in range(TRE_TILE)] + [_cyc(B, 4 * i, 4) for i in range(TRE_TILE)]
    return [craft(2 * G + 4, runs, hubs, mono, 102, target=(1, 2))]


def _case_b2(mono):
    """pose table: two neighbouring tiles seen by the same 70 (Mono 140) poses -- more than twice the table -- in opposite orders (what takes
    the slots is what comes first: a row gets one tile's flush and the other's direct atomics), and a ragged third"""
    G, big = GCAP[mono], B2_POSES[mono]
    hubs = (G + 2, 5) if mono else (G + 2,)
    P = list(range(big))
    runs = [_cyc(P[:G], 4 * i, 4) for i in range(64)] + [_cyc(P[G:], 4 * i, 4) for i in range(64)]
    runs += [_cyc(P[big - G:], 4 * i, 4) for i in range(64)] + [_cyc(P[:big - G], 4 * i, 4) for i in range(64)]
    runs += [_cyc(P, 9 * i, 4) for i in range(5)]
    return [craft(big + 2, runs, hubs, mono, 103, target=(1, 2))]


C_COUNTS = ((0, 1, 2, 5), (0, 1, 3))


def _case_c(mono):
    """hub blocks: 0, 1, 2 or 5 old blocks to the (first) hub; Mono: times 0, 1 or 3 to the second -- all nine combinations of {none, one,
    several} within the first tile; feature 17 has nothing but a hub block"""
    m = 16
    hubs = (4, 9) if mono else (4,)
    others = [p for p in range(m) if p not in hubs]
    runs = []
    for f in range(130):
        r = _cyc(others, 3 * f, 0 if f == 17 else 3)
        for j in range(C_COUNTS[0][f % 4]):
            r.insert((2 * j) % (len(r) + 1), hubs[0])
        for j in range(C_COUNTS[1][(f // 4) % 3] if mono else 0):
            r.insert((2 * j + 1) % (len(r) + 1), hubs[1])
        runs.append(r)
    return [craft(m, runs, hubs, mono, 104, target=(2, 13))]


def _case_d(c2fix, c3zero, fix):
    """Mono gauge on a 12-pose map: c2fix (the old reference pose becomes the scale pose), c3zero (the old scale pose becomes the reference)"""
    m, hubs = 12, (3, 7)
    runs = [_cyc(list(range(m)), 5 * f, 4) for f in range(20)]
    return [craft(m, runs, hubs, True, 105 + 4 * fix + 2 * c2fix + c3zero, target=(hubs[1] if c3zero else 1, hubs[0] if c2fix else 5), fix=fix, old_fix=(fix + 1) % 3,
                  old_sign=-1 if fix == 1 else 1)]


E_N = (70, 100, 90, 1, 130)
E_M = (20, 22, 24, 1, 40)
E_PATTERNS = ("ANAFA", "AFANA", "NAFAN", "AAAAA", "NFNFN")  # A transformed, N passed through (no target), F passed through (in that frame already)


def _case_e(mono, pattern):
    """batches: five unequal maps, every tile boundary inside a map, the third tile holds three maps; map 3 has one pose (Mono: two where it
    is transformed); feature 57 of map 1 -- the last of the first tile -- has a run of 300"""
    maps = []
    for b, (n, m) in enumerate(zip(E_N, E_M)):
        if m == 1 and mono and pattern[b] == "A":
            m = 2
        hubs = ((0, m - 1) if m <= 2 else (m // 3, 2 * m // 3)) if mono else (m // 2,)
        tgt = (1, 0) if m == 2 else (1, m - 1)
        runs = [_cyc(list(range(m)), 5 * f, 300 if (b, f) == (1, 57) else 3 + f % 3) for f in range(n)]
        maps.append(craft(m, runs, hubs, mono, 110 + b, target=tgt, id_base=1000 * b))
    return maps


def _case_f(mono):
    """U stage: 300 poses, diagonal and chain blocks -- a work-group's 128 blocks touch 128 poses --, the hub(s) in the middle of the range"""
    m = 300
    hubs = (150, 200) if mono else (150,)
    runs = [_cyc(list(range(m)), 37 * f, 5) + ([hubs[f % len(hubs)]] if f % 3 == 0 else []) for f in range(40)]
    return [craft(m, runs, hubs, mono, 120, target=(10, 290))]


SINGLE = {"a": _case_a, "b1": _case_b1, "b2": _case_b2, "c": _case_c, "f": _case_f}
D_CASES = [(c2, c3, fix) for c2 in (0, 1) for c3 in (0, 1) for fix in (0, 1, 2)]
# (name, mono) of every case; the batches: name e_<pattern>
CASES = [(k, mono) for k in SINGLE for mono in (False, True)] + [(f"d{c2}{c3}_{fix}", True) for c2, c3, fix in D_CASES] + \
        [(f"e_{p}", mono) for p in E_PATTERNS for mono in (False, True)]


@functools.lru_cache(maxsize=None)
def case(name, mono):
    """(maps, targets) of a case; the arrays are shared between the tests: nobody writes to them"""
    if name in SINGLE:
        maps = SINGLE[name](mono)
        return maps, [maps[0]["target"]]
    if name[0] == "d":
        assert mono
        maps = _case_d(int(name[1]), int(name[2]), int(name[4]))
        return maps, [maps[0]["target"]]
    pattern = name[2:]
    maps = _case_e(mono, pattern)
    return maps, [{"A": d["target"], "N": None, "F": own_frame(d, mono)}[c] for d, c in zip(maps, pattern)]


# ---- the comparison -----------------------------------------------------------------------------------------------------------------------
def block_err(got, exp, width):
    """Worst block of max |got - exp| over max(the block's largest |entry| in exp, the median over the array of the blocks' largest
    entries); returns (error, index of that block).  No constant from outside the data; no block left out."""
    got, exp = np.asarray(got, np.float64).reshape(-1, width), np.asarray(exp, np.float64).reshape(-1, width)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    if not exp.size:
        return 0.0, -1
    big = np.abs(exp).max(axis=1)
    diff, den = np.abs(got - exp).max(axis=1), np.maximum(big, np.median(big))
    with np.errstate(divide="ignore", invalid="ignore"):  # (a denominator of 0: more than half of the blocks are exactly zero, this one too)
        e = np.where(den > 0, diff / den, np.where(diff == 0, 0.0, np.inf))
    e = np.where(np.isfinite(e), e, np.inf)
    k = int(np.argmax(e))
    return float(e[k]), k


def state_err(got, exp):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    assert got.shape == exp.shape
    if not exp.size:
        return 0.0, -1
    e = np.abs(got - exp) / np.maximum(1.0, np.abs(exp))
    e = np.where(np.isfinite(e), e, np.inf)
    k = int(np.argmax(e))
    return float(e[k]), k


def compare(got, exp, mono):
    """Structure exact; values per block.  Returns {array: (error, which block it is)} for U, W, V, stVal."""
    from common import canon_u
    keys = ("m", "n", "Ref", "FRef") + (("ScaP", "Fix", "Sign") if mono else ())
    for k in keys:
        assert int(got[k]) == int(exp[k]), (k, got[k], exp[k])
    for k in ("stno", "photo", "feature", "FBlock", "Ui", "Uj"):
        assert np.array_equal(np.asarray(got[k]).ravel(), np.asarray(exp[k]).ravel()), k
    out = {}
    if mono:
        cg, ce = canon_u(got), canon_u(exp)
        assert cg.keys() == ce.keys()
        ks = sorted(ce)
        e, k = block_err(np.array([cg[k] for k in ks]), np.array([ce[k] for k in ks]), 36)
        out["U"] = (e, f"U pair {ks[k]}" if k >= 0 else "")
    else:
        e, k = block_err(got["U"], exp["U"], 36)
        out["U"] = (e, f"U block {k}: ({exp['Ui'][k]}, {exp['Uj'][k]})" if k >= 0 else "")
    e, k = block_err(got["W"], exp["W"], 18)
    out["W"] = (e, f"W block {k}: pose {exp['photo'][k]}, feature {exp['feature'][k]}" if k >= 0 else "")
    e, k = block_err(got["V"], exp["V"], 9)
    out["V"] = (e, f"V of feature {k}")
    e, k = state_err(got["stVal"], exp["stVal"])
    out["stVal"] = (e, f"state scalar {k}, label {exp['stno'][k]}" if k >= 0 else "")
    return out


def assert_identical(got, src, mono):
    """a passed-through map: every array bit for bit"""
    for k in ("m", "n", "Ref", "FRef") + (("ScaP", "Fix", "Sign", "FScaP", "FFix") if mono else ()):
        assert int(got[k]) == int(src[k]), k
    for k in ("stno", "stVal", "U", "Ui", "Uj", "W", "photo", "feature", "V", "FBlock"):
        assert np.array_equal(np.asarray(got[k]).ravel(), np.asarray(src[k]).ravel()), k
