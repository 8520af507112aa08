"""-m gpu: the per-feature and per-pose kernels of the transform where their work-group machinery can go wrong -- the records that
k_tr_feat_pre / k_tr_feat_post (and k_vinv of the level solve) move as the work-group's contiguous range through LDS (tile_records_load /
tile_records_store, csrc/lsfm_device.hpp: 16-byte pieces, an 8-byte piece at a misaligned head or tail), and the per-map sums
PP += C^T G that k_tr_feat_post and k_tr_poseslots collect in an LDS table of TR_PCAP rows per work-group (tile_wave_add) before they
leave it once (tile_flush); a map without a row adds to global memory directly.  Maps built with crafted_map.craft, through
lsfm_transform_* / lsfm_selftest_transform; k_vinv through lsfm_selftest_vinv.

Expected for the transform: the oracle's transform of each map alone, as in test_gpu_transform_crafted.py -- structure (labels, run
pointers FBlock, the place of every block: photo / feature, Ui / Uj) exact, values per block (crafted_map.compare) at
test_gpu_parity.py's STAGE_TOL = 1e-9; a passed-through map comes back bit for bit.
Expected for k_vinv: numpy's inverse of V in extended precision (longdouble), IV within VINV_TOL of it, and the record's own identities
L L^T = IV, y = L^T eb within VINV_TOL, all relative to the largest entry of the feature's IV.  V = A A^T + 3 I with standard normal A
has a condition number below 20 in these batches; an inverse by cofactors and a 3x3 Cholesky lose a few units of eps times the condition
number, 20 * 10 * 2.2e-16 = 4e-14: VINV_TOL = 1e-12 leaves a factor of 20 and catches a record of the neighbouring feature (O(1)).

Shapes (work-groups of 256 features, waves of 64; k_tr_poseslots: 128 poses):
  counts   one map of 1, 255, 256, 257, 513 features: a partial tile, an exact one, one feature / 257 features in the last work-group;
           an odd count ends the 9- and 3-double ranges 8 bytes behind a 16-byte boundary (the 8-byte tail piece)
  bounds   maps of 1, 63, 64, 65, 200 features in one batch: map boundaries inside a wave, on a wave's edge, inside a work-group
           (features 0 | 1 .. 63 | 64 .. 127 | 128 .. 192 | 193 .. 392), all transformed and with passed-through maps between (ANAFA)
  crowd    eight maps of 12 features, all transformed: 96 features of eight maps in ONE work-group, more than the table's rows (Stereo
           4 maps, Mono 16 / 3 = 5 maps): the later maps' sums take the direct path; its first wave holds six maps: the lanes of the
           last two go one by one
  hub      every batch has features with one old block to the hub pose and features with two (the hubJ == -2 walk of k_tr_feat_post)
  gauge    Mono: c2fix and c3zero, each on a map of 257 features
  poses    two maps, the first of 1, 127, 128, 129 poses: the map boundary at the start, just inside, on the edge and just behind the edge
           of k_tr_poseslots' work-group (Mono: a map of one pose cannot be transformed, it is passed through and the second map is)
  twice    the same input twice: V', x' (and everything else no atomic sums: labels, places, W' of kept blocks) and IV, LY bit for bit
k_vinv: 1, 255, 256, 257, 513 features, the device arrays on and 8 bytes off a 16-byte boundary (the 8-byte head piece) -- the same bits.

Measured on an MI355X (information, not the bar): worst of U / W / V / state over all transform cases 5.8e-15 (U of count_257 Mono);
k_vinv: IV 4.2e-16, L L^T 3.9e-16, L^T eb 2.2e-16.
"""
import functools

import numpy as np
import pytest

import crafted_map as cm
import crafted_stereo_records as sr
from test_gpu_parity import STAGE_TOL

pytestmark = pytest.mark.gpu

VINV_TOL = 1e-12
COUNTS = (1, 255, 256, 257, 513)
BOUND_N = (1, 63, 64, 65, 200)
POSE_COUNTS = (1, 127, 128, 129)
PCAP_MAPS = {False: 4, True: 5}  # maps that fit the LDS table of per-map sums (TR_PCAP rows; Mono: three rows per map)


def _runs(n, m, hubs, b=0):
    """runs of 2 .. 4 blocks; every fifth feature has one old block to the (first) hub, every seventh two (the -2 walk); Mono: the same
    for the second hub at other features.  A map of one pose: every block is the hub's"""
    others = [p for p in range(m) if p not in hubs] or list(range(m))
    runs = []
    for f in range(n):
        r = cm._cyc(others, 3 * f + b, 2 + f % 3)
        if f % 5 == 1:
            r.insert(1, hubs[0])
        if f % 7 == 3:
            r = [hubs[0]] + r + [hubs[0]]
        if len(hubs) > 1 and f % 4 == 2:
            r.append(hubs[1])
        if len(hubs) > 1 and f % 11 == 5:
            r = [hubs[1]] + r + [hubs[1]]
        runs.append(r)
    return runs


def _map(n, m, mono, seed, b=0, gauge=None):
    if mono and m == 1:
        return cm.craft(1, _runs(n, 1, (0, 0)), (0, 0), True, seed, target=None, id_base=1000 * b)
    assert not mono or m >= 6, "hubs and targets of a Mono map are four different poses"
    hubs = (m // 3, 2 * m // 3) if mono else (m // 2,)
    tgt = (1, m - 1)
    if gauge == "c2fix":     # the old reference pose becomes the scale pose
        tgt = (1, hubs[0])
    elif gauge == "c3zero":  # the old scale pose becomes the reference
        tgt = (hubs[1], m - 1)
    return cm.craft(m, _runs(n, m, hubs, b), hubs, mono, seed, target=tgt, id_base=1000 * b)


def _targets(maps, pattern, mono):
    return [{"A": d["target"], "N": None, "F": cm.own_frame(d, mono)}[c] for d, c in zip(maps, pattern)]


@functools.lru_cache(maxsize=None)
def case(name, mono):
    """(maps, targets); shared between the tests, nobody writes to the arrays"""
    kind, _, arg = name.partition("_")
    if kind == "count":
        maps = [_map(int(arg), 8, mono, 200 + int(arg))]
        return maps, _targets(maps, "A", mono)
    if kind == "gauge":
        maps = [_map(257, 12, True, 260, gauge=arg)]
        return maps, _targets(maps, "A", True)
    if kind == "bounds":
        maps = [_map(n, 6 + b, mono, 210 + b, b) for b, n in enumerate(BOUND_N)]
        return maps, _targets(maps, arg, mono)
    if kind == "crowd":
        maps = [_map(12, 6 + b % 2, mono, 220 + b, b) for b in range(8)]
        return maps, _targets(maps, "A" * 8, mono)
    if kind == "poses":
        m0 = int(arg)
        maps = [_map(30, m0, mono, 230 + m0, 0), _map(40, 6, mono, 240 + m0, 1)]
        return maps, _targets(maps, "NA" if mono and m0 == 1 else "AA", mono)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name, mono):
    """the oracle's transform of every transformed map alone (None: passed through); shared, never written to"""
    from oracle import pyoracle
    pyoracle.build()
    maps, targets = case(name, mono)
    return [pyoracle.transform(d, mono, *(t if mono else (t,))) if cm.is_active(d, t, mono) else None for d, t in zip(maps, targets)]


def _check_batch(ctx, name, mono, alias=False):
    maps, targets = case(name, mono)
    got = ctx.selftest_transform(maps, mono, targets, alias=alias)
    assert len(got) == len(maps)
    worst = 0.0
    for b, (g, d, e) in enumerate(zip(got, maps, expected(name, mono))):
        what = f"{name} {'Mono' if mono else 'Stereo'} map {b}"
        if e is None:
            cm.assert_identical(g, d, mono)
            continue
        for k in ("U", "W", "V", "stVal"):
            assert np.all(np.isfinite(g[k])), (what, k)
        errs = cm.compare(g, e, mono)  # (labels, run pointers and the place of every block: equality, inside)
        print(f"{what}: " + " ".join(f"{k} {v:.2e}" for k, (v, _) in errs.items()))
        for key, (v, where) in errs.items():
            assert v < STAGE_TOL, (what, key, v, where)
            worst = max(worst, v)
    print(f"{name} {'Mono' if mono else 'Stereo'}: worst {worst:.2e}")
    return got


def _hub_blocks(name, mono):
    maps, targets = case(name, mono)
    return cm.describe(maps, targets, mono)["hub_blocks"]


@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("n", COUNTS)
def test_feature_counts(ctx, n, mono):
    name = f"count_{n}"
    if n > 7:
        hb = _hub_blocks(name, mono)
        assert (hb[:, 0] == 1).any() and (hb[:, 0] == 2).any(), "one old block to the hub, and two (the -2 walk)"
    (d,), (t,) = case(name, mono)
    got = ctx.transform(d, mono, *(t if mono else (t,)))
    errs = cm.compare(got, expected(name, mono)[0], mono)
    print(f"{name} {'Mono' if mono else 'Stereo'}: " + " ".join(f"{k} {v:.2e}" for k, (v, _) in errs.items()))
    for key, (v, where) in errs.items():
        assert v < STAGE_TOL, (name, key, v, where)


@pytest.mark.parametrize("gauge", ["c2fix", "c3zero"])
def test_mono_gauge(ctx, gauge):
    (d,), (t,) = case(f"gauge_{gauge}", True)
    ids = -np.asarray(d["stno"])[:6 * d["m"]:6]
    if gauge == "c2fix":
        assert t[1] == ids[d["hubs"][0]] and t[0] != ids[d["hubs"][1]]
    else:
        assert t[0] == ids[d["hubs"][1]] and t[1] != ids[d["hubs"][0]]
    _check_batch(ctx, f"gauge_{gauge}", True)


@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("pattern", ["AAAAA", "ANAFA"])
def test_map_boundaries(ctx, pattern, mono):
    name = f"bounds_{pattern}"
    maps, targets = case(name, mono)
    desc = cm.describe(maps, targets, mono)
    if pattern == "AAAAA":
        assert desc["waves_feats"][0] == [0, 1] and desc["waves_feats"][1] == [2] and desc["waves_feats"][3] == [3, 4]
        assert desc["post_groups"] == [[0, 1, 2, 3, 4], [4]]
    else:
        assert desc["active"] == [True, False, True, False, True]
    _check_batch(ctx, name, mono, alias=(pattern == "ANAFA"))


@pytest.mark.parametrize("mono", [False, True])
def test_more_maps_than_rows(ctx, mono):
    maps, targets = case("crowd_8", mono)
    desc = cm.describe(maps, targets, mono)
    assert len(desc["post_groups"]) == 1 and len(desc["post_groups"][0]) == 8 > PCAP_MAPS[mono]
    assert max(len(w) for w in desc["waves_feats"]) > 4, "a wave with more than four maps: lanes left after four rounds"
    assert len(desc["pose_groups"][0]) == 8
    _check_batch(ctx, "crowd_8", mono)


@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("m0", POSE_COUNTS)
def test_pose_counts(ctx, m0, mono):
    name = f"poses_{m0}"
    maps, targets = case(name, mono)
    desc = cm.describe(maps, targets, mono)
    want = {1: [[0, 1]], 127: [[0, 1], [1]], 128: [[0], [1]], 129: [[0], [0, 1]]}[m0]
    assert maps[0]["m"] == m0 and desc["pose_groups"] == ([[1]] if mono and m0 == 1 else want)
    _check_batch(ctx, name, mono)


EXACT_KEYS = ("stno", "stVal", "V", "FBlock", "photo", "feature", "Ui", "Uj")


@pytest.mark.parametrize("mono", [False, True])
def test_twice_the_same_bits(ctx, mono):
    """what no atomic sums is the same bits in two runs: x' (stVal), V', the labels and places; and W' of the blocks that are not new hub blocks"""
    maps, targets = case("bounds_ANAFA", mono)
    one = ctx.selftest_transform(maps, mono, targets)
    two = ctx.selftest_transform(maps, mono, targets)
    for b, (g1, g2) in enumerate(zip(one, two)):
        for k in EXACT_KEYS:
            assert np.array_equal(np.asarray(g1[k]), np.asarray(g2[k])), (b, k)
    (d,), (t,) = case("count_513", mono)
    g1, g2 = (ctx.transform(d, mono, *(t if mono else (t,))) for _ in range(2))
    for k in EXACT_KEYS + ("W",):
        assert np.array_equal(np.asarray(g1[k]), np.asarray(g2[k])), k


def test_many_maps_of_the_record_batches(ctx):
    """crafted_stereo_records' batch of eight small maps (seven in the first 128 features) is eight maps in one work-group here"""
    maps, targets = sr.case("many")
    assert len(cm.describe(maps, targets, False)["post_groups"][0]) == 8 > PCAP_MAPS[False]
    from test_gpu_transform_stereo_records import expected as sr_expected
    got = ctx.selftest_transform(maps, False, targets)
    for b, (g, e) in enumerate(zip(got, sr_expected("many"))):
        for key, (v, where) in cm.compare(g, e, False).items():
            assert v < STAGE_TOL, (b, key, v, where)


# ---- k_vinv ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vinv_case(n):
    rng = np.random.default_rng(300 + n)
    A = rng.standard_normal((n, 3, 3))
    V = A @ A.transpose(0, 2, 1) + 3.0 * np.eye(3)
    eb = rng.standard_normal((n, 3))
    assert np.linalg.cond(V).max() < 20.0
    return V.reshape(n, 9), eb


@functools.lru_cache(maxsize=None)
def vinv_expected(n):
    """V^-1 by cofactors in extended precision"""
    V = vinv_case(n)[0].reshape(n, 3, 3).astype(np.longdouble)
    c = np.empty_like(V)
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != i]
            s = [k for k in range(3) if k != j]
            c[:, j, i] = (-1) ** (i + j) * (V[:, r[0], s[0]] * V[:, r[1], s[1]] - V[:, r[0], s[1]] * V[:, r[1], s[0]])
    det = (V[:, 0, :] * c[:, :, 0]).sum(axis=1)
    return (c / det[:, None, None]).astype(np.float64).reshape(n, 9)


@pytest.mark.parametrize("n", COUNTS)
def test_vinv_records(ctx, n):
    V, eb = vinv_case(n)
    IV, LY = ctx.selftest_vinv(V, eb)
    IV1, LY1 = ctx.selftest_vinv(V, eb, skip=1)   # every array 8 bytes off a 16-byte boundary: the 8-byte head piece
    IV2, LY2 = ctx.selftest_vinv(V, eb)
    assert np.array_equal(IV, IV1) and np.array_equal(LY, LY1), "the same bits wherever the arrays start"
    assert np.array_equal(IV, IV2) and np.array_equal(LY, LY2), "the same bits twice"
    assert np.array_equal(IV, ctx.inverse_v(V)), "lsfm_inverse_v is the same kernel"
    scale = np.abs(IV).max(axis=1)
    e_iv = (np.abs(IV - vinv_expected(n)).max(axis=1) / scale).max()
    L = np.zeros((n, 3, 3))
    L[:, 0, 0], L[:, 1, 0], L[:, 1, 1], L[:, 2, 0], L[:, 2, 1], L[:, 2, 2] = (LY[:, i] for i in range(6))
    e_l = (np.abs(L @ L.transpose(0, 2, 1) - IV.reshape(n, 3, 3)).reshape(n, 9).max(axis=1) / scale).max()
    y = np.einsum("nji,nj->ni", L, eb)
    e_y = (np.abs(LY[:, 6:] - y).max(axis=1) / np.maximum(1.0, np.abs(y).max(axis=1))).max()
    print(f"k_vinv n = {n}: IV {e_iv:.2e}  L L^T {e_l:.2e}  L^T eb {e_y:.2e}")
    assert e_iv < VINV_TOL and e_l < VINV_TOL and e_y < VINV_TOL, (e_iv, e_l, e_y)
