"""-m gpu: lsfm_map_feature_pair_candidates (csrc/lsfm_candidates.hip) -- every feature pair within a radius whose bound q = 1/2 d^T (Sigma_ff +
Sigma_gg)^-1 d is below tau, by a cell search.  No reference counterpart: the expected list is candidates_reference's brute force over
all pairs.

Bars: the pairs equal the reference's as a list (same set, same order); dist2 within 1e-15 relative (the sum is specified term by term:
it comes out bit-equal); q within 1e-12 relative (a 3x3 LDL^T of blocks whose condition number the tests keep below 1e3).  Pairs within
4 ulp of radius^2 or 1e-12 of tau are left open by the specification: every randomised case first asserts that its input has no pair
within 1e-9 of either threshold (candidates_reference.margin); the lattice and the cell-face cases sit EXACTLY on the radius with
coordinates whose products are exact in fp64."""
import numpy as np
import pytest

import candidates_reference as cref
from linearsfm_amd import api

pytestmark = pytest.mark.gpu
TAU = cref.TAU
RADII = (0.25, 0.9, 3.0)


def cloud(n, seed):
    """n points in clusters of about 40 (sigma 0.6) whose centres lie in [-8, 8]^3."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-8.0, 8.0, (max(1, n // 40), 3))
    return centres[rng.integers(0, len(centres), n)] + 0.6 * rng.standard_normal((n, 3))


def covs(n, seed, lo=-3.0, hi=-1.0):
    """n anisotropic SPD blocks: a random rotation, eigenvalues 10^U(lo, hi) -- condition number <= 100."""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    C = np.einsum("kij,kj,klj->kil", Q, 10.0 ** rng.uniform(lo, hi, (n, 3)), Q)
    return 0.5 * (C + C.transpose(0, 2, 1))


def check(ctx, x, radius, fcov=None, tau=None, exact=False, what=""):
    """The call against the brute force: the list, dist2, q.  Returns (got, expected)."""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    if not exact:
        assert len(cref.margin(x, radius, fcov, tau)) == 0, "the input has a pair on a threshold: pick another seed"
    exp = cref.candidates(x, radius, fcov, tau)
    got = ctx.feature_pair_candidates(cref.cloud_map(x), radius, fcov, tau)
    print(f"candidates {what}: n {len(x)}, radius {radius}, {'with' if fcov is not None else 'without'} feat_cov: {len(exp['pairs'])} pairs")
    assert got["pairs"].dtype == np.int32 and got["pairs"].shape == exp["pairs"].shape
    assert np.array_equal(got["pairs"], exp["pairs"])
    assert np.all(np.abs(got["dist2"] - exp["dist2"]) <= 1e-15 * exp["dist2"])
    if fcov is None:
        assert got["q"] is None
    else:
        nan = np.isnan(exp["q"])
        assert np.array_equal(np.isnan(got["q"]), nan)
        assert np.all(np.abs(got["q"][~nan] - exp["q"][~nan]) <= 1e-12 * exp["q"][~nan])
    return got, exp


# ---- 1. random clouds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_cov", [False, True])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257, 1500])
def test_random_clouds(ctx, n, with_cov):
    x = cloud(n, 100 + n)
    fcov = covs(n, 200 + n) if with_cov else None
    found = 0
    for radius in RADII:
        got, _ = check(ctx, x, radius, fcov, TAU if with_cov else None, what="cloud")
        found += len(got["pairs"])
    assert found > 0 or n < 63  # (n = 0, 1 are the empty calls; the clouds do find pairs)


# ---- 2. the exact boundary -------------------------------------------------------------------------------------------------------------------
def test_exact_boundary_on_a_lattice(ctx):
    """An integer lattice, radius 5: (0,0,0)-(3,4,0) and its like at dist2 == 25 are in, the pairs at 26 out.  Every coordinate, difference,
    product and sum is an exact integer in fp64: bit-exact whatever is contracted."""
    g = np.arange(-3, 5, dtype=np.float64)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    got, exp = check(ctx, x, 5.0, exact=True, what="lattice")
    assert np.array_equal(got["dist2"], exp["dist2"])
    at = {tuple(p): k for k, p in enumerate(x.tolist())}
    have = {tuple(p) for p in got["pairs"].tolist()}
    pair = lambda a, b: tuple(sorted((at[a], at[b])))
    for a, b in (((0, 0, 0), (3, 4, 0)), ((0, 0, 0), (0, -3, 4)), ((-3, -3, -3), (1, 0, -3)), ((3, 3, 3), (3, -2, 3)), ((-2, 1, 0), (2, 1, 3))):
        assert sum((u - v) ** 2 for u, v in zip(a, b)) == 25 and pair(a, b) in have, (a, b)
    for a, b in (((0, 0, 0), (1, 5 - 3, 0)), ((0, 0, 0), (3, 4, 1)), ((-3, -3, -3), (2, -2, -3)), ((-3, 0, 0), (2, 1, 0)), ((1, 1, 1), (2, -2, -3))):
        d2 = sum((u - v) ** 2 for u, v in zip(a, b))
        assert (d2 == 26 and pair(a, b) not in have) or (d2 < 25 and pair(a, b) in have), (a, b, d2)
    d2_all = np.sum((x[:, None, :] - x[None, :, :]) ** 2, axis=-1)[np.triu_indices(len(x), 1)]
    assert len(have) == int(np.sum(d2_all <= 25)) and np.sum(d2_all == 25) > 0 and np.sum(d2_all == 26) > 0
    assert np.sum(got["dist2"] == 25.0) == np.sum(d2_all == 25) and got["dist2"].max() == 25.0


# ---- 3. every neighbour direction ------------------------------------------------------------------------------------------------------------
def _cells(x, radius):
    """The cell of every point as the specification states it: floor((x - lo) / edge), edge = radius (1 + 2^-20), lo the box's minimum."""
    edge = radius * (1.0 + 2.0 ** -20)
    return np.floor((x - x.min(axis=0)) / edge).astype(np.int64)


def test_every_neighbour_direction(ctx):
    """27 pairs, one per cell offset in {-1, 0, 1}^3 (the cell itself included), 4 cells apart along x.  The points lie on exact
    multiples of the radius -- cell faces but for the edge's slack -- or exact halves / quarters of it; along the axes they are exactly
    one radius apart.  A missing offset of the half neighbourhood, or an edge without slack, loses a pair here."""
    r = 0.5
    pts = [(0.0, 0.0, 0.0)]  # the corner of the box: lo
    offsets = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
    for t, o in enumerate(offsets):
        k = np.array([4 * t + 4, 4, 4], np.float64)
        axial = sum(1 for v in o if v) == 1
        a, b = np.zeros(3), np.zeros(3)
        for ax in range(3):
            if o[ax] == 0:  # the same cell k: a quarter above its lower face
                a[ax] = b[ax] = (k[ax] + 0.25) * r
            elif axial:     # k r is the last point of cell k - 1, (k + 1) r of cell k: exactly one radius apart
                lo_, hi_ = k[ax] * r, (k[ax] + 1) * r
                a[ax], b[ax] = (lo_, hi_) if o[ax] > 0 else (hi_, lo_)
            else:
                lo_, hi_ = k[ax] * r, (k[ax] + 0.5) * r
                a[ax], b[ax] = (lo_, hi_) if o[ax] > 0 else (hi_, lo_)
        if o == (0, 0, 0):
            b[0] += r / 8
        pts += [tuple(a), tuple(b)]
    x = np.array(pts)
    c = _cells(x, r)
    assert [tuple(c[2 + 2 * t] - c[1 + 2 * t]) for t in range(27)] == offsets  # every pair realises its offset
    got, exp = check(ctx, x, r, exact=True, what="27 offsets")
    assert got["pairs"].tolist() == [[1 + 2 * t, 2 + 2 * t] for t in range(27)]
    assert np.array_equal(got["dist2"], exp["dist2"]) and np.sum(got["dist2"] == r * r) == 6
    # ... and with the pairs' order in the feature list turned round (the other half of every direction)
    y = x[np.concatenate([[0], np.arange(1, 55).reshape(27, 2)[:, ::-1].ravel()])]
    got, _ = check(ctx, y, r, exact=True, what="27 offsets, reversed")
    assert got["pairs"].tolist() == [[1 + 2 * t, 2 + 2 * t] for t in range(27)]


# ---- 4. one crowded cell ---------------------------------------------------------------------------------------------------------------------
def test_one_crowded_cell(ctx):
    """700 features within radius / 4 of each other: all 244 650 pairs, from one cell -- more than a slice, a wave, a work-group.  A cap
    one short: LSFM_ERR_ARG, the count right, pairs untouched; the next call is fine."""
    rng = np.random.default_rng(7)
    x = 3.0 + rng.uniform(0.0, 0.25 / np.sqrt(3.0), (700, 3))
    fcov = covs(700, 8, lo=-1.0, hi=0.0)  # wide: q stays far below tau
    got, _ = check(ctx, x, 1.0, what="crowded, radius alone")
    assert len(got["pairs"]) == 244650
    got, _ = check(ctx, x, 1.0, fcov, TAU, what="crowded")
    assert len(got["pairs"]) == 244650
    d = cref.cloud_map(x)
    rc, count, pr, dd, qq, _, _ = ctx.feature_pair_candidates_raw(d, 1.0, fcov, TAU, cap=244649)
    assert rc == -1 and count == 244650
    assert np.all(pr == -1) and np.all(dd == -1.0) and np.all(qq == -1.0)
    assert "cap" in api.lib().lsfm_last_error(ctx._h).decode()
    rc, count, pr, _, _, t, info = ctx.feature_pair_candidates_raw(d, 1.0, fcov, TAU, cap=244650, times=True)
    assert rc == 0 and count == 244650 and np.array_equal(pr, got["pairs"])
    assert info.tolist() == [1, 700, 244650, 244650] and np.all(t >= 0)


# ---- 5. far from the origin --------------------------------------------------------------------------------------------------------------------
def test_far_from_the_origin(ctx):
    x = cloud(257, 31) + 1e6
    check(ctx, x, 0.5, what="offset 1e6")
    check(ctx, x, 0.5, covs(257, 32), TAU, what="offset 1e6")


# ---- 6. blocks that are not positive definite ----------------------------------------------------------------------------------------------------
def test_not_positive_definite_blocks_are_kept(ctx):
    n, radius = 257, 0.9
    x = cloud(n, 41)
    clean = covs(n, 42)
    base = cref.candidates(x, radius)  # the radius alone
    near = lambda f: {tuple(p) for p in base["pairs"].tolist() if f in p}
    # two features with zero blocks that are in each other's radius; a NaN block; a block that makes every sum indefinite
    z0, z1 = (int(v) for v in base["pairs"][len(base["pairs"]) // 2])
    rest = [f for f in range(n) if f not in (z0, z1) and len(near(f)) >= 3]
    fnan, find = rest[0], rest[-1]
    fcov = clean.copy()
    fcov[z0] = fcov[z1] = 0.0
    fcov[fnan] = np.nan
    fcov[find] = np.diag([10.0, -10.0, 10.0])
    got, exp = check(ctx, x, radius, fcov, TAU, what="not positive definite")
    q = {tuple(p): v for p, v in zip(got["pairs"].tolist(), got["q"])}
    assert np.isnan(q[tuple(sorted((z0, z1)))])
    for f in (fnan, find):
        assert near(f) and all(p in q and np.isnan(q[p]) for p in near(f)), f
    # the rest is what the clean blocks give
    ref_clean, _ = check(ctx, x, radius, clean, TAU, what="clean")
    special = {z0, z1, fnan, find}
    keep = lambda r: [(tuple(p), v) for p, v in zip(r["pairs"].tolist(), r["q"]) if not special & set(p)]
    assert keep(got) == keep(ref_clean) and len(keep(got)) > 0


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx):
    x = cloud(65, 51)
    d = cref.cloud_map(x)
    fcov = covs(65, 52)
    good = cref.candidates(x, 0.9, fcov, TAU)

    def still_works():
        got = ctx.feature_pair_candidates(d, 0.9, fcov, TAU)
        assert np.array_equal(got["pairs"], good["pairs"])

    err = lambda: api.lib().lsfm_last_error(ctx._h).decode()
    for radius in (0.0, -1.0, np.inf, np.nan):
        rc, count, *_ = ctx.feature_pair_candidates_raw(d, radius)
        assert rc == -1 and count == 0 and "radius" in err(), radius
        still_works()
    for tau in (0.0, np.nan):
        rc, count, *_ = ctx.feature_pair_candidates_raw(d, 0.9, fcov, tau)
        assert rc == -1 and count == 0 and "tau" in err(), tau
        still_works()
    rc, *_ = ctx.feature_pair_candidates_raw(d, 0.9, None, None, cap=10, q=True)
    assert rc == -1 and "feat_cov" in err()
    still_works()
    bad = x.copy()
    bad[7, 1] = np.nan
    with pytest.raises(api.LsfmError, match="feature 7 "):
        ctx.feature_pair_candidates(cref.cloud_map(bad), 0.9)
    still_works()
    wide = x.copy()
    wide[3, 2] += 1e7
    with pytest.raises(api.LsfmError, match="radius too small for the map's extent"):
        ctx.feature_pair_candidates(cref.cloud_map(wide), 1.0)
    still_works()


# ---- 8. two calls agree ------------------------------------------------------------------------------------------------------------------------
def test_two_calls_agree_bit_for_bit(ctx):
    x, fcov = cloud(1500, 61), covs(1500, 62)
    d = cref.cloud_map(x)
    a = ctx.feature_pair_candidates(d, 0.9, fcov, TAU)
    ctx.feature_pair_candidates(cref.cloud_map(cloud(300, 63)), 3.0)  # (something else in between)
    b = ctx.feature_pair_candidates(d, 0.9, fcov, TAU)
    assert len(a["pairs"]) > 1000
    for k in ("pairs", "dist2", "q"):
        assert np.array_equal(a[k], b[k]), k


# ---- 9. the guarantee, through the real calls -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,count", [(2, 8), (3, 32), (6, 8), (7, 32)])
def test_guarantee_on_split_sets(ctx, i, count):
    """The device tree of a split set: candidates from lsfm_map_covariance's own feature blocks, then the exact gate on them and on 64
    seeded non-candidates.  No accepted pair is lost; every split pair is a candidate; the list is short."""
    from test_gpu_merge import _split
    mono, G, _, split = _split(ctx, i, count)
    x = cref.features_of(G)
    n = len(x)
    npairs = n * (n - 1) // 2
    fcov = ctx.covariance(G, mono)["feature"]
    splitset = {tuple(sorted(map(int, p))) for p in split}
    assert len(splitset) == count
    extent = float(np.max(np.ptp(x, axis=0)))
    for radius in (2.0 * extent, 1.0):  # one cell; then far below the extent and above the largest split distance (0.66)
        assert len(cref.margin(x, radius, fcov, TAU, rel=1e-6)) == 0
        exp = cref.candidates(x, radius, fcov, TAU)
        got = ctx.feature_pair_candidates(G, radius, fcov, TAU)
        assert np.array_equal(got["pairs"], exp["pairs"])                                  # (a)
        assert np.all(np.abs(got["dist2"] - exp["dist2"]) <= 1e-15 * exp["dist2"])
        assert np.all(np.abs(got["q"] - exp["q"]) <= 1e-12 * exp["q"])
        have = {tuple(p) for p in got["pairs"].tolist()}
        assert splitset <= have                                                             # (b)
        assert len(have) <= 0.01 * npairs                                                   # (c)
        print(f"guarantee {i} x{count}, radius {radius:.3g}: {len(have)} candidates of {npairs} pairs, extent {extent:.3g}")
    assert extent > 8.0 and max(float(np.linalg.norm(x[a] - x[b])) for a, b in splitset) < 1.0  # (radius 1: many cells, and no split pair cut off)
    # (d) the exact gate: q <= d2 on the candidates of the one-cell call, d2 > tau on pairs that are not candidates
    got = ctx.feature_pair_candidates(G, 2.0 * extent, fcov, TAU)
    have = {tuple(p) for p in got["pairs"].tolist()}
    rng = np.random.default_rng(9)
    others = []
    while len(others) < 64:
        f, g = sorted(int(v) for v in rng.choice(n, 2, replace=False))
        if (f, g) not in have and (f, g) not in others:
            others.append((f, g))
    pairs = np.concatenate([got["pairs"], np.array(others, np.int32)])
    gate = ctx.feature_pair_gate(G, mono, pairs)
    k = len(got["pairs"])
    assert gate["converged"] and not np.any(np.isnan(gate["d2"]))
    assert np.all(got["q"] <= gate["d2"][:k] * (1 + 1e-6))
    assert np.all(gate["d2"][k:] > TAU)
