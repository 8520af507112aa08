"""Joint systems built to order for the direct tests of K9 (test_crafted_cpu.py, test_gpu_schur_crafted.py): plain numpy, no GPU,
nothing of the reference.  Which code of K9 runs hangs on the index arrays alone -- the poses that see each tile of 128 consecutive
features, the lengths of the features' runs, repeated (pose, feature) blocks -- so craft() takes exactly that as its description.

The matrix is positive semi-definite by construction (so K9's Cauchy-Schwarz bound holds by construction): every observation
(pose p, feature f) draws A (3x6) and B (3x3) and adds A^T A to U_pp, A^T B as W_pf, B^T B to V_f; a multiple of I goes on V_f and a
prior, sized to the data term, on the diagonal of U_pp.  The columns of A that belong to pose scalar (p, r) are multiplied by 10^u,
u uniform in [-decades, decades]: a congruence, which drives the per-scalar exponents of the fixed-point sums apart."""
import functools

import numpy as np

from common import _inv3_longdouble, dense_reference_solve, schur_reference_solve

TILE = 128
EPS_V = 0.25   # V_f = sum B^T B + EPS_V I
PRIOR = 0.5    # U_pp += PRIOR diag(data term of U_pp)


def craft(m, tiles, seed, decades=0.0, dup=0.1, offdiag=False, bad_v=None, split_u=False):
    """tiles: one dict per tile of TILE consecutive features, in order: n (features, default TILE; only the last may have fewer),
    poses (the poses that see it: each of them sees at least one of its features, no other pose does), run (lo, hi: the number of
    poses that see a feature, uniform), dup_tail (optional (first feature of the tile, probability): repeats forced onto the blocks of
    the tile's last features).  dup: probability that an observation is stored as two W blocks that sum to A^T B (the second ones
    behind the feature's first blocks, as a join leaves them).  offdiag: U blocks (p, p + 1) of a chain.  bad_v (feature, rel): that
    V_f gets one eigenvalue of -rel times its largest.  split_u: every U block is stored as two addends, cut element by element like
    the repeats of W (those of a diagonal block stay symmetric).  Returns the system in the layout of common.golden_system, and beside it
    `scale` [m, 6] and `counts` (the poses of each tile as described)."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-decades, decades, (m, 6)) if decades else np.ones((m, 6))
    feat, pose, second_p = [], [], []
    f0 = 0
    for k, t in enumerate(tiles):
        nf = int(t.get("n", TILE))
        assert nf == TILE or k == len(tiles) - 1, "only the last tile may be ragged"
        ps = np.sort(np.asarray(t["poses"], np.int64))
        P = len(ps)
        assert len(np.unique(ps)) == P and ps[0] >= 0 and ps[-1] < m
        lo, hi = t["run"]
        c = -(-P // nf)  # poses a feature must take so that the tile's features cover its poses
        assert c <= lo <= hi <= P, (k, c, lo, hi, P)
        run = rng.integers(lo, hi + 1, nf)
        r = rng.random((nf, P))
        i = np.arange(nf)
        for j in range(c):
            r[i, (i * c + j) % P] = -1.0
        rank = np.argsort(np.argsort(r, axis=1), axis=1)
        fi, pi = np.nonzero(rank < run[:, None])  # (sorted by feature, then by pose)
        pr = np.full(nf, float(dup))
        if t.get("dup_tail") is not None:
            pr[t["dup_tail"][0]:] = t["dup_tail"][1]
        feat.append(f0 + fi); pose.append(ps[pi]); second_p.append(pr[fi])
        f0 += nf
    n = f0
    feat, pose, second_p = np.concatenate(feat), np.concatenate(pose), np.concatenate(second_p)
    nobs = len(feat)
    A = rng.standard_normal((nobs, 3, 6)) * scale[pose][:, None, :]
    B = rng.standard_normal((nobs, 3, 3))
    Wo = np.einsum("kai,kaj->kij", A, B)
    Ud = np.zeros((m, 6, 6))
    np.add.at(Ud, pose, np.einsum("kai,kaj->kij", A, A))
    V = np.zeros((n, 3, 3))
    np.add.at(V, feat, np.einsum("kai,kaj->kij", B, B))
    V += EPS_V * np.eye(3)
    V = 0.5 * (V + V.transpose(0, 2, 1))
    if bad_v is not None:
        f, rel = bad_v
        w, Q = np.linalg.eigh(V[f])
        w[0] = -rel * w[2]
        V[f] = (Q * w) @ Q.T
        V[f] = 0.5 * (V[f] + V[f].T)
    # repeats: the observation's block cut in two, element by element
    two = rng.random(nobs) < second_p
    T = rng.uniform(-1.0, 2.0, (int(two.sum()), 6, 3))
    first = Wo.copy()
    first[two] = Wo[two] * T
    second = Wo[two] - first[two]
    Wb = np.concatenate([first, second])
    fb, pb = np.concatenate([feat, feat[two]]), np.concatenate([pose, pose[two]])
    sb = np.concatenate([np.zeros(nobs, np.int64), np.ones(len(second), np.int64)])
    order = np.lexsort((pb, sb, fb))
    Wb, fb, pb = Wb[order], fb[order], pb[order]
    # U: a chain's off-diagonal blocks, the prior, one block per pose pair
    Ui, Uj, Uo = [np.arange(m)], [np.arange(m)], []
    if offdiag and m > 1:
        cnt = np.bincount(pose, minlength=m)
        g = np.sqrt(np.maximum(1.0, cnt) / 4.0)
        C = rng.standard_normal((m - 1, 6, 6)) * (scale[:-1] * g[:-1, None])[:, None, :]
        D = rng.standard_normal((m - 1, 6, 6)) * (scale[1:] * g[1:, None])[:, None, :]
        Ud[:-1] += np.einsum("kai,kaj->kij", C, C)
        Ud[1:] += np.einsum("kai,kaj->kij", D, D)
        Uo = np.einsum("kai,kaj->kij", C, D)
        Ui.append(np.arange(m - 1)); Uj.append(np.arange(1, m))
    Ud = 0.5 * (Ud + Ud.transpose(0, 2, 1))
    d = np.einsum("kii->ki", Ud)
    Ud[:, np.arange(6), np.arange(6)] += np.where(d > 0, PRIOR * d, scale ** 2)  # (a pose nothing sees: the prior alone)
    U = np.concatenate([Ud, Uo]) if len(Uo) else Ud
    if split_u:
        T = rng.uniform(-1.0, 2.0, U.shape)
        T[:m] = 0.5 * (T[:m] + T[:m].transpose(0, 2, 1))
        U = np.concatenate([U * T, U - U * T])
        Ui, Uj = Ui + Ui, Uj + Uj
    return dict(m=int(m), n=int(n), U=U.reshape(-1, 36), Ui=np.concatenate(Ui).astype(np.int32), Uj=np.concatenate(Uj).astype(np.int32),
                W=Wb.reshape(-1, 18), V=V.reshape(-1, 9), photo=pb.astype(np.int32), feature=fb.astype(np.int32),
                scale=scale, counts=[len(t["poses"]) for t in tiles])


# ---- yardsticks ---------------------------------------------------------------------------------------------------------------------------
def dense_u(J):
    """The camera part [6m, 6m] of the information matrix, symmetric, blocks with equal coordinates summed."""
    m = int(J["m"])
    U = np.asarray(J["U"], np.float64).reshape(-1, 6, 6)
    Ui, Uj = np.asarray(J["Ui"], np.int64), np.asarray(J["Uj"], np.int64)
    S = np.zeros((m, 6, m, 6))
    np.add.at(S, (Ui, slice(None), Uj), U)
    off = Ui != Uj
    np.add.at(S, (Uj[off], slice(None), Ui[off]), U[off].transpose(0, 2, 1))
    return S.reshape(6 * m, 6 * m)


def schur_by_feature(J, dtype=np.float64, drop=None, eb=None):
    """S = U - sum_f W_f V_f^-1 W_f^T over the (dropped) features, feature by feature, in `dtype` (V^-1: numpy's inverse in fp64, the
    adjugate in long double); with eb also g = -sum_f W_f V_f^-1 eb_f."""
    m, n = int(J["m"]), int(J["n"])
    ld = dtype is np.longdouble
    S = dense_u(J).astype(dtype)
    V = np.asarray(J["V"], np.float64).reshape(-1, 3, 3)
    Vi = _inv3_longdouble(V) if ld else np.linalg.inv(V)
    W = np.asarray(J["W"], np.float64).reshape(-1, 6, 3).astype(dtype)
    ph, fe = np.asarray(J["photo"], np.int64), np.asarray(J["feature"], np.int64)
    fptr = np.searchsorted(fe, np.arange(n + 1))
    g = np.zeros(6 * m, dtype)
    ebl = None if eb is None else np.asarray(eb, np.float64).reshape(n, 3).astype(dtype)
    r6 = np.arange(6)
    for f in range(n):
        if drop is not None and not drop[f]:
            continue
        a, b = fptr[f], fptr[f + 1]
        ps, inv = np.unique(ph[a:b], return_inverse=True)
        Wf = np.zeros((len(ps), 6, 3), dtype)
        np.add.at(Wf, inv, W[a:b])
        P = Wf.reshape(-1, 3)
        rows = (6 * ps[:, None] + r6).reshape(-1)
        PV = P @ Vi[f]
        S[np.ix_(rows, rows)] -= PV @ P.T
        if ebl is not None:
            g[rows] -= PV @ ebl[f]
    return (S, g) if eb is not None else S


def info_metric(got, exp, diag):
    """max |d_ij| / sqrt(I_ii I_jj), I the input's diagonal (test_gpu_marginalise.info_err without its zero rows: there are none here)"""
    d = np.sqrt(np.asarray(diag, np.float64))
    return float(np.max(np.abs(np.asarray(got - exp, np.float64)) / np.outer(d, d)))


def state_metric(x, ref, m):
    """max |d| / max(1, |x|), over the poses and over the features"""
    e = np.abs(np.asarray(x) - ref) / np.maximum(1.0, np.abs(ref))
    return float(np.max(e[:6 * m])), float(np.max(e[6 * m:]))


def plain_schur_solve(J, ea, eb, mono, sa):
    """The solve as K9-K11 do it, in plain fp64 numpy: S and the reduced right-hand side feature by feature, a dense Cholesky solve, the
    features' back-substitution."""
    import scipy.linalg as sl
    m, n = int(J["m"]), int(J["n"])
    S, g = schur_by_feature(J, np.float64, eb=eb)
    g = g + np.asarray(ea, np.float64)
    keep = np.ones(6 * m, bool)
    if mono:
        keep[6 * sa[0]:6 * sa[0] + 6] = False
        keep[sa[2]] = False
    xp = np.zeros(6 * m)
    xp[keep] = sl.cho_solve(sl.cho_factor(S[np.ix_(keep, keep)]), g[keep])
    W = np.asarray(J["W"], np.float64).reshape(-1, 6, 3)
    ph, fe = np.asarray(J["photo"]), np.asarray(J["feature"])
    rf = np.asarray(eb, np.float64).reshape(n, 3).copy()
    np.add.at(rf, fe, -np.einsum("kij,ki->kj", W, xp.reshape(m, 6)[ph]))
    xf = np.einsum("fij,fj->fi", np.linalg.inv(np.asarray(J["V"], np.float64).reshape(-1, 3, 3)), rf)
    out = np.concatenate([xp, xf.reshape(-1)])
    if mono:
        out[sa[2]] = sa[3]
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def _win(start, count, m):
    return (start + np.arange(count)) % m


def _one(count, m, run, **kw):
    """one tile seen by `count` of m poses, spread over them"""
    return [dict(poses=np.random.default_rng(count).permutation(m)[:count], run=run, **kw)]


def _many(m, counts, last_n=None):
    tiles = [dict(poses=_win(7 * k + 3, c, m), run=(2, min(c, 10))) for k, c in enumerate(counts)]
    if last_n is not None:
        tiles[-1]["n"] = last_n
    return tiles


B_COUNTS = (16, 17, 32, 33, 48, 49, 62, 63, 64, 65, 100)
D1 = [12, 55, 10, 20, 8, 60, 25, 16, 14, 30, 6, 18, 11, 13, 9, 15, 36]
D2 = [20, 40, 24, 45, 28, 17, 36, 32]
D3 = [50, 63, 70, 12, 33, 56, 48, 62]

# name -> (m, tiles, keyword arguments of craft)
CASES = {
    # a. the 8- and the 16-slot variant launched alone (no system of the call has more poses)
    "a8": (8, [dict(poses=np.arange(8), run=(8, 8)), dict(poses=np.arange(1, 6), run=(1, 3)), dict(n=37, poses=np.arange(8), run=(1, 3))], {}),
    "a9": (9, [dict(poses=np.arange(9), run=(2, 5)), dict(n=50, poses=np.arange(2, 6), run=(1, 4))], {}),
    "a16": (16, [dict(poses=np.arange(16), run=(4, 16))], {"offdiag": True}),
    # c. dense wide tiles: more blocks than the LDS slot list holds, repeats behind its end, more than PM_BF blocks a pass
    "c32": (32, [dict(poses=np.arange(32), run=(32, 32), dup_tail=(112, 0.5))], {}),
    "c48": (48, [dict(poses=np.arange(48), run=(48, 48), dup_tail=(80, 0.5))], {}),
    "c63": (63, [dict(poses=np.arange(63), run=(30, 40), dup_tail=(80, 0.5))], {}),
    # d. several tiles: the lists of the wide variants, cut into parts
    "d1": (100, _many(100, D1, last_n=40), {"offdiag": True}),
    "d2": (100, _many(100, D2), {}),
    "d3": (100, _many(100, D3, last_n=70), {}),
    # f. the system of the Mono gauge case, g. the one with a V_f that has no factor
    "f33": (36, _one(33, 36, (2, 12)), {"offdiag": True}),
    "g20": (23, _one(20, 23, (2, 10)), {"bad_v": (50, 1e-3)}),
}
# b. one tile per system, at the edges of the variants' capacities; 100 poses with runs of about 70: more than SCHUR_CAP pose pairs
for _c in B_COUNTS:
    CASES[f"b{_c}"] = (_c + 3, _one(_c, _c + 3, (65, 75) if _c == 100 else (2, 12)), {"offdiag": _c in (33, 64)})
S_CASES = [k for k in CASES if k != "g20"]
SOLVE_CASES = S_CASES
LIST_CASES = ("d1", "d2", "d3")
DENSE_LIMIT = 4000  # unknowns up to which the solve cases are held to dense_reference_solve


@functools.lru_cache(maxsize=None)
def system(name, decades):
    m, tiles, kw = CASES[name]
    seed = sorted(CASES).index(name) + 1000 * int(decades)
    return craft(m, tiles, seed, decades=decades, **kw)


def gauge(J):
    """Mono call-site arguments (Ref, ScaP, Fix, Sign, FixBlk; common.golden_system, include/lsfm.h) that fix the block of one pose
    that features see and one scalar of another."""
    seen = np.unique(J["photo"])
    ref, other = int(seen[2]), int(seen[7])
    fix = 6 * other + 4
    return [ref, 6 * ref, fix, -1, other]


@functools.lru_cache(maxsize=None)
def rhs(name, decades):
    """ea with the scalars' scales, eb a unit normal"""
    J = system(name, decades)
    rng = np.random.default_rng(77 + sorted(CASES).index(name))
    ea = np.sqrt(np.diag(dense_u(J))) * rng.standard_normal(6 * J["m"])
    return ea, rng.standard_normal(3 * J["n"])


@functools.lru_cache(maxsize=None)
def expected_s(name, decades):
    """long-double U - sum W_f V_f^-1 W_f^T of a case.  Shared, never changed."""
    return schur_by_feature(system(name, decades), np.longdouble)


@functools.lru_cache(maxsize=None)
def expected_x(name, decades):
    """(expected state, mono, sa) of a solve case.  Shared, never changed."""
    J = system(name, decades)
    ea, eb = rhs(name, decades)
    mono = name == "f33"
    sa = gauge(J) if mono else None
    solve = dense_reference_solve if 6 * J["m"] + 3 * J["n"] <= DENSE_LIMIT else schur_reference_solve
    return solve(J, ea, eb, mono, sa), mono, sa


def half_dropped(name, decades):
    """every second feature of a case dropped: (drop flags, the system of the dropped features alone as K9 gets it)"""
    J = system(name, decades)
    drop = np.zeros(J["n"], bool)
    drop[::2] = True
    fe = np.asarray(J["feature"])
    wk = drop[fe]
    new = np.cumsum(drop) - 1
    return drop, dict(n=int(drop.sum()), photo=np.asarray(J["photo"])[wk], feature=new[fe[wk]])


def parts_of_list(nlist, ntiles, ncu):
    """k9_kernel's rule: the parts a listed tile is cut into, by the length of its variant's list against the launch's work-groups"""
    room = min(ntiles, ncu)
    return 0 if nlist == 0 else (8 if nlist * 8 <= room else 4 if nlist * 4 <= room else 2 if nlist * 2 <= room else 1)


def list_lengths(counts):
    """tiles on the lists of the 32-, 48- and 64-slot variants"""
    c = np.asarray(counts)
    return [int(np.sum((c > 16) & (c <= 32))), int(np.sum((c > 32) & (c <= 48))), int(np.sum((c > 48) & (c <= 63)))]
