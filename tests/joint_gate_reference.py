"""Host statements of lsfm_map_feature_pair_joint_gate (include/lsfm.h), plain numpy, no GPU: the sequential joint-compatibility
selection among K feature pairs.  With A the matrix of rows e_f - e_g, C = A Sigma A^T and d = A x^; in processing order a pair is
    implied (status 2, delta 0)   when its endpoints are already connected by the accepted pairs (union-find: structural, exact),
    accepted (status 1)           when delta = e^T S^-1 e <= tau, S = C_bb - C_bAcc C_AccAcc^-1 C_Accb, e = d_b - C_bAcc C_AccAcc^-1 d_Acc,
    rejected (status 0)           otherwise; delta = NaN where a pivot of S is not > 0 or the individual d2 is NaN.
Two routes that share no factorisation:
    select(route="conditional")   a growing Cholesky factor of C_AccAcc, any dtype (np.longdouble: the reference of the GPU tests)
    select(route="differences")   delta_b = D2(Acc + b) - D2(Acc), D2(X) = d_X^T C_XX^-1 d_X by numpy.linalg.solve (LU)
Their disagreement on a given C is the host floor of delta and D^2."""
import numpy as np

TAU = 11.344866730144373  # chi^2_3 at 0.99
REL = 1e-6                # a delta within REL relative of tau may fall on either side (lsfm.h)


def joint_matrix(Sig, m, pairs):
    """C = A Sigma A^T [3K, 3K] from a dense Sigma [6m + 3n]^2, exactly symmetric by the call's rule: block (a, b), a < b, from the
    upper triangle and mirrored, a diagonal block (X + X^T) / 2."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    o = 6 * m
    idx = lambda col: (o + 3 * pairs[:, col][:, None] + np.arange(3)[None, :]).ravel()
    f, g = idx(0), idx(1)
    R = Sig[f, :] - Sig[g, :]
    C = R[:, f] - R[:, g]
    K = len(pairs)
    blk = np.repeat(np.arange(K), 3)
    same = blk[:, None] == blk[None, :]
    up = np.triu(C, 1)
    return np.where(same, 0.5 * (C + C.T), up + up.T)


def candidate_list(G, Sig, tau_c):
    """The candidate pairs of DESIGN.md section 19 for a joined map G with dense covariance Sig: every f < g with q = 1/2 d^T (Sigma_ff +
    Sigma_gg)^-1 d <= tau_c (no radius), sorted by (f, g); [K, 2] int32."""
    import candidates_reference as cref
    m, n = int(G["m"]), int(G["n"])
    o = 6 * m
    fcov = np.stack([Sig[o + 3 * a: o + 3 * a + 3, o + 3 * a: o + 3 * a + 3] for a in range(n)])
    f, g, q, bad = cref.all_q(cref.features_of(G), fcov)
    assert not bad.any()
    k = q <= tau_c
    return np.stack([f[k], g[k]], axis=1).astype(np.int32)


def state_diff(G, pairs):
    m = int(G["m"])
    x = np.asarray(G["stVal"], np.float64)[6 * m:].reshape(-1, 3)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    return (x[pairs[:, 0]] - x[pairs[:, 1]]).ravel()


def _chol3(S, e):
    """(delta, L, y) of a 3 x 3 block by the Cholesky the device takes; delta = NaN (L, y None) where a pivot is not > 0."""
    L = np.zeros((3, 3), S.dtype)
    for j in range(3):
        p = S[j, j] - L[j, :j] @ L[j, :j]
        if not p > 0:
            return S.dtype.type(np.nan), None, None
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, 3):
            L[i, j] = (S[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(3, S.dtype)
    for i in range(3):
        y[i] = (e[i] - L[i, :i] @ y[:i]) / L[i, i]
    return y @ y, L, y


def individual_d2(C, d):
    """d_b^T C_bb^-1 d_b per pair (float64), NaN where C_bb has a pivot that is not > 0."""
    C, d = np.asarray(C, np.float64), np.asarray(d, np.float64)
    return np.array([float(_chol3(C[3 * b: 3 * b + 3, 3 * b: 3 * b + 3], d[3 * b: 3 * b + 3])[0]) for b in range(len(d) // 3)])


def default_order(d2):
    """Ascending d2, ties by input index, NaN last."""
    d2 = np.asarray(d2, np.float64)
    return np.array(sorted(range(len(d2)), key=lambda b: (bool(np.isnan(d2[b])), 0.0 if np.isnan(d2[b]) else d2[b], b)), np.int64)


class _UnionFind:
    def __init__(self):
        self.p = {}

    def find(self, x):
        self.p.setdefault(x, x)
        while self.p[x] != x:
            self.p[x] = self.p[self.p[x]]
            x = self.p[x]
        return x

    def union(self, a, b):
        self.p[max(a, b)] = min(a, b)


def select(C, d, ends, tau, order=None, d2=None, route="conditional", dtype=np.float64):
    """The selection.  C [3K, 3K] symmetric, d [3K], ends [K, 2] the pairs' endpoints (any labels), order a permutation or None (ascending
    d2), d2 the individual distances (None: individual_d2).  Returns dict(status [K] int, delta [K] float64, D2, accepted (indices in
    processing order), implied (count), order, d2, delta_x [K] in `dtype`)."""
    C, d = np.asarray(C, dtype), np.asarray(d, dtype)
    ends = np.asarray(ends, np.int64).reshape(-1, 2)
    K = len(ends)
    if d2 is None:
        d2 = individual_d2(C, d)
    order = default_order(d2) if order is None else np.asarray(order, np.int64)
    assert sorted(order.tolist()) == list(range(K))
    status, delta = np.zeros(K, np.int64), np.full(K, np.nan, dtype)
    uf, acc = _UnionFind(), []
    L = np.zeros((0, 0), dtype)   # conditional: the factor of C_AccAcc ...
    y = np.zeros(0, dtype)        # ... and L^-1 d_Acc
    D2 = dtype(0)                 # differences: D2(Acc)
    sl = lambda b: slice(3 * b, 3 * b + 3)
    for b in (int(b) for b in order):
        if np.isnan(d2[b]):
            continue
        f, g = uf.find(int(ends[b, 0])), uf.find(int(ends[b, 1]))
        if f == g:
            status[b], delta[b] = 2, 0
            continue
        rows = np.concatenate([np.arange(3 * a, 3 * a + 3) for a in acc]).astype(np.int64) if acc else np.zeros(0, np.int64)
        if route == "conditional":
            n = len(rows)
            Wt = np.zeros((n, 3), dtype)   # L^-1 C_Acc,b
            rhs = C[rows, sl(b)]
            for i in range(n):
                Wt[i] = (rhs[i] - L[i, :i] @ Wt[:i]) / L[i, i]
            S = C[sl(b), sl(b)] - Wt.T @ Wt
            e = d[sl(b)] - Wt.T @ y
            dl, L3, y3 = _chol3(S, e)
            if not np.isnan(dl) and dl <= tau:
                Ln = np.zeros((n + 3, n + 3), dtype)
                Ln[:n, :n], Ln[n:, :n], Ln[n:, n:] = L, Wt.T, L3
                L, y = Ln, np.concatenate([y, y3])
        else:
            both = np.concatenate([rows, np.arange(3 * b, 3 * b + 3)])
            Cb = np.asarray(C[np.ix_(both, both)], np.float64)
            p = np.linalg.eigvalsh(Cb[-3:, -3:] - (Cb[-3:, :-3] @ np.linalg.solve(Cb[:-3, :-3], Cb[:-3, -3:]) if len(rows) else 0.0))
            Dn = float(np.asarray(d[both], np.float64) @ np.linalg.solve(Cb, np.asarray(d[both], np.float64)))
            dl = dtype(Dn) - D2 if p.min() > 0 else dtype(np.nan)
        delta[b] = dl
        if not np.isnan(dl) and dl <= tau:
            status[b] = 1
            acc.append(b)
            uf.union(f, g)
            if route != "conditional":
                D2 = dtype(Dn)
    tot = dtype(0)
    for b in acc:
        tot = tot + delta[b]
    return dict(status=status, delta=np.asarray(delta, np.float64), D2=float(tot), accepted=acc, implied=int(np.sum(status == 2)), order=order,
                d2=np.asarray(d2, np.float64), delta_x=delta)


def margins(sel, tau):
    """The smallest |x / tau - 1| over the finite, non-implied delta and the finite d2 of a selection: the tests assert it is above REL
    before they compare statuses."""
    v = np.concatenate([sel["delta"][sel["status"] != 2], sel["d2"]])
    v = v[np.isfinite(v)]
    return float(np.min(np.abs(v / tau - 1.0))) if len(v) and np.isfinite(tau) else np.inf


def scaled_condition(C, acc):
    """kappa_2 of C_AccAcc scaled to unit diagonal."""
    rows = np.concatenate([np.arange(3 * a, 3 * a + 3) for a in acc])
    Ca = np.asarray(C, np.float64)[np.ix_(rows, rows)]
    s = np.sqrt(np.diag(Ca))
    return float(np.linalg.cond(Ca / np.outer(s, s)))


def crafted_world(points, seed=0, rank=None):
    """(Sigma [3 points]^2 random SPD, x ~ N(0, Sigma)) on `points` 3-d points.  rank None: a full random Gram matrix (well conditioned,
    dense); an int: 0.5 I + U U^T / rank with U of that many columns -- cheap to build at thousands of points."""
    rng = np.random.default_rng(seed)
    n = 3 * points
    if rank is None:
        G = rng.normal(size=(n, n + 8))
        Sig = G @ G.T / n + 0.05 * np.eye(n)
        return Sig, np.linalg.cholesky(Sig) @ rng.normal(size=n)
    U = rng.normal(size=(n, rank)) / np.sqrt(rank)
    Sig = U @ U.T
    Sig[np.diag_indices(n)] += 0.5
    return Sig, U @ rng.normal(size=rank) + np.sqrt(0.5) * rng.normal(size=n)


def crafted_tree(points, K, seed=0):
    """ends [K, 2]: K <= points - 1 edges of a random tree on the points -- a cycle-free list; edge k joins a new point to one met before."""
    assert K <= points - 1
    rng = np.random.default_rng(seed + 1000)
    perm = rng.permutation(points)
    return np.array([(int(perm[k + 1]), int(perm[rng.integers(0, k + 1)])) for k in range(K)], np.int64).reshape(-1, 2)


def crafted_problem(Sig, x, ends, scale=1.0):
    """(C = A Sigma A^T, d = scale A x) for the pairs `ends` of a crafted world."""
    ends = np.asarray(ends, np.int64).reshape(-1, 2)
    x3 = np.asarray(x).reshape(-1, 3)
    return joint_matrix(Sig, 0, ends), scale * (x3[ends[:, 0]] - x3[ends[:, 1]]).ravel()
