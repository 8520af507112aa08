"""Host statement of lsfm_map_feature_pair_candidates (include/lsfm.h): a numpy brute force over ALL pairs f < g.

    dist2 = (dx^2 + dy^2) + dz^2, every product and sum rounded on its own; kept when dist2 <= radius^2
    q     = 1/2 d^T (Sigma_ff + Sigma_gg)^-1 d by the LDL^T of the sum; kept when q <= tau, and kept with q = NaN when a pivot is not > 0

margin(...) lists the pairs the specification leaves open at the tests' precision: within REL of radius^2 or of tau.  Every randomised
test asserts that its inputs have none."""
import numpy as np

TAU = 11.344866730144373  # chi^2_3 at 0.99
REL = 1e-9


def cloud_map(x, first_label=1):
    """A map dict with no poses whose features are the rows of x [n, 3] -- the call reads the sizes and the estimates alone."""
    x = np.ascontiguousarray(x, np.float64).reshape(-1, 3)
    n = len(x)
    e = np.zeros(0)
    i = np.zeros(0, np.int32)
    return dict(Ref=0, FRef=0, m=0, n=n, stno=np.repeat(np.arange(first_label, first_label + n, dtype=np.int32), 3), stVal=x.ravel().copy(),
                U=e, Ui=i, Uj=i, W=e, photo=i, feature=i, V=np.zeros(9 * n), FBlock=np.zeros(n, np.int32))


def features_of(d):
    return np.asarray(d["stVal"], np.float64)[6 * int(d["m"]):].reshape(-1, 3)


def _all_pairs(n):
    f, g = np.triu_indices(n, 1)
    return f.astype(np.int64), g.astype(np.int64)


def _dist2(x, f, g):
    d = x[f] - x[g]
    return d, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def bound_q(d, cov_f, cov_g):
    """(q, bad) for the rows of d [K, 3] and the blocks cov_f, cov_g [K, 3, 3]: the upper triangle of the sum, LDL^T, q = 1/2 d^T M^-1 d;
    bad where a pivot is not > 0 (q is NaN there)."""
    M = np.asarray(cov_f, np.float64) + np.asarray(cov_g, np.float64)
    with np.errstate(all="ignore"):
        m00, m01, m02, m11, m12, m22 = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]
        d0 = m00
        l10, l20 = m01 / d0, m02 / d0
        d1 = m11 - l10 * m01
        t = m12 - l20 * m01
        l21 = t / d1
        d2 = m22 - l20 * m02 - l21 * t
        y0 = d[:, 0]
        y1 = d[:, 1] - l10 * y0
        y2 = d[:, 2] - l20 * y0 - l21 * y1
        q = 0.5 * (y0 * y0 / d0 + y1 * y1 / d1 + y2 * y2 / d2)
        bad = ~((d0 > 0) & (d1 > 0) & (d2 > 0))
    return np.where(bad, np.nan, q), bad


def candidates(x, radius, feat_cov=None, tau=None, chunk=2_000_000):
    """dict(pairs [K, 2] int32 sorted by (f, g), dist2 [K], q [K] or None) over all pairs of the rows of x."""
    x = np.ascontiguousarray(x, np.float64).reshape(-1, 3)
    n = len(x)
    r2 = float(radius) * float(radius)
    F, G = _all_pairs(n)
    P, D, Q = [], [], []
    for a in range(0, len(F), chunk):
        f, g = F[a: a + chunk], G[a: a + chunk]
        d, d2 = _dist2(x, f, g)
        k = d2 <= r2
        f, g, d, d2 = f[k], g[k], d[k], d2[k]
        if feat_cov is not None:
            C = np.asarray(feat_cov, np.float64).reshape(-1, 3, 3)
            q, bad = bound_q(d, C[f], C[g])
            with np.errstate(invalid="ignore"):
                k = bad | (q <= tau)
            f, g, d2, q = f[k], g[k], d2[k], q[k]
            Q.append(q)
        P.append(np.stack([f, g], axis=1))
        D.append(d2)
    pairs = np.concatenate(P).astype(np.int32) if P else np.zeros((0, 2), np.int32)
    return dict(pairs=pairs.reshape(-1, 2), dist2=np.concatenate(D) if D else np.zeros(0), q=(np.concatenate(Q) if Q else np.zeros(0)) if feat_cov is not None else None)


def margin(x, radius, feat_cov=None, tau=None, rel=REL):
    """The pairs [K, 2] within `rel` relative of radius^2, or -- among those inside the radius, with feat_cov -- of tau."""
    x = np.ascontiguousarray(x, np.float64).reshape(-1, 3)
    r2 = float(radius) * float(radius)
    f, g = _all_pairs(len(x))
    d, d2 = _dist2(x, f, g)
    near = np.abs(d2 - r2) <= rel * r2
    if feat_cov is not None:
        C = np.asarray(feat_cov, np.float64).reshape(-1, 3, 3)
        q, bad = bound_q(d, C[f], C[g])
        with np.errstate(invalid="ignore"):
            near |= (d2 <= r2) & ~bad & (np.abs(q - tau) <= rel * tau)
    return np.stack([f[near], g[near]], axis=1)


def all_q(x, feat_cov):
    """(f, g, q, bad) over ALL pairs: what the bound q <= d^2 is checked on."""
    x = np.ascontiguousarray(x, np.float64).reshape(-1, 3)
    f, g = _all_pairs(len(x))
    d = x[f] - x[g]
    C = np.asarray(feat_cov, np.float64).reshape(-1, 3, 3)
    q, bad = bound_q(d, C[f], C[g])
    return f, g, q, bad


def gate_d2(Sig, m, x, f, g):
    """The exact gate on a dense Sigma [6 m + 3 n]^2: d^T Var(x_f - x_g)^-1 d for the pairs (f[k], g[k])."""
    out = np.zeros(len(f))
    for k, (a, b) in enumerate(zip(f, g)):
        ia, ib = 6 * m + 3 * int(a), 6 * m + 3 * int(b)
        Sd = Sig[ia: ia + 3, ia: ia + 3] + Sig[ib: ib + 3, ib: ib + 3] - Sig[ia: ia + 3, ib: ib + 3] - Sig[ib: ib + 3, ia: ia + 3]
        d = x[a] - x[b]
        out[k] = d @ np.linalg.solve(Sd, d)
    return out
