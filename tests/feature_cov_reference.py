"""Host statements of the feature-pair gate (lsfm_map_feature_pair_gate), plain numpy / LAPACK, no GPU:
    Sigma_d = Var(x_f - x_g) = Sigma_ff + Sigma_gg - Sigma_fg - Sigma_gf,   d^2 = (x_f - x_g)^T Sigma_d^-1 (x_f - x_g)
Route A reads the blocks off a dense inverse of the whole information matrix (test_gpu_covariance.dense_sigma).  Route B is the
difference formulation the device uses: B = -(W_f V_f^-1 - W_g V_g^-1), X = S^-1 B by a Cholesky factor of S with one refinement step,
Sigma_d = V_f^-1 + V_g^-1 + B^T X -- a sum of positive semi-definite terms.  The bars of the GPU tests are derived here as well."""
import numpy as np
import scipy.linalg as sla

from test_gpu_covariance import _fixed, _sparse_parts

BAR = 1e-9       # the project's flat bar on |dSigma_ij| / sqrt(v_i v_j)
N_PAIRS = 200
BAR_D2_CAP = 1e-3  # no tested pair's derived d^2 bar may exceed this: the bar must not become vacuous


def seeded_pairs(n, count=N_PAIRS, seed=1):
    """count pairs (f, g), f != g, of n features from default_rng(seed); every pair f < g where there are no more than count."""
    if n * (n - 1) // 2 <= count:
        return np.array([(f, g) for f in range(n) for g in range(f + 1, n)], np.int32).reshape(-1, 2)
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(n, size=2, replace=False) for _ in range(count)]).astype(np.int32)


def state_diff(G, pairs):
    m = int(G["m"])
    x = np.asarray(G["stVal"], np.float64)[6 * m:].reshape(-1, 3)
    return x[pairs[:, 0]] - x[pairs[:, 1]]


def d2_of(cov, dx):
    return np.array([float(d @ np.linalg.solve(c, d)) for c, d in zip(cov, dx)])


def symmetric_blocks(G):
    """G with its diagonal U blocks and its V blocks replaced by (X + X^T) / 2.  An information matrix is symmetric; a tree stores
    these blocks symmetric to rounding only (the oracle's 40-map Mono tree: 1.2e-12 of sqrt(I_ii I_jj)), and kappa(I) carries that into
    Sigma: there the exact inverse of the matrix as stored and the exact inverse of its symmetric part differ by 1.0e-10 of the
    variances, and the first is itself 2e-10 from symmetric.  A general inverse (route A) follows the one, a Cholesky factor (route B)
    the other, so two host routes can only be compared on a symmetric input."""
    d = dict(G)
    U = np.array(G["U"], np.float64).reshape(-1, 6, 6)
    diag = np.asarray(G["Ui"]) == np.asarray(G["Uj"])
    U[diag] = 0.5 * (U[diag] + np.transpose(U[diag], (0, 2, 1)))
    V = np.array(G["V"], np.float64).reshape(-1, 3, 3)
    d["U"], d["V"] = U.reshape(-1, 36), (0.5 * (V + np.transpose(V, (0, 2, 1)))).reshape(-1, 9)
    return d


def route_a(Sig, G, pairs):
    """From the dense Sigma: (Sigma_d [K,3,3], Sigma_ff + Sigma_gg [K,3,3])."""
    o = 6 * int(G["m"])
    blk = lambda a, b: Sig[o + 3 * a: o + 3 * a + 3, o + 3 * b: o + 3 * b + 3]
    marg = np.stack([blk(f, f) + blk(g, g) for f, g in pairs])
    cross = np.stack([blk(f, g) + blk(g, f) for f, g in pairs])
    return marg - cross, marg


def route_b(G, mono, pairs):
    """The difference formulation with LAPACK and one refinement step: Sigma_d [K,3,3]."""
    Usp, Wsp, _, IVsp, IV = _sparse_parts(G)
    keep = ~_fixed(G, mono)
    S = (Usp - Wsp @ IVsp @ Wsp.T).toarray()[np.ix_(keep, keep)]
    WIV = (Wsp @ IVsp).toarray()[keep]  # column block h: W_h V_h^-1
    K = len(pairs)
    B = np.zeros((S.shape[0], 3 * K))
    for a, (f, g) in enumerate(pairs):
        B[:, 3 * a: 3 * a + 3] = -(WIV[:, 3 * f: 3 * f + 3] - WIV[:, 3 * g: 3 * g + 3])
    cf = sla.cho_factor(S)
    X = sla.cho_solve(cf, B)
    X += sla.cho_solve(cf, B - S @ X)
    out = np.zeros((K, 3, 3))
    for a, (f, g) in enumerate(pairs):
        c = IV[f] + IV[g] + B[:, 3 * a: 3 * a + 3].T @ X[:, 3 * a: 3 * a + 3]
        out[a] = 0.5 * (c + c.T)
    return out


def cov_err(got, exp, diag):
    """max |got - exp|_ij / sqrt(diag_i diag_j) over blocks [K,3,3] with the normalising variances diag [K,3]."""
    den = np.sqrt(diag[:, :, None] * diag[:, None, :])
    return float(np.max(np.abs(got - exp) / den)) if len(got) else 0.0


def d2_bars(cov_ref, marg):
    """Per pair the bar on |d2 - d2_ref| / d2_ref that follows to first order from the bar BAR on Sigma_d normalised by diag(Sigma_ff +
    Sigma_gg): with D = diag(Sigma_d)^1/2 and C = D^-1 Sigma_d D^-1, an error E with |E_ij| <= BAR sqrt(m_i m_j) is |D^-1 E D^-1|_ij <=
    BAR rho, |.|_2 <= 3 BAR rho, and d2 = y^T C^-1 y moves by at most kappa(C) |D^-1 E D^-1|_2 relative: 3 kappa_c rho BAR."""
    bars = np.zeros(len(cov_ref))
    for a, (c, mg) in enumerate(zip(cov_ref, marg)):
        d = np.sqrt(np.diag(c))
        kc = np.linalg.cond(c / np.outer(d, d))
        rho = float(np.max(np.diag(mg) / np.diag(c)))
        bars[a] = 3.0 * kc * rho * BAR
    return bars


def split_block(G, f):
    """G with the first W block of feature f stored as two adjacent halves (a repeated (pose, feature) block, as a join leaves them)."""
    fe = np.asarray(G["feature"])
    w = int(np.nonzero(fe == f)[0][0])
    W = np.asarray(G["W"], np.float64).reshape(-1, 18)
    d = dict(G)
    d["W"] = np.concatenate([W[:w], 0.5 * W[w: w + 1], 0.5 * W[w: w + 1], W[w + 1:]]).reshape(-1)
    d["photo"] = np.insert(np.asarray(G["photo"]), w, np.asarray(G["photo"])[w]).astype(np.int32)
    d["feature"] = np.insert(fe, w, f).astype(np.int32)
    d["FBlock"] = np.searchsorted(d["feature"], np.arange(int(G["n"]))).astype(np.int32)  # first W index of each feature
    d["nW"] = len(d["photo"])
    return d
