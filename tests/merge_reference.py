"""Host statements of lsfm_map_merge_features, plain numpy / LAPACK, no GPU.  Declaring x_f = x_g for pairs of features of a joined map
(x^, I) is the linear constraint A x = 0; with x = T y:
    route A (merged_dense): the constraint form on the dense Sigma = I^-1 (test_gpu_covariance.dense_sigma): C = A Sigma A^T, d = A x^,
             y^ = (x^ - Sigma A^T C^-1 d) at the representatives, D^2 = d^T C^-1 d, Sigma_c = Sigma - Sigma A^T C^-1 A Sigma
    route B (route_b): the device's formulation -- the merged map I' = T^T I T, its Schur system with a LAPACK Cholesky factor and one
             refinement step, D^2 = sum_g r_g^T V_g r_g - eta^T delta
merged_blocks states V', W' and the index arrays with the device's own order of additions: they are compared bit for bit."""
import numpy as np
import scipy.linalg as sla

from test_gpu_covariance import _diag, _feat_blocks, _fixed, _norm_err, _pose_blocks, _sparse_parts

BAR = 1e-9        # the project's flat bar
CAP = 1e-3        # BAR times the cancellation factor of D^2 may not exceed this on any tested case
SPLIT_OFFSET = 100000


def classes(n, pairs):
    """The partition of n features by the pairs [K, 2]: connected components of the pair graph.  Returns (rep [n]: the output feature
    of every input feature, members: per output feature its members ascending).  A class's representative is its smallest member;
    output feature c is the c-th representative in ascending order."""
    root = list(range(n))

    def find(f):
        while root[f] != f:
            root[f] = root[root[f]]
            f = root[f]
        return f
    for f, g in np.asarray(pairs, np.int64).reshape(-1, 2):
        a, b = find(int(f)), find(int(g))
        if a != b:
            root[max(a, b)] = min(a, b)
    roots = [find(f) for f in range(n)]
    order = {r: c for c, r in enumerate(sorted(set(roots)))}
    rep = np.array([order[r] for r in roots], np.int32)
    members = [[] for _ in order]
    for f in range(n):
        members[rep[f]].append(f)
    return rep, members


def feature_ids(d):
    m = int(d["m"])
    return np.asarray(d["stno"])[6 * m:: 3]


def split_candidates(dicts):
    """(the ids of the features held by >= 2 local maps, ascending; per id the maps that hold it, in map order)."""
    holders = {}
    for k, d in enumerate(dicts):
        for i in feature_ids(d):
            holders.setdefault(int(i), []).append(k)
    return sorted(i for i, hs in holders.items() if len(hs) >= 2), holders


def split_set(dicts, count, seed=3):
    """The local map dicts with `count` features split in two: candidates are the features held by >= 2 local maps, sorted by id;
    default_rng(seed).choice picks `count` of them without replacement; from the middle holder on (holders[len // 2:]) a chosen
    feature carries the label id + SPLIT_OFFSET.  Returns (dicts, the chosen ids ascending)."""
    cands, holders = split_candidates(dicts)
    assert len(cands) >= count, (len(cands), count)
    chosen = sorted(int(i) for i in np.random.default_rng(seed).choice(cands, size=count, replace=False))
    out = [dict(d) for d in dicts]
    for d in out:
        d["stno"] = np.array(d["stno"], np.int32, copy=True)
    for i in chosen:
        hs = holders[i]
        for k in hs[len(hs) // 2:]:
            st, m = out[k]["stno"], int(out[k]["m"])
            st[6 * m:][st[6 * m:] == i] = i + SPLIT_OFFSET
    return out, chosen


def split_pairs(G, chosen):
    """The pairs (index of id, index of id + SPLIT_OFFSET) in the joined map G of a split set."""
    at = {int(i): f for f, i in enumerate(feature_ids(G))}
    return np.array([(at[i], at[i + SPLIT_OFFSET]) for i in chosen], np.int32).reshape(-1, 2)


def expansion(m, n, rep):
    """T [(6 m + 3 n), (6 m + 3 n')]: x = T y."""
    no = int(rep.max()) + 1 if n else 0
    T = np.zeros((6 * m + 3 * n, 6 * m + 3 * no))
    T[: 6 * m, : 6 * m] = np.eye(6 * m)
    for f in range(n):
        T[6 * m + 3 * f: 6 * m + 3 * f + 3, 6 * m + 3 * rep[f]: 6 * m + 3 * rep[f] + 3] = np.eye(3)
    return T


def kept_scalars(m, members):
    """Indices into x of the scalars of y: the poses, then every class's representative."""
    return np.concatenate([np.arange(6 * m)] + [6 * m + 3 * c[0] + np.arange(3) for c in members]).astype(np.int64)


def quad_term(G, members):
    """sum_g r_g^T V_g r_g over the merged-away features: the minuend of the device's D^2."""
    m = int(G["m"])
    x = np.asarray(G["stVal"], np.float64)[6 * m:].reshape(-1, 3)
    V = np.asarray(G["V"], np.float64).reshape(-1, 3, 3)
    return float(sum((x[g] - x[c[0]]) @ V[g] @ (x[g] - x[c[0]]) for c in members for g in c[1:]))


def merged_dense(G, mono, pairs, Sig=None):
    """Route A on Sig = dense_sigma(G, mono) (computed here unless the caller shares one): dict(T, I1 = T^T I T, y, d2, Sigma_c (in y's numbering), dof, c = quad_term / d2)."""
    import scipy.sparse as sp
    from test_gpu_covariance import dense_sigma
    if Sig is None:
        Sig = dense_sigma(G, mono)
    m, n = int(G["m"]), int(G["n"])
    rep, members = classes(n, pairs)
    Usp, Wsp, Vsp, _, _ = _sparse_parts(G)
    I = sp.bmat([[Usp, Wsp], [Wsp.T, Vsp]]).toarray()
    T = expansion(m, n, rep)
    x = np.asarray(G["stVal"], np.float64)
    away = [(g, c[0]) for c in members for g in c[1:]]
    A = np.zeros((3 * len(away), len(x)))
    for a, (g, r) in enumerate(away):
        A[3 * a: 3 * a + 3, 6 * m + 3 * g: 6 * m + 3 * g + 3] = np.eye(3)
        A[3 * a: 3 * a + 3, 6 * m + 3 * r: 6 * m + 3 * r + 3] = -np.eye(3)
    d = A @ x
    SA = Sig @ A.T
    C = A @ SA
    C = 0.5 * (C + C.T)
    cf = sla.cho_factor(C)
    kept = kept_scalars(m, members)
    y = (x - SA @ sla.cho_solve(cf, d))[kept]
    d2 = float(d @ sla.cho_solve(cf, d))
    Sc = (Sig - SA @ sla.cho_solve(cf, SA.T))[np.ix_(kept, kept)]
    return dict(T=T, I1=T.T @ I @ T, y=y, d2=d2, Sigma_c=Sc, dof=3 * len(away), c=quad_term(G, members) / d2, rep=rep, members=members)


def merged_blocks(G, pairs):
    """The merged map at y0 (every class at its representative's estimate) with the device's order of additions: V'_c = its members'
    V in ascending order, added one after the other; a class of one keeps its W run as it stands; a larger class has one block per
    pose, ascending, the sum of its sources by (member, position in the input).  Returns (map dict, rep, sptr, sidx)."""
    m, n = int(G["m"]), int(G["n"])
    rep, members = classes(n, pairs)
    fe, ph = np.asarray(G["feature"]), np.asarray(G["photo"])
    fptr = np.searchsorted(fe, np.arange(n + 1))
    W = np.asarray(G["W"], np.float64).reshape(-1, 18)
    V = np.asarray(G["V"], np.float64).reshape(-1, 9)
    st, x = np.asarray(G["stno"]), np.asarray(G["stVal"], np.float64)
    oV, oW, ophoto, ofeat, FBlock, sptr, sidx = [], [], [], [], [], [0], []
    for c, mem in enumerate(members):
        v = V[mem[0]].copy()
        for g in mem[1:]:
            v = v + V[g]
        oV.append(v)
        FBlock.append(len(ophoto))
        blocks = [w for g in mem for w in range(fptr[g], fptr[g + 1])]
        if len(mem) == 1:
            groups = [[w] for w in blocks]
        else:
            blocks.sort(key=lambda w: ph[w])  # (stable: (member, position) inside a pose)
            groups = []
            for w in blocks:
                if groups and ph[groups[-1][0]] == ph[w]:
                    groups[-1].append(w)
                else:
                    groups.append([w])
        for grp in groups:
            acc = W[grp[0]].copy()
            for w in grp[1:]:
                acc = acc + W[w]
            oW.append(acc); ophoto.append(int(ph[grp[0]])); ofeat.append(c)
            sidx += grp; sptr.append(len(sidx))
    reps = np.array([mem[0] for mem in members], np.int64)
    d = dict(G)
    d["n"], d["nW"] = len(members), len(ophoto)
    d["stno"] = np.concatenate([st[: 6 * m], st[6 * m:].reshape(-1, 3)[reps].reshape(-1)]).astype(np.int32)
    d["stVal"] = np.concatenate([x[: 6 * m], x[6 * m:].reshape(-1, 3)[reps].reshape(-1)])
    d["W"] = np.array(oW).reshape(-1, 18)
    d["V"] = np.array(oV).reshape(-1, 9)
    d["photo"], d["feature"], d["FBlock"] = np.array(ophoto, np.int32), np.array(ofeat, np.int32), np.array(FBlock, np.int32)
    return d, rep, np.array(sptr, np.int32), np.array(sidx, np.int32)


def route_b(G, mono, pairs):
    """The device's formulation with LAPACK: (merged map dict at y^, y^, D^2)."""
    m, n = int(G["m"]), int(G["n"])
    Gm, rep, _, _ = merged_blocks(G, pairs)
    _, members = classes(n, pairs)
    no = len(members)
    x = np.asarray(G["stVal"], np.float64)[6 * m:].reshape(-1, 3)
    V = np.asarray(G["V"], np.float64).reshape(-1, 3, 3)
    _, Wsp, _, _, _ = _sparse_parts(G)
    r = np.zeros((n, 3))
    eta_c = np.zeros((no, 3))
    for c, mem in enumerate(members):
        for g in mem[1:]:
            r[g] = x[g] - x[mem[0]]
            eta_c[c] += V[g] @ r[g]
    eta_p = Wsp @ r.reshape(-1)
    U1, W1, _, IV1sp, IV1 = _sparse_parts(Gm)
    keep = ~_fixed(Gm, mono)
    S = (U1 - W1 @ IV1sp @ W1.T).toarray()[np.ix_(keep, keep)]
    B = (eta_p - W1 @ (IV1sp @ eta_c.reshape(-1)))[keep]
    cf = sla.cho_factor(S)
    dp = sla.cho_solve(cf, B)
    dp += sla.cho_solve(cf, B - S @ dp)
    dpf = np.zeros(6 * m)
    dpf[keep] = dp
    dc = IV1sp @ (eta_c.reshape(-1) - W1.T @ dpf)
    y = np.asarray(Gm["stVal"], np.float64) + np.concatenate([dpf, dc])
    d2 = quad_term(G, members) - float(eta_p[keep] @ dp + eta_c.reshape(-1) @ dc)
    Gm = dict(Gm)
    Gm["stVal"] = y
    return Gm, y, d2


def state_err(y, y_ref, Sig, kept, d2_ref):
    """max |y_i - y_ref,i| / (sigma_i max(1, sqrt(D^2_ref))), sigma_i^2 = Sigma_ii of the UNMERGED map: Cauchy-Schwarz bounds the move of
    scalar i by sigma_i sqrt(D^2), so this is the error relative to what the merge can move.  Gauge scalars (sigma = 0) are left out:
    they are compared bit for bit."""
    sig = np.sqrt(np.diag(Sig)[kept])
    on = sig > 0
    return float(np.max(np.abs(y - y_ref)[on] / (sig[on] * max(1.0, np.sqrt(d2_ref)))))


def sigma_err(pose, feat, Sigma_c, Sig, kept, m, no):
    """The pose blocks [m,6,6] and feature blocks [n',3,3] of a merged map's covariance against those of Sigma_c (route A, in y's
    numbering), metric of test_gpu_covariance._norm_err with the variances of the UNMERGED map at the kept scalars.  Sigma_c = Sigma -
    Sigma A^T C^-1 A Sigma is a difference of two terms of the unmerged size -- merging unrelated features shrinks a variance by orders
    of magnitude --, so its rounding error is relative to Sigma_ii, not to its own diagonal: measured on the seeded pairs of the Mono
    sets, the two host routes are 8.4e-10 apart in units of diag(Sigma_c) and 9.9e-12 in units of diag(Sigma).  (The merged map's own
    covariance in its own units is test_gpu_covariance's subject: the GPU tests check `out` that way as well.)"""
    var = np.diag(Sig)[kept]
    vP, vF = var[: 6 * m].reshape(m, 6), var[6 * m:].reshape(no, 3)
    Pc, Fc = _pose_blocks(Sigma_c, m), _feat_blocks(Sigma_c, m, no)
    return max(_norm_err(pose, Pc, vP, vP), _norm_err(feat, Fc, vF, vF))
