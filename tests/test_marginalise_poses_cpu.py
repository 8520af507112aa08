"""No device: the structure of lsfm_map_marginalise_poses (lsfm_marg_pose_structure: flags, connected components of the dropped poses,
their boundaries, the pattern of U') against a union-find written here, its refusals, and -- with numpy alone -- the yardsticks the
bars of tests/test_gpu_marginalise_poses.py are read against.

Yardsticks, in the project's metric |d_ij| / sqrt(I_ii I_jj) with the INPUT's diagonal, on the oracle's tree results of the six sets
of test_gpu_linearise.SETS, stage A (the features) by expected_info, then the dropped poses taken out of U1 in three ways:
  (a) long double elimination, scalar by scalar (the reference of the other two)
  (b) LAPACK fp64, the form the library computes: A = D^-1/2 U1_DD D^-1/2 = L L^T, Y = L^-1 D^-1/2 U1_DK, T = Y^T Y
  (c) U1_KD X with X = U1_DD^-1 U1_DK solved in fp64 and refined with long double residuals until it stops moving
Measured here (worst of the two masks, every third pose kept / first half kept):
                                                        (b) against (a)    (c) against (a)
  stereo2 / stereo9 / stereo40                          <= 2.0e-16         <= 2.7e-16
  mono2 / mono9                                         <= 9.3e-16         <= 1.7e-16
  mono40 (the spiral; kappa of the scaled U1_DD 6e5)    4.1e-14            3.0e-16
(b) is asserted against (a) at 1e-12: that licenses LAPACK Y^T Y as the yardstick on the sets too large for long double.  (c) is
printed, not asserted.  All three take stage A's matrix made exactly symmetric (stage_a): fed the two slightly different triangles
that fp64 leaves, the forms read them differently and (c) lands 1.2e-10 from (a) on mono40 -- a property of the input, not of a form.
With a symmetric input (c), refined to convergence, is as good as (b) on these sets; the library forms Y^T Y because it needs the
forward sweep alone, no refinement loop, and gives exactly symmetric diagonal blocks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from linearsfm_amd import api, synth
from refdump import dense_info
from test_gpu_linearise import IDS, SETS
from test_gpu_marginalise import _case, expected_info, kept_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["lsfm_map_marginalise_poses", "lsfm_map_marginalise_poses_timed", "lsfm_marg_pose_structure"]
ERR_ARG = -1
CHAIN_RUN = 3  # poses per kept / dropped run of the open chain (see chain_case)


# ---- masks ----------------------------------------------------------------------------------------------------------------------------
def gauge_poses(G, mono):
    """Positions of the poses the rules hold: Ref where it is in the state, for Mono ScaP too."""
    ids = -np.asarray(G["stno"])[:6 * int(G["m"]):6]
    want = [int(G["Ref"])] + ([int(G["ScaP"])] if mono else [])
    return [int(p) for w in want for p in np.nonzero(ids == w)[0]]


def pose_masks(G, mono):
    m = int(G["m"])
    g = gauge_poses(G, mono)
    third = np.zeros(m, bool); third[::3] = True
    half = np.zeros(m, bool); half[:(m + 1) // 2] = True
    one = np.ones(m, bool)
    one[[p for p in range(m - 1, -1, -1) if p not in g][0]] = False
    out = {"third": third, "half": half, "one": one, "none": np.ones(m, bool)}
    for k in out.values():
        k[g] = True
    return out


# ---- the structure from labels, by a union-find of the test's own ---------------------------------------------------------------------------
def seen_by_dropped(G, keep):
    fe, ph = np.asarray(G["feature"]), np.asarray(G["photo"])
    drop = np.zeros(int(G["n"]), bool)
    drop[fe[~keep[ph]]] = True
    return drop


def label_structure(G, keep, drop):
    """(comp [m], N(c) as a list of sorted lists, Bd, sorted output pairs in the output's numbering) from labels and flags alone."""
    m = int(G["m"])
    fe, ph = np.asarray(G["feature"]), np.asarray(G["photo"])
    pairs = {(p, p) for p in range(m)} | {(int(min(a, b)), int(max(a, b))) for a, b in zip(G["Ui"], G["Uj"])}
    for f in np.nonzero(drop)[0]:
        ps = np.unique(ph[fe == f])
        pairs.update((int(a), int(b)) for k, a in enumerate(ps) for b in ps[k:])
    par = list(range(m))

    def find(x):
        while par[x] != x:
            x = par[x]
        return x
    for a, b in pairs:
        if not keep[a] and not keep[b]:
            ra, rb = find(a), find(b)
            if ra != rb:
                par[max(ra, rb)] = min(ra, rb)
    comp = np.full(m, -1, np.int64)
    nc = 0
    for p in range(m):
        if not keep[p]:
            r = find(p)
            if r == p:
                comp[p] = nc
                nc += 1
            else:
                comp[p] = comp[r]
    N = [set() for _ in range(nc)]
    for a, b in pairs:
        if keep[a] != keep[b]:
            k, d = (a, b) if keep[a] else (b, a)
            N[comp[d]].add(k)
    N = [sorted(s) for s in N]
    bd = sorted(set().union(*N)) if N else []
    new = np.cumsum(keep) - 1
    outp = {(int(new[a]), int(new[b])) for a, b in pairs if keep[a] and keep[b]}
    for s in N:
        outp.update((int(new[a]), int(new[b])) for k, a in enumerate(s) for b in s[k:])
    return comp, N, bd, sorted(outp)


def check_structure(G, mono, keep, drop_feat=None):
    s = api.marg_pose_structure(G, mono, keep, drop_feat)
    drop = seen_by_dropped(G, keep) if drop_feat is None else np.asarray(drop_feat, bool)
    assert np.array_equal(s["drop"], drop)
    comp, N, bd, outp = label_structure(G, keep, drop)
    assert np.array_equal(s["comp"], comp)
    assert len(s["nptr"]) == len(N) + 1 and s["nptr"][0] == 0
    for c, want in enumerate(N):
        assert s["nidx"][s["nptr"][c]:s["nptr"][c + 1]].tolist() == want, c
    assert s["bd"].tolist() == bd
    assert list(zip(s["Ui"].tolist(), s["Uj"].tolist())) == outp
    assert s["info"][:5].tolist() == [int(np.sum(~keep)), len(bd), len(N), len(outp), sum(len(x) for x in N)]
    return s, N


def test_symbols_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "lsfm.h")).read()
    for name in SYMBOLS:
        assert getattr(api.lib(), name) is not None
        assert name in api.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert callable(getattr(api.Context, "marginalise_poses", None)) and callable(api.marg_pose_structure)


@pytest.mark.parametrize("i", range(len(SETS)), ids=IDS)
def test_structure_against_union_find(oracle, i):
    c = _case(oracle, i)
    G, mono = c["G"], c["mono"]
    for name, keep in pose_masks(G, mono).items():
        s, N = check_structure(G, mono, keep)
        print(f"{IDS[i]} {name}: |D| {s['info'][0]} |Bd| {s['info'][1]} components {s['info'][2]} blocks {s['info'][3]} dropped features {s['info'][5]} of {G['n']}")
    # flags given: the features a dropped pose sees and every fourth one beyond them
    keep = pose_masks(G, mono)["third"]
    fl = seen_by_dropped(G, keep)
    fl[::4] = True
    check_structure(G, mono, keep, fl)


def chain_map(m=27, seed=11):
    """An open Stereo chain made here, from labels: m poses (ids 1..m, the Ref pose not in the state), pose p tied to p + 1 and p + 2 by
    relative-pose terms, two features per triple (p, p + 1, p + 2) seen by its three poses.  I = sum J^T J over those terms plus a prior
    on pose 0: positive definite, angles and positions on different scales.  U has the pairs (p, p), (p, p + 1), (p, p + 2) alone, and
    so has U1 whatever features go."""
    rng = np.random.default_rng(seed)
    trip = [(p, p + 1, p + 2) for p in range(m - 2) for _ in range(2)]
    n = len(trip)
    N = 6 * m + 3 * n
    I = np.zeros((N, N))
    scale = np.array([30.0, 30.0, 30.0, 1.0, 1.0, 1.0])

    def add(cols, rows, sc):
        J = rng.standard_normal((rows, len(cols))) * sc
        I[np.ix_(cols, cols)] += J.T @ J
    for p in range(m):
        for q in (p + 1, p + 2):
            if q < m:
                add(np.r_[6 * p:6 * p + 6, 6 * q:6 * q + 6], 6, np.r_[scale, scale])
    for f, ps in enumerate(trip):
        for p in ps:
            add(np.r_[6 * p:6 * p + 6, 6 * m + 3 * f:6 * m + 3 * f + 3], 3, np.r_[scale, 5.0, 5.0, 5.0])
    I[:6, :6] += np.diag(scale ** 2)
    pairs = [(p, q) for p in range(m) for q in (p, p + 1, p + 2) if q < m]
    photo = np.array([p for ps in trip for p in ps], np.int32)
    feature = np.repeat(np.arange(n), 3).astype(np.int32)
    G = dict(Ref=1000, FRef=1000, ScaP=0, Fix=0, Sign=1, FScaP=0, FFix=0, m=m, n=n,
             stno=np.concatenate([np.repeat(-(np.arange(m) + 1), 6), np.repeat(np.arange(n) + 1, 3)]).astype(np.int32), stVal=rng.standard_normal(N),
             Ui=np.array([a for a, _ in pairs], np.int32), Uj=np.array([b for _, b in pairs], np.int32),
             U=np.stack([I[6 * a:6 * a + 6, 6 * b:6 * b + 6].reshape(36) for a, b in pairs]), photo=photo, feature=feature,
             W=np.stack([I[6 * p:6 * p + 6, 6 * m + 3 * f:6 * m + 3 * f + 3].reshape(18) for p, f in zip(photo, feature)]),
             V=np.stack([I[6 * m + 3 * f:6 * m + 3 * f + 3, 6 * m + 3 * f:6 * m + 3 * f + 3].reshape(9) for f in range(n)]),
             FBlock=np.arange(0, 3 * n, 3).astype(np.int32), pose_origin=(np.arange(m) // 3).astype(np.int32))
    G["nU"], G["nW"] = len(pairs), len(photo)
    return G


def chain_case():
    """chain_map with runs of CHAIN_RUN = 3 kept and 3 dropped poses alternating, a kept run first and last.  U1 reaches two poses ahead,
    so from the labels: every dropped run is a component of its own (the next one is 4 poses away) -- (m / 3 - 1) / 2 = 4 of them; the
    middle pose of an inner kept run is two away from the dropped runs on both sides and borders both; pose 0 is three away from the
    first dropped pose and borders none."""
    G = chain_map()
    m = int(G["m"])
    assert m % (2 * CHAIN_RUN) == CHAIN_RUN
    keep = (np.arange(m) // CHAIN_RUN) % 2 == 0
    return G, keep


def test_open_chain_structure():
    G, keep = chain_case()
    assert np.allclose(dense_info(G), dense_info(G).T) and np.all(np.linalg.eigvalsh(dense_info(G)) > 0)
    s, N = check_structure(G, False, keep)
    m = int(G["m"])
    assert len(N) == (m // CHAIN_RUN - 1) // 2 >= 3
    borders = np.zeros(m, int)
    for x in N:
        borders[x] += 1
    print(f"chain: m {m}, {len(N)} components, |Bd| {len(s['bd'])}, kept poses bordering 0 / 1 / 2 components: "
          f"{int(np.sum(keep & (borders == 0)))} / {int(np.sum(borders == 1))} / {int(np.sum(borders == 2))}")
    assert borders[2 * CHAIN_RUN + 1] == 2  # the middle pose of the second kept run borders two components
    assert keep[0] and borders[0] == 0      # and pose 0 borders none


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _raw_structure(G, mono, keep, drop_feat=None):
    h = api.HostMap(G)
    ub = C.c_ubyte
    kp = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    fl = None if drop_feat is None else np.ascontiguousarray(drop_feat, np.uint8)
    why = C.create_string_buffer(512)
    rc = api.lib().lsfm_marg_pose_structure(C.byref(h.c), int(mono), None if kp is None else kp.ctypes.data_as(C.POINTER(ub)),
                                            None if fl is None else fl.ctypes.data_as(C.POINTER(ub)), None, None, None, None, 0, None, None, None, 0, None, why, len(why))
    return rc, why.value.decode()


def refusals(G, mono):
    """(name, keep_pose, drop_feat, what the message must say) of every call the rules refuse."""
    m, n = int(G["m"]), int(G["n"])
    ids = -np.asarray(G["stno"])[:6 * m:6]
    out = [("null", None, None, "keep_pose")]
    for who in ["Ref"] + (["ScaP"] if mono else []):
        pos = np.nonzero(ids == int(G[who]))[0]
        if len(pos):
            k = np.ones(m, bool)
            k[pos[0]] = False
            out.append((who, k, None, who))
    keep = pose_masks(G, mono)["third"]
    fl = seen_by_dropped(G, keep)
    f = int(np.nonzero(fl)[0][len(np.nonzero(fl)[0]) // 2])
    fl[f] = False
    out.append(("kept feature", keep, fl, f"feature {int(np.asarray(G['stno'])[6 * m + 3 * f])} "))
    return out


@pytest.mark.parametrize("i", [1, 4], ids=[IDS[1], IDS[4]])
def test_refusals_need_no_device(oracle, i):
    c = _case(oracle, i)
    G, mono = c["G"], c["mono"]
    cases = refusals(G, mono)
    assert len(cases) >= (4 if mono else 2)
    for name, keep, fl, say in cases:
        rc, why = _raw_structure(G, mono, keep, fl)
        assert rc == ERR_ARG and say in why, (name, why)
        # the device entry refuses its arguments before it needs a context
        h, out = api.HostMap(G), api.LsfmMap()
        kp = None if keep is None else np.ascontiguousarray(keep, np.uint8)
        assert api.lib().lsfm_map_marginalise_poses(None, C.byref(h.c), int(mono), None if kp is None else kp.ctypes.data_as(C.POINTER(C.c_ubyte)), None, C.byref(out)) == ERR_ARG
        assert out.m == 0 and not out.U


# ---- yardsticks ---------------------------------------------------------------------------------------------------------------------------
def stage_a(I, m, n, drop):
    """Stage A's yardstick: expected_info, the features one by one, [poses, kept features]; made exactly symmetric (W_f V_f^-1 W_f^T in
    fp64 is symmetric only to rounding, and the three forms below read the two triangles differently: on mono40 that alone moves them
    1e-10 apart, the library reads the upper one)."""
    E = expected_info(I, m, n, drop)
    return 0.5 * (E + E.T)


def eliminate_longdouble(E, scalars):
    """E (symmetric, positive definite on `scalars`) with the scalars eliminated one by one in long double; the other rows / columns."""
    P = np.array(E, np.longdouble)
    for s in scalars:
        P -= np.outer(P[:, s], P[s, :]) / P[s, s]
    rest = np.setdiff1d(np.arange(len(E)), scalars)
    return P[np.ix_(rest, rest)]


def _solve_lower(L, B):
    """L^-1 B by forward substitution, row by row in fp64 (what LAPACK's triangular solve does; no pivoting, no inverse)."""
    Y = np.array(B, np.float64)
    for r in range(len(L)):
        Y[r] = (Y[r] - L[r, :r] @ Y[:r]) / L[r, r]
    return Y


def yty(E, D, K):
    """The library's form on LAPACK: T = Y^T Y, Y = L^-1 D^-1/2 E_DK with L L^T = D^-1/2 E_DD D^-1/2 (D^-1/2: powers of two)."""
    A, B = E[np.ix_(D, D)], E[np.ix_(D, K)]
    s = 2.0 ** -np.round(0.5 * np.log2(np.diag(A)))
    L = np.linalg.cholesky(A * np.outer(s, s))
    Y = _solve_lower(L, B * s[:, None])
    out = E[np.ix_(K, K)] - Y.T @ Y
    return out, float(np.linalg.cond(A * np.outer(s, s)))


def solve_refined_then_multiply(E, D, K):
    A, B = E[np.ix_(D, D)], E[np.ix_(D, K)]
    X = np.linalg.solve(A, B)
    Al, Bl = A.astype(np.longdouble), B.astype(np.longdouble)
    for _ in range(5):
        X = X + np.linalg.solve(A, (Bl - Al @ X.astype(np.longdouble)).astype(np.float64))
    return E[np.ix_(K, K)] - E[np.ix_(K, D)] @ X


def metric(got, exp, diag):
    d = np.sqrt(np.where(diag == 0, 1.0, diag))
    return float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(exp, np.float64)) / np.outer(d, d)))


def pose_scalars(poses):
    return (6 * np.asarray(poses, np.int64)[:, None] + np.arange(6)).reshape(-1)


@pytest.mark.parametrize("i", range(len(SETS)), ids=IDS)
def test_yardsticks(oracle, i):
    c = _case(oracle, i)
    G, mono, I = c["G"], c["mono"], c["I"]
    m, n = int(G["m"]), int(G["n"])
    for name in ("third", "half"):
        keep = pose_masks(G, mono)[name]
        drop = seen_by_dropped(G, keep)
        E = stage_a(I, m, n, drop)
        diag = np.diag(I)[kept_index(m, n, drop)]
        D = pose_scalars(np.nonzero(~keep)[0])
        K = np.setdiff1d(np.arange(len(E)), D)
        ref = eliminate_longdouble(E, D)
        b, kappa = yty(E, D, K)
        r = solve_refined_then_multiply(E, D, K)
        eb, er, ebr = metric(b, ref, diag[K]), metric(r, ref, diag[K]), metric(b, r, diag[K])
        print(f"{IDS[i]} {name}: |D| {len(D) // 6} kappa(scaled U1_DD) {kappa:.1e}; Y^T Y against long double {eb:.1e}, refined solve against long double {er:.1e}, "
              f"the two fp64 forms apart {ebr:.1e}")
        assert eb <= 1e-12
