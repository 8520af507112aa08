"""-m gpu: lsfm_map_marginalise_poses (csrc/lsfm_marg_poses.hip) -- poses marginalised out of a map on the device, after the features
that go with them: U'_KK = U1_KK - U1_KD U1_DD^-1 U1_DK, formed as Y^T Y from a forward sweep against the factor of U1_DD.  No reference
counterpart.

Metric everywhere: |d_ij| / sqrt(I_ii I_jj), I the INPUT map's diagonal; bar 1e-9, the project's bar for assembled blocks; rows and
columns with I_ii = 0 (the gauge scalars of a Mono map) exactly zero.
Yardsticks (tests/test_marginalise_poses_cpu.py has their own floors): on the six small sets stage A feature by feature as
test_gpu_marginalise.expected_info does, then long double elimination of the dropped poses; on the larger maps stage A is
Context.marginalise with the same flags (tested on its own) and the poses go by LAPACK Y^T Y on its result, which the CPU file holds to
4.1e-14 of the long double elimination.

Measured on an MI355X (pytest -s prints every figure): the six sets worst per set 6.5e-16, 2.5e-15, 2.9e-14 (Stereo 2 / 9 / 40 maps) and
1.2e-14, 4.1e-12, 1.2e-10 (Mono; the last is the 40-map spiral with the first half kept, kappa of the scaled U1_DD 6e5); the chain
4.0e-16; mono200 first half kept 3.4e-10 and 4.1e-10 in two runs (the sweeps add with atomics); stereo512 every 8th kept 1.8e-12 and
3.5e-12; the 33 boundary poses 1.9e-16; the covariances of the reduced map <= 5.9e-10."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.linalg

from linearsfm_amd import api
from refdump import dense_info
from test_gpu_covariance import LARGE, _tree_map
from test_gpu_linearise import COV_SETS, IDS, SETS, _dense_sigma, _sigma_err
from test_gpu_marginalise import _case, info_err, kept_index
from test_marginalise_poses_cpu import (chain_case, chain_map, eliminate_longdouble, gauge_poses, label_structure, pose_masks, pose_scalars, refusals,
                                        seen_by_dropped, stage_a)

pytestmark = pytest.mark.gpu
BAR = 1e-9
NOT_SPD, ERR_ARG = -7, -1


# ---- yardsticks -----------------------------------------------------------------------------------------------------------------------
def kept_rows(m, n, keep, drop):
    """Positions, in the input's state vector, of the reduced map's variables."""
    kp, kf = np.nonzero(keep)[0], np.nonzero(~np.asarray(drop, bool))[0]
    return np.concatenate([pose_scalars(kp), (6 * m + 3 * kf[:, None] + np.arange(3)).reshape(-1)]).astype(np.int64)


def expected_small(I, m, n, keep, drop):
    """Stage A feature by feature, then the dropped poses eliminated in long double: the reduced map's dense matrix."""
    E = stage_a(I, m, n, drop)
    return np.asarray(eliminate_longdouble(E, pose_scalars(np.nonzero(~keep)[0])), np.float64)


def check_small(ctx, G, I, mono, keep, drop_feat, what):
    m, n = int(G["m"]), int(G["n"])
    drop = seen_by_dropped(G, keep) if drop_feat is None else drop_feat
    out, info = ctx.marginalise_poses(G, mono, keep, drop_feat, info=True)
    assert out["m"] == int(np.sum(keep)) and out["n"] == n - int(np.sum(drop)) and info["dropped"] == int(np.sum(~keep))
    e = info_err(dense_info(out), expected_small(I, m, n, keep, drop), np.diag(I)[kept_rows(m, n, keep, drop)])
    print(f"{what}: |D| {info['dropped']} |Bd| {info['boundary']} components {info['components']} blocks {info['blocks']} chunks {info['chunks']}, "
          f"{int(np.sum(drop))} of {n} features dropped, U' error {e:.3e}")
    assert e <= BAR
    return out, info


def dense_u(d):
    """The pose part of the information matrix, dense and symmetric (duplicates summed)."""
    m = int(d["m"])
    P = np.zeros((6 * m, 6 * m))
    U = np.asarray(d["U"]).reshape(-1, 6, 6)
    for k, (a, b) in enumerate(zip(d["Ui"], d["Uj"])):
        P[6 * a:6 * a + 6, 6 * b:6 * b + 6] += U[k]
        if a != b:
            P[6 * b:6 * b + 6, 6 * a:6 * a + 6] += U[k].T
    return P


def yty(P, D, K):
    """LAPACK: P_KK - Y^T Y, Y = L^-1 D^-1/2 P_DK, L L^T = D^-1/2 P_DD D^-1/2 (powers of two).  P is read from its upper triangle, as the
    library reads a map's diagonal blocks (stage A leaves their two triangles different in the last bits)."""
    P = np.triu(P) + np.triu(P, 1).T
    A, B = P[np.ix_(D, D)], P[np.ix_(D, K)]
    s = 2.0 ** -np.round(0.5 * np.log2(np.diag(A)))
    L = np.linalg.cholesky(A * np.outer(s, s))
    Y = scipy.linalg.solve_triangular(L, B * s[:, None], lower=True)
    return P[np.ix_(K, K)] - Y.T @ Y


def check_large(ctx, G, mono, keep, what):
    """Cases 3-5: stage A = Context.marginalise with the same flags, the poses by LAPACK Y^T Y on its result."""
    m = int(G["m"])
    drop = seen_by_dropped(G, keep)
    A = ctx.marginalise(G, drop)
    out, info = ctx.marginalise_poses(G, mono, keep, info=True)
    D, K = pose_scalars(np.nonzero(~keep)[0]), pose_scalars(np.nonzero(keep)[0])
    Ui, Uj, U = np.asarray(G["Ui"]), np.asarray(G["Uj"]), np.asarray(G["U"]).reshape(-1, 6, 6)
    dg = np.zeros((m, 6))
    np.add.at(dg, Ui[Ui == Uj], np.einsum("kii->ki", U[Ui == Uj]))  # the INPUT's diagonal
    diag = dg.reshape(-1)[K]
    e = info_err(dense_u(out), yty(dense_u(A), D, K), diag)
    # the features are stage A's, the poses of their blocks renumbered
    new = np.cumsum(keep) - 1
    for k in ("W", "V", "feature", "FBlock"):
        assert np.array_equal(out[k], A[k]), k
    assert np.array_equal(out["photo"], new[np.asarray(A["photo"])])
    print(f"{what}: m {m} |D| {info['dropped']} |Bd| {info['boundary']} components {info['components']} blocks {info['blocks']} chunks {info['chunks']} "
          f"leaf tasks {info['leaf_tasks']} groups {info['groups']} levels {info['group_levels']}, U' error {e:.3e}")
    assert e <= BAR
    return out, info


# ---- 1. values on the six sets ------------------------------------------------------------------------------------------------------------
def small_masks(G, mono):
    m, n = int(G["m"]), int(G["n"])
    out = [(k, v, None) for k, v in pose_masks(G, mono).items()]
    g = gauge_poses(G, mono)
    only = np.zeros(m, bool)
    only[g if g else [0]] = True  # (a Stereo state holds no gauge pose: its first pose stands in)
    out.append(("gauge", only, None))
    keep = pose_masks(G, mono)["third"]
    fl = seen_by_dropped(G, keep)
    fl[::4] = True
    out.append(("third+features", keep, fl))
    return out


@pytest.mark.parametrize("i", range(len(SETS)), ids=IDS)
def test_values_against_long_double(ctx, oracle, i):
    c = _case(oracle, i)
    seen_r = set()
    for name, keep, fl in small_masks(c["G"], c["mono"]):
        _, info = check_small(ctx, c["G"], c["I"], c["mono"], keep, fl, f"{IDS[i]} {name}")
        seen_r.add(6 * info["boundary"] % 16)
        if name == "one":
            assert info["dropped"] == 1   # 6 |D| = 6: one whole step of four rows and the K tail
        if name == "none":
            assert info["dropped"] == 0 and info["chunks"] == 0
    if i in (2, 5):
        assert len(seen_r) >= 3  # R = 6 |Bd| with several remainders by 16: partial column tiles


# ---- 2. the chain -----------------------------------------------------------------------------------------------------------------------------
def test_chain_with_several_components(ctx):
    G, keep = chain_case()
    drop = seen_by_dropped(G, keep)
    _, N, _, _ = label_structure(G, keep, drop)
    assert len(N) >= 3
    _, info = check_small(ctx, G, dense_info(G), False, keep, None, "chain")
    assert info["components"] == len(N)


# ---- 3.-5. more than one chunk ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _large(ctx, name):
    mono, make = LARGE[name]
    return mono, _tree_map(ctx, make(), mono)


def test_mono200_first_half_kept(ctx):
    mono, G = _large(ctx, "mono200")
    _, info = check_large(ctx, G, mono, pose_masks(G, mono)["half"], "mono200 half")
    assert info["chunks"] >= 2


def test_stereo512_every_eighth_kept(ctx):
    mono, G = _large(ctx, "stereo512")
    keep = np.zeros(int(G["m"]), bool)
    keep[::8] = True
    keep[gauge_poses(G, mono)] = True
    _, info = check_large(ctx, G, mono, keep, "stereo512 every 8th")
    assert info["chunks"] >= 2
    assert info["groups"] > 0  # the group sweeps and the panel product ran under this call


def mask_with_33_boundary_poses():
    """chain_map(42): U1 reaches two poses ahead.  Dropped: pose 0 (borders 1, 2), poses 5, 10, .., 35 (four neighbours each, all
    distinct) and pose 40 (borders 38, 39, 41): 2 + 7 * 4 + 3 = 33 boundary poses = one full chunk and one pose."""
    G = chain_map(42, seed=12)
    keep = np.ones(42, bool)
    keep[[0, 40] + list(range(5, 36, 5))] = False
    return G, keep


def test_33_boundary_poses(ctx):
    G, keep = mask_with_33_boundary_poses()
    _, N, bd, _ = label_structure(G, keep, seen_by_dropped(G, keep))
    assert len(bd) == 33 and len(N) == 9
    _, info = check_large(ctx, G, False, keep, "33 boundary poses")
    assert info["boundary"] == 33 and info["chunks"] == 2 and info["components"] == 9
    check_small(ctx, G, dense_info(G), False, keep, None, "33 boundary poses, long double")


# ---- 6. canonical form ---------------------------------------------------------------------------------------------------------------------------
INDEX_ARRAYS = ("stno", "Ui", "Uj", "photo", "feature", "FBlock", "pose_origin")


@pytest.mark.parametrize("i", range(len(SETS)), ids=IDS)
def test_canonical_form(ctx, oracle, i):
    c = _case(oracle, i)
    G, mono, I = c["G"], c["mono"], c["I"]
    m, n = int(G["m"]), int(G["n"])
    # keeping every pose is Context.marginalise
    fl = np.zeros(n, bool)
    fl[1::3] = True
    a, b = ctx.marginalise_poses(G, mono, np.ones(m, bool), fl), ctx.marginalise(G, fl)
    for k in INDEX_ARRAYS + ("stVal", "W", "V"):
        assert np.array_equal(a[k], b[k]), k
    e = info_err(dense_info(a), dense_info(b), np.diag(I)[kept_index(m, n, fl)])
    print(f"{IDS[i]}: every pose kept against Context.marginalise {e:.3e}")
    assert e <= BAR
    # the form, array by array
    for name, keep, fl in small_masks(G, mono):
        drop = seen_by_dropped(G, keep) if fl is None else fl
        out = ctx.marginalise_poses(G, mono, keep, fl)
        A = ctx.marginalise(G, drop)
        idx = kept_rows(m, n, keep, drop)
        assert np.array_equal(out["stno"], np.asarray(G["stno"])[idx]) and np.array_equal(out["stVal"], np.asarray(G["stVal"])[idx])
        assert np.array_equal(out["pose_origin"], np.asarray(G["pose_origin"])[keep])
        for k in ("Ref", "FRef", "ScaP", "Fix", "Sign", "FScaP", "FFix"):
            assert out[k] == G[k], k
        new = np.cumsum(keep) - 1
        for k in ("W", "V", "feature", "FBlock"):
            assert np.array_equal(out[k], A[k]), k
        assert np.array_equal(out["photo"], new[np.asarray(A["photo"])])
        _, _, _, outp = label_structure(G, keep, drop)
        assert list(zip(out["Ui"].tolist(), out["Uj"].tolist())) == outp and out["nU"] == len(outp)
        U = np.asarray(out["U"]).reshape(-1, 6, 6)
        dg = U[out["Ui"] == out["Uj"]]
        assert len(dg) == out["m"] and np.array_equal(dg, dg.transpose(0, 2, 1)), name  # bitwise symmetric


@pytest.mark.parametrize("i", range(len(SETS)), ids=IDS)
def test_dropping_a_then_b_is_dropping_both(ctx, oracle, i):
    c = _case(oracle, i)
    G, mono, I = c["G"], c["mono"], c["I"]
    m, n = int(G["m"]), int(G["n"])
    rng = np.random.default_rng(3)
    g = gauge_poses(G, mono)
    dA = rng.random(m) < 0.3
    dB = ~dA & (rng.random(m) < 0.4)
    dA[g] = dB[g] = False
    if not np.any(~(dA | dB)):
        dA[0] = dB[0] = False
    first = ctx.marginalise_poses(G, mono, ~dA)
    two = ctx.marginalise_poses(first, mono, ~dB[~dA])
    both = ctx.marginalise_poses(G, mono, ~(dA | dB))
    for k in INDEX_ARRAYS:
        assert np.array_equal(two[k], both[k]), k
    keep = ~(dA | dB)
    e = info_err(dense_info(two), dense_info(both), np.diag(I)[kept_rows(m, n, keep, seen_by_dropped(G, keep))])
    print(f"{IDS[i]}: {int(np.sum(dA))} then {int(np.sum(dB))} of {m} poses against both at once {e:.3e}")
    assert e <= BAR


# ---- 7. covariances ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", COV_SETS, ids=[IDS[i] for i in COV_SETS])
def test_covariances_of_the_reduced_map(ctx, oracle, i):
    """Marginalising leaves the covariance of what is kept unchanged: lsfm_map_covariance of the reduced map against the dense inverse of
    the FULL map's information matrix (Mono: gauge removed), kept rows only; section 10's metric and bar."""
    c = _case(oracle, i)
    mono, G = c["mono"], c["G"]
    m, n = int(G["m"]), int(G["n"])
    S = _dense_sigma(c["I"], G, mono)
    var = np.diag(S)
    for name in ("third", "half"):
        keep = pose_masks(G, mono)[name]
        kp, kf = np.nonzero(keep)[0], np.nonzero(~seen_by_dropped(G, keep))[0]
        out = ctx.marginalise_poses(G, mono, keep)
        cov = ctx.covariance(out, mono)
        P = np.stack([S[6 * p:6 * p + 6, 6 * p:6 * p + 6] for p in kp])
        vp = var[:6 * m].reshape(m, 6)[kp]
        ep, ef = _sigma_err(cov["pose"], P, vp, vp), 0.0
        if len(kf):
            Fb = np.stack([S[6 * m + 3 * f:6 * m + 3 * f + 3, 6 * m + 3 * f:6 * m + 3 * f + 3] for f in kf])
            vf = var[6 * m:].reshape(n, 3)[kf]
            ef = _sigma_err(cov["feature"], Fb, vf, vf)
        print(f"{IDS[i]} {name}: {len(kp)} of {m} poses, {len(kf)} of {n} features kept: Sigma error poses {ep:.3e} features {ef:.3e}")
        assert ep <= BAR and ef <= BAR


# ---- 8. statuses -----------------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, d, mono, keep, fl=None):
    h = api.HostMap(d)
    out = api.LsfmMap()
    ub = C.POINTER(C.c_ubyte)
    kp = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    fl = None if fl is None else np.ascontiguousarray(fl, np.uint8)
    rc = api.lib().lsfm_map_marginalise_poses(ctx._h, C.byref(h.c), int(mono), None if kp is None else kp.ctypes.data_as(ub), None if fl is None else fl.ctypes.data_as(ub),
                                              C.byref(out))
    return rc, out


def test_a_dropped_pose_whose_block_is_not_positive_definite(ctx, oracle):
    c = _case(oracle, 1)
    G, mono = c["G"], c["mono"]
    keep = pose_masks(G, mono)["third"]
    p = int(np.nonzero(~keep)[0][1])
    e = int(np.nonzero((np.asarray(G["Ui"]) == p) & (np.asarray(G["Uj"]) == p))[0][0])
    U = np.array(G["U"], copy=True).reshape(-1, 36)
    U[e] = -U[e]
    rc, out = _raw(ctx, dict(G, U=U), mono, keep)
    assert rc == NOT_SPD
    assert out.m == 0 and out.n == 0 and not out.U and not out.stno  # untouched
    check_small(ctx, G, c["I"], mono, keep, None, "after the refused call")  # the context is usable


def test_refusals_through_a_live_context(ctx, oracle):
    for i in (1, 4):
        c = _case(oracle, i)
        G, mono = c["G"], c["mono"]
        for name, keep, fl, say in refusals(G, mono):
            rc, out = _raw(ctx, G, mono, keep, fl)
            assert rc == ERR_ARG and out.m == 0 and not out.U, name
            if keep is not None:
                with pytest.raises(api.LsfmError, match=say.strip()):
                    ctx.marginalise_poses(G, mono, keep, fl)
