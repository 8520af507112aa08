"""-m gpu: lsfm_map_marginalise and lsfm_tree_export_reduced_* (csrc/lsfm_marg.hip) -- features marginalised out of a map on the
device, U' = U - sum_{f dropped} W_f V_f^-1 W_f^T, as a map in canonical form and as a reduced pack of a resident tree result.  No
reference counterpart: the reference keeps every feature to the end.

Yardstick: numpy on refdump.dense_info, the expected U' formed feature by feature with a 3x3 inverse of each dropped V_f (on the CPU
that evaluation and a long-double one differ by at most 1.7e-12 in the metric below on the six sets; a single dense solve over all the
dropped features is the worse yardstick and is not used).
Metric: |d_ij| / sqrt(I_ii I_jj), I the INPUT map's diagonal -- what K9's fixed-point unit is relative to.  Bar 1e-9, the project's bar
for assembled U / W / V, three decades above the yardstick's own floor.  Rows and columns with I_ii = 0 (the gauge
scalars of a Mono map) must be exactly zero in the result."""
import ctypes as C
import functools

import numpy as np
import pytest

from common import GOLD_WIDE, feat_param_err, golden_system, load_golden, pose_param_err
from linearsfm_amd import api, synth
from refdump import dense_info
from test_gpu_linearise import COV_SETS, IDS, SETS, _dense_sigma, _sigma_err

pytestmark = pytest.mark.gpu
BAR = 1e-9
STATE_BAR = 1e-6  # the project's bar on pose / feature parameters
NOT_SPD, ERR_ARG = -7, -1


# ---- yardstick ------------------------------------------------------------------------------------------------------------------------
def kept_index(m, n, drop):
    keep = np.nonzero(~np.asarray(drop, bool))[0]
    return np.concatenate([np.arange(6 * m), (6 * m + 3 * keep[:, None] + np.arange(3)).reshape(-1)]).astype(np.int64)


def expected_info(I, m, n, drop):
    """The marginal of the dense information matrix I over the dropped features, feature by feature (3x3 inverses)."""
    P = I[:6 * m, :6 * m].copy()
    for f in np.nonzero(np.asarray(drop, bool))[0]:
        r = slice(6 * m + 3 * f, 6 * m + 3 * f + 3)
        Wf = I[:6 * m, r]
        P -= Wf @ np.linalg.inv(I[r, r]) @ Wf.T
    idx = kept_index(m, n, drop)
    E = I[np.ix_(idx, idx)].copy()
    E[:6 * m, :6 * m] = P
    return E


def info_err(got, exp, diag):
    """The metric; rows / columns with a zero input diagonal must be exactly zero in `got`."""
    zero = diag == 0
    assert not np.any(got[zero]) and not np.any(got[:, zero])
    d = np.sqrt(np.where(zero, 1.0, diag))
    return float(np.max(np.abs(got - exp) / np.outer(d, d)))


@functools.lru_cache(maxsize=None)
def _case(oracle, i):
    """Set i of test_gpu_linearise.py: the oracle's tree result (with pose origins added), its dense information matrix.  Shared,
    never changed."""
    mono, n, npf, vis, kw = SETS[i]
    maps = synth.make_mono_set(n, npf, vis, seed=9, **kw) if mono else synth.make_stereo_set(n, npf, vis, seed=9, **kw)
    d = [oracle.localmap_to_dict(x) for x in maps]
    G, _, rc = oracle.divide_conquer(d, mono)
    assert rc == 0
    G = dict(G, pose_origin=(np.arange(int(G["m"])) % len(d)).astype(np.int32))
    return dict(mono=mono, G=G, I=dense_info(G))


def _masks(i, n):
    out = {"half": np.random.default_rng(3).random(n) < 0.5, "all": np.ones(n, bool), "none": np.zeros(n, bool)}
    one = np.zeros(n, bool)
    one[n // 3] = True
    out["one"] = one
    if i in (2, 5):
        t = np.zeros(n, bool)
        t[100:228] = True
        out["tile"] = t
    return out


def _check_against_yardstick(ctx, G, I, drop, what):
    m, n = int(G["m"]), int(G["n"])
    out = ctx.marginalise(G, drop)
    assert out["m"] == m and out["n"] == n - int(np.sum(drop))
    e = info_err(dense_info(out), expected_info(I, m, n, drop), np.diag(I)[kept_index(m, n, drop)])
    print(f"{what}: {int(np.sum(drop))} of {n} features dropped, U' error {e:.3e}")
    assert e <= BAR
    return out


# ---- 1. against the yardstick -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SETS)), ids=IDS)
def test_marginal_against_numpy(ctx, oracle, i):
    c = _case(oracle, i)
    n = int(c["G"]["n"])
    for name, drop in _masks(i, n).items():
        _check_against_yardstick(ctx, c["G"], c["I"], drop, f"{IDS[i]} {name}")


def _wide_map():
    J = golden_system(load_golden(GOLD_WIDE[0]), 0)[0]
    m, n = int(J["m"]), int(J["n"])
    fe = np.asarray(J["feature"])
    stno = np.concatenate([np.repeat(-(np.arange(m) + 1), 6), np.repeat(np.arange(n) + 1, 3)]).astype(np.int32)
    return dict(J, Ref=0, FRef=0, stno=stno, stVal=np.zeros(len(stno)), FBlock=np.searchsorted(fe, np.arange(n)).astype(np.int32))


def test_wide_panel_on_a_compacted_input(ctx):
    """A joint system the reference assembled whose one tile is seen by 48 poses: every second feature dropped, so that a wide panel
    variant of K9 reads runs that the partition pass compacted."""
    assert GOLD_WIDE[0] == "stereo_n48_wide_top1.npz"
    G = _wide_map()
    n = int(G["n"])
    drop = np.zeros(n, bool)
    drop[::2] = True
    _check_against_yardstick(ctx, G, dense_info(G), drop, "stereo_n48_wide")


# ---- 2. canonical form --------------------------------------------------------------------------------------------------------------------
def _pairs_from_labels(G, drop):
    m = int(G["m"])
    P = {(p, p) for p in range(m)}
    P.update((int(min(a, b)), int(max(a, b))) for a, b in zip(G["Ui"], G["Uj"]))
    ph, fe = np.asarray(G["photo"]), np.asarray(G["feature"])
    for f in np.nonzero(drop)[0]:
        ps = np.unique(ph[fe == f])
        P.update((int(a), int(b)) for k, a in enumerate(ps) for b in ps[k:])
    return P


@pytest.mark.parametrize("i", range(len(SETS)), ids=IDS)
def test_canonical_form(ctx, oracle, i):
    c = _case(oracle, i)
    G = c["G"]
    m, n = int(G["m"]), int(G["n"])
    for name, drop in _masks(i, n).items():
        out = ctx.marginalise(G, drop)
        keep = np.nonzero(~drop)[0]
        nk = len(keep)
        assert out["m"] == m and out["n"] == nk and out["nU"] == len(out["Ui"]) and out["nW"] == len(out["photo"])
        for k in ("Ref", "FRef", "ScaP", "Fix", "Sign", "FScaP", "FFix"):
            assert out[k] == G[k], k
        idx = kept_index(m, n, drop)
        assert np.array_equal(out["stno"], np.asarray(G["stno"])[idx]) and np.array_equal(out["stVal"], np.asarray(G["stVal"])[idx])
        assert np.array_equal(out["pose_origin"], G["pose_origin"])
        fe = np.asarray(G["feature"])
        wk = ~drop[fe]
        assert np.array_equal(out["V"], np.asarray(G["V"])[keep])
        assert np.array_equal(out["W"], np.asarray(G["W"])[wk]) and np.array_equal(out["photo"], np.asarray(G["photo"])[wk])
        new = np.cumsum(~drop) - 1
        assert np.array_equal(out["feature"], new[fe[wk]])
        assert np.array_equal(out["FBlock"], np.searchsorted(out["feature"], np.arange(nk)))
        Ui, Uj = out["Ui"].astype(np.int64), out["Uj"].astype(np.int64)
        assert np.all(Ui <= Uj) and np.all(np.diff(Ui * m + Uj) > 0)
        assert set(zip(Ui.tolist(), Uj.tolist())) == _pairs_from_labels(G, drop), name


# ---- 3. composition -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SETS)), ids=IDS)
def test_dropping_a_then_b_is_dropping_both(ctx, oracle, i):
    c = _case(oracle, i)
    G = c["G"]
    m, n = int(G["m"]), int(G["n"])
    rng = np.random.default_rng(3)
    A = rng.random(n) < 0.4
    B = ~A & (rng.random(n) < 0.5)
    first = ctx.marginalise(G, A)
    two = ctx.marginalise(first, B[~A])
    both = ctx.marginalise(G, A | B)
    for k in ("stno", "Ui", "Uj", "photo", "feature", "FBlock", "pose_origin"):
        assert np.array_equal(two[k], both[k]), k
    e = info_err(dense_info(two), dense_info(both), np.diag(c["I"])[kept_index(m, n, A | B)])
    print(f"{IDS[i]}: A then B against A | B {e:.3e}")
    assert e <= BAR


# ---- 4. covariances -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", COV_SETS, ids=[IDS[i] for i in COV_SETS])
def test_covariances_of_the_reduced_map(ctx, oracle, i):
    """Marginalising leaves the covariance of what is kept unchanged: lsfm_map_covariance of the reduced map against the dense inverse
    of the FULL map's information matrix (Mono: gauge removed), kept rows only; section 10's metric and bar."""
    c = _case(oracle, i)
    mono, G = c["mono"], c["G"]
    m, n = int(G["m"]), int(G["n"])
    S = _dense_sigma(c["I"], G, mono)
    var = np.diag(S)
    P = np.stack([S[6 * p:6 * p + 6, 6 * p:6 * p + 6] for p in range(m)])
    vp = var[:6 * m].reshape(m, 6)
    for name, drop in (("half", _masks(i, n)["half"]), ("all", np.ones(n, bool))):
        out = ctx.marginalise(G, drop)
        cov = ctx.covariance(out, mono)
        ep = _sigma_err(cov["pose"], P, vp, vp)
        keep = np.nonzero(~drop)[0]
        ef = 0.0
        if len(keep):
            Fb = np.stack([S[6 * m + 3 * f:6 * m + 3 * f + 3, 6 * m + 3 * f:6 * m + 3 * f + 3] for f in keep])
            vf = var[6 * m:].reshape(n, 3)[keep]
            ef = _sigma_err(cov["feature"], Fb, vf, vf)
        else:
            assert out["n"] == 0 and out["nW"] == 0 and len(cov["feature"]) == 0
            t = ctx.tree_upload([out], mono)  # the pose graph is a map like any other: it uploads, runs (one map: nothing to join) and comes back
            _, rc = ctx.tree_run(t)
            back = ctx.tree_download(t)
            ctx.tree_free(t)
            assert rc == 0 and back["n"] == 0 and np.array_equal(back["Ui"], out["Ui"]) and np.array_equal(back["U"], out["U"])
        print(f"{IDS[i]} {name}: Sigma error poses {ep:.3e} features {ef:.3e}")
        assert ep <= BAR and ef <= BAR


# ---- 5. the use: reduced sub-tree roots -------------------------------------------------------------------------------------------------------
USE = [(False, 8, 4), (False, 32, 8), (True, 8, 4), (True, 32, 8)]
USE_IDS = ["stereo8", "stereo32", "mono8", "mono32"]


def _by_label(full, red):
    """Positions in full's state vector of red's entries (labels are unique in these sets)."""
    fs, rs = np.asarray(full["stno"]), np.asarray(red["stno"])
    pos = {}
    for k, lab in enumerate(fs):
        pos.setdefault(int(lab), []).append(k)
    seen = {}
    idx = np.empty(len(rs), np.int64)
    for k, lab in enumerate(rs):
        j = seen.get(int(lab), 0)
        idx[k] = pos[int(lab)][j]
        seen[int(lab)] = j + 1
    return idx


@pytest.mark.parametrize("mono,N,blk", USE, ids=USE_IDS)
def test_reduced_roots_join_like_full_ones(ctx, oracle, mono, N, blk):
    import torch
    _, n40, npf, vis, kw = SETS[5] if mono else SETS[2]
    maps = (synth.make_mono_set(n40, npf, vis, seed=9, **kw) if mono else synth.make_stereo_set(n40, npf, vis, seed=9, **kw))[:N]
    dicts = [oracle.localmap_to_dict(x) for x in maps]
    bounds = [(lo, lo + blk) for lo in range(0, N, blk)]
    held = [set(int(v) for d in dicts[lo:hi] for v in np.asarray(d["stno"])[6 * int(d["m"])::3]) for lo, hi in bounds]
    allids = sorted(set().union(*held))
    keep_ids = np.array([f for f in allids if sum(f in h for h in held) >= 2], np.int32)
    full_bufs, red_bufs, roots = [], [], []
    dropped = total = 0
    for r, (lo, hi) in enumerate(bounds):
        part = [dict(d, pose_origin=np.full(int(d["m"]), lo + k, np.int32)) for k, d in enumerate(dicts[lo:hi])]
        t = ctx.tree_upload(part, mono)
        ctx.tree_set_final_reanchor(t, r % 2 == 1)
        _, rc = ctx.tree_run(t)
        assert rc == 0
        nb = ctx.tree_export_size(t)
        fb = torch.empty(nb, dtype=torch.uint8, device="cuda:0")
        ctx.tree_export_dev(t, fb.data_ptr(), nb)
        # ids in any order, with ids no root holds
        ids = np.concatenate([keep_ids[::-1], np.array([10 ** 8, -5], np.int32)])
        nr = ctx.tree_export_reduced_size(t, ids)
        assert 256 < nr < nb
        rb = torch.empty(nr, dtype=torch.uint8, device="cuda:0")
        ctx.tree_export_reduced_dev(t, ids, rb.data_ptr(), nr)
        hdr = rb[:256].cpu().numpy().tobytes()
        assert api.lib().lsfm_packed_size(hdr) == nr
        root = ctx.tree_download(t)  # the result is intact: every feature is still there
        assert set(np.asarray(root["stno"])[6 * int(root["m"])::3].tolist()) == held[r]
        ctx.tree_free(t)
        total += int(root["n"])
        dropped += int(root["n"]) - len(held[r] & set(keep_ids.tolist()))
        full_bufs.append(fb); red_bufs.append(rb); roots.append(root)
    torch.cuda.synchronize()

    def top(bufs):
        t = ctx.tree_upload_dev([b.data_ptr() for b in bufs], mono)
        _, rc = ctx.tree_run(t)
        out = ctx.tree_download(t)
        ctx.tree_free(t)
        assert rc == 0
        return out
    full, red = top(full_bufs), top(red_bufs)
    assert int(red["m"]) == int(full["m"]) and set(np.asarray(red["stno"])[6 * int(red["m"])::3].tolist()) == set(keep_ids.tolist())
    idx = _by_label(full, red)
    ep, ef = pose_param_err(red["stVal"], np.asarray(full["stVal"])[idx], red["stno"]), feat_param_err(red["stVal"], np.asarray(full["stVal"])[idx], red["stno"])
    print(f"{'Mono' if mono else 'Stereo'} {N} maps in blocks of {blk}: {dropped} of {total} features dropped; reduced packs against full packs: poses {ep:.3e} features {ef:.3e}")
    assert ep <= STATE_BAR and ef <= STATE_BAR
    # the same roots downloaded, reduced on the host route and joined through lsfm_tree_upload
    hroots = []
    for root in roots:
        ids = np.asarray(root["stno"])[6 * int(root["m"])::3]
        hroots.append(ctx.marginalise(root, ~np.isin(ids, keep_ids)))
    hred, _, rc = ctx.divide_conquer(hroots, mono)
    assert rc == 0
    assert np.array_equal(hred["stno"], red["stno"])
    ep, ef = pose_param_err(hred["stVal"], np.asarray(full["stVal"])[idx], red["stno"]), feat_param_err(hred["stVal"], np.asarray(full["stVal"])[idx], red["stno"])
    print(f"  host route: poses {ep:.3e} features {ef:.3e}")
    assert ep <= STATE_BAR and ef <= STATE_BAR


# ---- 6. status and arguments ------------------------------------------------------------------------------------------------------------------
def _raw(ctx, d, drop):
    h = api.HostMap(d)
    out = api.LsfmMap()
    fl = None if drop is None else np.ascontiguousarray(drop, np.uint8)
    rc = api.lib().lsfm_map_marginalise(ctx._h, C.byref(h.c), None if fl is None else fl.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(out))
    return rc, out


def test_a_dropped_v_that_is_not_positive_definite(ctx, oracle):
    c = _case(oracle, 1)
    G = c["G"]
    n = int(G["n"])
    f = n // 2
    V = np.array(G["V"], copy=True)
    V[f] = -V[f]
    bad = dict(G, V=V)
    drop = np.zeros(n, bool)
    drop[f] = True
    rc, out = _raw(ctx, bad, drop)
    assert rc == NOT_SPD
    assert out.m == 0 and out.n == 0 and not out.U and not out.stno  # untouched
    _check_against_yardstick(ctx, G, c["I"], drop, "after the refused call")  # the context is usable
    keep = np.zeros(n, bool)
    keep[(f + 1) % n] = True
    rc, out = _raw(ctx, bad, keep)  # as a kept feature its V is never inverted
    assert rc == 0 and out.n == n - 1
    api.lib().lsfm_map_release(C.byref(out))


def test_arguments(ctx, oracle):
    import torch
    c = _case(oracle, 0)
    G = c["G"]
    n = int(G["n"])
    assert _raw(ctx, G, None)[0] == ERR_ARG
    fe = np.asarray(G["feature"])
    assert _raw(ctx, dict(G, feature=fe[::-1].copy()), np.zeros(n, bool))[0] == ERR_ARG
    maps = synth.make_stereo_set(6, 5, 4, seed=2)
    ids = np.arange(1, 1000, 2, dtype=np.int32)
    t = ctx.tree_upload(maps, False)
    try:
        with pytest.raises(api.LsfmError, match="has not been run"):
            ctx.tree_export_reduced_size(t, ids)
        ctx.tree_run(t)
        ctx.transform(maps[0].__dict__, False, maps[0].Ref + 1)  # another call on the same context
        with pytest.raises(api.LsfmError, match="overwritten"):
            ctx.tree_export_reduced_size(t, ids)
        ctx.tree_run(t)
        nb = ctx.tree_export_reduced_size(t, ids)
        buf = torch.empty(nb, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(api.LsfmError, match=f"too small: {nb} bytes"):
            ctx.tree_export_reduced_dev(t, ids, buf.data_ptr(), nb - 1)
        ctx.tree_export_reduced_dev(t, ids, buf.data_ptr(), nb)
        assert api.lib().lsfm_packed_size(buf[:256].cpu().numpy().tobytes()) == nb
    finally:
        ctx.tree_free(t)
