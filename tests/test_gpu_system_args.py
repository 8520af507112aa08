"""-m gpu: the index arrays of a system handed over in host arrays are checked on the host, alike by every entry point that takes one
(csrc/lsfm_system.cpp): lsfm_solve_stereo / lsfm_solve_mono, lsfm_map_covariance, lsfm_map_covariance_columns, lsfm_map_marginalise and
lsfm_schur_pattern.  Every malformed input below is refused with LSFM_ERR_ARG (-1) before anything is uploaded or launched, and the
well-formed call directly after it, on the same context, returns 0.  The systems are the final maps of a 4-map Stereo and a 9-map Mono
tree."""
import ctypes as C

import numpy as np
import pytest

from linearsfm_amd import api, synth

pytestmark = pytest.mark.gpu
CALLS = ("solve", "covariance", "covariance_columns", "marginalise", "schur_pattern")


@pytest.fixture(scope="module", params=["Stereo", "Monocular"])
def final_map(ctx, request):
    mono = request.param == "Monocular"
    maps = synth.make_mono_set(9, 8, 4, seed=5) if mono else synth.make_stereo_set(4, 8, 4, seed=5)
    G, _, rc = ctx.divide_conquer(maps, mono)
    assert rc == 0
    assert int(G["m"]) > 1 and int(G["n"]) > 2 and len(G["Ui"]) > 1
    return G, mono


def _reversed_w(G):
    d = dict(G)
    for k in ("W", "photo", "feature"):
        d[k] = np.asarray(G[k])[::-1].copy()
    return d, {}


def _blockless_feature(G):
    """a feature without a W block in the middle: the features from k on are renumbered, V / the state get a slot for it"""
    d = dict(G)
    m, n, k = int(G["m"]), int(G["n"]), int(G["n"]) // 2
    fe = np.asarray(G["feature"]).copy()
    fe[fe >= k] += 1
    d["feature"] = fe
    d["n"] = n + 1
    d["V"] = np.insert(np.asarray(G["V"]).reshape(-1, 9), k, np.eye(3).ravel(), axis=0)
    at = 6 * m + 3 * k
    d["stno"] = np.insert(np.asarray(G["stno"]), at, [10 ** 6] * 3)
    d["stVal"] = np.insert(np.asarray(G["stVal"]), at, [0.0] * 3)
    d["FBlock"] = np.insert(np.asarray(G["FBlock"]), k, 0)
    return d, {}


def _set(key, at, value):
    def make(G):
        d = dict(G)
        a = np.asarray(G[key]).copy()
        a[at] = value(G) if callable(value) else value
        d[key] = a
        return d, {}
    return make


def _ui_above_uj(G):
    d = dict(G)
    k = int(np.nonzero(np.asarray(G["Ui"]) < np.asarray(G["Uj"]))[0][0])
    ui, uj = np.asarray(G["Ui"]).copy(), np.asarray(G["Uj"]).copy()
    ui[k], uj[k] = uj[k], ui[k]
    d["Ui"], d["Uj"] = ui, uj
    return d, {}


MALFORMED = {
    "W runs reversed": _reversed_w,
    "feature without a block": _blockless_feature,
    "photo = -1": _set("photo", 3, -1),
    "photo = m": _set("photo", -1, lambda G: int(G["m"])),
    "Ui > Uj": _ui_above_uj,
    "Uj = m": _set("Uj", -1, lambda G: int(G["m"])),
    "n = 0": lambda G: (dict(G), {"n": 0}),
    "nW = 0": lambda G: (dict(G), {"nW": 0}),
    "m = 1": lambda G: (dict(G), {"m": 1}),
}


def _call(ctx, call, d, mono, counts, room):
    """The entry point as it is, counts (m, n, nW) overridden where the case says so; every output has room for the well-formed map."""
    h = api.HostMap(d)
    for k, v in counts.items():
        setattr(h.c, k, v)
    c, L, dbl, i32 = h.c, api.lib(), C.c_double, C.c_int
    M, N = room
    if call == "solve":
        rng = np.random.default_rng(1)
        st, ea, eb = np.zeros(6 * M + 3 * N + 3), rng.standard_normal(6 * M), rng.standard_normal(3 * N + 3)
        args = [ctx._h, api._ptr(st, dbl), api._ptr(eb, dbl), api._ptr(ea, dbl), c.U, c.W, c.V, c.Ui, c.Uj, c.photo, c.feature, c.m, c.n, c.nU, c.nW]
        if not mono:
            return L.lsfm_solve_stereo(*args, None)
        ids = -np.asarray(d["stno"])[: 6 * int(d["m"]): 6]
        pr, ps = int(np.nonzero(ids == d["Ref"])[0][0]), int(np.nonzero(ids == d["ScaP"])[0][0])
        if counts.get("m") == 1:
            pr = ps = 0  # (the gauge must name scalars of the system for the call to get as far as its index arrays)
        return L.lsfm_solve_mono(*args, pr, 6 * pr, 6 * ps + int(d["Fix"]), int(d["Sign"]), 0, None)
    if call == "covariance":
        pose, feat = np.zeros((M, 36)), np.zeros((N + 1, 9))
        return L.lsfm_map_covariance(ctx._h, C.byref(c), int(mono), api._ptr(pose, dbl), api._ptr(feat, dbl), None, 0, None)
    if call == "covariance_columns":
        q, pose = np.zeros(1, np.int32), np.zeros((M, 36))
        steps, corr = C.c_int(0), np.zeros(1)
        return L.lsfm_map_covariance_columns(ctx._h, C.byref(c), int(mono), api._ptr(q, i32), 1, api._ptr(pose, dbl), None, None, C.byref(steps), api._ptr(corr, dbl))
    if call == "marginalise":
        drop = np.zeros(N + 1, np.uint8)
        drop[::2] = 1
        out = api.LsfmMap()
        rc = L.lsfm_map_marginalise(ctx._h, C.byref(c), api._ptr(drop, C.c_ubyte), C.byref(out))
        if rc == 0:
            L.lsfm_map_release(C.byref(out))
        return rc
    cap = M * (M + 1) // 2
    rowptr, colidx, nnzb = np.zeros(M + 1, np.int32), np.zeros(cap, np.int32), C.c_int(0)
    return L.lsfm_schur_pattern(ctx._h, c.Ui, c.Uj, c.photo, c.feature, c.m, c.n, c.nU, c.nW, api._ptr(rowptr, i32), api._ptr(colidx, i32), cap, C.byref(nnzb))


@pytest.mark.parametrize("call", CALLS)
def test_malformed_index_arrays_are_refused_on_the_host(ctx, final_map, call):
    G, mono = final_map
    room = (int(G["m"]), int(G["n"]))
    assert _call(ctx, call, G, mono, {}, room) == 0
    for name, make in MALFORMED.items():
        d, counts = make(G)
        if call == "schur_pattern" and name == "nW = 0":
            continue  # (every feature block-less: not malformed for this call)
        rc = _call(ctx, call, d, mono, counts, room)
        if call == "schur_pattern" and name == "feature without a block":
            # (lsfm_schur_pattern has always taken it: such a feature adds nothing to the pattern)
            assert rc == 0, (call, name, api.lib().lsfm_last_error(ctx._h))
            continue
        assert rc == -1, (call, name, rc)
        assert _call(ctx, call, G, mono, {}, room) == 0, (call, name, api.lib().lsfm_last_error(ctx._h))
