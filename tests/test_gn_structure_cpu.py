"""No device: the structure of the Gauss-Newton polish's joint system (csrc/lsfm_gn_structure.cpp, lsfm_gn_structure) from labels alone --
the joint and the coalesced U / W against test_gpu_linearise.label_structure, the correction slots of the feature weights against a few
lines written here, and the refusals of what cannot be placed, on the six sets of test_gpu_linearise.SETS and the crafted maps of
test_gpu_robust_features (a repeated (pose, feature) pair, a map without features)."""
import functools
import os
import re
import time

import numpy as np
import pytest

import robust_features_ref as rf
from linearsfm_amd import api, synth
from test_gpu_linearise import IDS, SETS, label_structure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(range(len(SETS))) + ["crafted"]
CASE_IDS = IDS + ["crafted"]


@functools.lru_cache(maxsize=None)
def _case(oracle, i):
    """(map dicts, mono, the oracle's tree result); computed once, changed by no test."""
    if i == "crafted":
        d, G = rf.crafted_set(oracle)
        return d, False, G
    mono, n, npf, vis, kw = SETS[i]
    maps = synth.make_mono_set(n, npf, vis, seed=9, **kw) if mono else synth.make_stereo_set(n, npf, vis, seed=9, **kw)
    d = [oracle.localmap_to_dict(x) for x in maps]
    G, _, rc = oracle.divide_conquer(d, mono)
    assert rc == 0
    return d, mono, G


def expected_slots(dicts):
    """Per map, in map order: the distinct pairs a <= b of local poses that see a common feature, sorted, each with the number of common
    features (a repeated (pose, feature) pair counts once)."""
    out = []
    for k, L in enumerate(dicts):
        seen = {}
        for p, f in zip(np.asarray(L["photo"]).tolist(), np.asarray(L["feature"]).tolist()):
            seen.setdefault(f, set()).add(p)
        count = {}
        for ps in seen.values():
            ps = sorted(ps)
            for q, a in enumerate(ps):
                for b in ps[q:]:
                    count[(a, b)] = count.get((a, b), 0) + 1
        out += [(k, a, b, c) for (a, b), c in sorted(count.items())]
    return out


def test_symbol_is_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "lsfm.h")).read()
    assert getattr(api.lib(), "lsfm_gn_structure") is not None and "lsfm_gn_structure" in api.EXPORTS
    assert re.search(r"\bint\s+lsfm_gn_structure\s*\(", header) and callable(api.gn_structure)


@pytest.mark.parametrize("i", CASES, ids=CASE_IDS)
def test_joint_and_coalesced_form(oracle, i):
    d, mono, G = _case(oracle, i)
    W, U, nWJ, nUJ = label_structure(d, mono, G)
    t0 = time.perf_counter()
    s = api.gn_structure(d, mono, G, coalesce=True)
    assert time.perf_counter() - t0 < 0.5  # (measured: at most 0.02 s, the 40-map sets)
    v = s["info"]
    m, n = int(G["m"]), int(G["n"])
    assert (v["M"], v["NFG"], v["P"], v["FI"]) == (m, n, sum(int(L["m"]) for L in d), sum(int(L["n"]) for L in d))
    assert v["NUJ"] == nUJ and v["NWJ"] == nWJ and v["slots"] == 0 and v["contributors"] == 0
    # the working form: row <= column, every pair the labels give and no other
    UiJ, UjJ = s["UiJ"].astype(np.int64), s["UjJ"].astype(np.int64)
    assert len(UiJ) == nUJ and np.all((0 <= UiJ) & (UiJ <= UjJ) & (UjJ < m))
    assert set(zip(UiJ.tolist(), UjJ.tolist())) == U
    fptrJ, photoJ = s["fptrJ"], s["photoJ"]
    assert fptrJ[0] == 0 and fptrJ[-1] == nWJ and np.all(np.diff(fptrJ) > 0) and len(photoJ) == nWJ
    featJ = np.repeat(np.arange(n), np.diff(fptrJ))
    assert set(zip(photoJ.tolist(), featJ.tolist())) == W
    # an instance's run starts with its map's nh hubs; a Stereo map in the global frame has none
    hubs = s["map_hubs"]
    f = 0
    for k, L in enumerate(d):
        nh = int(hubs[k, 0])
        if mono:
            assert nh == 2
        else:
            assert nh == (0 if int(L["Ref"]) == int(G["Ref"]) else 1)
        for _ in range(int(L["n"])):
            assert photoJ[s["wdst"][f]:s["wdst"][f] + nh].tolist() == hubs[k, 1:1 + nh].tolist()
            f += 1
    assert f == v["FI"]
    # the coalesced form: what test_gpu_linearise.test_canonical_form asserts of the map handed out
    Ui, Uj = s["Ui"].astype(np.int64), s["Uj"].astype(np.int64)
    assert v["nU"] == len(Ui) and v["nW"] == len(s["photo"])
    assert np.all(Ui <= Uj) and np.all(np.diff(Ui * m + Uj) > 0)
    fe, ph = s["feature"].astype(np.int64), s["photo"].astype(np.int64)
    assert np.all(np.diff(fe) >= 0) and np.all(np.diff(fe * m + ph) > 0)
    assert np.array_equal(s["FBlock"], np.searchsorted(fe, np.arange(n)))
    assert np.all(fe[s["FBlock"]] == np.arange(n))
    assert set(zip(Ui.tolist(), Uj.tolist())) == U and v["nU"] == len(U) < nUJ
    assert set(zip(ph.tolist(), fe.tolist())) == W and v["nW"] == len(W) < nWJ
    assert np.count_nonzero(Ui == Uj) == m


@pytest.mark.parametrize("i", CASES, ids=CASE_IDS)
def test_correction_slots(oracle, i):
    d, mono, G = _case(oracle, i)
    t0 = time.perf_counter()
    plain = api.gn_structure(d, mono, G)
    s = api.gn_structure(d, mono, G, slots=True)
    assert time.perf_counter() - t0 < 0.5
    exp = expected_slots(d)
    got = list(zip(s["slot_map"].tolist(), s["slot_a"].tolist(), s["slot_b"].tolist(), s["slot_count"].tolist()))
    assert got == exp
    assert s["info"]["slots"] == len(exp) and s["info"]["contributors"] == sum(e[3] for e in exp)
    assert plain["info"]["slots"] == 0 and plain["info"]["NUJ"] == s["info"]["NUJ"] - len(exp)
    assert plain["info"]["NWJ"] == s["info"]["NWJ"] and np.array_equal(plain["photoJ"], s["photoJ"])
    # the slots' joint coordinates: every map's own pairs first, then its slots'
    _, U, _, _ = label_structure(d, mono, G)
    m = int(G["m"])
    pid = {int(-G["stno"][6 * p]): p for p in range(m)}
    for k, a, b, _ in exp:
        ls = np.asarray(d[k]["stno"])
        ga, gb = pid[int(-ls[6 * a])], pid[int(-ls[6 * b])]
        U.add((min(ga, gb), max(ga, gb)))
    assert set(zip(s["UiJ"].tolist(), s["UjJ"].tolist())) == U and np.all(s["UiJ"] <= s["UjJ"])


def test_crafted_maps_hold_the_cases(oracle):
    """The crafted set is what the header says: a repeated (pose, feature) pair that counts once, and a map without features."""
    d, _, G = _case(oracle, "crafted")
    A, Cm = d[-3], d[-1]
    pairs = list(zip(np.asarray(A["photo"]).tolist(), np.asarray(A["feature"]).tolist()))
    assert len(pairs) > len(set(pairs)) and int(Cm["n"]) == 0
    exp = {(a, b): c for k, a, b, c in expected_slots(d) if k == len(d) - 3}
    assert len(exp) == 210 and exp[(3, 5)] == 2 and exp[(3, 3)] == 2 and exp[(5, 5)] == 2 and exp[(7, 7)] == 2 and exp[(0, 19)] == 1
    assert not [e for e in expected_slots(d) if e[0] == len(d) - 1]


def test_refusals(oracle):
    """What test_gpu_gn.test_polish_refuses_what_it_cannot_place and test_gpu_robust_features.test_refusals refuse because of labels,
    and a bad Fix and an empty map: LSFM_ERR_ARG with the message the device calls give."""
    d = [oracle.localmap_to_dict(m) for m in synth.make_stereo_set(5, 6, 4, seed=2)]
    G, _, rc = oracle.divide_conquer(d, False)
    assert rc == 0

    def refused(maps, mono, x, text, **kw):
        with pytest.raises(api.LsfmError) as e:
            api.gn_structure(maps, mono, x, **kw)
        assert "rc=-1" in str(e.value) and str(e.value).endswith(": " + text), str(e.value)

    short = dict(G, n=G["n"] - 1, stno=G["stno"][:-3], stVal=G["stVal"][:-3])
    last = int(G["stno"][-1])
    k = 1 + next(k for k, L in enumerate(d) if last in np.asarray(L["stno"])[6 * int(L["m"]):].tolist())
    for kw in ({}, dict(slots=True), dict(coalesce=True)):
        refused(d, False, short, f"gn polish: a feature of local map {k} is not in the global state", **kw)
    more = dict(G, n=G["n"] + 1, stno=np.concatenate([G["stno"], [999999] * 3]).astype(np.int32), stVal=np.concatenate([G["stVal"], [0.0, 0.0, 1.0]]))
    refused(d, False, more, "gn polish: a feature of the global state is in no local map")
    m = int(G["m"])
    pose = dict(G, m=m + 1, stno=np.concatenate([G["stno"][:6 * m], [-999999] * 6, G["stno"][6 * m:]]).astype(np.int32),
                stVal=np.concatenate([G["stVal"][:6 * m], np.zeros(6), G["stVal"][6 * m:]]))
    refused(d, False, pose, "gn polish: a pose of the global state is in no local map")
    fewer = dict(G, m=m - 1, stno=G["stno"][6:], stVal=G["stVal"][6:])
    gone = int(-G["stno"][0])  # the first map, in map order, that needs the pose: as its hub (checked first) or as one of its poses
    for k, L in enumerate(d):
        if int(L["Ref"]) == gone and int(L["Ref"]) != int(G["Ref"]):
            refused(d, False, fewer, f"gn polish: the reference pose of local map {k + 1} is not in the global state")
            break
        if gone in (-np.asarray(L["stno"])[:6 * int(L["m"]):6]).tolist():
            refused(d, False, fewer, f"gn polish: a pose of local map {k + 1} is not in the global state (Stereo: the global reference pose cannot be a variable of a map)")
            break
    else:
        raise AssertionError("the removed pose is in no map")
    empty = dict(d[2], m=0, n=0, stno=np.zeros(0, np.int32), stVal=np.zeros(0), U=np.zeros((0, 36)), Ui=[], Uj=[], W=np.zeros((0, 18)), photo=[],
                 feature=[], V=np.zeros((0, 9)), FBlock=[])
    refused(d[:2] + [empty] + d[3:], False, G, "gn polish: local map 3 is empty")
    # Mono: Fix of a map and of the state
    dm = [oracle.localmap_to_dict(x) for x in synth.make_mono_set(3, 6, 4, seed=2)]
    Gm, _, rc = oracle.divide_conquer(dm, True)
    assert rc == 0
    refused([dm[0], dict(dm[1], Fix=3), dm[2]], True, Gm, "gn polish: Fix must be 0, 1 or 2")
    refused(dm, True, dict(Gm, Fix=-1), "gn polish: the global state's reference / scale pose (Ref, ScaP, Fix) is not in it")
    assert api.gn_structure(dm, True, Gm)["info"]["M"] == int(Gm["m"])


def test_structure_under_asan_ubsan():
    """tests/sanitize/sanitize_gn_structure.cpp: a stand-alone program over lsfm_gn_structure.cpp, built with -fsanitize=address,undefined."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    out = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "sanitize_gn_structure")
    csrc = os.path.join(ROOT, "linearsfm_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "sanitize", "sanitize_gn_structure.cpp"), os.path.join(csrc, "lsfm_gn_structure.cpp"), os.path.join(csrc, "lsfm_system.cpp")]
    deps = srcs + [os.path.join(csrc, "lsfm_gn_structure.hpp"), os.path.join(csrc, "lsfm_system.hpp"), os.path.join(ROOT, "include", "lsfm.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                               "-o", exe] + srcs)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "sanitize_gn_structure: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-6000:])
