"""No device: what lsfm_gn_linearise_features rests on -- the structure with the correction slots AND the coalesced form together
(csrc/lsfm_gn_structure.cpp), the host floor of the reference the GPU tests hold it to, and the new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import linearise_features_ref as lf
import robust_features_ref as rf
from linearsfm_amd import api
from test_gpu_linearise import IDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(range(len(IDS))) + [lf.CRAFTED]
CASE_IDS = IDS + [lf.CRAFTED]


@pytest.mark.parametrize("i", CASES, ids=CASE_IDS)
def test_structure_with_slots_and_coalescing_together(oracle, i):
    """lsfm_gn_structure(slots, coalesce): the coalesced Ui / Uj are the plain call's pattern united with the joint image of every
    co-observation pair, stated here from the labels; sorted by (Ui, Uj), every pair once; W, feature and FBlock are the plain call's.
    gn_structure took both flags before lsfm_gn_linearise_features existed (no caller set both): this test may pass without it.
    On the six synthetic sets the union adds nothing -- a map's co-observing poses already meet through its hub roles (Mono: local
    poses 1 and 2 of a 3-pose map are ScaP and a pose of its) or its own U blocks; the crafted set's 20-pose map adds 170 pairs."""
    c = lf.base(oracle, i)
    d, mono, G = c["d"], c["mono"], c["G"]
    m = int(G["m"])
    plain = api.gn_structure(d, mono, G, coalesce=True)
    s = api.gn_structure(d, mono, G, slots=True, coalesce=True)
    Ui, Uj = s["Ui"].astype(np.int64), s["Uj"].astype(np.int64)
    assert np.all(Ui <= Uj) and np.all(np.diff(Ui * m + Uj) > 0)
    assert set(zip(plain["Ui"].tolist(), plain["Uj"].tolist())) == c["U"]
    assert set(zip(Ui.tolist(), Uj.tolist())) == c["UX"] and s["info"]["nU"] == len(c["UX"])
    assert s["info"]["NUJ"] == plain["info"]["NUJ"] + s["info"]["slots"] and s["info"]["slots"] > 0
    for k in ("photo", "feature", "FBlock", "photoJ", "fptrJ", "wdst"):
        assert np.array_equal(s[k], plain[k]), k
    assert s["info"]["nW"] == plain["info"]["nW"] and s["info"]["NWJ"] == plain["info"]["NWJ"]
    if i == lf.CRAFTED:
        assert len(c["UX"]) - len(c["U"]) == 170
    else:
        assert c["UX"] == c["U"]


@pytest.mark.parametrize("i", [0, 1, 3, 4, lf.CRAFTED], ids=[IDS[0], IDS[1], IDS[3], IDS[4], lf.CRAFTED])
def test_host_floor_of_the_reference(oracle, i):
    """The oracle's H on the maps I_k(w) written two ways on the host: rf.reweight (appended U blocks, W and V scaled) and
    rf.dense_reweight of the dense I_k (the column formula), put back into a dict.  With the GPU tests' weights (uniform in [0.1, 1], a
    tenth exactly 1) the two agree far inside the 1e-9 bar those tests hold the device to: the reference holds the bar on its own.
    Measured: at most 5.1e-15 (the 2- and 9-map sets, the crafted set)."""
    c = lf.base(oracle, i)
    d, fw = c["d"], c["fw"]
    assert min(np.min(x) for x in fw if len(x)) >= 0.1 and sum(int(np.sum(x == 1.0)) for x in fw) >= sum(len(x) for x in fw) // 10
    one = lf.weighted_h(oracle, i)
    two = [lf.dict_from_dense(L, rf.dense_reweight(rf.dense_info(L), int(L["m"]), int(L["n"]), x)) for L, x in zip(d, fw)]
    H2 = lf.oracle_dense_h_by_pose_columns(oracle, two, c["mono"], c["G"])
    e = lf.h_err(H2, one)
    print(f"{i}: host floor of H on re-weighted maps {e:.3e}")
    assert e <= 1e-11  # (two orders inside the device's bar)


def test_symbols_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "lsfm.h")).read()
    for name in ("lsfm_gn_linearise_features", "lsfm_gn_linearise_features_timed"):
        assert name in api.EXPORTS and getattr(api.lib(), name) is not None
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    import inspect
    assert "feature_weight" in inspect.signature(api.Context.gn_linearise).parameters
    assert "not offered" not in header
    # refused without a device: no maps, no feature weights, a bad type
    L = api.lib()
    m = api.LsfmMap()
    w = (C.c_double * 1)(1.0)
    assert L.lsfm_gn_linearise_features(None, None, 1, 0, C.byref(m), None, w, C.byref(m), None, None) == -1
    assert L.lsfm_gn_linearise_features(None, C.byref(m), 1, 0, C.byref(m), None, None, C.byref(m), None, None) == -1
    assert L.lsfm_gn_linearise_features(None, C.byref(m), 1, 2, C.byref(m), None, w, C.byref(m), None, None) == -1
