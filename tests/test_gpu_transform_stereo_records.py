"""-m gpu: the Stereo transform where a tile of 128 features holds more maps than k_tr_entries<1> keeps records of in LDS (TRE_MAPS), so
that lanes take R, dRA, dRB, dRG, t of their map from global memory; where both sources serve one tile; and where a tile starts with a
map that is not the batch's first (crafted_stereo_records.py; test_stereo_records_cpu.py counts that the batches are what they claim).
Through the test entry lsfm_selftest_transform, alias_passthrough off and on.

Expected: the oracle's transform of each map alone, as in test_gpu_transform_crafted.py.  Structure exact; values per block
(crafted_map.compare) at test_gpu_parity.py's STAGE_TOL = 1e-9; a passed-through map comes back bit for bit.  Every map has its own
reference pose and state: a record of the wrong map is an error of O(1) in every block of the map.

Measured on an MI355X (information, not the bar), worst of U / W / V / state over the maps:
  many 1.5e-15   alternate 7.4e-16   boundary 3.3e-15   (alias_passthrough off and on alike)
"""
import functools

import pytest

import crafted_map as cm
import crafted_stereo_records as sr
from test_gpu_parity import STAGE_TOL

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's transform of every transformed map of the batch alone (None: passed through); shared, never written to"""
    from oracle import pyoracle
    pyoracle.build()
    maps, targets = sr.case(name)
    return [pyoracle.transform(d, False, t) if cm.is_active(d, t, False) else None for d, t in zip(maps, targets)]


@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("name", sr.CASES)
def test_batch(ctx, name, alias):
    maps, targets = sr.case(name)
    got = ctx.selftest_transform(maps, False, targets, alias=alias)
    assert len(got) == len(maps)
    worst = 0.0
    for b, (g, d, e) in enumerate(zip(got, maps, expected(name))):
        what = f"{name} alias {int(alias)} map {b}"
        if e is None:
            cm.assert_identical(g, d, False)
            continue
        errs = cm.compare(g, e, False)
        print(f"{what}: " + " ".join(f"{k} {v:.2e}" for k, (v, _) in errs.items()))
        for key, (v, where) in errs.items():
            assert v < STAGE_TOL, (what, key, v, where)
            worst = max(worst, v)
    print(f"{name} alias {int(alias)}: worst {worst:.2e}")
