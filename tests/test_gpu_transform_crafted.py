"""-m gpu: the batched coordinate transform (csrc/lsfm_transform.hip) on maps and batches built to order (crafted_map.py), so that the
length of every run, the poses of every tile, the old blocks to the hub poses and the transformed / passed-through maps of a batch
are chosen, not met by chance.  Single maps go through lsfm_transform_stereo / lsfm_transform_mono, batches through the test entry
lsfm_selftest_transform (N maps, one transform_batch call, per-map targets, alias_passthrough off and on).

Expected: the oracle's transform of each map alone (pinned to the real reference at 1e-12 on every fixture; no shape-dependent code).
Structure is exact.  Values are compared PER BLOCK: max |got - exp| over max(the block's largest |entry|, the median over the array of
the blocks' largest entries) for U (Mono: by coordinates, canon_u), W and V, per scalar with a floor of 1 for the state -- at
test_gpu_parity.py's STAGE_TOL = 1e-9.  A passed-through map comes back bit for bit.  No block is left out.
test_crafted_map_cpu.py shows on the CPU that every case reaches the path named here and that two evaluations of the reference's own
arithmetic (features reordered) lie at most 6.8e-15 apart in this metric.

Which path a case reaches (Stereo and Mono unless noted):
  a    n = 129: runs of 513 (three chunks, the tile's first feature), 260 (a middle one), 257, 300 (its last); rounds of exactly 256 blocks
       (1 + 255, then one run of 256); 255 followed by 2 (the feature with 2 blocks starts a round); 1-block features between; the chunked
       features' hub blocks, single and repeated, lie behind their first chunk (Gsum added to, hubJ set from a later chunk, -2 walk)
  b1   tiles seen by exactly GCAP and by GCAP + 1 poses (32 / 33, Mono 64 / 65)
  b2   two tiles seen by the same 70 (Mono 140) poses in opposite orders, and a ragged third: lanes without a slot add to the rows
       the other tile flushes its table into
  c    0, 1, 2, 5 old blocks to the hub; Mono: all nine combinations of {none, one, several} over the two hubs; a feature with nothing else
  d    Mono: (c2fix, c3zero) in all four combinations, each with a new Fix of 0, 1, 2, on a 12-pose map
  e    batches of five maps (70 / 100 / 90 / 1 / 130 features, 20 / 22 / 24 / 1 / 40 poses): every tile boundary inside a map, one tile
       with three maps, a run of 300 as the last feature of the first tile; A transformed, N passed through without a target,
       F passed through because it is in that frame: ANAFA, AFANA, NAFAN, AAAAA (Stereo: the first tile is seen by 42 poses of two
       maps), NFNFN; a map of one pose (Mono: two poses where it is transformed)
  f    300 poses, diagonal + chain U blocks: every work-group of k_tr_ublocks touches more than 64 poses; the hubs mid-range

Measured on an MI355X (information, not the bar), worst of U / W / V / state, Stereo | Mono:
  a 3.2e-15 | 4.5e-15   b1 1.8e-15 | 2.0e-15   b2 9.0e-16 | 3.1e-15   c 1.4e-15 | 1.6e-15   d - | 5.3e-15   e 2.5e-15 | 7.7e-15
  f 8.6e-16 | 9.3e-16.  No case exposed a fault of the transform; DESIGN.md §3 "Direct tests of the transform" names the case that
  caught each of five arithmetic-only changes of the kernel.
"""
import functools

import numpy as np
import pytest

import crafted_map as cm
from linearsfm_amd import api
from test_gpu_parity import STAGE_TOL

pytestmark = pytest.mark.gpu

SINGLE_CASES = [(k, mono) for k, mono in cm.CASES if k[0] != "e"]


@functools.lru_cache(maxsize=None)
def expected(name, mono):
    """the oracle's transform of every transformed map of the case alone (None: passed through); shared, never written to"""
    from oracle import pyoracle
    pyoracle.build()
    maps, targets = cm.case(name, mono)
    return [pyoracle.transform(d, mono, *(t if mono else (t,))) if cm.is_active(d, t, mono) else None for d, t in zip(maps, targets)]


def _check(got, exp, mono, what):
    for k in ("U", "W", "V", "stVal"):
        assert np.all(np.isfinite(got[k])), (what, k)
    errs = cm.compare(got, exp, mono)
    print(f"{what}: " + " ".join(f"{k} {e:.2e}" for k, (e, _) in errs.items()))
    for key, (e, where) in errs.items():
        assert e < STAGE_TOL, (what, e, where)
    return errs


@pytest.mark.parametrize("name,mono", SINGLE_CASES)
def test_single_map(ctx, name, mono):
    (d,), (t,) = cm.case(name, mono)
    got = ctx.transform(d, mono, *(t if mono else (t,)))
    _check(got, expected(name, mono)[0], mono, f"{name} {'Mono' if mono else 'Stereo'}")


@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("pattern", cm.E_PATTERNS)
def test_batch(ctx, pattern, mono, alias):
    name = f"e_{pattern}"
    maps, targets = cm.case(name, mono)
    got = ctx.selftest_transform(maps, mono, targets, alias=alias)
    assert len(got) == len(maps)
    for b, (g, d, e) in enumerate(zip(got, maps, expected(name, mono))):
        what = f"{name} {'Mono' if mono else 'Stereo'} alias {int(alias)} map {b}"
        if e is None:
            cm.assert_identical(g, d, mono)
        else:
            _check(g, e, mono, what)


@pytest.mark.parametrize("mono", [False, True])
def test_one_map_as_a_batch_is_the_single_call(ctx, mono):
    """the entry point adds nothing of its own: a batch of one map is lsfm_transform_* bit for bit in everything no atomic sums"""
    (d,), (t,) = cm.case("c", mono)
    one = ctx.selftest_transform([d], mono, [t])[0]
    ref = ctx.transform(d, mono, *(t if mono else (t,)))
    for k in ("stno", "stVal", "Ui", "Uj", "photo", "feature", "FBlock", "V"):
        assert np.array_equal(one[k], ref[k]), k
    _check(one, expected("c", mono)[0], mono, f"c as a batch of one, {'Mono' if mono else 'Stereo'}")


def test_arguments(ctx):
    maps, targets = cm.case("e_ANAFA", False)
    with pytest.raises(api.LsfmError):
        ctx.selftest_transform(maps, False, targets[:-1])
    with pytest.raises(api.LsfmError, match="not found"):
        ctx.selftest_transform(maps, False, [t if b else 999999 for b, t in enumerate(targets)])
    got = ctx.selftest_transform(maps[:1], False, targets[:1])  # (the context is usable afterwards)
    assert got[0]["Ref"] == targets[0]
