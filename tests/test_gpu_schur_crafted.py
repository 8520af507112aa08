"""-m gpu: K9 -- the Schur assembly S = U - sum_f W_f V_f^-1 W_f^T, E = ea - sum_f W_f V_f^-1 eb_f (csrc/lsfm_schur_panel.hip; k_vinv,
k_schur_scale, k_schur_w, k_schur_finish in csrc/lsfm_solve.hip) -- on systems built to order (crafted_system.py), so that the pose
count of every tile, the split of every list and the place of every repeated block are chosen, not met by chance.

S: lsfm_map_marginalise with every feature dropped returns U' = S as K9's launch sequence (build_schur_values) leaves it; held to the
long-double sum over the features in the metric of test_gpu_marginalise.py, max |d_ij| / sqrt(I_ii I_jj), at that file's BAR = 1e-9.
The pose scalars' scales are spread over +-3 decades.  A pose no feature sees keeps its row of U bit for bit.
E: lsfm_solve_stereo / lsfm_solve_mono through the pipeline (set_small_solve(0)) on the same systems at +-1 decade, against
dense_reference_solve (up to 4000 unknowns) or schur_reference_solve, max |d| / max(1, |x|) over poses and over features, at
test_gpu_parity.py's DENSE_TOL = 1e-10.
test_crafted_cpu.py shows on the CPU that every system has the tile pose counts named here and that the yardsticks' own floors are
below 1e-13.

Which branch a case reaches (poses of its tiles in brackets):
  a8 [8, 5, 8 (37 features)]   the 8-slot variant launched alone: runs of 8, runs of 1-3, a ragged tile
  a9 [9, 4], a16 [16]          the 16-slot variant launched alone, at its smallest and with all slots taken
  b16 .. b100, one tile each   the edges of PmShared<SMAX>::CAP: 16 | 17, 32 | 33, 48 | 49; 62 and 63 (the right-hand side's two rows
                               in the last strip of the widest panel); 64 (k_schur_w: one more than the widest panel takes); 65 (the
                               slot kernel's hash table is full); 100 with runs of ~70 (both LDS tables of k_schur_w overflow to
                               global atomics).  m = poses + 3: three poses are seen by nothing
  c32, c48, c63                every feature seen by every pose (4096 / 6144 first blocks; c63: runs of 30-40): blocks behind the LDS
                               slot list (PM_MAXE = 3584; 2560 in the 64-slot variant), repeats among them, passes of more than
                               PM_BF = 352 blocks (the search of the run pointers)
  d1 (17 tiles, the last of 40 features), d2, d3 (8 tiles each, m = 100)
                               the lists of the 32- / 48- / 64-slot variants cut into 4 / 8 / 8, 1 / 2 / -, - / 4 / 2 parts; d1's ragged
                               last tile is the 36-pose tile of a list cut into 8 (empty parts behind its end), d3's a 62-pose tile
                               cut into 2; d3 has a 70-pose tile (k_schur_w) and a 12-pose tile (16-slot variant) beside the lists
  e                            d2 with every second feature dropped: wide variants on runs the partition pass compacted
  f33                          Mono gauge: a pose block that features see and a scalar of another pose fixed (sexp = 400 rows)
  g20                          one V_f with an eigenvalue of -1e-3 of its largest: refused, or S within the bar
Repeated (pose, feature) blocks (PM_DUP) are in every case, one observation in ten.

Measured on an MI355X (information, not the bar):
  S error, decades 3:  a8 1.7e-16  a9 2.6e-16  a16 2.1e-16  c32 2.1e-16  c48 2.1e-16  c63 1.9e-16  d1 2.0e-16  d2 2.0e-16  d3 1.9e-16
                       f33 2.1e-16  b16 1.9e-16  b17 1.9e-16  b32 2.1e-16  b33 2.0e-16  b48 2.0e-16  b49 2.0e-16  b62 1.9e-16
                       b63 1.8e-16  b64 2.1e-16  b65 1.9e-16  b100 2.2e-16;  e (d2, every second feature dropped) 1.0e-15
  solve, decades 1, poses / features:  a8 2.2e-16 / 1.9e-15  a9 5.6e-16 / 6.2e-16  a16 2.2e-16 / 2.2e-16  c32 3.9e-16 / 2.9e-17
                       c48 2.8e-16 / 2.1e-17  c63 1.0e-15 / 2.8e-17  d1 4.4e-16 / 6.2e-16  d2 7.0e-16 / 5.6e-16  d3 1.3e-15 / 8.9e-16
                       f33 (Mono gauge) 1.1e-15 / 2.2e-16  b16 2.9e-16 / 3.3e-16  b17 3.3e-16 / 1.2e-16  b32 1.0e-15 / 6.7e-16
                       b33 6.7e-16 / 4.4e-16  b48 1.2e-15 / 5.6e-16  b49 8.0e-16 / 4.4e-16  b62 1.3e-15 / 4.4e-16  b63 7.8e-16 / 3.3e-16
                       b64 1.1e-15 / 4.4e-16  b65 8.9e-16 / 2.2e-16  b100 9.4e-16 / 1.9e-17
  g20: refused with the not-positive-definite error.  256 CUs: the lists' parts as named above.  No case exposed a fault of K9.
"""
import numpy as np
import pytest

import crafted_system as cs
from linearsfm_amd import api
from refdump import dense_info
from test_gpu_marginalise import BAR, _check_against_yardstick, info_err
from test_gpu_parity import DENSE_TOL

pytestmark = pytest.mark.gpu


def _as_map(J):
    """the keys a map needs beside the system's, as test_gpu_marginalise._wide_map sets them"""
    m, n = int(J["m"]), int(J["n"])
    fe = np.asarray(J["feature"])
    stno = np.concatenate([np.repeat(-(np.arange(m) + 1), 6), np.repeat(np.arange(n) + 1, 3)]).astype(np.int32)
    keys = ("m", "n", "U", "Ui", "Uj", "W", "V", "photo", "feature")
    return dict({k: J[k] for k in keys}, Ref=0, FRef=0, stno=stno, stVal=np.zeros(len(stno)), FBlock=np.searchsorted(fe, np.arange(n)).astype(np.int32))


def _s_of(ctx, J):
    out = ctx.marginalise(_as_map(J), np.ones(J["n"], bool))
    assert out["m"] == J["m"] and out["n"] == 0 and out["nW"] == 0
    return dense_info(out)


@pytest.mark.parametrize("name", cs.S_CASES)
def test_s_against_the_long_double_sum(ctx, name):
    J = cs.system(name, 3)
    m = J["m"]
    got = _s_of(ctx, J)
    Uin = cs.dense_u(J)
    assert np.all(np.isfinite(got))
    e = info_err(got, np.asarray(cs.expected_s(name, 3), np.float64), np.diag(Uin))
    print(f"{name} {J['counts']}: S error {e:.3e}")
    assert e <= BAR
    unseen = np.setdiff1d(np.arange(m), np.unique(J["photo"]))
    assert len(unseen) >= (3 if name[0] in "bf" else 0)  # (b, f: m = poses + 3; the windows of d2 / d3 leave poses out too)
    rows = (6 * unseen[:, None] + np.arange(6)).reshape(-1)
    assert np.array_equal(got[rows], Uin[rows]) and np.array_equal(got[:, rows], Uin[:, rows])


def test_list_splits_occur():
    """Coverage accounting, nothing about the kernel: over the systems of (d) each of 8, 4, 2 and 1 parts occurs for a listed variant
    on this device (k9_kernel's rule, restated in crafted_system.parts_of_list)."""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    seen = {}
    for name in cs.LIST_CASES:
        counts = cs.system(name, 3)["counts"]
        seen[name] = [cs.parts_of_list(n, len(counts), ncu) for n in cs.list_lengths(counts)]
    print(f"{ncu} CUs: parts of the 32- / 48- / 64-slot lists {seen}")
    assert {8, 4, 2, 1} <= {p for v in seen.values() for p in v}
    assert seen["d1"][1] == 8  # (the list of d1's ragged 36-pose tile)


def test_s_of_a_compacted_input(ctx):
    J = cs.system("d2", 3)
    G = _as_map(J)
    drop, _ = cs.half_dropped("d2", 3)
    _check_against_yardstick(ctx, G, dense_info(G), drop, "d2, every second feature dropped")


@pytest.fixture()
def pipeline(ctx):
    """the sparse pipeline for every system, whatever its size; leaves the default (5) behind, as test_gpu_small.py does"""
    try:
        ctx.set_small_solve(0)
        yield ctx
    finally:
        ctx.set_small_solve(5)


@pytest.mark.parametrize("name", cs.SOLVE_CASES)
def test_solve_against_the_exact_solution(pipeline, name):
    J = cs.system(name, 1)
    ea, eb = cs.rhs(name, 1)
    x, mono, sa = cs.expected_x(name, 1)
    st, rc = pipeline.solve(J, ea, eb, mono, sa)
    assert rc == 0
    ep, ef = cs.state_metric(st, x, J["m"])
    print(f"{name} {J['counts']}{' Mono gauge ' + str(sa) if mono else ''}: poses {ep:.3e} features {ef:.3e}")
    assert ep < DENSE_TOL and ef < DENSE_TOL
    if mono:
        assert st[sa[2]] == sa[3] and np.all(st[6 * sa[0]:6 * sa[0] + 6] == 0.0)


def test_a_feature_without_a_factor(ctx):
    """The only input that is not positive semi-definite: refused with the not-positive-definite error, or an S within the bar --
    never a finite S outside it."""
    J = cs.system("g20", 3)
    try:
        got = _s_of(ctx, J)
    except api.LsfmError as err:
        assert "not positive definite" in str(err)
        print(f"g20: refused ({err})")
        return
    e = info_err(got, np.asarray(cs.schur_by_feature(J, np.longdouble), np.float64), np.diag(cs.dense_u(J))) if np.all(np.isfinite(got)) else float("nan")
    print(f"g20: S error {e:.3e}")
    assert e <= BAR
