"""No GPU: the feature-column and pair-gate entry points are built, declared and bound (lsfm_map_covariance_feature_columns(_timed),
lsfm_map_feature_pair_gate(_timed)), the -gateout file format round-trips (lsfm_save_pair_gate / lsfm_read_pair_gate, host code), and
the two host statements of the gate that the GPU tests measure against (feature_cov_reference.py) agree with each other on the
oracle's trees of the eight small sets -- the floor under the GPU tests' bars -- and show why the cross term matters."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from linearsfm_amd import api
import feature_cov_reference as ref
from test_gpu_covariance import SMALL, _small_set, dense_sigma

NAMES = ("lsfm_map_covariance_feature_columns", "lsfm_map_covariance_feature_columns_timed", "lsfm_map_feature_pair_gate",
         "lsfm_map_feature_pair_gate_timed", "lsfm_save_pair_gate", "lsfm_read_pair_gate")


def test_symbols_exported_declared_and_bound():
    L = C.CDLL(api.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "lsfm.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in api.EXPORTS
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert getattr(api.lib(), name).argtypes is not None
    for meth in ("covariance_feature_columns", "covariance_feature_columns_raw", "feature_pair_gate", "feature_pair_gate_raw"):
        assert callable(getattr(api.Context, meth, None)), meth
    assert callable(getattr(api, "save_pair_gate", None)) and callable(getattr(api, "read_pair_gate", None))


def test_gate_reader_hand_written(tmp_path):
    """A hand-written file: per line the two labels, d2, then the upper triangle of Sigma_d row by row."""
    p = tmp_path / "gate.txt"
    p.write_text("17 9021 2.5 1 2 3 4 5 6\n3 4 nan 0 0 0 0 0 0\n")
    ids, d2, cov = api.read_pair_gate(str(p))
    assert ids.tolist() == [[17, 9021], [3, 4]]
    assert d2[0] == 2.5 and np.isnan(d2[1])
    assert np.array_equal(cov[0], [[1, 2, 3], [2, 4, 5], [3, 5, 6]]) and not cov[1].any()


def test_gate_round_trip(tmp_path):
    """save -> read is the identity at %.17g, negative zero and 1e300 included, pairs in the order given."""
    rng = np.random.default_rng(2)
    K = 5
    ids = np.array([[9, 2], [30, 5], [2, 9], [7, 8], [1, 100000]])
    d2 = rng.random(K)
    A = rng.normal(size=(K, 3, 3))
    cov = A + np.transpose(A, (0, 2, 1))
    cov[0, 0, 1] = cov[0, 1, 0] = -0.0
    cov[1, 2, 2] = 1e300
    d2[2] = 1e300
    d2[3] = -0.0
    path = str(tmp_path / "g.txt")
    api.save_pair_gate(path, ids, d2, cov)
    i2, dd, cc = api.read_pair_gate(path)
    assert np.array_equal(i2, ids) and np.array_equal(dd, d2) and np.array_equal(cc, cov)
    assert np.array_equal(np.signbit(dd), np.signbit(d2)) and np.array_equal(np.signbit(cc), np.signbit(cov))
    assert len(open(path).readline().split()) == 9
    assert not os.path.exists(path + ".tmp")


def test_gate_truncated_line_is_refused(tmp_path):
    p = tmp_path / "cut.txt"
    full = "1 2 0.5 1 0 0 1 0 1\n"
    p.write_text(full + "1 3 0.5 1 0 0\n")
    with pytest.raises(api.LsfmError):
        api.read_pair_gate(str(p))
    p.write_text(full + "4\n")
    with pytest.raises(api.LsfmError):
        api.read_pair_gate(str(p))
    with pytest.raises(api.LsfmError):
        api.save_pair_gate(str(tmp_path / "x.txt"), [[1, 2]], [0.5, 0.25], np.zeros((1, 3, 3)))


# ---- the host reference: two routes on the oracle's trees -----------------------------------------------------------------------------
_ROUTES = {}


def _routes(oracle, i):
    if i not in _ROUTES:
        mono, n, kw = SMALL[i]
        G, _, rc = oracle.divide_conquer([oracle.localmap_to_dict(mp) for mp in _small_set(mono, n, kw)], mono)
        assert rc == 0
        G = ref.symmetric_blocks(G)  # (both routes on the same SYMMETRIC matrix: see there)
        pairs = ref.seeded_pairs(int(G["n"]))
        covA, marg = ref.route_a(dense_sigma(G, mono), G, pairs)
        _ROUTES[i] = (G, pairs, covA, marg, ref.route_b(G, mono, pairs))
    return _ROUTES[i]


@pytest.mark.parametrize("i", range(len(SMALL)))
def test_host_routes_agree(oracle, i):
    """The floor: the dense inverse and the difference formulation agree on Sigma_d below 1e-10 in both normalisations (its own
    diagonal, the marginals' diagonal) and on d2 below 1e-10 relative, on the oracle's tree with its diagonal blocks made exactly
    symmetric (feature_cov_reference.symmetric_blocks: on the tree as stored a general inverse and a Cholesky route answer for two
    different matrices -- 1.1e-10 apart on the 40-map Mono set).  Measured: Stereo <= 1.1e-13 / 1.2e-13, d2 3.0e-14; Mono <= 1.8e-11
    (own diagonal), 3.1e-11 (marginal diagonal), d2 1.9e-11.  The derived d2 bar of the GPU tests stays below its cap on every pair
    (largest 1.2e-4)."""
    G, pairs, covA, marg, covB = _routes(oracle, i)
    dx = ref.state_diff(G, pairs)
    own = ref.cov_err(covB, covA, np.einsum("kii->ki", covA))
    mar = ref.cov_err(covB, covA, np.einsum("kii->ki", marg))
    dA, dB = ref.d2_of(covA, dx), ref.d2_of(covB, dx)
    rel = float(np.max(np.abs(dB - dA) / dA))
    bars = ref.d2_bars(covA, marg)
    print(f"host routes {SMALL[i][:2]}: {len(pairs)} pairs, Sigma_d own {own:.2e} marginal {mar:.2e}, d2 {rel:.2e}, largest d2 bar {bars.max():.2e}")
    assert own < 1e-10 and mar < 1e-10 and rel < 1e-10
    assert bars.max() < ref.BAR_D2_CAP


@pytest.mark.parametrize("i,bound", [(6, 0.5), (2, 0.3)])
def test_cross_term_matters(oracle, i, bound):
    """Why the feature exists: a gate that ignores Sigma_fg reports d2 far below the true value for some pair -- below 0.5x on the
    Mono 9-map set (measured 0.45), below 0.3x on the Stereo 9-map set (measured 0.20)."""
    assert SMALL[i][1] == 9
    G, pairs, covA, marg, _ = _routes(oracle, i)
    dx = ref.state_diff(G, pairs)
    ratio = ref.d2_of(marg, dx) / ref.d2_of(covA, dx)
    print(f"marginal-only / exact d2 {SMALL[i][:2]}: min {ratio.min():.3f}")
    assert ratio.min() < bound
