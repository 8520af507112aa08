"""No GPU: the covariance entry point is built and bound (lsfm_map_covariance, api.Context.covariance), and the -cov / -covf file
format (lsfm_save_covariances / lsfm_read_covariances, host code) round-trips."""
import ctypes as C

import numpy as np

from linearsfm_amd import api


def test_library_exports_covariance():
    L = C.CDLL(api.LIB_PATH)
    for name in ("lsfm_map_covariance", "lsfm_map_covariance_timed", "lsfm_save_covariances", "lsfm_read_covariances"):
        assert hasattr(L, name), name
    assert "lsfm_map_covariance" in api.EXPORTS


def test_context_has_covariance():
    assert callable(getattr(api.Context, "covariance", None))
    assert callable(getattr(api.Context, "covariance_raw", None))


def test_cov_file_reader_hand_written(tmp_path):
    """A hand-written -cov line: the id, then the 21 upper-triangle entries row by row."""
    A = np.arange(1, 37, dtype=float).reshape(6, 6)
    A = A + A.T
    up = [A[r, c] for r in range(6) for c in range(r, 6)]
    p = tmp_path / "pose_cov.txt"
    p.write_text("7 " + " ".join(repr(float(v)) for v in up) + "\n12 " + " ".join("0" for _ in up) + "\n")
    ids, cov = api.read_covariances(str(p), 6)
    assert list(ids) == [7, 12]
    assert np.array_equal(cov[0], A) and not cov[1].any()
    q = tmp_path / "feat_cov.txt"
    q.write_text("3 1 2 3 4 5 6\n")
    ids, cov = api.read_covariances(str(q), 3)
    assert list(ids) == [3] and np.array_equal(cov[0], np.array([[1, 2, 3], [2, 4, 5], [3, 5, 6]], float))


def test_cov_file_round_trip(tmp_path):
    """save -> read gives the same bits (%.17g), in ascending id order whatever the map's own order."""
    rng = np.random.default_rng(1)
    m, n = 4, 5
    pose_ids = np.array([9, 2, 30, 5])
    feat_ids = np.array([11, 4, 8, 1, 6])
    stno = np.concatenate([np.repeat(-pose_ids, 6), np.repeat(feat_ids, 3)]).astype(np.int32)
    P = rng.normal(size=(m, 6, 6)); P = P @ np.transpose(P, (0, 2, 1))
    F = rng.normal(size=(n, 3, 3)); F = F @ np.transpose(F, (0, 2, 1))
    d = dict(stno=stno, m=m, n=n)
    pp, fp = str(tmp_path / "p.txt"), str(tmp_path / "f.txt")
    api.save_covariances(pp, fp, d, P, F)
    ids, cov = api.read_covariances(pp, 6)
    o = np.argsort(pose_ids)
    assert np.array_equal(ids, pose_ids[o]) and np.array_equal(cov, P[o])
    ids, cov = api.read_covariances(fp, 3)
    o = np.argsort(feat_ids)
    assert np.array_equal(ids, feat_ids[o]) and np.array_equal(cov, F[o])
    assert len(open(pp).readline().split()) == 22
