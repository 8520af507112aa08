"""No GPU: the covariance-columns entry points are built and bound (lsfm_map_covariance_columns(_timed), api.Context.covariance_columns),
and the -covcols file format (lsfm_save_cov_columns / lsfm_read_cov_columns, host code) round-trips."""
import ctypes as C

import numpy as np
import pytest

from linearsfm_amd import api


def test_library_exports_cov_columns():
    L = C.CDLL(api.LIB_PATH)
    for name in ("lsfm_map_covariance_columns", "lsfm_map_covariance_columns_timed", "lsfm_save_cov_columns", "lsfm_read_cov_columns"):
        assert hasattr(L, name), name
        assert name in api.EXPORTS


def test_context_has_cov_columns():
    assert callable(getattr(api.Context, "covariance_columns", None))
    assert callable(getattr(api.Context, "covariance_columns_raw", None))
    assert callable(getattr(api, "save_cov_columns", None)) and callable(getattr(api, "read_cov_columns", None))


def test_cov_columns_reader_hand_written(tmp_path):
    """A hand-written file: per line the requested pose's id, the pose's id, then the 36 entries of the block row by row."""
    A = np.arange(1, 37, dtype=float).reshape(6, 6)
    p = tmp_path / "cols.txt"
    p.write_text("7 3 " + " ".join(repr(float(v)) for v in A.ravel()) + "\n7 12 " + " ".join("0" for _ in range(36)) + "\n")
    iq, ip, blk = api.read_cov_columns(str(p))
    assert list(iq) == [7, 7] and list(ip) == [3, 12]
    assert np.array_equal(blk[0], A) and not blk[1].any()


@pytest.mark.parametrize("k", [1, 3])
def test_cov_columns_round_trip(tmp_path, k):
    """save -> read is the identity at %.17g (negative zero and 1e300 included): requested poses in the order given, within one the
    poses in ascending id whatever the map's own order."""
    rng = np.random.default_rng(2)
    m = 4
    pose_ids = np.array([9, 2, 30, 5])
    stno = np.concatenate([np.repeat(-pose_ids, 6), np.repeat([4, 1], 3)]).astype(np.int32)
    poses = [2, 0, 3][:k]  # ids 30, 9, 5: out of order
    P = rng.normal(size=(k, m, 6, 6))
    P[0, 1, 0, 0] = -0.0
    P[0, 2, 5, 5] = 1e300
    P[0, 3, 2, 1] = -1e-300
    path = str(tmp_path / "c.txt")
    api.save_cov_columns(path, dict(stno=stno, m=m, n=2), poses, P)
    iq, ip, blk = api.read_cov_columns(path)
    o = np.argsort(pose_ids)
    assert len(iq) == k * m
    assert np.array_equal(iq, np.repeat(pose_ids[poses], m))
    assert np.array_equal(ip, np.tile(pose_ids[o], k))
    exp = P[:, o].reshape(k * m, 6, 6)
    assert np.array_equal(blk, exp)
    assert np.array_equal(np.signbit(blk), np.signbit(exp))
    assert len(open(path).readline().split()) == 38


def test_cov_columns_truncated_line_is_refused(tmp_path):
    p = tmp_path / "cut.txt"
    full = "1 2 " + " ".join("0.5" for _ in range(36)) + "\n"
    p.write_text(full + "1 3 " + " ".join("0.5" for _ in range(20)) + "\n")
    with pytest.raises(api.LsfmError):
        api.read_cov_columns(str(p))
    p.write_text(full + "4\n")
    with pytest.raises(api.LsfmError):
        api.read_cov_columns(str(p))
    # an index outside the map is refused by the writer
    with pytest.raises(api.LsfmError):
        api.save_cov_columns(str(tmp_path / "x.txt"), dict(stno=np.repeat([-1, -2], 6).astype(np.int32), m=2, n=0), [2], np.zeros((1, 2, 6, 6)))
