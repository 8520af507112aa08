"""-m gpu: the command line's -keepp <file> (the final map reduced to the listed poses, every other one marginalised out with the
features it sees: lsfm_map_marginalise_poses).  No reference counterpart."""
import os

import numpy as np
import pytest

from linearsfm_amd import api, synth
from refdump import dense_info
from test_gpu_cli_marg import _lines, _run
from test_gpu_linearise import _dense_sigma
from test_marginalise_poses_cpu import gauge_poses, seen_by_dropped

pytestmark = pytest.mark.gpu


def _set(tmp_path, mono, n=7):
    maps = synth.make_mono_set(n, 8, 4, seed=4) if mono else synth.make_stereo_set(n, 8, 4, seed=4)
    dd = tmp_path / "set"
    synth.write_set(str(dd), maps)
    return dd


def _keep_list(full, mono):
    """Every second pose of the plain run's map, and the gauge poses."""
    m = int(full["m"])
    keep = np.zeros(m, bool)
    keep[::2] = True
    keep[gauge_poses(full, mono)] = True
    return keep, -np.asarray(full["stno"])[:6 * m:6][keep]


@pytest.mark.parametrize("typ", ["Stereo", "Monocular"])
def test_keepp(ctx, tmp_path, typ):
    mono = typ == "Monocular"
    dd = _set(tmp_path, mono)
    plain, _ = _run(dd, typ, 7, str(tmp_path / "plain"), [])
    full = api.read_localmap(plain["Info"], mono)
    m, n = int(full["m"]), int(full["n"])
    keep, ids = _keep_list(full, mono)
    assert 0 < np.sum(keep) < m
    kp = tmp_path / "keep.txt"
    kp.write_text(" ".join(str(int(v)) for v in ids[::-1]) + "\n 99999999\t-3\n")  # any order, any whitespace, ids nobody holds
    red, _ = _run(dd, typ, 7, str(tmp_path / "red"), ["-keepp", str(kp)])
    # -info: Context.marginalise_poses of the plain run's map
    exp = ctx.marginalise_poses(full, mono, keep)
    got = api.read_localmap(red["Info"], mono)
    for k in ("stno", "Ui", "Uj", "photo", "feature", "FBlock"):
        assert np.array_equal(got[k], exp[k]), k
    drop = seen_by_dropped(full, keep)
    I = dense_info(full)
    idx = np.concatenate([(6 * np.nonzero(keep)[0][:, None] + np.arange(6)).reshape(-1), (6 * m + 3 * np.nonzero(~drop)[0][:, None] + np.arange(3)).reshape(-1)]).astype(np.int64)
    dg = np.diag(I)[idx]
    d = np.sqrt(np.where(dg == 0, 1.0, dg))
    e = float(np.max(np.abs(dense_info(got) - dense_info(exp)) / np.outer(d, d)))
    print(f"{typ}: {int(np.sum(keep))} of {m} poses, {int(np.sum(~drop))} of {n} features kept; -info against Context.marginalise_poses {e:.3e}")
    assert e <= 1e-9
    # -st / -p / -f: exactly the kept ids, every line byte for byte a line of the run without the flag
    for k in ("State", "Pose", "Feature"):
        a, b = _lines(plain[k]), _lines(red[k])
        assert set(b) <= set(a), k
    assert [int(x.split()[0]) for x in _lines(red["State"])] == np.asarray(got["stno"]).tolist()
    assert np.array_equal(np.asarray(got["stno"]), np.asarray(full["stno"])[idx])
    fid = np.asarray(full["stno"])[6 * m::3]
    assert sorted(int(x.split()[0]) for x in _lines(red["Feature"])) == sorted(int(v) for v in fid[~drop])
    # -cov: the dense inverse of the FULL map's information matrix (Mono: gauge removed), the kept poses
    S = _dense_sigma(I, full, mono)
    cid, blocks = api.read_covariances(red["Cov"], 6)
    row = {int(-s): p for p, s in enumerate(np.asarray(full["stno"])[:6 * m:6])}
    assert sorted(int(i) for i in cid) == sorted(int(v) for v in ids)
    expc = np.stack([S[6 * row[int(i)]:6 * row[int(i)] + 6, 6 * row[int(i)]:6 * row[int(i)] + 6] for i in cid])
    var = np.einsum("kii->ki", expc)
    den = np.sqrt(np.maximum(var[:, :, None] * var[:, None, :], 1e-300))
    ec = float(np.max(np.abs(blocks - expc) / den))
    print(f"{typ}: -cov of the reduced map against the dense inverse of the full one {ec:.3e}")
    assert ec <= 1e-9
    # -chi2 is evaluated on the full state: index, dof and weight exactly the plain run's, chi2 within what two runs of one command differ by
    ta, tc = (np.array([x.split() for x in _lines(f["Chi2"])]) for f in (plain, red))
    assert ta.shape == tc.shape and np.array_equal(ta[:, [0, 1, 3]], tc[:, [0, 1, 3]])
    assert float(np.max(np.abs(tc[:, 2].astype(float) - ta[:, 2].astype(float)) / np.abs(ta[:, 2].astype(float)))) <= 1e-9


def test_keepp_with_keepf(ctx, tmp_path):
    """Together with -keepf the dropped features are those -keepf drops plus those a dropped pose sees."""
    dd = _set(tmp_path, False)
    plain, _ = _run(dd, "Stereo", 7, str(tmp_path / "plain"), [])
    full = api.read_localmap(plain["Info"], False)
    m = int(full["m"])
    keep = np.ones(m, bool)
    keep[m - 1] = False
    fid = np.asarray(full["stno"])[6 * m::3]
    kf, kp = tmp_path / "kf.txt", tmp_path / "kp.txt"
    kf.write_text("\n".join(str(int(v)) for v in fid[::2]))
    kp.write_text("\n".join(str(int(v)) for v in -np.asarray(full["stno"])[:6 * m:6][keep]))
    red, _ = _run(dd, "Stereo", 7, str(tmp_path / "red"), ["-keepp", str(kp), "-keepf", str(kf)])
    drop = seen_by_dropped(full, keep) | ~np.isin(fid, fid[::2])
    assert 0 < np.sum(~drop) < len(fid[::2])  # both flags took features away
    exp = ctx.marginalise_poses(full, False, keep, drop)
    got = api.read_localmap(red["Info"], False)
    for k in ("stno", "Ui", "Uj", "photo", "feature", "FBlock"):
        assert np.array_equal(got[k], exp[k]), k


def test_the_error_exits_write_no_file(tmp_path):
    dd = _set(tmp_path, True, 3)
    files, p = _run(dd, "Monocular", 3, str(tmp_path / "a"), ["-keepp", str(tmp_path / "missing.txt")], check=False)
    assert p.returncode != 0 and "keepp" in p.stderr
    assert not any(os.path.exists(f) for f in files.values())
    # a list without the gauge poses
    plain, _ = _run(dd, "Monocular", 3, str(tmp_path / "plain"), [])
    full = api.read_localmap(plain["Info"], True)
    ids = [int(v) for v in -np.asarray(full["stno"])[:6 * int(full["m"]):6]]
    nog = tmp_path / "nogauge.txt"
    nog.write_text(" ".join(str(v) for v in ids if v != int(full["Ref"])))
    files, p = _run(dd, "Monocular", 3, str(tmp_path / "b"), ["-keepp", str(nog)], check=False)
    assert p.returncode != 0 and "Ref pose" in p.stderr
    assert not any(os.path.exists(f) for f in files.values())
    # -covposes naming a dropped pose
    gone = [v for v in ids if v not in (int(full["Ref"]), int(full["ScaP"]))][-1]
    most = tmp_path / "most.txt"
    most.write_text(" ".join(str(v) for v in ids if v != gone))
    cols = str(tmp_path / "c" / "cols.txt")
    files, p = _run(dd, "Monocular", 3, str(tmp_path / "c"), ["-keepp", str(most), "-covcols", cols, "-covposes", str(gone)], check=False)
    assert p.returncode != 0 and f"no pose {gone}" in p.stderr
    assert not any(os.path.exists(f) for f in list(files.values()) + [cols])
