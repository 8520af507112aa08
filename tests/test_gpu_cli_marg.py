"""-m gpu: the command line's -keepf <file> (the final map reduced to the listed features, every other one marginalised out:
lsfm_map_marginalise).  No reference counterpart."""
import os
import subprocess

import numpy as np
import pytest

from linearsfm_amd import api, synth
from refdump import dense_info
from test_gpu_linearise import _dense_sigma

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "linearsfm_amd", "LinearSFM")
NAMES = ("State", "Pose", "Feature", "Info", "Cov", "Chi2")


def _run(d, typ, num, outdir, extra, check=True):
    os.makedirs(outdir, exist_ok=True)
    files = {k: os.path.join(outdir, k + ".txt") for k in NAMES}
    cmd = [EXE, "-path", str(d), "-num", str(num), "-type", typ, "-st", files["State"], "-p", files["Pose"], "-f", files["Feature"],
           "-info", files["Info"], "-cov", files["Cov"], "-chi2", files["Chi2"], "-quiet", "1"] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, check=check, timeout=300)
    return files, p


def _lines(path):
    return open(path, "rb").read().splitlines()


@pytest.mark.parametrize("typ", ["Stereo", "Monocular"])
def test_keepf(ctx, tmp_path, typ):
    mono = typ == "Monocular"
    maps = synth.make_mono_set(7, 8, 4, seed=4) if mono else synth.make_stereo_set(7, 8, 4, seed=4)
    dd = tmp_path / "set"
    synth.write_set(str(dd), maps)
    ids = np.unique(np.concatenate([np.asarray(m.stno)[6 * m.m::3] for m in maps]))
    keep = ids[::3]
    kf = tmp_path / "keep.txt"
    kf.write_text(" ".join(str(int(v)) for v in keep[::-1]) + "\n 99999999\t-3\n")  # any order, any whitespace, ids nobody holds
    plain, _ = _run(dd, typ, 7, str(tmp_path / "plain"), [])
    red, _ = _run(dd, typ, 7, str(tmp_path / "red"), ["-keepf", str(kf)])
    # -info: Context.marginalise of the plain run's map
    full = api.read_localmap(plain["Info"], mono)
    fid = np.asarray(full["stno"])[6 * int(full["m"])::3]
    drop = ~np.isin(fid, keep)
    assert 0 < np.sum(~drop) == len(keep) < len(fid)
    exp = ctx.marginalise(full, drop)
    got = api.read_localmap(red["Info"], mono)
    for k in ("stno", "Ui", "Uj", "photo", "feature", "FBlock"):
        assert np.array_equal(got[k], exp[k]), k
    m, n = int(full["m"]), int(full["n"])
    I = dense_info(full)
    idx = np.concatenate([np.arange(6 * m), (6 * m + 3 * np.nonzero(~drop)[0][:, None] + np.arange(3)).reshape(-1)]).astype(np.int64)
    dg = np.diag(I)[idx]
    d = np.sqrt(np.where(dg == 0, 1.0, dg))
    e = float(np.max(np.abs(dense_info(got) - dense_info(exp)) / np.outer(d, d)))
    print(f"{typ}: -info against Context.marginalise {e:.3e}")
    assert e <= 1e-9
    # -st / -p / -f: exactly the kept ids, every line byte for byte a line of the run without the flag
    for k in ("State", "Pose", "Feature"):
        a, b = _lines(plain[k]), _lines(red[k])
        assert set(b) <= set(a), k
    assert _lines(red["Pose"]) == _lines(plain["Pose"])
    fl = _lines(red["Feature"])
    assert sorted(int(x.split()[0]) for x in fl) == sorted(int(v) for v in keep)
    sl = [int(x.split()[0]) for x in _lines(red["State"])]
    assert sl == np.asarray(got["stno"]).tolist()
    # -cov: the dense inverse of the FULL map's information matrix (Mono: gauge removed)
    S = _dense_sigma(I, full, mono)
    cid, blocks = api.read_covariances(red["Cov"], 6)
    row = {int(-s): p for p, s in enumerate(np.asarray(full["stno"])[:6 * m:6])}
    expc = np.stack([S[6 * row[int(i)]:6 * row[int(i)] + 6, 6 * row[int(i)]:6 * row[int(i)] + 6] for i in cid])
    var = np.einsum("kii->ki", expc)
    den = np.sqrt(np.maximum(var[:, :, None] * var[:, None, :], 1e-300))
    ec = float(np.max(np.abs(blocks - expc) / den))
    print(f"{typ}: -cov of the reduced map against the dense inverse of the full one {ec:.3e}")
    assert len(cid) == m and ec <= 1e-9
    # -chi2 is evaluated on the full state, before the reduction: byte for byte the file of the run without the flag, wherever the program
    # itself repeats its bytes from one process to the next.  It does not always: the tree's transforms and U sums add with atomics, two
    # runs of the SAME command were seen to differ in the 13th digit of a chi2 (4.4457...2306 against ...3068 on the Stereo set) -- nothing
    # can be identical to both.  Then index, dof and weight are held exactly and chi2 to 1e-9 relative, the bar test_gpu_parity.py holds two
    # runs of one resident tree to and test_gpu_cli_relin.py the -fullbin file of two runs of one command.
    a, c = (open(x["Chi2"], "rb").read() for x in (plain, red))
    if c != a:
        ta, tc = np.array([x.split() for x in a.splitlines()]), np.array([x.split() for x in c.splitlines()])
        assert ta.shape == tc.shape and np.array_equal(ta[:, [0, 1, 3]], tc[:, [0, 1, 3]])
        va, vc = ta[:, 2].astype(float), tc[:, 2].astype(float)
        e = float(np.max(np.abs(vc - va) / np.abs(va)))
        print(f"{typ}: the two runs' -chi2 bytes differ; with the flag against without: {e:.3e} relative")
        assert e <= 1e-9


def test_an_unreadable_keepf_file_ends_the_run(tmp_path):
    maps = synth.make_stereo_set(3, 6, 4, seed=4)
    dd = tmp_path / "set"
    synth.write_set(str(dd), maps)
    files, p = _run(dd, "Stereo", 3, str(tmp_path / "out"), ["-keepf", str(tmp_path / "missing.txt")], check=False)
    assert p.returncode != 0 and "keepf" in p.stderr
    assert not any(os.path.exists(f) for f in files.values())
