"""-m gpu: the command line's -robust and -chi2 flags (lsfm_gn_polish_robust, lsfm_map_chi2).  No reference counterpart.  The -chi2 file
holds the library's chi^2 of every local map at the state the program wrote, and the flag changes none of the other output files."""
import os
import subprocess

import numpy as np
import pytest

from linearsfm_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "linearsfm_amd", "LinearSFM")


def _run(d, typ, num, outdir, extra, check=True):
    os.makedirs(outdir, exist_ok=True)
    files = {k: os.path.join(outdir, k) for k in ("Pose.txt", "Feature.txt", "State.txt", "Full.bin")}
    cmd = [EXE, "-path", str(d), "-num", str(num), "-type", typ, "-p", files["Pose.txt"], "-f", files["Feature.txt"], "-st", files["State.txt"],
           "-fullbin", files["Full.bin"], "-quiet", "1"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, check=check, timeout=300)
    return files, r


def _state(path):
    raw = open(path, "rb").read()
    n = int(np.frombuffer(raw[:4], np.int32)[0])
    return np.frombuffer(raw[8:8 + 4 * n], np.int32), np.frombuffer(raw[8 + 4 * (n + (n & 1)):], np.float64)


def _chi2_file(path):
    rows = [l.split() for l in open(path).read().splitlines()]
    return (np.array([int(r[0]) for r in rows]), np.array([int(r[1]) for r in rows]), np.array([float(r[2]) for r in rows]),
            np.array([float(r[3]) for r in rows]))


@pytest.mark.parametrize("typ", ["Stereo", "Monocular"])
def test_robust_gn_writes_chi2_of_the_written_state(ctx, oracle, tmp_path, typ):
    """-gn 3 -robust cauchy 0.5 -chi2 f: f has one line per local map (1-based index, dof, chi2, weight), and its chi2 values are what
    Context.map_chi2 gives at the state the program wrote (raw doubles: -fullbin)."""
    mono = typ == "Monocular"
    num = 7
    maps = synth.make_mono_set(num, 8, 4, seed=4) if mono else synth.make_stereo_set(num, 8, 4, seed=4)
    d = tmp_path / "set"
    synth.write_set(str(d), maps)
    f = str(tmp_path / "chi2.txt")
    files, r = _run(d, typ, num, str(tmp_path / "rob"), ["-gn", "3", "-robust", "cauchy", "0.5", "-chi2", f])
    idx, dof, chi2, w = _chi2_file(f)
    assert np.array_equal(idx, np.arange(1, num + 1))
    assert np.array_equal(dof, [6 * m.m + 3 * m.n for m in maps])
    assert np.all((w > 0) & (w <= 1)) and np.min(w) < 1
    dd = [oracle.localmap_to_dict(m) for m in maps]
    G, _, rc = ctx.divide_conquer(dd, mono)
    assert rc == 0
    stno, st = _state(files["Full.bin"])
    assert np.array_equal(stno, G["stno"])
    exp, edof = ctx.map_chi2(dd, mono, dict(G, stVal=st))
    assert np.array_equal(dof, edof)
    assert np.max(np.abs(chi2 - exp) / exp) <= 1e-9
    np.testing.assert_allclose(w, 1.0 / (1.0 + (exp / edof) / 0.25), rtol=1e-9)


@pytest.mark.parametrize("typ", ["Stereo", "Monocular"])
def test_chi2_flag_alone_changes_no_other_file(tmp_path, typ):
    mono = typ == "Monocular"
    num = 6
    maps = synth.make_mono_set(num, 8, 4, seed=5) if mono else synth.make_stereo_set(num, 8, 4, seed=5)
    d = tmp_path / "set"
    synth.write_set(str(d), maps)
    f = str(tmp_path / "chi2.txt")
    plain, _ = _run(d, typ, num, str(tmp_path / "plain"), [])
    flagged, _ = _run(d, typ, num, str(tmp_path / "flagged"), ["-chi2", f])
    # the text files are byte-identical; the raw doubles of -fullbin carry the tree's own run-to-run variation in their last bits (present
    # without the flag too: the chi2 call runs after every file is written), so they are held to their labels and to 1e-6
    for k in ("Pose.txt", "Feature.txt", "State.txt"):
        assert open(plain[k], "rb").read() == open(flagged[k], "rb").read(), k
    (sa, va), (sb, vb) = _state(plain["Full.bin"]), _state(flagged["Full.bin"])
    assert np.array_equal(sa, sb) and np.max(np.abs(va - vb) / np.maximum(1.0, np.abs(va))) < 1e-6
    idx, dof, chi2, w = _chi2_file(f)
    assert len(idx) == num and np.all(w == 1.0) and np.all(chi2 > 0)


@pytest.mark.parametrize("extra", [["-gn", "2", "-robust", "tukey", "1"], ["-gn", "2", "-robust", "cauchy", "-1"],
                                   ["-gn", "2", "-robust", "huber", "abc"], ["-gn", "2", "-robust", "huber", "0"],
                                   ["-gn", "2", "-robust", "cauchy", "inf"], ["-gn", "2", "-robust", "cauchy"], ["-robust", "huber", "1"]])
def test_bad_robust_arguments_end_with_a_message(tmp_path, extra):
    maps = synth.make_stereo_set(3, 6, 4, seed=2)
    d = tmp_path / "set"
    synth.write_set(str(d), maps)
    _, r = _run(d, "Stereo", 3, str(tmp_path / "out"), extra, check=False)
    assert r.returncode != 0
    assert "-robust" in r.stderr
