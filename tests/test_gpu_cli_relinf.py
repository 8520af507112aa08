"""-m gpu: the command line's -relinf 1 (lsfm_gn_linearise_features at the state -gn -robustf ended at, with that polish's feature
weights: the matrix -info, -cov and every later flag describe is the one the polish's last step solved with).  No reference counterpart."""
import os
import subprocess

import numpy as np
import pytest

from linearsfm_amd import api, synth
from refdump import dense_info

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "linearsfm_amd", "LinearSFM")
NUM = 9
ROBUSTF = ["-gn", "3", "-robustf", "huber", "1.5"]


def _run(d, typ, outdir, extra, check=True):
    os.makedirs(outdir, exist_ok=True)
    files = {k: os.path.join(outdir, k + ".txt") for k in ("State", "Pose", "Feature", "Info", "Cov", "Chi2f")}
    cmd = [EXE, "-path", str(d), "-num", str(NUM), "-type", typ, "-st", files["State"], "-p", files["Pose"], "-f", files["Feature"],
           "-info", files["Info"], "-cov", files["Cov"], "-chi2f", files["Chi2f"], "-quiet", "1"] + extra
    return files, subprocess.run(cmd, capture_output=True, text=True, check=check, timeout=300)


def _set(tmp_path, mono):
    """A 9-map set with the estimate of feature 2 of map 4 moved by 30 sigma (as rf.corrupt_features moves it): a weight far below 1."""
    maps = synth.make_mono_set(NUM, 8, 4, seed=4) if mono else synth.make_stereo_set(NUM, 8, 4, seed=4)
    m, f = maps[3], 2
    st = np.array(m.stVal, np.float64, copy=True)
    st[6 * m.m + 3 * f:6 * m.m + 3 * f + 3] += 30.0 * np.sqrt(np.diag(np.linalg.inv(np.asarray(m.V, np.float64).reshape(-1, 3, 3)[f]))) * np.array([1.0, -1.0, 1.0])
    m.stVal = st
    dd = tmp_path / "set"
    synth.write_set(str(dd), maps)
    return dd, [m.__dict__ for m in maps]


def _h_err(got, exp):
    d = np.sqrt(np.diag(exp))
    return float(np.max(np.abs(got - exp) / np.outer(d, d)))


@pytest.mark.parametrize("typ", ["Stereo", "Monocular"])
def test_relinf_after_the_feature_robust_polish(ctx, tmp_path, typ):
    """-gn 3 -robustf huber 1.5 -relinf 1 -info -cov -chi2f on a 9-map set.  The -info file against Context.gn_linearise at the state
    it holds with the weights of the -chi2f file (written at %.17g: they come back exactly): values to 1e-13 (two assemblies at the same
    bits differ by the order of their atomic sums), the index arrays the same; the -cov file to 1e-9; -st, -p and -f byte for byte what
    the run without the flag writes; the matrix is not the one of that run."""
    mono = typ == "Monocular"
    dd, d = _set(tmp_path, mono)
    files, _ = _run(dd, typ, str(tmp_path / "relinf"), ROBUSTF + ["-relinf", "1"])
    plain, _ = _run(dd, typ, str(tmp_path / "plain"), ROBUSTF)
    rows = [l.split() for l in open(files["Chi2f"]).read().splitlines()]
    w = np.array([float(r[3]) for r in rows])
    assert len(w) == sum(int(m["n"]) for m in d) and np.all((w > 0) & (w <= 1)) and np.any(w < 1)
    x = api.read_localmap(files["Info"], mono)  # (the state at %.17g, Ref / ScaP / Fix and the pose origins)
    H, _, _ = ctx.gn_linearise(d, mono, x, feature_weight=w)
    got = synth.read_localmap(files["Info"], mono).__dict__
    e = _h_err(dense_info(got), dense_info(H))
    print(f"{typ}: -info against the call {e:.3e}; {int(np.sum(w < 1))} of {len(w)} weights below 1, smallest {np.min(w):.3f}")
    assert e <= 1e-13
    for k in ("Ui", "Uj", "photo", "feature", "FBlock"):
        assert np.array_equal(x[k], H[k]), k
    cov = ctx.covariance(H, mono)["pose"]
    ids, blocks = api.read_covariances(files["Cov"], 6)
    row = {int(-s): p for p, s in enumerate(np.asarray(H["stno"])[:6 * int(H["m"]):6])}
    exp = cov[[row[int(i)] for i in ids]]
    var = np.einsum("kii->ki", exp)
    den = np.sqrt(np.maximum(var[:, :, None] * var[:, None, :], 1e-300))
    assert float(np.max(np.abs(blocks - exp) / den)) <= 1e-9
    for k in ("State", "Pose", "Feature"):
        assert open(files[k], "rb").read() == open(plain[k], "rb").read(), k
    assert open(files["Info"], "rb").read() != open(plain["Info"], "rb").read()
    # the unweighted linearisation at the same state is another matrix: the weights did arrive
    H1, _, _ = ctx.gn_linearise(d, mono, x)
    assert _h_err(dense_info(got), dense_info(H1)) > 1e-6


@pytest.mark.parametrize("extra,word", [(["-gn", "3", "-relinf", "1"], "-robustf"), (["-relinf", "1"], "-robustf"),
                                        (["-gn", "3", "-robust", "huber", "1.5", "-relinf", "1"], "-robustf"),
                                        (["-gn", "3", "-relinf", "1", "-relin", "1"], "-relin")])
def test_relinf_refusals_write_no_file(tmp_path, extra, word):
    """-relinf without -robustf, or together with -relin 1: a message that names both, a non-zero exit, no file written."""
    dd = tmp_path / "set"
    synth.write_set(str(dd), synth.make_stereo_set(NUM, 6, 4, seed=2))
    files, r = _run(dd, "Stereo", str(tmp_path / "out"), extra, check=False)
    assert r.returncode != 0
    assert "-relinf" in r.stderr and word in r.stderr
    assert not any(os.path.exists(p) for p in files.values())
