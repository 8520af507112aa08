"""-m gpu: the command line's -relin 1 (lsfm_gn_linearise at the final state: the information matrix that -info, -cov, -covf and -covcols
describe is the one of the estimate the other files hold).  No reference counterpart."""
import os
import subprocess

import numpy as np
import pytest

from linearsfm_amd import api, synth
from refdump import dense_info

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "linearsfm_amd", "LinearSFM")
STATE_FILES = ("State", "Pose", "Feature", "FullBin")


def _run(d, typ, num, outdir, extra):
    os.makedirs(outdir, exist_ok=True)
    files = {k: os.path.join(outdir, k + ".txt") for k in STATE_FILES + ("Info", "Cov")}
    cmd = [EXE, "-path", str(d), "-num", str(num), "-type", typ, "-st", files["State"], "-p", files["Pose"], "-f", files["Feature"],
           "-fullbin", files["FullBin"], "-info", files["Info"], "-cov", files["Cov"], "-quiet", "1"] + extra
    subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=300)
    return files


def _h_err(got, exp):
    d = np.sqrt(np.diag(exp))
    return float(np.max(np.abs(got - exp) / np.outer(d, d)))


def _set(tmp_path, mono):
    maps = synth.make_mono_set(7, 8, 4, seed=4) if mono else synth.make_stereo_set(7, 8, 4, seed=4)
    dd = tmp_path / "set"
    synth.write_set(str(dd), maps)
    return dd, [m.__dict__ for m in maps]


def _against_the_api(ctx, d, mono, files):
    """The -info and -cov files of a -relin run against Context.gn_linearise / Context.covariance at the state the run wrote."""
    x = api.read_localmap(files["Info"], mono)  # (the state at %.17g, Ref / ScaP / Fix and the pose origins; its U / W / V are not read)
    H, _, _ = ctx.gn_linearise(d, mono, x)
    # two assemblies at the same bits differ by the order of their atomic sums only: the bar of test_gpu_linearise.py::test_weights
    got = synth.read_localmap(files["Info"], mono).__dict__
    assert _h_err(dense_info(got), dense_info(H)) <= 1e-13
    for k in ("Ui", "Uj", "photo", "feature", "FBlock"):
        assert np.array_equal(x[k], H[k]), k
    cov = ctx.covariance(H, mono)["pose"]
    ids, blocks = api.read_covariances(files["Cov"], 6)
    row = {int(-s): p for p, s in enumerate(np.asarray(H["stno"])[:6 * int(H["m"]):6])}
    exp = cov[[row[int(i)] for i in ids]]
    var = np.einsum("kii->ki", exp)
    den = np.sqrt(np.maximum(var[:, :, None] * var[:, None, :], 1e-300))
    assert float(np.max(np.abs(blocks - exp) / den)) <= 1e-9
    return blocks


@pytest.mark.parametrize("typ", ["Stereo", "Monocular"])
def test_relin_after_gn(ctx, tmp_path, typ):
    mono = typ == "Monocular"
    dd, d = _set(tmp_path, mono)
    relin = _run(dd, typ, 7, str(tmp_path / "relin"), ["-gn", "2", "-relin", "1"])
    plain = _run(dd, typ, 7, str(tmp_path / "plain"), ["-gn", "2"])
    again = _run(dd, typ, 7, str(tmp_path / "again"), ["-gn", "2"])
    blocks = _against_the_api(ctx, d, mono, relin)
    # the flag changes what describes the estimate, not the estimate: the state files are byte-identical with and without it wherever the
    # program itself repeats its bytes from one process to the next.  The polish sums with atomics, so two runs of the SAME command differ
    # in the last bits of the raw doubles (-fullbin; measured in bytes 1040.. of the file) -- nothing can be identical to both; there the
    # file is held to its size, its labels and to 1e-9, the bar test_gpu_robust.py holds two calls of the plain polish to.
    for k in STATE_FILES:
        a, b, c = (open(x[k], "rb").read() for x in (plain, again, relin))
        if a == b:
            assert a == c, k
        else:
            assert k == "FullBin" and len(a) == len(c), k
            n = int(np.frombuffer(a[:4], np.int32)[0])
            o = 8 + 4 * (n + (n & 1))
            assert a[:o] == c[:o]
            va, vc = np.frombuffer(a[o:], np.float64), np.frombuffer(c[o:], np.float64)
            assert np.max(np.abs(va - vc) / np.maximum(1.0, np.abs(va))) <= 1e-9
    _, pb = api.read_covariances(plain["Cov"], 6)
    assert pb.shape == blocks.shape and not np.array_equal(pb, blocks)
    assert open(relin["Info"], "rb").read() != open(plain["Info"], "rb").read()


@pytest.mark.parametrize("typ", ["Stereo", "Monocular"])
def test_relin_without_gn(ctx, tmp_path, typ):
    """The tree's state, relinearised."""
    mono = typ == "Monocular"
    dd, d = _set(tmp_path, mono)
    _against_the_api(ctx, d, mono, _run(dd, typ, 7, str(tmp_path / "relin"), ["-relin", "1"]))

