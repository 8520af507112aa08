"""-m gpu: the command line's -cov / -covf files (marginal covariances of the final map: lsfm_map_covariance, lsfm_save_covariances).
No reference counterpart.  The files hold what the library's entry point gives for the same map, bit for bit through %.17g, and the
flags change none of the other output files."""
import os
import subprocess

import numpy as np
import pytest

from linearsfm_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "linearsfm_amd", "LinearSFM")


def _run(d, typ, num, outdir, extra):
    os.makedirs(outdir, exist_ok=True)
    files = {k: os.path.join(outdir, k + ".txt") for k in ("Pose", "Feature", "State", "Full", "Info")}
    cmd = [EXE, "-path", str(d), "-num", str(num), "-type", typ, "-p", files["Pose"], "-f", files["Feature"], "-st", files["State"],
           "-full", files["Full"], "-info", files["Info"], "-quiet", "1"] + extra
    subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=300)
    return files


@pytest.mark.parametrize("typ", ["Stereo", "Monocular"])
def test_cov_files_match_api(ctx, tmp_path, typ):
    mono = typ == "Monocular"
    num = 7
    maps = synth.make_mono_set(num, 8, 4, seed=43, lap=5, home=2) if mono else synth.make_stereo_set(num, 8, 4, seed=43, lap=5, home=2)
    d = tmp_path / "set"
    synth.write_set(str(d), maps)
    cov, covf = str(tmp_path / "pose_cov.txt"), str(tmp_path / "feat_cov.txt")
    plain = _run(d, typ, num, str(tmp_path / "plain"), [])
    again = _run(d, typ, num, str(tmp_path / "again"), [])
    flagged = _run(d, typ, num, str(tmp_path / "flagged"), ["-cov", cov, "-covf", covf])
    # the existing outputs: byte-identical with and without the flags wherever the program itself repeats its bytes from one process to
    # the next (the %.17g files carry the tree's own run-to-run variation in the last digits -- present without the flags, the covariance
    # call runs after they are written; measured up to 1.4e-9 relative in a Mono -info file); those are held to their layout and to 1e-6
    for k in plain:
        a, b, c = (open(x[k], "rb").read() for x in (plain, again, flagged))
        if a == b:
            assert a == c, k
        else:
            ta, tc = a.decode().split(), c.decode().split()
            assert len(ta) == len(tc), k
            for u, v in zip(ta, tc):
                if u != v:
                    assert abs(float(u) - float(v)) <= 1e-6 * max(1.0, abs(float(u))), (k, u, v)
    # the map the command line wrote (-info: %.17g, pose origins included) through the library's entry point
    G = api.read_localmap(flagged["Info"], mono)
    out = ctx.covariance(G, mono)
    m, n = int(G["m"]), int(G["n"])
    pids, pc = api.read_covariances(cov, 6)
    fids, fc = api.read_covariances(covf, 3)
    # one line per pose / feature, in the order of the pose / feature files
    pose_ids = np.loadtxt(plain["Pose"], ndmin=2)[:, 0].astype(int)
    feat_ids = np.loadtxt(plain["Feature"], ndmin=2)[:, 0].astype(int)
    assert np.array_equal(pids, pose_ids) and np.array_equal(fids, feat_ids)
    stno = np.asarray(G["stno"])
    prow = {int(-stno[6 * p]): p for p in range(m)}
    frow = {int(stno[6 * m + 3 * f]): f for f in range(n)}
    assert np.array_equal(pc, out["pose"][[prow[i] for i in pids]])
    assert np.array_equal(fc, out["feature"][[frow[i] for i in fids]])
    # the file's text is %.17g of those values
    first = open(cov).readline().split()
    assert len(first) == 22 and len(open(covf).readline().split()) == 7
