"""-m gpu: the command line's -covcols <file> -covposes <id,id,...> (whole covariance columns of the final map for poses named by label:
lsfm_map_covariance_columns, lsfm_save_cov_columns).  No reference counterpart.  The file holds what the library's entry point gives
for the same map (to the tolerance test_gpu_cli_cov.py holds the other %.17g files to: the columns are not bit-reproducible from call
to call), one line per (requested pose, pose), and the flags change none of the other output files."""
import os
import subprocess

import numpy as np
import pytest

from linearsfm_amd import api, synth
from test_gpu_cli_cov import EXE, _run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("typ", ["Stereo", "Monocular"])
def test_covcols_file_matches_api(ctx, tmp_path, typ):
    mono = typ == "Monocular"
    num = 7
    maps = synth.make_mono_set(num, 8, 4, seed=43, lap=5, home=2) if mono else synth.make_stereo_set(num, 8, 4, seed=43, lap=5, home=2)
    d = tmp_path / "set"
    synth.write_set(str(d), maps)
    cols = str(tmp_path / "cols.txt")
    plain = _run(d, typ, num, str(tmp_path / "plain"), [])
    again = _run(d, typ, num, str(tmp_path / "again"), [])
    pose_ids = np.loadtxt(plain["Pose"], ndmin=2)[:, 0].astype(int)
    want = [int(pose_ids[-1]), int(pose_ids[1]), int(pose_ids[len(pose_ids) // 2])]  # by label, out of order
    flagged = _run(d, typ, num, str(tmp_path / "flagged"), ["-covcols", cols, "-covposes", ",".join(str(i) for i in want)])
    # the other outputs: as test_gpu_cli_cov.py holds them
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
    G = api.read_localmap(flagged["Info"], mono)
    m = int(G["m"])
    stno = np.asarray(G["stno"])
    prow = {int(-stno[6 * p]): p for p in range(m)}
    out = ctx.covariance_columns(G, mono, [prow[i] for i in want])
    iq, ip, blk = api.read_cov_columns(cols)
    # one line per (requested pose, pose): requested poses in the order given, within one the pose file's order
    assert len(iq) == len(want) * m == sum(1 for line in open(cols) if line.strip())
    assert np.array_equal(iq, np.repeat(want, m)) and np.array_equal(ip, np.tile(pose_ids, len(want)))
    exp = np.stack([out["pose"][a, prow[i]] for a in range(len(want)) for i in pose_ids])
    assert np.all(np.abs(blk - exp) <= 1e-6 * np.maximum(1.0, np.abs(exp))), float(np.max(np.abs(blk - exp)))
    assert len(open(cols).readline().split()) == 38
    assert not os.path.exists(cols + ".tmp")


def test_covcols_flag_errors(tmp_path):
    num = 3
    d = tmp_path / "set"
    synth.write_set(str(d), synth.make_stereo_set(num, 8, 4, seed=43))
    cols = str(tmp_path / "cols.txt")
    pose = str(tmp_path / "Pose.txt")
    base = [EXE, "-path", str(d), "-num", str(num), "-type", "Stereo", "-quiet", "1", "-p", pose, "-f", str(tmp_path / "Feature.txt")]

    def run(extra):
        return subprocess.run(base + extra, capture_output=True, text=True, timeout=300)

    r = run([])
    assert r.returncode == 0, r.stderr
    ids = np.loadtxt(pose, ndmin=2)[:, 0].astype(int)
    os.remove(pose)
    two = f"{ids[0]},{ids[-1]}"
    for extra in (["-covcols", cols], ["-covposes", two], ["-covcols", cols, "-covposes", f"{ids[0]},x"]):
        r = run(extra)
        assert r.returncode != 0 and "-covposes" in r.stderr, (extra, r.returncode, r.stderr)
        assert not os.path.exists(cols) and not os.path.exists(pose)
    r = run(["-covcols", cols, "-covposes", f"{ids[0]},999999"])  # an id no pose has: a message, nothing written
    assert r.returncode != 0 and "999999" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(cols) and not os.path.exists(pose)
    r = run(["-covcols", cols, "-covposes", two])
    assert r.returncode == 0, r.stderr
    assert os.path.exists(cols) and os.path.exists(pose)
    assert sum(1 for line in open(cols) if line.strip()) == 2 * len(ids)
