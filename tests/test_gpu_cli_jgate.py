"""-m gpu: the command line's -jgate <pairs file> -jgateout <file> [-jgatetau <tau>] [-jgatepairs <file>] (lsfm_map_feature_pair_joint_gate,
lsfm_save_joint_gate).  No reference counterpart.  On the 9-map set with features split in two (merge_reference.split_set) the report holds
what the library's entry point gives for the map -info wrote, the -jgatepairs file is what -merge reads in a second run, and every refusal
ends the run non-zero with nothing written."""
import json
import os
import subprocess

import numpy as np
import pytest

import joint_gate_reference as jref
import merge_reference as ref
from linearsfm_amd import api
from test_gpu_cli_cov import EXE, _run
from test_gpu_covariance import dense_sigma
from test_gpu_cli_merge import COUNT, _split_files

pytestmark = pytest.mark.gpu


def _pairs_text(chosen, G):
    """The split pairs (every second one reversed), one of them again, and two wrong pairs between features of different split points."""
    want = [(i, i + ref.SPLIT_OFFSET) if k % 2 == 0 else (i + ref.SPLIT_OFFSET, i) for k, i in enumerate(chosen)]
    want.append(want[0][::-1])
    want += [(chosen[0], chosen[1]), (chosen[2] + ref.SPLIT_OFFSET, chosen[3])]
    return want


@pytest.mark.parametrize("typ", ["Stereo", "Monocular"])
def test_jgate_files_match_api_and_feed_the_merge(ctx, tmp_path, typ):
    mono = typ == "Monocular"
    num = 9
    d, chosen = _split_files(tmp_path, mono, num)
    plain_js = str(tmp_path / "plain.json")
    plain = _run(d, typ, num, str(tmp_path / "plain"), ["-json", plain_js])
    G = api.read_localmap(plain["Info"], mono)
    want = _pairs_text(chosen, G)
    pairs_file = tmp_path / "pairs.txt"
    pairs_file.write_text("\n".join(f"{a} {b}" for a, b in want) + "\n")
    report, acc_file, js = str(tmp_path / "jgate.txt"), str(tmp_path / "accepted.txt"), str(tmp_path / "run.json")
    run = _run(d, typ, num, str(tmp_path / "j"), ["-jgate", str(pairs_file), "-jgateout", report, "-jgatepairs", acc_file, "-json", js])
    at = {int(l): f for f, l in enumerate(ref.feature_ids(G))}
    idx = np.array([(at[a], at[b]) for a, b in want], np.int32)
    exp = ctx.feature_pair_joint_gate(G, mono, idx)
    sel = jref.select(jref.joint_matrix(dense_sigma(G, mono), int(G["m"]), idx), jref.state_diff(G, idx), idx, jref.TAU,
                      order=jref.default_order(exp["d2"]))
    assert jref.margins(sel, jref.TAU) > 1e-4  # (two processes, two trees: the file and the API agree to 1e-5 below)
    r = api.read_joint_gate(report)
    print(f"-jgate {typ}: K {r['K']}, accepted {r['accepted']}, implied {r['implied']}, D2 file {r['D2']:.9g}, API on the plain run's map {exp['D2']:.9g}")
    assert r["ids"].tolist() == [list(p) for p in want]
    # pair COUNT is pair 0 reversed: the two tie in d2 up to the last bits of a run, so which of them is accepted and which implied may differ
    # between the file's process and this one; every other status is the same
    twins = [0, COUNT]
    rest = [b for b in range(len(want)) if b not in twins]
    assert np.array_equal(exp["status"], sel["status"])
    assert np.array_equal(r["status"][rest], exp["status"][rest]) and sorted(r["status"][twins]) == sorted(exp["status"][twins]) == [1, 2]
    assert (r["K"], r["accepted"], r["implied"], r["dof"]) == (len(want), exp["accepted"], exp["implied"], exp["dof"])
    assert r["accepted"] == COUNT and r["implied"] == 1 and r["status"][rest].tolist() == [1] * (COUNT - 1) + [0, 0]
    assert np.all(np.isfinite(r["delta"])) and np.all(np.isfinite(exp["delta"]))
    assert np.all(np.abs(r["delta"][rest] - exp["delta"][rest]) <= 1e-5 * np.maximum(1.0, exp["delta"][rest])) and np.all(np.abs(r["d2"] - exp["d2"]) <= 1e-5 * exp["d2"])
    assert abs(r["delta"][twins].sum() - exp["delta"][twins].sum()) <= 1e-5 * max(1.0, exp["delta"][twins].sum())
    assert abs(r["D2"] - exp["D2"]) <= 1e-5 * exp["D2"]
    assert len(open(report).read().splitlines()) == len(want) + 1 and not os.path.exists(report + ".tmp") and not os.path.exists(acc_file + ".tmp")
    j = json.load(open(js))["joint_gate"]
    assert (j["accepted"], j["implied"]) == (r["accepted"], r["implied"]) and j["D2"] == r["D2"]
    assert "joint_gate" not in json.load(open(plain_js))
    # without the flags nothing changes: the other files hold the same map
    for name in ("Pose", "Feature", "State"):
        a, b = open(plain[name]).read().split(), open(run[name]).read().split()
        assert len(a) == len(b) and all(u == v or abs(float(u) - float(v)) <= 1e-6 * max(1.0, abs(float(u))) for u, v in zip(a, b)), name
    # the accepted pairs: exactly what -merge reads in a second run
    acc = api.read_pair_list(acc_file)
    assert acc.tolist() == [list(p) for p, s in zip(want, r["status"]) if s == 1]
    mreport = str(tmp_path / "merge.txt")
    merged = _run(d, typ, num, str(tmp_path / "m"), ["-merge", acc_file, "-mergeout", mreport])
    mr = api.read_merge_report(mreport)
    assert (mr["K"], mr["removed"], mr["dof"]) == (COUNT, COUNT, r["dof"])
    assert abs(mr["d2"] - r["D2"]) <= 1e-5 * r["D2"]  # the joint compatibility of exactly the accepted pairs
    assert int(api.read_localmap(merged["Info"], mono)["n"]) == int(G["n"]) - COUNT


def test_jgate_flag_errors(tmp_path):
    num = 9
    d, chosen = _split_files(tmp_path, False, num)
    report, acc_file, pairs = str(tmp_path / "jgate.txt"), str(tmp_path / "accepted.txt"), tmp_path / "pairs.txt"
    pose, fea = str(tmp_path / "Pose.txt"), str(tmp_path / "Feature.txt")
    good = f"{chosen[0]} {chosen[0] + ref.SPLIT_OFFSET}\n"
    pairs.write_text(good)
    base = [EXE, "-path", str(d), "-num", str(num), "-type", "Stereo", "-quiet", "1", "-p", pose, "-f", fea]

    def run(extra):
        return subprocess.run(base + extra, capture_output=True, text=True, timeout=300)

    def nothing_written():
        return not any(os.path.exists(p) for p in (report, acc_file, pose, fea, report + ".tmp", acc_file + ".tmp"))

    both = ["-jgate", str(pairs), "-jgateout", report]
    for extra in (["-jgate", str(pairs)], ["-jgateout", report], ["-jgatetau", "5"], ["-jgatepairs", acc_file], ["-jgate", str(tmp_path / "missing.txt"), "-jgateout", report],
                  both + ["-jgatetau", "0"], both + ["-jgatetau", "-1"], both + ["-jgatetau", "nan"], both + ["-jgatetau", "abc"], both + ["-jgatetau", ""],
                  both + ["-jgatepairs", ""]):
        r = run(extra)
        assert r.returncode != 0 and "-jgate" in r.stderr, (extra, r.returncode, r.stderr)
        assert nothing_written(), extra
    for text in ("1 2 3\n", f"{chosen[0]} {chosen[0]}\n", "1 x\n", "", "\n".join(f"{a} {a + 1}" for a in range(1, 2 * api.JOINT_GATE_MAX + 4, 2)) + "\n"):
        pairs.write_text(text)
        r = run(both + ["-jgatepairs", acc_file])
        assert r.returncode != 0 and "-jgate" in r.stderr, (text[:20], r.returncode, r.stderr)
        assert nothing_written(), text[:20]
    pairs.write_text(f"{chosen[0]} 987654\n")  # an id the final map does not have: after the tree, before any file
    r = run(both)
    assert r.returncode != 0 and "no feature 987654" in r.stderr and nothing_written()
    # tau = inf is a value; the run that works writes everything
    pairs.write_text(good)
    r = run(both + ["-jgatetau", "inf", "-jgatepairs", acc_file])
    assert r.returncode == 0, r.stderr
    rep = api.read_joint_gate(report)
    assert rep["status"].tolist() == [1] and os.path.exists(pose) and api.read_pair_list(acc_file).tolist() == [[chosen[0], chosen[0] + ref.SPLIT_OFFSET]]
