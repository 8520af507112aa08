"""-m gpu: the command line's -merge <pairs file> [-mergeout <file>] (feature pairs named by label declared one point each:
lsfm_map_merge_features, lsfm_save_merge_report).  No reference counterpart.  On a 9-map set with features split in two
(merge_reference.split_set) the output files describe the merged map -- what the library's entry point makes of the unmerged run's own
-info map --, the report reads back, -gate after -merge resolves its ids in the merged map, and the refused combinations write nothing.
(The program's tree is not bit-reproducible from one process to the next: values are held to 1e-6, labels and index arrays exactly.)"""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

import merge_reference as ref
from linearsfm_amd import api, synth
from test_gpu_cli_cov import EXE, _run

pytestmark = pytest.mark.gpu
COUNT = 4


def _split_files(tmp_path, mono, num=9):
    maps = synth.make_mono_set(num, 8, 4, seed=43, lap=5, home=2) if mono else synth.make_stereo_set(num, 8, 4, seed=43, lap=5, home=2)
    dicts, chosen = ref.split_set([dict(vars(mp)) for mp in maps], COUNT)
    out = []
    for mp, d in zip(maps, dicts):
        c = copy.copy(mp)
        c.stno = d["stno"]
        out.append(c)
    d = tmp_path / "set"
    synth.write_set(str(d), out)
    return d, chosen


def _close(a, b, what):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    assert a.shape == b.shape, what
    assert np.all(np.abs(a - b) <= 1e-6 * np.maximum(1.0, np.abs(b))), (what, float(np.max(np.abs(a - b))))


@pytest.mark.parametrize("typ", ["Stereo", "Monocular"])
def test_merge_files_describe_the_merged_map(ctx, tmp_path, typ):
    mono = typ == "Monocular"
    num = 9
    d, chosen = _split_files(tmp_path, mono, num)
    pairs_file, report, gate = tmp_path / "pairs.txt", str(tmp_path / "merge.txt"), str(tmp_path / "gate.txt")
    want = [(i, i + ref.SPLIT_OFFSET) if k % 2 == 0 else (i + ref.SPLIT_OFFSET, i) for k, i in enumerate(chosen)]
    pairs_file.write_text("\n".join(f"{a} {b}" for a, b in want) + "\n")
    plain = _run(d, typ, num, str(tmp_path / "plain"), [])
    G = api.read_localmap(plain["Info"], mono)
    m, n = int(G["m"]), int(G["n"])
    at = {int(l): f for f, l in enumerate(ref.feature_ids(G))}
    idx = np.array([(at[a], at[b]) for a, b in want], np.int32)
    exp = ctx.merge_features(G, mono, idx)
    kept = [int(ref.feature_ids(exp["map"])[exp["rep"][f]]) for f, _ in idx]
    # -gate after -merge: the kept ids against another feature of the merged map
    other = int([l for l in ref.feature_ids(exp["map"]) if l not in kept][0])
    gpairs = tmp_path / "gpairs.txt"
    gpairs.write_text("".join(f"{k} {other}\n" for k in kept))
    run = _run(d, typ, num, str(tmp_path / "merged"), ["-merge", str(pairs_file), "-mergeout", report, "-gate", str(gpairs), "-gateout", gate])
    M = api.read_localmap(run["Info"], mono)
    g = exp["map"]
    assert int(M["n"]) == n - COUNT == int(g["n"]) and int(M["m"]) == m
    for k in ("stno", "photo", "feature", "Ui", "Uj"):
        assert np.array_equal(M[k], g[k]), k
    for k in ("U", "V", "W", "stVal"):
        _close(M[k], g[k], k)
    # the state, pose and feature files hold the merged map's variables
    full = np.loadtxt(run["Full"], ndmin=2)
    assert np.array_equal(full[:, 0].astype(int), g["stno"])
    _close(full[:, 1], g["stVal"], "Full")
    fids = np.loadtxt(run["Feature"], ndmin=2)[:, 0].astype(int)
    away = {a if k == b else b for (a, b), k in zip(want, kept)}
    assert len(fids) == n - COUNT and not away & set(fids.tolist()) and set(kept) <= set(fids.tolist())
    # the report
    r = api.read_merge_report(report)
    assert (r["K"], r["removed"], r["dof"]) == (COUNT, COUNT, 3 * COUNT)
    assert r["ids"].tolist() == [[a, b, k] for (a, b), k in zip(want, kept)]
    assert abs(r["d2"] - exp["d2"]) <= 1e-5 * exp["d2"]
    assert len(open(report).read().splitlines()) == COUNT + 1 and not os.path.exists(report + ".tmp")
    print(f"-merge {typ}: {COUNT} pairs, D2 file {r['d2']:.9g}, API on the unmerged run's map {exp['d2']:.9g}")
    # the gate file describes the merged map
    gi, d2, _ = api.read_pair_gate(gate)
    assert gi.tolist() == [[k, other] for k in kept]
    mat = {int(l): f for f, l in enumerate(ref.feature_ids(g))}
    ge = ctx.feature_pair_gate(g, mono, [(mat[k], mat[other]) for k in kept])["d2"]
    assert np.all(np.abs(d2 - ge) <= 1e-5 * ge)


def test_merge_flag_errors(tmp_path):
    num = 9
    d, chosen = _split_files(tmp_path, False, num)
    report, pairs, gate = str(tmp_path / "merge.txt"), tmp_path / "pairs.txt", str(tmp_path / "gate.txt")
    pose, fea, chi2 = str(tmp_path / "Pose.txt"), str(tmp_path / "Feature.txt"), str(tmp_path / "chi2.txt")
    base = [EXE, "-path", str(d), "-num", str(num), "-type", "Stereo", "-quiet", "1", "-p", pose, "-f", fea]
    a, b = chosen[0], chosen[0] + ref.SPLIT_OFFSET

    def run(extra):
        return subprocess.run(base + extra, capture_output=True, text=True, timeout=300)

    def nothing_written():
        return not any(os.path.exists(p) for p in (report, pose, fea, chi2, gate))

    pairs.write_text(f"{a} {b}\n")
    for extra in (["-mergeout", report], ["-merge", str(tmp_path / "missing.txt"), "-mergeout", report],
                  ["-merge", str(pairs), "-mergeout", report, "-chi2", chi2], ["-merge", str(pairs), "-chi2f", chi2]):
        r = run(extra)
        assert r.returncode != 0 and "-merge" in r.stderr, (extra, r.returncode, r.stderr)
        assert nothing_written(), extra
    for text, word in ((f"{a} {b} {chosen[1]}\n", "pairs"), (f"{a} {a}\n", "twice"), (f"{a} x\n", "pairs"), (f"{a} 999999\n", "999999")):
        pairs.write_text(text)  # an odd count, f == g, not a number, an id no feature has
        r = run(["-merge", str(pairs), "-mergeout", report])
        assert r.returncode != 0 and word in r.stderr, (text, r.returncode, r.stderr)
        assert nothing_written(), text
    # a -gate id that was merged away is the gate's "no feature" error: one of the two labels is gone, whichever was kept
    pairs.write_text(f"{a} {b}\n")
    gp = tmp_path / "gpairs.txt"
    gone = 0
    for lab in (a, b):
        gp.write_text(f"{lab} {chosen[1]}\n")
        r = run(["-merge", str(pairs), "-mergeout", report, "-gate", str(gp), "-gateout", gate])
        if r.returncode != 0:
            gone += 1
            assert "no feature" in r.stderr and str(lab) in r.stderr and nothing_written()
        else:
            assert os.path.exists(gate) and api.read_merge_report(report)["ids"][0, 2] == lab
            for p in (report, pose, fea, gate):
                os.remove(p)
    assert gone == 1
    # -merge alone: no report asked for, the files are written
    r = run(["-merge", str(pairs)])
    assert r.returncode == 0 and os.path.exists(fea) and not os.path.exists(report), r.stderr


# ---- without -merge nothing changes ---------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_before_merge")
UNFLAGGED = {"Stereo": lambda: synth.make_stereo_set(5, 8, 4, seed=43, lap=5, home=2), "Monocular": lambda: synth.make_mono_set(5, 8, 4, seed=43, lap=5, home=2)}


def unflagged_command(exe, typ, setdir, outdir):
    """The run whose files tests/golden/cli_before_merge holds, recorded with the program as it was before -merge existed: every
    output file the program had, -gate included (its pair reading is shared with -merge now).  Returns (argv, file names)."""
    names = ("Pose", "Feature", "State", "Full", "Info", "Gate")
    f = {k: os.path.join(outdir, f"{typ}_{k}.txt") for k in names}
    return [exe, "-path", setdir, "-num", "5", "-type", typ, "-p", f["Pose"], "-f", f["Feature"], "-st", f["State"], "-full", f["Full"], "-info", f["Info"],
            "-gate", os.path.join(setdir, "pairs.txt"), "-gateout", f["Gate"]], f


def write_unflagged_set(typ, setdir):
    maps = UNFLAGGED[typ]()
    synth.write_set(setdir, maps)
    ids = sorted(set(int(i) for mp in maps for i in np.asarray(mp.stno)[6 * mp.m:: 3]))
    with open(os.path.join(setdir, "pairs.txt"), "w") as f:
        f.write(f"{ids[0]} {ids[1]}\n{ids[2]}  {ids[0]} {ids[-1]} {ids[3]}\n")


def _same_file(got, exp, what):
    """Byte for byte, or -- the tree is not bit-reproducible from one process to the next -- the same lines and tokens: a line of
    integers alone (counts, index arrays) exactly, every number of any other line to 1e-6 of max(1, |value|) -- which holds a label in
    front of a value (all below 1e6) exactly too.  (A value may print as "0" in one run and as 7e-10 in the next: the kind of a token
    cannot be told from the token.)"""
    a, b = open(got, "rb").read(), open(exp, "rb").read()
    if a == b:
        return True
    la, lb = a.decode().splitlines(), b.decode().splitlines()
    assert len(la) == len(lb), what
    for x, y in zip(la, lb):
        tx, ty = x.split(), y.split()
        assert len(tx) == len(ty), (what, x, y)
        if all(re.fullmatch(r"[-+]?\d+", v) for v in ty):
            assert tx == ty, (what, x, y)
            continue
        for u, v in zip(tx, ty):
            if u != v:
                assert abs(float(u) - float(v)) <= 1e-6 * max(1.0, abs(float(v))), (what, u, v)
    return False


@pytest.mark.parametrize("typ", ["Stereo", "Monocular"])
def test_without_merge_the_files_are_the_parents(tmp_path, typ):
    """An unflagged run against the files the program wrote before this flag existed (tests/golden/cli_before_merge, recorded on an
    MI355X with a build of the commit before): labels, counts and index arrays byte for byte, values to 1e-6, no report, no
    "Merged" line."""
    setdir, outdir = str(tmp_path / "set"), str(tmp_path / "out")
    os.makedirs(outdir)
    write_unflagged_set(typ, setdir)
    cmd, files = unflagged_command(EXE, typ, setdir, outdir)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Merged" not in r.stdout and "merge" not in r.stderr.lower()
    same = {k: _same_file(p, os.path.join(GOLDEN, os.path.basename(p)), k) for k, p in files.items()}
    print(f"unflagged {typ}: byte for byte {sorted(k for k, v in same.items() if v)}, to 1e-6 {sorted(k for k, v in same.items() if not v)}")
    assert sorted(os.listdir(outdir)) == sorted(os.path.basename(p) for p in files.values())
