"""-m gpu: the command line's -gate <pairs file> -gateout <file> (the exact gate of candidate feature pairs named by label:
lsfm_map_feature_pair_gate, lsfm_save_pair_gate).  No reference counterpart.  The file holds what the library's entry point gives for
the same map, one line per pair in input order, to the bars of test_gpu_feature_gate.py (the columns are not bit-reproducible from call
to call), and the flags change none of the other output files."""
import os
import subprocess

import numpy as np
import pytest

import feature_cov_reference as ref
from linearsfm_amd import api, synth
from test_gpu_cli_cov import EXE, _run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("typ", ["Stereo", "Monocular"])
def test_gate_file_matches_api(ctx, tmp_path, typ):
    mono = typ == "Monocular"
    num = 9
    maps = synth.make_mono_set(num, 8, 4, seed=43, lap=5, home=2) if mono else synth.make_stereo_set(num, 8, 4, seed=43, lap=5, home=2)
    d = tmp_path / "set"
    synth.write_set(str(d), maps)
    gate, cols, chi2 = str(tmp_path / "gate.txt"), "cols.txt", "chi2.txt"
    plain = _run(d, typ, num, str(tmp_path / "plain"), [])
    pose_ids = np.loadtxt(plain["Pose"], ndmin=2)[:, 0].astype(int)
    feat_ids = np.loadtxt(plain["Feature"], ndmin=2)[:, 0].astype(int)
    rng = np.random.default_rng(4)
    want = np.stack([rng.choice(feat_ids, size=2, replace=False) for _ in range(20)])
    want[1] = want[0][::-1]  # a pair in both orders: a feature in several pairs
    pairs_file = tmp_path / "pairs.txt"
    pairs_file.write_text("\n".join(f"{a}  {b}" for a, b in want[:10]) + "\n" + " ".join(f"{a} {b}" for a, b in want[10:]) + "\n")
    # the parent's flag set with and without the gate: -st / -p / -f / -covcols / -chi2
    common = lambda o: ["-covcols", os.path.join(o, cols), "-covposes", f"{pose_ids[0]},{pose_ids[-1]}", "-chi2", os.path.join(o, chi2)]
    outs = {k: str(tmp_path / k) for k in ("a", "b", "g")}
    runs = {k: _run(d, typ, num, o, common(o) + (["-gate", str(pairs_file), "-gateout", gate] if k == "g" else [])) for k, o in outs.items()}
    for k in runs:
        runs[k].update(Cols=os.path.join(outs[k], cols), Chi2=os.path.join(outs[k], chi2))
    for k in runs["a"]:
        a, b, c = (open(runs[x][k], "rb").read() for x in ("a", "b", "g"))
        if a == b:
            assert a == c, k
        else:  # (files the program itself does not repeat byte for byte from one process to the next: held to their layout and to 1e-6)
            ta, tc = a.decode().split(), c.decode().split()
            assert len(ta) == len(tc), k
            for u, v in zip(ta, tc):
                if u != v:
                    assert abs(float(u) - float(v)) <= 1e-6 * max(1.0, abs(float(u))), (k, u, v)
    G = api.read_localmap(runs["g"]["Info"], mono)
    m, n = int(G["m"]), int(G["n"])
    frow = {int(np.asarray(G["stno"])[6 * m + 3 * f]): f for f in range(n)}
    idx = np.array([[frow[a], frow[b]] for a, b in want], np.int32)
    out = ctx.feature_pair_gate(G, mono, idx)
    ids, d2, cov = api.read_pair_gate(gate)
    assert np.array_equal(ids, want)
    assert sum(1 for line in open(gate) if line.strip()) == len(want) and len(open(gate).readline().split()) == 9
    assert not os.path.exists(gate + ".tmp")
    vF = np.einsum("kii->ki", ctx.covariance(G, mono)["feature"])
    marg = vF[idx[:, 0]] + vF[idx[:, 1]]
    e = ref.cov_err(cov, out["cov_diff"], marg)
    bars = ref.d2_bars(out["cov_diff"], np.stack([np.diag(v) for v in marg]))
    rel = np.abs(d2 - out["d2"]) / out["d2"]
    print(f"-gate {typ}: Sigma_d file vs API {e:.2e}, d2 {rel.max():.2e} (largest bar {bars.max():.2e})")
    assert e < ref.BAR and bars.max() < ref.BAR_D2_CAP and np.all(rel < bars)


def test_gate_flag_errors(tmp_path):
    num = 3
    d = tmp_path / "set"
    synth.write_set(str(d), synth.make_stereo_set(num, 8, 4, seed=43))
    gate, pairs = str(tmp_path / "gate.txt"), tmp_path / "pairs.txt"
    pose, fea = str(tmp_path / "Pose.txt"), str(tmp_path / "Feature.txt")
    base = [EXE, "-path", str(d), "-num", str(num), "-type", "Stereo", "-quiet", "1", "-p", pose, "-f", fea]

    def run(extra):
        return subprocess.run(base + extra, capture_output=True, text=True, timeout=300)

    r = run([])
    assert r.returncode == 0, r.stderr
    ids = np.loadtxt(fea, ndmin=2)[:, 0].astype(int)
    os.remove(pose)
    pairs.write_text(f"{ids[0]} {ids[1]}\n")
    for extra in (["-gate", str(pairs)], ["-gateout", gate], ["-gate", str(tmp_path / "missing.txt"), "-gateout", gate]):
        r = run(extra)
        assert r.returncode != 0 and "-gate" in r.stderr, (extra, r.returncode, r.stderr)
        assert not os.path.exists(gate) and not os.path.exists(pose)
    for text, word in ((f"{ids[0]} {ids[1]} {ids[2]}\n", "pairs"), (f"{ids[0]} {ids[0]}\n", "twice"), (f"{ids[0]} x\n", "pairs"), (f"{ids[0]} 999999\n", "999999")):
        pairs.write_text(text)  # an odd count, f == g, not a number, an id no feature has
        r = run(["-gate", str(pairs), "-gateout", gate])
        assert r.returncode != 0 and word in r.stderr, (text, r.returncode, r.stderr)
        assert not os.path.exists(gate) and not os.path.exists(pose)
    pairs.write_text(f"{ids[0]} {ids[1]}\n{ids[2]} {ids[0]}\n")
    r = run(["-gate", str(pairs), "-gateout", gate])
    assert r.returncode == 0, r.stderr
    assert os.path.exists(gate) and os.path.exists(pose)
    got, d2, _ = api.read_pair_gate(gate)
    assert got.tolist() == [[ids[0], ids[1]], [ids[2], ids[0]]] and np.all(d2 > 0)
