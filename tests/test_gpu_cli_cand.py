"""-m gpu: the command line's -cand <file> -candr <radius> [-candtau <tau>] (the candidate feature pairs of the final map:
lsfm_map_feature_pair_candidates, lsfm_save_pair_list).  No reference counterpart.  The file holds, as feature ids, the pairs the library's
entry point gives for the map -info wrote; -gate reads it; the flags change none of the other output files; every refusal ends the run
non-zero with no file written."""
import json
import os
import subprocess

import numpy as np
import pytest

import candidates_reference as cref
from linearsfm_amd import api, synth
from test_gpu_cli_cov import EXE, _run

pytestmark = pytest.mark.gpu
RADIUS, TAU = 2.5, 1000.0  # (the sets' features are distinct points: at the gate's own tau, chi^2_3 at 0.99, no pair is a candidate)


@pytest.mark.parametrize("typ", ["Stereo", "Monocular"])
def test_cand_file_matches_api_and_feeds_the_gate(ctx, tmp_path, typ):
    mono = typ == "Monocular"
    num = 7
    maps = synth.make_mono_set(num, 8, 4, seed=43, lap=5, home=2) if mono else synth.make_stereo_set(num, 8, 4, seed=43, lap=5, home=2)
    d = tmp_path / "set"
    synth.write_set(str(d), maps)
    plain_js = str(tmp_path / "plain.json")
    plain = _run(d, typ, num, str(tmp_path / "plain"), ["-json", plain_js])
    again = _run(d, typ, num, str(tmp_path / "again"), [])
    runs = {}
    for k, extra in (("r", []), ("t", ["-candtau", repr(TAU)])):
        cand, js = str(tmp_path / f"cand_{k}.txt"), str(tmp_path / f"run_{k}.json")
        runs[k] = (_run(d, typ, num, str(tmp_path / k), ["-cand", cand, "-candr", str(RADIUS), "-json", js] + extra), cand, js)
    for k, (files, cand, js) in runs.items():
        # -st / -p / -f (and the rest): byte-identical with and without the flags wherever the program repeats its own bytes
        for name in plain:
            a, b, c = (open(x[name], "rb").read() for x in (plain, again, files))
            if a == b:
                assert a == c, (k, name)
            else:
                ta, tc = a.decode().split(), c.decode().split()
                assert len(ta) == len(tc), (k, name)
                for u, v in zip(ta, tc):
                    if u != v:
                        assert abs(float(u) - float(v)) <= 1e-6 * max(1.0, abs(float(u))), (k, name, u, v)
        # the map the command line wrote, through the library's entry point
        G = api.read_localmap(files["Info"], mono)
        m = int(G["m"])
        label = np.asarray(G["stno"])[6 * m:: 3]
        fcov = ctx.covariance(G, mono)["feature"] if k == "t" else None
        x = cref.features_of(G)
        assert len(cref.margin(x, RADIUS, fcov, TAU if k == "t" else None)) == 0
        out = ctx.feature_pair_candidates(G, RADIUS, fcov, TAU if k == "t" else None)
        ids = api.read_pair_list(cand)
        print(f"-cand {typ} {'with' if k == 't' else 'without'} -candtau: {len(ids)} pairs of {len(label) * (len(label) - 1) // 2}")
        assert len(ids) > 0 and np.array_equal(ids, label[out["pairs"]])
        assert np.array_equal(out["pairs"], cref.candidates(x, RADIUS, fcov, TAU if k == "t" else None)["pairs"])
        assert [len(l.split()) for l in open(cand).read().splitlines()] == [2] * len(ids)
        assert not os.path.exists(cand + ".tmp")
        assert json.load(open(js))["candidates"] == len(ids)
    assert len(api.read_pair_list(runs["t"][1])) < len(api.read_pair_list(runs["r"][1]))
    assert "candidates" not in json.load(open(plain_js))
    # a second run gates the candidates of the first
    gate = str(tmp_path / "gate.txt")
    _run(d, typ, num, str(tmp_path / "g"), ["-gate", runs["t"][1], "-gateout", gate])
    gids, d2, _ = api.read_pair_gate(gate)
    assert np.array_equal(gids, api.read_pair_list(runs["t"][1])) and not np.any(np.isnan(d2))


def test_cand_flag_errors(tmp_path):
    num = 3
    d = tmp_path / "set"
    synth.write_set(str(d), synth.make_stereo_set(num, 8, 4, seed=43))
    cand = str(tmp_path / "cand.txt")
    pose, fea = str(tmp_path / "Pose.txt"), str(tmp_path / "Feature.txt")
    base = [EXE, "-path", str(d), "-num", str(num), "-type", "Stereo", "-quiet", "1", "-p", pose, "-f", fea]

    def run(extra):
        return subprocess.run(base + extra, capture_output=True, text=True, timeout=300)

    for extra in (["-cand", cand], ["-candr", "1.0"], ["-candtau", "11.3"], ["-candr", "1.0", "-candtau", "11.3"],
                  ["-cand", cand, "-candr", "0"], ["-cand", cand, "-candr", "-2"], ["-cand", cand, "-candr", "abc"], ["-cand", cand, "-candr", "1.0x"],
                  ["-cand", cand, "-candr", "inf"], ["-cand", cand, "-candr", "1.0", "-candtau", "0"], ["-cand", cand, "-candr", "1.0", "-candtau", "nan"],
                  ["-cand", cand, "-candr", "1.0", "-candtau", ""]):
        r = run(extra)
        assert r.returncode != 0 and "-cand" in r.stderr, (extra, r.returncode, r.stderr)
        assert not os.path.exists(cand) and not os.path.exists(pose) and not os.path.exists(fea), extra
    # the library refuses: more than 2^21 cells along an axis
    r = run(["-cand", cand, "-candr", "1e-9"])
    assert r.returncode != 0 and "radius too small for the map's extent" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(cand) and not os.path.exists(pose) and not os.path.exists(fea)
    r = run(["-cand", cand, "-candr", "1.0"])
    assert r.returncode == 0, r.stderr
    assert os.path.exists(cand) and os.path.exists(pose) and not os.path.exists(cand + ".tmp")
    ids = api.read_pair_list(cand)
    have = set(np.loadtxt(fea, ndmin=2)[:, 0].astype(int).tolist())
    assert len(ids) > 0 and all(a in have and b in have and a != b for a, b in ids.tolist())
