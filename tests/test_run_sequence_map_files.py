"""GPU: tools/run_sequence.py --save-map / --save-clouds on a short image sequence at a small image size (a child process,
which is what the test is about): the files parse with the independent reader of tests/cloud_file_oracle.py, the map has the
points of --map's assembled cloud, and every node with a valid estimate has its two files."""
import json
import os
import subprocess
import sys

import pytest

import cloud_file_oracle as co

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["map.ply", "map"])
def test_save_map_and_save_clouds(tmp_path, name):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_sequence.py"), "--images", "--frames", "6", "--width", "320",
                        "--height", "240", "--map", "--save-map", str(tmp_path / name), "--save-clouds", str(tmp_path / "node")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.splitlines()[-1])
    mf = res["map_files"]
    written = {"map.ply": "map.ply", "map": "map.pcd"}[name]
    assert mf["map"]["path"] == str(tmp_path / written) and mf["map"]["format"] == written[-3:]
    assert mf["nodes"] == res["map"]["nodes"] >= 2 and mf["map"]["points"] == res["map"]["points"] > 0
    rows, info = co.read((tmp_path / written).read_bytes())
    assert info["points"] == res["map"]["points"] and rows.shape == (1, info["points"], 4)
    assert mf["clouds_written"] == mf["nodes"]
    clouds = sorted(f for f in os.listdir(tmp_path) if f.startswith("node_"))
    assert len(clouds) == 2 * mf["nodes"] and clouds[0] == "node_0000.pcd" and clouds[1] == "node_0000.txt"
    for f in clouds[0::2]:
        rows, info = co.read((tmp_path / f).read_bytes())
        assert (info["width"], info["height"]) == (320 // 8, 240 // 8) and info["viewpoint_text"].count(" ") == 6
    assert (tmp_path / "node_0000.txt").read_text() == "1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1\n"   # the first node is the origin
