"""Native scene ingest (include/rrt.h rrt_collada_load; csrc/rrt_ingest.cpp) against the
reference's own loader.

Goldens: tests/golden/ingest.json holds the SHA-256 of the flattened scene (.rrts) and camera
record (.rrtc) that the reference's Collada parser + Application::load + get_static_scene +
Camera::configure/place/set_screen_size produce for every scene asset the reference ships
(tests/golden/make_ingest_golden.py, oracle harness in dump-only mode).  The ingest must
reproduce both files byte for byte: vertex order, halfedge vertex normals, triangle order and
winding, per-object BSDF records, light records and the placed camera.  Inputs: the copies under
tests/golden/dae/ (input data; golden_cases.dae_input rebuilds the large assets from their stored
form).  No GPU is involved.
"""
import hashlib
import json
import os
import tempfile

import numpy as np
import pytest

import rrt
from golden_cases import GOLD, dae_input

INGEST = json.load(open(os.path.join(GOLD, "ingest.json")))


def _input(name):
    assert name in INGEST
    path = dae_input(name)
    assert path is not None, f"{name}: input not stored under tests/golden/dae/"
    return path


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


@pytest.mark.parametrize("name", sorted(INGEST))
def test_collada_scene_and_camera_match_reference(name, tmp_path):
    e = INGEST[name]
    sc, cam = rrt.load_collada(_input(name), e["w"], e["h"])
    sc.save(str(tmp_path / "s.rrts"))
    assert _sha(tmp_path / "s.rrts") == e["rrts_sha256"], "flattened scene differs from the reference's"
    with open(tmp_path / "c.rrtc", "wb") as f:
        f.write(b"RRTCAM1\0" + bytes(cam))
    assert _sha(tmp_path / "c.rrtc") == e["rrtc_sha256"], "camera record differs from the reference's"


def test_committed_scene_fixtures_equal_ingest():
    """The .rrts fixtures the render parity tests use are exactly what the ingest produces."""
    names = sorted(f[:-5] for f in os.listdir(os.path.join(GOLD, "scenes")) if f.endswith(".rrts"))
    assert names
    for name in names:
        sc, _ = rrt.load_collada(_input(name))
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "s.rrts")
            sc.save(p)
            assert open(p, "rb").read() == open(os.path.join(GOLD, "scenes", name + ".rrts"), "rb").read(), name


def _case_dirs():
    return sorted(d for d in os.listdir(GOLD) if os.path.exists(os.path.join(GOLD, d, "case.json")))


@pytest.mark.parametrize("case", _case_dirs())
def test_camera_placement_per_render_case(case):
    """Every golden render case's camera (its -r/-b/-d) is what the ingest places."""
    c = json.load(open(os.path.join(GOLD, case, "case.json")))
    a = c["args"]
    w, h = (int(a[a.index("-r") + 1]), int(a[a.index("-r") + 2])) if "-r" in a else (800, 600)
    lr = float(a[a.index("-b") + 1]) if "-b" in a else 0.25
    fd = float(a[a.index("-d") + 1]) if "-d" in a else 4.7
    if c["dae"].startswith("@"):  # generated asset (rrt_scenes.py); the digest is pinned
        import rrt_scenes
        import tempfile
        path = os.path.join(tempfile.mkdtemp(), "gen.dae")
        assert {"@cfg4": rrt_scenes.write_cfg4_dae}[c["dae"]](path) == c["dae_sha256"]
    else:
        path = _input(os.path.basename(c["dae"])[:-4])
    _, cam = rrt.load_collada(path, w, h, lr, fd)
    ref = rrt.load_camera_state(os.path.join(GOLD, case, "camera.rrtc"))
    assert bytes(cam) == bytes(ref)
    # and the rrt_set_camera subset agrees with the .rrtc loader's
    d1, d2 = rrt.camera_desc(cam), rrt.load_camera(os.path.join(GOLD, case, "camera.rrtc"))
    assert bytes(d1) == bytes(d2)


def test_camera_settings_text_roundtrip(tmp_path):
    """Camera::dump_settings / load_settings format (the -c flag): what the reference would dump
    (%g, 6 significant digits) reads back to the same values at that precision."""
    _, cam = rrt.load_collada(_input("CBbunny"), 1920, 1080)
    p = str(tmp_path / "cam.txt")
    assert rrt.lib().rrt_camera_settings_save(p.encode(), cam) == 0
    back = rrt.load_camera_settings(p)
    a, b = cam.to_array(), back.to_array()
    np.testing.assert_allclose(b, a, rtol=1e-5, atol=1e-9)
    text = open(p).read().split()
    assert len(text) == 30 and text[25] == "1920" and text[26] == "1080"


@pytest.mark.parametrize("bad,msg", [
    ("<COLLADA><asset><up_axis>W_UP</up_axis></asset></COLLADA>", "up_axis"),
    ("<notcollada/>", "not a COLLADA"),
    ("<COLLADA><scene></scene></COLLADA>", "instance_visual_scene"),
    ("<COLLADA><unclosed></COLLADA>", "XML"),
])
def test_malformed_input_fails_with_message(tmp_path, bad, msg):
    p = tmp_path / "x.dae"
    p.write_text(bad)
    with pytest.raises(rrt.RRTError) as ei:
        rrt.load_collada(str(p))
    assert ei.value.code == rrt.RRT_E_INVALID and msg in str(ei.value)


def test_missing_file_is_io_error():
    with pytest.raises(rrt.RRTError) as ei:
        rrt.load_collada("/nonexistent/scene.dae")
    assert ei.value.code == rrt.RRT_E_IO


def test_polygon_quirk_one_triangle_per_face(tmp_path):
    """A quad contributes ONE triangle (last, first, second vertex): object.cpp:35-40 takes the
    face's halfedge, which HalfedgeMesh::build leaves at the polygon's last edge."""
    dae = """<?xml version="1.0"?>
<COLLADA><asset><up_axis>Y_UP</up_axis></asset>
<library_geometries><geometry id="g"><mesh>
<source id="g-pos"><float_array id="g-arr" count="12">0 0 0 1 0 0 1 1 0 0 1 0</float_array></source>
<vertices id="g-v"><input semantic="POSITION" source="#g-pos"/></vertices>
<polylist count="1"><input semantic="VERTEX" source="#g-v" offset="0"/><vcount>4</vcount><p>0 1 2 3</p></polylist>
</mesh></geometry></library_geometries>
<library_visual_scenes><visual_scene id="s"><node id="n" name="n"><instance_geometry url="#g"/></node></visual_scene></library_visual_scenes>
<scene><instance_visual_scene url="#s"/></scene></COLLADA>"""
    p = tmp_path / "q.dae"
    p.write_text(dae)
    sc, cam = rrt.load_collada(str(p), 32, 32)
    out = str(tmp_path / "q.rrts")
    sc.save(out)
    raw = open(out, "rb").read()
    n_bsdf, n_obj, n_light = np.frombuffer(raw[8:20], np.uint32)
    assert (n_bsdf, n_obj, n_light) == (1, 1, 0)
    off = 24 + 64
    kind, bsdf, nv, nt = np.frombuffer(raw[off:off + 16], np.uint32)
    assert (kind, nv, nt) == (0, 4, 1)
    idx = np.frombuffer(raw[off + 16 + nv * 48: off + 16 + nv * 48 + 12], np.uint32)
    assert list(idx) == [3, 0, 1]
    # default material: DiffuseBSDF(0.5) (dynamic_scene/mesh.cpp:30-34)
    t = np.frombuffer(raw[24:28], np.uint32)[0]
    refl = np.frombuffer(raw[32:44], np.float32)
    assert t == 0 and np.all(refl == np.float32(0.5))
