"""examples/rpt_render_main.cpp --events FILE: the raw records the example host writes equal Renderer.read_events() for cube.txt and
bunny.txt.  The C++ host reads textures with the library's PPM reader, so both sides load the scene from a scratch asset root whose
textures are the shipped JPEGs converted to PPM (the records do not depend on the texels, only on whether an object has a texture)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from relativitypathtracer_amd.events import EVENT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "relativitypathtracer_amd")
ASSETS = os.path.join(ROOT, "assets", "reference")
SCENES = {"cube": ("Textures/box.jpg",), "bunny": ("Textures/StanfordBunnyTerracotta.jpg",)}


def _build(tmp_path):
    exe = str(tmp_path / "rpt_render")
    cmd = ["g++", "-O2", "-std=c++17", f"-I{ROOT}/include", f"{ROOT}/examples/rpt_render_main.cpp", "-o", exe,
           f"-L{PKG}", "-lrpt_hip", "-lrpt_scene", f"-Wl,-rpath,{PKG}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return exe


def _scratch_assets(tmp_path, name):
    """A scratch asset root with PPM textures and the scene text naming them (and Models/bunny.obj under the name bunny.txt asks for)."""
    from PIL import Image
    root = tmp_path / "assets"
    (root / "Textures").mkdir(parents=True, exist_ok=True)
    (root / "Models").mkdir(exist_ok=True)
    shutil.copy(os.path.join(ASSETS, "Models", "bunny.obj"), root / "Models" / "StanfordBunny.obj")
    text = open(os.path.join(ASSETS, "Scenes", name + ".txt")).read()
    for jpg in SCENES[name]:
        ppm = os.path.splitext(jpg)[0] + ".ppm"
        with Image.open(os.path.join(ASSETS, jpg)) as im:
            im.convert("RGB").save(root / ppm)
        text = text.replace(jpg, ppm)
    return str(root), text


def test_example_host_without_the_flag_and_with_a_bad_flag(tmp_path):
    exe = _build(tmp_path)
    p = subprocess.run([exe, "--events"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "--events needs a file name" in p.stderr
    p = subprocess.run([exe, "64", "48"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "[--events FILE]" in p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_events_file_equals_read_events(tmp_path, name):
    from relativitypathtracer_amd import Scene
    from relativitypathtracer_amd.renderer import Renderer
    exe = _build(tmp_path)
    root, text = _scratch_assets(tmp_path, name)
    W, H = 320, 184
    ppm, ev = tmp_path / "frame.ppm", tmp_path / "frame.events"
    p = subprocess.run([exe, "--events", str(ev), str(W), str(H), str(ppm), "0", "0", "0.5", "0"], input=text, capture_output=True, text=True,
                       env={**os.environ, "RPT_ASSETS": root}, timeout=300)
    assert p.returncode == 0, p.stderr
    data = ev.read_bytes()
    assert len(data) == W * H * 32
    got = np.frombuffer(data, dtype=EVENT_DTYPE).reshape(H, W)
    plain = tmp_path / "plain.ppm"
    p = subprocess.run([exe, str(W), str(H), str(plain), "0", "0", "0.5", "0"], input=text, capture_output=True, text=True,
                       env={**os.environ, "RPT_ASSETS": root}, timeout=300)
    assert p.returncode == 0, p.stderr
    assert plain.read_bytes() == ppm.read_bytes(), "--events changed the picture"
    s = Scene(asset_root=root, aliases={})
    s.inputScene(text)
    s.set_camera((0.0, 0.0, 0.5), 0.0)
    s.update_objects()
    r = Renderer(0)
    try:
        r.upload_scene(s)
        r.set_scene_params(s, W, H)
        r.set_output(None)
        r.render()
        r.render_events(async_=True)
        r.sync()
        want = r.read_events()
    finally:
        r.close()
    assert (want["object"] >= 0).any() and (want["object"] < 0).any()
    assert got.tobytes() == want.tobytes()
