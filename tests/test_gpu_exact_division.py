"""The triangle test's exact reciprocal (csrc/rpt_device_math.hip.h rcp_newton / rcp_exact) on the device: bit for bit the IEEE
1.0f / s over every float of its domain, and frames of kernels 41 / 43 (exact reciprocal) identical to 48 / 49 (IEEE division)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHIPPED_FORM = 1          # the rcp_newton form rcp_exact takes (rpt_device_math.hip.h)


def _bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


@pytest.fixture(scope="module")
def renderer():
    from relativitypathtracer_amd.renderer import Renderer
    r = Renderer(0)
    yield r
    r.close()


@pytest.mark.parametrize("lo, hi", [(1e-7, 2.0 ** 60), (2.0 ** -125, 2.0 ** 125)])
def test_reciprocal_every_float(renderer, lo, hi):
    """Every float with lo <= |s| <= hi, both signs: [1e-7, 2^60] is what the triangle test can meet on a scene in the domain
    (|det| >= 1e-7, |det| <= |e1| |e2| (1 + 2^-20) <= 2^60 (1 + 2^-20)), [2^-125, 2^125] the range the source claims."""
    counts, samples = renderer.probe_reciprocal(lo, hi, 8)
    n = 2 * (_bits(hi) - _bits(np.float32(lo)) + 1)
    assert counts[0] == n, (counts, n)
    assert counts[SHIPPED_FORM] == 0, (counts, samples[: min(8, counts[4])].tolist())
    assert counts[3] == 0, (counts, samples[: min(8, counts[4])].tolist())          # the form whose correctness is argued in the source


def test_reciprocal_all_ones_significands(renderer):
    """The one case a Newton step cannot settle by itself: significands that are all ones, checked on their own as well."""
    for e in range(-24, 61, 7):
        s = np.float32(2.0 ** e) * np.float32(2.0 - 2.0 ** -23)
        counts, _ = renderer.probe_reciprocal(float(s), float(s), 4)
        assert counts[0] == 2 and counts[SHIPPED_FORM] == 0 and counts[3] == 0, (e, counts)


def _frame(r, scene, W, H, variant):
    r.set_scene_params(scene, W, H)
    r.set_output(None)
    r.set_variant(variant)
    r.render()
    px = r.read_framebuffer()
    return px["rgba"].copy(), r.last_variant(), r.last_exact_rcp()


@pytest.mark.parametrize("name, t", [("bunny", 0.0), ("shadows", 16.0)])
def test_exact_reciprocal_frames_equal_ieee_frames(renderer, name, t):
    """41 / 43 on a shipped scene take the exact reciprocal; 48 / 49 the IEEE division: the same pixels, and the oracle's."""
    import oracle_ffi
    from relativitypathtracer_amd import Scene
    W, H = 480, 270
    scene = Scene.from_file(name)
    scene.set_camera((0, 0, 0), t)
    scene.update_objects()
    renderer.upload_scene(scene)
    opx, _, _ = oracle_ffi.render(scene, W, H, want_rgb=False)
    for fast, ieee in ((41, 48), (43, 49)):
        a, va, ea = _frame(renderer, scene, W, H, fast)
        b, vb, eb = _frame(renderer, scene, W, H, ieee)
        assert (va, ea) == (fast, True) and (vb, eb) == (ieee, False)
        assert np.array_equal(a, b), (name, fast)
        assert np.array_equal(a, opx["rgba"]), (name, fast)
    renderer.set_variant(0)
    _frame(renderer, scene, W, H, 0)
    assert renderer.last_exact_rcp()


def test_scene_outside_the_domain_takes_the_ieee_division(renderer, tmp_path):
    """A mesh with |e1| |e2| > 2^60: kernels 41 / 43 run with the IEEE division (rpt_last_exact_rcp), and still match the oracle."""
    import oracle_ffi
    from relativitypathtracer_amd import Scene
    obj = tmp_path / "huge.obj"
    obj.write_text("v -2147483648 -2147483648 8589934592\nv 2147483648 -2147483648 8589934592\nv 0 2147483648 8589934592\n"
                   "vt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1\n")
    scene = Scene.from_file("bunny")
    scene.ReadOBJ(str(obj))          # (in the scene's mesh pool, named by no object: its triangles alone put the scene outside)
    scene.set_camera((0, 0, 0), 0.0)
    scene.update_objects()
    renderer.upload_scene(scene)
    W, H = 320, 180
    opx, _, _ = oracle_ffi.render(scene, W, H, want_rgb=False)
    for variant in (41, 43, 0):
        a, v, e = _frame(renderer, scene, W, H, variant)
        assert not e and v in (41, 43)
        assert np.array_equal(a, opx["rgba"]), variant
    renderer.set_variant(0)
