"""rpt_set_doppler on the MI355X: the colour operator bit for bit against its float32 restatement, the neutral cases against the
oracle, the per-pixel factors and their composition from the debug record, the culls, and the plumbing (DESIGN.md "Doppler and
beaming")."""
import math

import numpy as np
import pytest

import doppler_model as dm
import oracle_ffi
from conftest import CONFIGS, load_config
from relativitypathtracer_amd import Scene
from relativitypathtracer_amd.renderer import RenderError, Renderer
from scene_fuzz import close_scene_text, extreme_scene_text, random_scene_text, walls_scene_text

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


def _setup(r, scene, W, H, variant=0, doppler=(True, True)):
    r.set_variant(variant)
    r.set_msaa(1)
    r.upload_scene(scene)
    r.set_scene_params(scene, W, H)
    r.set_rows(0, 1, False)
    r.set_plane_output(None)
    r.set_output(None)
    r.set_debug_rgb(False)
    r.set_debug_doppler(False)
    r.set_doppler(*doppler)


def _scene(text, v=(0.0, 0.0, 0.0), t=0.0, interval=None):
    s = Scene()
    s.inputScene(text)
    if interval is not None:
        s.set_interval(interval)
    s.set_camera(v, t)
    s.update_objects()
    return s


# ---- 1. KAT ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_operator_probe_bit_exact(renderer, flags):
    rng = np.random.default_rng(100 + flags)
    D, c = dm.kat_inputs(1_000_000, rng)
    inp = np.empty((D.shape[0], 5), np.float32)
    inp[:, 0], inp[:, 1:4], inp[:, 4] = D, c, flags
    got = renderer.probe(6, inp, 3)
    want = dm.S32(D, c, flags)
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {D.shape[0]} differ, e.g. D={D[bad[:3]]} c={c[bad[:3]]} got={got[bad[:3]]} want={want[bad[:3]]}"
    assert D.shape[0] >= 1_000_000 and (D == 1).sum() >= 16


# ---- 2. neutral cases equal the reference ---------------------------------------------------------------------------------------
def _assert_oracle(r, scene, W, H, lsb=0):
    r.render()
    px = r.read_framebuffer()
    opx, _, _ = oracle_ffi.render(scene, W, H, want_rgb=False)
    d = np.abs(px["rgba"].astype(np.int16) - opx["rgba"].astype(np.int16)).max()
    assert d <= lsb, f"max |d| = {d} LSB"


@pytest.mark.parametrize("name", list(CONFIGS))
def test_at_rest_and_interval_zero_equal_the_oracle(renderer, name):
    W, H = 256, 144
    scene = load_config(name)
    at_rest = not np.any(scene.velocities()[:, :3]) and not any(CONFIGS[name]["v"])
    if at_rest:
        _setup(renderer, scene, W, H)
        _assert_oracle(renderer, scene, W, H)
        assert renderer.last_variant() in (243, 244)
    scene.set_interval(0)               # light propagation off (the cube1 state): no light travel, D = 1
    scene.update_objects()
    _setup(renderer, scene, W, H)
    _assert_oracle(renderer, scene, W, H)


def test_at_rest_configs_exist():
    assert any(not any(c["v"]) and not np.any(load_config(n).velocities()[:, :3]) for n, c in CONFIGS.items())


@pytest.mark.parametrize("v", [(0.0, 0.0, 0.6), (0.5, 0.0, -0.3), (0.0, 0.9, 0.0)])
def test_co_moving_scene_within_one_lsb(renderer, v):
    vs = ",".join(str(c) for c in v)
    text = (f"MModels/cube.obj\nOc\n p0,0,6,0.5,0,1,0,1,1,1\n c0.8,0.4,0.2\n v{vs}\nOs\n p-2,1,9,0,0,1,0,1,1,1\n c0.2,0.6,0.9\n v{vs}\n"
            f"Om0\n p1.5,-1,7,0.3,1,1,0,1,1,1\n c0.9,0.9,0.9\n v{vs}\nOs\n p0,3,4,0,0,1,0,0.3,0.3,0.3\n c2,2,1.5\n l1\n v{vs}\nA0.2\nR\n")
    W, H = 256, 144
    scene = _scene(text, v=v, t=1.5)
    _setup(renderer, scene, W, H)
    _assert_oracle(renderer, scene, W, H, lsb=1)


# ---- 3. / 4. the debug record --------------------------------------------------------------------------------------------------
def _record(r, scene, W, H, flags=(True, True)):
    _setup(r, scene, W, H, doppler=flags)
    r.set_debug_rgb(True)
    r.set_debug_doppler(True)
    r.render()
    assert r.last_variant() == 240
    return r.read_debug_doppler(), r.read_framebuffer(), r.read_debug_rgb()


def _cam_dirs(W, H):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack([(x / W - 0.5) * (W / H), y / H - 0.5, np.full_like(x, 0.5)], axis=-1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


@pytest.mark.parametrize("name", ["arch", "cubes"])
def test_camera_factor_per_pixel(renderer, name):
    W, H = 256, 144
    scene = load_config(name)
    rec, _, _ = _record(renderer, scene, W, H)
    hit = rec[..., 0] != 0
    assert hit.sum() > 1000
    n = _cam_dirs(W, H)
    ray = np.concatenate([np.full((H, W, 1), float(scene.params["interval"])), n], axis=-1)
    L0 = scene.objects()["Lorentz"][:, 0, :].astype(np.float64)          # (objects, 4)
    cands = scene.params["interval"] / np.einsum("hwk,ok->hwo", ray, L0)  # D_cam of every object along every pixel's ray
    rel = np.min(np.abs(cands - rec[..., 0:1].astype(np.float64)) / np.abs(cands), axis=-1)
    assert rel[hit].max() <= 1e-5, rel[hit].max()
    assert np.ptp(rec[..., 0][hit]) > 0.1          # the factor does vary over the frame


@pytest.mark.parametrize("name,flags", [("arch", (True, True)), ("cubes", (True, True)), ("cubes", (True, False)), ("cubes", (False, True))])
def test_final_colour_is_the_camera_operator_of_the_lit_colour(renderer, name, flags):
    W, H = 256, 144
    scene = load_config(name)
    rec, px, rgb = _record(renderer, scene, W, H, flags)
    f = (dm.SHIFT if flags[0] else 0) | (dm.BEAMING if flags[1] else 0)
    hit = rec[..., 0] != 0
    r = rec[hit]
    want = dm.S32(r[:, 0], r[:, 5:8], f)
    assert np.array_equal(want.view(np.uint32), r[:, 8:11].view(np.uint32))
    # the packed output is the tonemap of the final linear colour
    wp = np.asarray(scene.params["white_point"], np.float32)
    hwp = renderer.probe(3, wp[None, :], 3)[0]
    fin = rec[..., 8:11].reshape(-1, 3)
    mapped = np.minimum(renderer.probe(3, fin, 3) / hwp[None, :], np.float32(1)).astype(np.float32).reshape(H, W, 3)
    assert np.array_equal(mapped[hit].view(np.uint32), rgb[hit].view(np.uint32))
    t = mapped * np.float32(255)
    u8 = np.where(np.isnan(t), 0, np.clip(t, 0, 255)).astype(np.int64).astype(np.uint8)
    assert np.array_equal(u8[hit], px["rgba"].reshape(H, W, 4)[..., :3][hit])


@pytest.mark.parametrize("lv", [-0.8, -0.4, 0.4, 0.8])
def test_light_factor_composition(renderer, lv):
    """One light moving toward (lv < 0) or away from the lit wall, ambient 0, untextured non-emissive wall: the colour after the
    light factors is k * hcolor * S(D_light, lcolor), with k from the reference colour."""
    hc, lc = np.float32([0.7, 0.5, 0.9]), np.float32([1.6, 1.2, 0.8])
    text = (f"Oc\n p0,0,10,0,0,1,0,6,6,0.2\n c{hc[0]},{hc[1]},{hc[2]}\n"
            f"Os\n p0,0,5,0,0,1,0,0.2,0.2,0.2\n c{lc[0]},{lc[1]},{lc[2]}\n l1\n v0,0,{-lv}\nA0\nR\n")
    W, H = 256, 144
    # camera clock 15: the wall (10 away) is seen as it was at t = 5 and lit by light the sphere sent from about its start, z = 5, at
    # t = 0 — in front of the wall whichever way it moves
    scene = _scene(text, t=15.0)
    rec, _, _ = _record(renderer, scene, W, H)
    lit = (rec[..., 0] != 0) & (rec[..., 1] != 1) & (rec[..., 3] > 0)
    assert lit.sum() > 500
    r = rec[lit]
    k = r[:, 3].astype(np.float64) / (float(hc[1]) * float(lc[1]))
    want = k[:, None] * hc[None, :].astype(np.float64) * dm.S32(r[:, 1], np.repeat(lc[None, :], r.shape[0], 0), 3).astype(np.float64)
    rel = np.abs(r[:, 5:8] - want) / np.maximum(np.abs(want), 1e-30)
    assert rel.max() <= 1e-5, rel.max()
    # the light moves at -lv along z: toward the wall behind it (lv < 0) its light arrives blue-shifted, away from it red-shifted
    dl = r[:, 1]
    assert np.median(dl) > 1 if lv < 0 else np.median(dl) < 1


# ---- 5. the culls stay sound ----------------------------------------------------------------------------------------------------
GENERATORS = {"random": lambda rng: random_scene_text(rng)[0], "extreme": extreme_scene_text, "close": close_scene_text, "walls": walls_scene_text}


@pytest.mark.parametrize("gen", list(GENERATORS))
def test_verify_frame_with_doppler(renderer, gen):
    rng = np.random.default_rng(31337 + len(gen))
    seen = set()
    for i in range(10):
        scene = _scene(GENERATORS[gen](rng))
        v = rng.normal(size=3)
        v = v / np.linalg.norm(v) * rng.choice([0.0, 0.5, 0.95])
        scene.set_camera(tuple(float(c) for c in v), float(rng.uniform(-3, 20)))
        scene.update_objects()
        W, H = (2560, 1440) if i == 0 else (320, 184)      # above RPT_LATENCY_KERNEL_MAX_PIXELS the async choice is 41's twin
        _setup(renderer, scene, W, H)
        assert renderer.verify_frame() == 0, f"{gen} scene {i}"
        seen.add(renderer.last_variant())
    assert seen <= {241, 243, 244} and seen


def test_verify_frame_mesh_free_scenes(renderer):
    rng = np.random.default_rng(4)
    for i in range(8):
        lines = []
        for k in range(5):
            x, y, z = rng.uniform(-4, 4), rng.uniform(-3, 3), rng.uniform(3, 14)
            lines += [f"O{rng.choice(['s', 'c'])}", f" p{x:.3f},{y:.3f},{z:.3f},0,0,1,0,1,1,1", f" c{rng.uniform(0.1, 1):.2f},0.5,0.5",
                      f" v{rng.uniform(-0.6, 0.6):.3f},0,{rng.uniform(-0.6, 0.6):.3f}"]
            if k == 0:
                lines.append(" l1")
        scene = _scene("\n".join(lines + ["A0.2", "R"]) + "\n", v=(0.0, 0.0, 0.5), t=float(i))
        _setup(renderer, scene, 640, 360)
        assert renderer.verify_frame() == 0
        assert renderer.last_variant() == 244


# ---- 6. plumbing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,twin", [("cubes", 244), ("bunny", 243)])
def test_row_tiles_equal_the_whole_frame(renderer, name, twin):
    W, H = 320, 184
    scene = load_config(name)
    scene.set_camera((0.3, 0.0, 0.1), 3.0)          # (the bunny: a moving camera, so that D != 1 on every hit pixel)
    scene.update_objects()
    _setup(renderer, scene, W, H)
    renderer.render()
    whole32 = renderer.read_framebuffer()["rgba"].reshape(H, W, 4).copy().view(np.uint32).reshape(H, W)
    tiles = (H + 7) // 8
    for first, step, run in ((0, 3, 1), (1, 3, 1), (2, 3, 1), (0, 5, 2)):
        if run == 1:
            renderer.set_rows(first, step, True)
        else:
            renderer.set_tile_pattern(first, step, run, True)
        renderer.render()
        plane = renderer.read_colour_plane()
        local = [t for t in range(tiles) if (t - first) % step < run and t >= first]
        for k, t in enumerate(local):
            rows = slice(t * 8, min(H, t * 8 + 8))
            assert np.array_equal(plane[k * 8:k * 8 + (rows.stop - rows.start)], whole32[rows]), (first, step, t)
    assert renderer.last_variant() == twin


def test_frames_in_flight_equal_blocking_frames():
    W, H = 2560, 1440          # above RPT_LATENCY_KERNEL_MAX_PIXELS: in flight 41's twin, blocking 43's
    scene = load_config("bunny")
    slots = [Renderer(0) for _ in range(3)]
    try:
        slots[0].upload_scene(scene)
        for s in slots[1:]:
            s.share_scene(slots[0])
        for s in slots:
            s.set_scene_params(scene, W, H)
            s.set_output(None)
            s.set_doppler(True, True)
        frames = []
        for f in range(3):
            scene.set_camera((0.3, 0.0, 0.1), 3.0 + 0.1 * f)
            scene.update_objects()
            slots[f].set_objects(scene)
            slots[f].render_async()
            assert slots[f].last_variant() == 241
        for s in slots:
            s.sync()
            frames.append(s.read_framebuffer())
        for f in range(3):
            scene.set_camera((0.3, 0.0, 0.1), 3.0 + 0.1 * f)
            scene.update_objects()
            slots[0].set_objects(scene)
            slots[0].render()
            assert slots[0].last_variant() == 243
            assert np.array_equal(slots[0].read_framebuffer().view(np.uint8), frames[f].view(np.uint8)), f
    finally:
        for s in slots:
            s.close()


def test_variants_name_the_twins_and_refusals(renderer):
    scene = load_config("bunny")
    W, H = 256, 144
    for variant, twin in ((0, 243), (3, 203), (41, 241), (43, 243), (48, 248), (49, 249)):
        _setup(renderer, scene, W, H, variant)
        renderer.render()
        assert renderer.last_variant() == twin
        assert renderer.last_exact_rcp() == (twin in (241, 243))
    arch = load_config("arch")
    _setup(renderer, arch, W, H)
    renderer.render()
    assert renderer.last_variant() == 244
    for variant in (1, 50, 51):
        _setup(renderer, scene, W, H, variant)
        with pytest.raises(RenderError, match=r"\(1\)"):
            renderer.render()
    _setup(renderer, scene, W, H)
    renderer.set_msaa(2)
    with pytest.raises(RenderError, match=r"\(1\)"):
        renderer.render()
    renderer.set_msaa(1)
    # the setting itself: 0..3, per context, off again restores the reference's kernels
    assert renderer._lib.rpt_set_doppler(renderer._h, 4) == 1
    assert renderer._lib.rpt_set_doppler(renderer._h, -1) == 1
    renderer.set_doppler(False, False)
    renderer.render()
    assert renderer.last_variant() == 43
    other = Renderer(0)
    try:
        other.share_scene(renderer)
        other.set_scene_params(scene, W, H)
        other.set_output(None)
        renderer.set_doppler(True, True)
        other.render()
        assert other.last_variant() == 43          # not shared by rpt_share_scene
    finally:
        other.close()
