"""Every Doppler kernel on the MI355X against the CPU restatement of Doppler for rays that hit (tests/native/doppler_oracle.c, itself
held to float64 physics by tests/test_doppler_oracle.py): the 16-byte pixel and debug_rgb byte for byte on scenes where D != 1 on hit
pixels — the product twins 203 / 241 / 243 / 244 / 248 / 249, the record kernels 240 / 540, the lens 813 / 851 / 853 / 854, the panorama
503 / 541 / 544, the environment kernels with Doppler flags, and 30 generated scenes.  Small frames; the kernels that a frame's size would
choose are reached through set_variant.  Each comparison prints kernel number, hit pixels and pixels compared."""
import ctypes as C

import numpy as np
import pytest

import aa_support
import doppler_oracle as do
from conftest import CONFIGS
from relativitypathtracer_amd import Scene, _ffi
from relativitypathtracer_amd.renderer import Renderer, orient_objects
from scene_fuzz import close_scene_text, extreme_scene_text, random_scene_text, walls_scene_text
from test_gpu_events import HUGE_OBJ
from test_gpu_kat import KAT_SCENE

pytestmark = pytest.mark.gpu
W, H = 128, 72
PW, PH = 144, 72
TURN = (0.4, -0.2, 0.3)
REDUCED = dict(h_fov=2.4, v_fov=1.4, yaw=0.3)


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return do.build_oracle(tmp_path_factory.mktemp("doppler"))


@pytest.fixture(scope="module")
def aa_lib(tmp_path_factory):
    return aa_support.build_oracle(tmp_path_factory.mktemp("aa"))


def moving_scene(name):
    """Every shipped configuration with a moving camera (the ones at rest get (0.3, 0, 0.1) at t = 3), and KAT_SCENE: the moving bunny
    with the pear as second mesh.  cube, rulers and ladder ship with light delay off (interval 0), where Doppler is skipped by
    definition: "<name>+delay" is the same scene with light delay on, so that its flashes and textures are seen shifted as well."""
    if name.endswith("+delay"):
        s = moving_scene(name[:-len("+delay")])
        assert s.params["interval"] == 0
        s.set_interval(-1)
    elif name == "kat":
        s = Scene()
        s.inputScene(KAT_SCENE)
        s.set_camera((0.2, -0.1, 0.4), 3.0)
    else:
        s = Scene.from_file(CONFIGS[name]["scene"])
        if any(CONFIGS[name]["v"]):
            s.set_camera(CONFIGS[name]["v"], CONFIGS[name]["t"])
        else:
            s.set_camera((0.3, 0.0, 0.1), 3.0)
    s.update_objects()
    return s


DELAY_OFF = ("cube", "rulers", "ladder")                # the shipped scenes with interval 0
SCENES = list(CONFIGS) + ["kat"] + [n + "+delay" for n in DELAY_OFF]


def _setup(r, scene, w, h, variant=0, flags=3, upload=True):
    r.set_variant(variant)
    r.set_msaa(1)
    r.set_adaptive_aa(1, 8)
    r.set_projection("pinhole")
    r.set_debug_doppler(False)
    r.set_environment(None)
    r.set_environment_frame(None)
    r.set_orientation(0, 0, 0)
    r.set_field_of_view(0)
    if upload:
        r.upload_scene(scene)
    r.set_scene_params(scene, w, h)
    r.set_rows(0, 1, False)
    r.set_plane_output(None)
    r.set_output(None)
    r.set_debug_rgb(True)
    r.set_doppler(bool(flags & 1), bool(flags & 2))


def _frame(r, in_flight=False):
    if in_flight:
        r.render_async()
        r.sync()
    else:
        r.render()
    return r.read_framebuffer().copy(), r.read_debug_rgb().copy()


def _same_bits(a, b):
    """Bit for bit; a NaN must be matched by a NaN (its sign and payload are the platform's)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _compare(got, want, rec, kernel, what):
    """The whole frame, 16 bytes a pixel and debug_rgb, hit pixels and misses alike."""
    hit = rec["object"].reshape(-1) >= 0
    gb, wb = got[0].view(np.uint8).reshape(-1, 16), want[0].view(np.uint8).reshape(-1, 16)
    bad = (gb != wb).any(axis=1)
    print(f"kernel {kernel}: {what}: {int(hit.sum())} hit pixels, {hit.size} pixels compared")
    assert not bad.any(), f"{what} kernel {kernel}: {int(bad.sum())} pixels differ ({int((bad & hit).sum())} of them hit), first at {np.flatnonzero(bad)[:5]}"
    ok = _same_bits(got[1], want[1]).reshape(-1, 3).all(axis=1)
    assert ok.all(), f"{what} kernel {kernel}: debug_rgb differs on {int((~ok).sum())} pixels, first at {np.flatnonzero(~ok)[:5]}"
    return hit


def _doppler_acts(rec, what, interval=-1):
    """D_cam != 1 on some hit pixel; with light delay off both factors are skipped, and the record says so: D_cam = D_i = 1."""
    r = rec.reshape(-1)
    hit = r["object"] >= 0
    assert hit.any(), what
    if interval == 0:
        assert (r["dcam"][hit] == 1).all() and (r["dlight"][hit] == 1).all(), what
    else:
        assert (r["dcam"][hit] != 1).any(), what


# ---- 1. the product twins --------------------------------------------------------------------------------------------------------------------
MESH_TWINS = ((3, 203), (41, 241), (43, 243), (48, 248), (49, 249), (0, 243))
ANALYTIC_TWINS = ((3, 203), (0, 244), (44, 244))


@pytest.mark.parametrize("name", SCENES)
def test_twins_equal_the_cpu_restatement(renderer, lib, name):
    scene = moving_scene(name)
    has_mesh = bool((scene.objects()["type"] == 2).any())
    renderer.upload_scene(scene)
    for flags in (1, 2, 3):
        *want, rec = do.render(lib, scene, W, H, flags)
        _doppler_acts(rec, name, scene.params["interval"])
        for variant, twin in (MESH_TWINS if has_mesh else ANALYTIC_TWINS):
            for in_flight in (False, True):
                _setup(renderer, scene, W, H, variant, flags, upload=False)
                got = _frame(renderer, in_flight)
                assert renderer.last_variant() == twin, (name, variant, renderer.last_variant())
                if twin not in (241, 243):
                    assert not renderer.last_exact_rcp(), (name, twin)
                elif name == "bunny":
                    assert renderer.last_exact_rcp(), (name, twin)
                _compare(got, want, rec, twin, f"{name} flags {flags} variant {variant} in flight {in_flight}")


def test_scene_sets_hold_what_they_must():
    """rulers flashes, soccer has a textured sphere, shadows a mesh and a moving light, KAT_SCENE a moving mesh and a second mesh; the
    shipped scenes with light delay off are exactly the ones that run a second time with it on."""
    assert tuple(n for n in CONFIGS if moving_scene(n).params["interval"] == 0) == DELAY_OFF
    assert all(moving_scene(n + "+delay").params["interval"] == -1 for n in DELAY_OFF)
    o = {n: moving_scene(n).objects() for n in ("rulers", "rulers+delay", "soccer", "shadows", "kat")}
    assert (o["rulers"]["flashPeriod"] > 0).any() and (o["rulers+delay"]["flashPeriod"] > 0).any()
    assert ((o["soccer"]["type"] == 0) & (o["soccer"]["textureIndex"] != -1)).any()
    sh = moving_scene("shadows")
    assert (o["shadows"]["type"] == 2).any() and np.any(sh.velocities()[o["shadows"]["light"] != 0, :3])
    kat = moving_scene("kat")
    mesh = o["kat"]["type"] == 2
    assert len(set(o["kat"]["meshIndex"][mesh])) == 2 and np.any(kat.velocities()[mesh, :3])


def test_twins_outside_the_exact_reciprocals_domain(renderer, lib, tmp_path):
    """A mesh with |e1| |e2| > 2^60 in the scene's pool: 241 / 243 run 248's / 249's code (rpt_last_exact_rcp 0)."""
    obj = tmp_path / "huge.obj"
    obj.write_text(HUGE_OBJ)
    scene = Scene.from_file("bunny")
    scene.ReadOBJ(str(obj))
    scene.set_camera((0.3, 0.0, 0.1), 3.0)
    scene.update_objects()
    assert _ffi.hip().rpt_scene_exact_rcp(C.byref(scene.desc())) == 0
    for flags in (1, 2, 3):
        *want, rec = do.render(lib, scene, W, H, flags)
        _doppler_acts(rec, "bunny + huge mesh")
        for variant, twin in ((41, 241), (43, 243), (0, 243)):
            _setup(renderer, scene, W, H, variant, flags)
            got = _frame(renderer)
            assert renderer.last_variant() == twin and not renderer.last_exact_rcp()
            _compare(got, want, rec, twin, f"outside the exact reciprocal's domain, flags {flags} variant {variant}")


# ---- 2. the record kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["arch", "cubes", "shadows", "rulers+delay", "kat"])
@pytest.mark.parametrize("pano", [False, True])
def test_record_kernels_equal_the_c_record(renderer, lib, name, pano):
    scene = moving_scene(name)
    w, h = (PW, PH) if pano else (W, H)
    dirs = do.pano_dirs(w, h) if pano else None
    for flags in (1, 2, 3):
        *want, rec = do.render(lib, scene, w, h, flags, dirs=dirs)
        _doppler_acts(rec, name)
        _setup(renderer, scene, w, h, 0, flags)
        if pano:
            renderer.set_projection("equirect")
        renderer.set_debug_doppler(True)
        got = _frame(renderer)
        kernel = 540 if pano else 240
        assert renderer.last_variant() == kernel
        hit = _compare(got, want, rec, kernel, f"{name} flags {flags}")
        got11 = renderer.read_debug_doppler().reshape(-1, 11)
        want11 = do.record11(rec).reshape(-1, 11)
        ok = _same_bits(got11, want11).all(axis=1)
        assert ok[hit].all(), f"{name} kernel {kernel}: the record differs on {int((~ok[hit]).sum())} hit pixels, first {np.flatnonzero(~ok & hit)[:5]}"
        assert not got11[~hit].any()
        renderer.set_debug_doppler(False)
    renderer.set_projection("pinhole")


# ---- 3. lens and panorama ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant,v_fov,kernel", [("shadows", 3, 0.6, 813), ("shadows", 41, 0.6, 851), ("shadows", 0, 0.6, 853),
                                                       ("cubes", 0, 0.6, 854), ("arch", 0, 0.6, 854), ("kat", 41, 0.6, 851),
                                                       ("shadows", 0, 2.0, 813), ("cubes", 0, 2.0, 813), ("kat", 0, 2.0, 813)])
def test_lens_kernels(renderer, lib, name, variant, v_fov, kernel):
    scene = moving_scene(name)
    objects = orient_objects(scene, *TURN)
    dirs = do.lens_dirs(W, H, v_fov)
    for flags in (1, 2, 3):
        *want, rec = do.render(lib, scene, W, H, flags, dirs=dirs, objects=objects)
        _doppler_acts(rec, name)
        for in_flight in (False, True):
            _setup(renderer, scene, W, H, variant, flags)
            renderer.set_orientation(*TURN)
            renderer.set_field_of_view(v_fov)
            got = _frame(renderer, in_flight)
            assert renderer.last_variant() == kernel, (name, variant, v_fov, renderer.last_variant())
            _compare(got, want, rec, kernel, f"lens {name} v_fov {v_fov} flags {flags} in flight {in_flight}")
    renderer.set_orientation(0, 0, 0)
    renderer.set_field_of_view(0)


@pytest.mark.parametrize("name,variant,kernel", [("shadows", 3, 503), ("shadows", 0, 541), ("kat", 0, 541), ("cubes", 0, 544), ("arch", 0, 544)])
@pytest.mark.parametrize("proj", [{}, REDUCED], ids=["sphere", "reduced"])
def test_panorama_kernels(renderer, lib, name, variant, kernel, proj):
    scene = moving_scene(name)
    dirs = do.pano_dirs(PW, PH, **proj)
    for flags in (1, 2, 3):
        *want, rec = do.render(lib, scene, PW, PH, flags, dirs=dirs)
        _doppler_acts(rec, name)
        _setup(renderer, scene, PW, PH, variant, flags)
        renderer.set_projection("equirect", **proj)
        got = _frame(renderer, in_flight=(flags == 2))
        assert renderer.last_variant() == kernel, (name, variant, renderer.last_variant())
        _compare(got, want, rec, kernel, f"panorama {name} {proj} flags {flags}")
    renderer.set_projection("pinhole")


# ---- 4. the environment kernels with Doppler flags: whole frames ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant,pano,kernel", [("shadows", 3, False, 603), ("shadows", 41, False, 641), ("shadows", 0, False, 643),
                                                      ("cubes", 0, False, 644), ("shadows", 3, True, 703), ("kat", 0, True, 741),
                                                      ("cubes", 0, True, 744)])
def test_environment_kernels_with_doppler(renderer, lib, aa_lib, name, variant, pano, kernel):
    scene = moving_scene(name)
    w, h = (PW, PH) if pano else (W, H)
    dirs = do.pano_dirs(w, h) if pano else do.lens_dirs(w, h)
    img = aa_support.sky_image(96, 48)
    E = scene.camera_lorentz()[1]
    for flags in (1, 2, 3):
        *want, hits = aa_support.oracle_supersampled(aa_lib, scene, w, h, 1, dirs, env=(E, img), flags=flags)
        rec = do.render(lib, scene, w, h, flags, dirs=dirs)[2]
        assert np.array_equal(hits != 0, rec["object"].reshape(-1) >= 0) and 0 < (hits != 0).sum() < w * h
        _doppler_acts(rec, name)
        _setup(renderer, scene, w, h, variant, flags)
        if pano:
            renderer.set_projection("equirect")
        renderer.set_environment(img)
        renderer.set_environment_frame(E)
        got = _frame(renderer)
        assert renderer.last_variant() == kernel, (name, variant, renderer.last_variant())
        _compare(got, want, rec, kernel, f"sky {name} flags {flags}")
    renderer.set_environment(None)
    renderer.set_projection("pinhole")


# ---- 5. generated scenes -----------------------------------------------------------------------------------------------------------------------
GENERATORS = {"random": (lambda rng: random_scene_text(rng)[0], 8), "extreme": (extreme_scene_text, 8), "close": (close_scene_text, 7),
              "walls": (walls_scene_text, 7)}


def test_thirty_generated_scenes_in_all():
    assert sum(n for _, n in GENERATORS.values()) == 30


@pytest.mark.parametrize("gen", list(GENERATORS))
def test_generated_scenes(renderer, lib, gen):
    """Default variant, shift and beaming.  An extreme scene's D may overflow: S_f is total, and a NaN must be matched by a NaN."""
    make, count = GENERATORS[gen]
    rng = np.random.default_rng(777 + len(gen))
    seen, hits = set(), 0
    for i in range(count):
        scene = Scene()
        scene.inputScene(make(rng))
        v = rng.normal(size=3)
        v = v / np.linalg.norm(v) * (0.0, 0.5, 0.95)[i % 3]
        scene.set_camera(tuple(float(c) for c in v), float(rng.uniform(-3, 20)))
        scene.update_objects()
        *want, rec = do.render(lib, scene, W, H, 3)
        _setup(renderer, scene, W, H, 0, 3)
        got = _frame(renderer)
        seen.add(renderer.last_variant())
        hits += int(_compare(got, want, rec, renderer.last_variant(), f"{gen} scene {i}").sum())
    assert seen and seen <= {241, 243, 244} and hits > 0
