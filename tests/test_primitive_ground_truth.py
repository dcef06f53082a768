"""Spheres, cubes, the nearest-object choice, the boosts, the flash, the time windows, the texture fetch, a mesh hit's normal and (u, v)
and the light-delay shading against the float64 model of tests/primitive_truth.py, without a GPU: the CPU
restatements — oracle_ffi.render's float RGB, events_oracle.oracle_events and window_oracle — on every case of tests/primitive_cases.py;
the corruptions that the comparison must catch (sections 2 and 2a); the front end's per-frame matrices against float64 boosts.
tests/test_gpu_primitive_ground_truth.py holds the device to the same assertions, constants and caps, imported from here.

What is asserted per frame (`check_frame`): on well-conditioned pixels the object index equals the model's with no exception and dist,
event and (u, v) are within the bounds derived in primitive_truth's docstring; the colour is within COLOUR_FACTOR x the error MEASURED on
the CPU oracle, plus, on a textured or mesh hit, the pixel's own derived texture and normal terms (the model's `rgb_extra`); an
ill-conditioned pixel may differ only towards an object the model's conditioning names (unexplained: 0); and the
filters do not hide the frame (the caps)."""
import functools

import numpy as np
import pytest

import events_oracle as eo
import mesh_truth
import oracle_ffi
import primitive_cases as pc
import primitive_truth as pt
import window_oracle as wo

# The colour's error chain is not derived (primitive_truth, "Bounds"): measured on the CPU oracle over the committed case list — the
# largest error of a tonemapped channel relative to max(model, COLOUR_FLOOR) over the well-conditioned pixels of every case — and
# asserted at 8 x that value, as MEASURED_NULL_CONE_RESIDUAL / NULL_CONE_FACTOR are in tests/test_events_model.py.  Run with -s to see
# each case's figure.  Measured against the oracle, never against device output.
# The pixel that sets it is (24, 11) of shadows-rest-i-1: the small sphere (object 2, three pixels wide at 64 x 36), lit, no occluder near its
# segment (the mesh occluder's silhouette is flagged by mesh_truth's margin); its neighbours on the same sphere show 8.5e-06, 6.5e-06 and
# 5.6e-06.  The hit distance there is off by 2e-05 relative (its derived bound's size), which moves the object-space point, hence the
# normal and cos(theta) = 0.29, by that over a radius of 1: an error of the record carried into the weight, not a shadow edge.  The
# other cases lie between 0 and 6.6e-06.
# Textured and mesh hits, which carry a colour since the model fetches textures and interpolates mesh normals, are held to the SAME
# allowance on top of their derived per-pixel terms; no second constant was needed.  What is left of their error beyond the derived terms,
# measured the same way on the CPU oracle: at most 2.94e-05 (tex-room-oblique; 1.27e-05 on tex-room-rest, every other
# case with textured or mesh hits below that) — inside 8 x 1.40e-05.  The figure above stays what the untextured spheres and cubes measure.
MEASURED_COLOUR_ERROR = 1.40e-05
COLOUR_FACTOR = 8.0
COLOUR_FLOOR = 1e-3
CAP_RECORDS, CAP_COLOURS, CAP_OVERALL = 0.90, 0.85, 0.95


def colour_bound():
    return COLOUR_FACTOR * MEASURED_COLOUR_ERROR


@pytest.fixture(scope="module")
def wlib(tmp_path_factory):
    return wo.build_library(tmp_path_factory.mktemp("primitive_truth_w"))


@pytest.fixture(scope="module")
def elib(tmp_path_factory):
    return eo.build_library(tmp_path_factory.mktemp("primitive_truth_e"))


# ---- the model's frames: computed once per case and shared ------------------------------------------------------------------------------
_CASES = {c[0]: c for c in pc.cases()}


@functools.lru_cache(maxsize=None)
def case_scene(name):
    return _CASES[name][2]()


def model_frame(scene, objs, dirs, windows=None, interval=None):
    p = scene.params
    has_mesh = bool((np.asarray(objs)["type"] == 2).any())
    textured = bool((np.asarray(objs)["textureIndex"] != -1).any())
    return pt.frame(objs, dirs, p["interval"] if interval is None else interval, p["ambient"], p["white_point"], windows=windows,
                    mesh_arrays=mesh_truth.arrays(scene) if has_mesh else None, textures=scene.buffers()["textures"] if textured else None)


_MODEL = {}


def case_model(name, wlib):
    """(scene, W, H, dirs, windows, model frame) of a case, the model's frame computed once."""
    if name not in _MODEL:
        _, _, _, W, H, rule, v_fov = _CASES[name]
        scene = case_scene(name)
        dirs = eo.pinhole_dirs(W, H, None if v_fov is None else eo.lens_scale(v_fov))
        windows = None
        if rule is not None:
            windows = wo.choose_windows(wlib, scene, W, H, dirs=dirs, flip=(rule == "choose_flip"))
            assert np.isfinite(windows).any(), f"{name}: no window acts"
        _MODEL[name] = (scene, W, H, dirs, windows, model_frame(scene, scene.objects(), dirs, windows))
    return _MODEL[name]


def check_frame(label, model, objs, rec, rgb, caps=True, report=None):
    """The assertions of this file's docstring for one frame of a float program (oracle or device): rec (N) records, rgb (N, 3)
    tonemapped floats or None.  Returns the figures; `report`, a dict, collects them by label."""
    r = pt.compare_records(model, rec, objs)
    c = pt.compare_colours(model, rgb, COLOUR_FLOOR) if rgb is not None else None
    line = (f"{label}: {r['hits']} model hit pixels, records well-conditioned {r['well_share']:.1%}, ill-conditioned differences {len(r['ill_diff'])} "
            f"(unexplained {len(r['unexplained'])}); error / bound: dist {r['ratio_dist']:.3f}, event {r['ratio_event']:.3f}, uv {r['ratio_uv']:.3f}; "
            f"largest relative dist error {r['rel_dist']:.2e}")
    if c is not None:
        line += f"; colours well-conditioned {c['well_share']:.1%} of {c['coloured']}, relative error median {c['median']:.2e} max {c['rel']:.2e}, miss {c['miss']:.2e}"
    print(line)
    if report is not None:
        report[label] = (r, c)
    assert r["index_bad"].size == 0, (label, "object index differs on well-conditioned pixels", r["index_bad"][:8])
    assert r["attr_bad"].size == 0, (label, "dist, event or (u, v) beyond its derived bound", r["attr_bad"][:8], r["ratio_dist"], r["ratio_event"], r["ratio_uv"])
    assert r["unexplained"].size == 0, (label, "an ill-conditioned difference that no conditioning figure explains", r["unexplained"][:8])
    if c is not None:
        assert c["rel"] <= colour_bound(), (label, f"colour error {c['rel']:.3e} > {colour_bound():.3e} at pixel {c['worst']}")
        assert c["miss"] <= colour_bound(), (label, "the background's colour", c["miss"])
    if caps:
        assert r["hits"] >= pc.MIN_HIT_PIXELS, (label, "too few model hit pixels: change the camera, not the threshold", r["hits"])
        assert r["well_share"] >= CAP_RECORDS, (label, "records: well-conditioned share below the cap", r["well_share"])
        if c is not None and c["coloured"]:
            assert c["well_share"] >= CAP_COLOURS, (label, "colours: well-conditioned share below the cap", c["well_share"])
    return r, c


# ---- 1. the CPU restatements against the model on every case ----------------------------------------------------------------------------
_REPORT = {}


@pytest.mark.parametrize("name", pc.case_ids())
def test_cpu_restatements_agree_with_the_model(wlib, elib, name):
    scene, W, H, dirs, windows, model = case_model(name, wlib)
    objs = scene.objects()
    _, rgb, rec, _ = wo.render(wlib, scene, W, H, windows, dirs=dirs)
    check_frame(name, model, objs, rec, rgb, report=_REPORT)
    if windows is None and _CASES[name][6] is None:
        # the un-windowed restatements are the same program: oracle_ffi.render's float RGB and events_oracle's records, bit for bit
        _, rgb2, _ = oracle_ffi.render(scene, W, H)
        assert np.array_equal(rgb2.view(np.uint32), rgb.view(np.uint32)), f"{name}: oracle_ffi.render and window_oracle differ"
        rec2 = eo.oracle_events(elib, scene, W, H)
        assert rec2.tobytes() == rec.tobytes(), f"{name}: events_oracle and window_oracle differ"


def test_the_needles_of_ellipsoids_seed_2_keep_their_records(wlib):
    """ellipsoids seed 2 left the case list when textured hits began to carry a colour (primitive_cases.SEEDS): 95 % of its pixels have
    no finite texture term, so it cannot meet the colours' cap.  Its records — the list's largest error / bound, 0.23, on needles of
    scale ratio 236 — and the colours of its well-conditioned pixels stay held here, without the caps."""
    scene = pc.generated("ellipsoids", 2)
    W, H = 128, 72
    dirs = eo.pinhole_dirs(W, H)
    objs = scene.objects()
    _, rgb, rec, _ = wo.render(wlib, scene, W, H, None, dirs=dirs)
    r, _ = check_frame("ellipsoids-2 (records)", model_frame(scene, objs, dirs), objs, rec, rgb, caps=False)
    assert r["hits"] >= pc.MIN_HIT_PIXELS and r["well_share"] >= CAP_RECORDS


def test_caps_over_all_cases_and_non_vacuity(wlib):
    """Over all cases at least CAP_OVERALL of the model's hit pixels are well-conditioned for records and for colours, and each group
    of cases shows what primitive_cases.NON_VACUITY says it must."""
    hits = well = coloured = well_c = 0
    seen = {g: set() for g in pc.NON_VACUITY}
    worst_null = 0.0
    for name, group, *_ in pc.cases():
        scene, W, H, dirs, windows, m = case_model(name, wlib)
        objs = scene.objects()
        h = m["object"] >= 0
        col = h & np.isfinite(m["rgb"]).all(axis=1)
        hits, well = hits + int(h.sum()), well + int((m["well_rec"] & h).sum())
        coloured, well_c = coloured + int(col.sum()), well_c + int((m["well_col"] & col).sum())
        worst_null = max(worst_null, m.get("null_residual", 0.0))
        speed = np.linalg.norm(scene.velocities().astype(np.float64)[:, :3], axis=1)
        moving = speed > 0
        fast = np.flatnonzero((speed >= pc.FAST) & (objs["type"] != 2))
        flashy = np.zeros(len(h), dtype=bool)
        flashy[h] = objs["flashPeriod"][m["object"][h]] > 0
        wc, wr = m["well_col"], m["well_rec"]
        on_fast = np.isin(m["object"], fast)
        which = np.where(h, m["object"], 0)
        textured = h & (objs["textureIndex"][which] != -1)
        on_mesh = h & (objs["type"][which] == 2)
        vt_less = np.zeros(len(h), dtype=bool)
        for i in np.flatnonzero(objs["type"] == 2):
            a = mesh_truth.arrays(scene)
            ids, _ = mesh_truth.mesh_triangles(a, i)
            words = a["triangles"].astype(np.int64)
            if len(np.unique(np.concatenate([words[9 * ids + 1], words[9 * ids + 4], words[9 * ids + 7]]))) == 1:
                vt_less |= m["object"] == i
        lit_any, dark_any = m["lit"].any(axis=0), m["shadowed"].any(axis=0)
        by_other = m["shadow_by"].copy()                       # shadowed by an object other than the one that is hit
        by_other[which[h], np.flatnonzero(h)] = False
        for ax, side in {(int(a), int(s)) for a, s in zip(m["face"][textured & wc], m["face_side"][textured & wc]) if a >= 0}:
            seen[group].add(f"textured_cube_face_{'xyz'[ax]}{'+' if side > 0 else '-'}")
        props = {
            "textured_lit": (textured & lit_any & wc).any(), "textured_shadowed": (textured & dark_any & wc).any(),
            "textured_flashing": (textured & m["flashing"] & wc).any(), "textured_not_flashing": (textured & flashy & ~m["flashing"] & wc).any(),
            "mesh_lit": (on_mesh & lit_any & wc).any(), "mesh_shadowed": (on_mesh & by_other.any(axis=0) & wc).any(),
            "mesh_self_shadowed": (on_mesh & m["self_shadow"] & wc).any(), "clamped_tap": (m["clamped_tap"] & wc).any(),
            "second_texture_in_pool": (textured & (objs["textureIndex"][which] > 0) & wc).any(), "vt_less_mesh_textured": (vt_less & textured & wc).any(),
            "sphere_seam_both_sides": all((textured & (objs["type"][which] == 0) & wc & near).any() for near in (m["uv"][:, 0] < 0.02, m["uv"][:, 0] > 0.98)),
            "sphere_both_poles": all((textured & (objs["type"][which] == 0) & wc & near).any() for near in (m["uv"][:, 1] < 0.1, m["uv"][:, 1] > 0.9)),
            "lit": (m["lit"].any(axis=0) & wc).any(), "shadowed": (m["shadowed"].any(axis=0) & wc).any(),
            "lit_by_moving_lamp": (m["lit"][moving].any(axis=0) & wc).any(), "shadowed_by_moving_occluder": (m["shadow_by"][moving].any(axis=0) & wc).any(),
            "self_shadowed": (m["self_shadow"] & wc).any(),
            "flashing": (m["flashing"] & wc).any(), "not_flashing": (flashy & ~m["flashing"] & wc).any(),
            "flashing_clock": (m["flashing"] & wr & (m["figures"]["flash_dist"] > pt.FLASH_MARGIN)).any(),
            "not_flashing_clock": (flashy & ~m["flashing"] & wr & (m["figures"]["flash_dist"] > pt.FLASH_MARGIN)).any(),
            "windowed_out": (m["windowed_out"] & wr).any(), "inside": (m["inside"] & wr).any(),
            "fast_primitive_hit": (on_fast & wr).any(), "fast_primitive_coloured": (on_fast & wc).any(),
            "fast_primitive_lit": (on_fast & wc & m["lit"].any(axis=0) & (m["rgb"] < 1.0).any(axis=1)).any(),
        }
        seen[group] |= {k for k, v in props.items() if v}
    for g in seen:
        if all(f"textured_cube_face_{a}{sg}" in seen[g] for a in "xyz" for sg in "+-"):
            seen[g].add("all_cube_faces_textured")
    print(f"all cases: records well-conditioned {well / hits:.2%} of {hits} hit pixels, colours {well_c / coloured:.2%} of {coloured}; "
          f"largest null residual of a hit -> emission displacement {worst_null:.2e}")
    print("shown per group: " + "; ".join(f"{g}: {sorted(v)}" for g, v in seen.items()))
    assert well >= CAP_OVERALL * hits and well_c >= CAP_OVERALL * coloured
    for group, wanted in pc.NON_VACUITY.items():
        missing = set(wanted) - seen[group]
        assert not missing, f"group {group}: no well-conditioned pixel shows {sorted(missing)}"


# ---- 2. the tests must bite ----------------------------------------------------------------------------------------------------------------
def _five(interval=-1, t=2.0, text=pc.FIVE):
    return eo.scene_from_text(text, t=t, interval=interval)


def _fails(model, objs, rec, rgb):
    try:
        check_frame("corrupted", model, objs, rec, rgb, caps=False)
    except AssertionError:
        return True
    return False


def _pair(wlib, scene, corrupted_objects=None, windows=None, corrupted_windows=None, model_kw=None, W=128, H=72):
    """(clean passes, corrupted fails) for the five-object scene: the model is of the CLEAN objects and windows, the oracle gets the
    corrupted ones."""
    dirs = eo.pinhole_dirs(W, H)
    objs = scene.objects()
    model = model_frame(scene, objs, dirs, windows)
    _, rgb, rec, _ = wo.render(wlib, scene, W, H, windows, dirs=dirs)
    check_frame("clean", model, objs, rec, rgb, caps=False)
    _, rgb, rec, _ = wo.render(wlib, scene, W, H, windows if corrupted_windows is None else corrupted_windows, dirs=dirs, objects=corrupted_objects)
    return _fails(model, objs, rec, rgb)


def test_bites_a_lamps_velocity_off_by_1e_3(wlib):
    clean = _five()
    other = _five(text=pc.FIVE.replace("v0.8,0,0", "v0.801,0,0"))
    bad = clean.objects().copy()
    bad[pc.FIVE_MOVING_LAMP] = other.objects()[pc.FIVE_MOVING_LAMP]
    assert _pair(wlib, clean, corrupted_objects=bad)


def test_bites_an_inverse_boosts_time_column_negated(wlib):
    clean = _five()
    bad = clean.objects().copy()
    bad["InvLorentz"][pc.FIVE_FLOOR][:, 0] *= -1
    assert _pair(wlib, clean, corrupted_objects=bad)


def test_bites_the_falloff_distance_taken_in_the_lamps_frame(wlib, monkeypatch):
    """The one corruption that is a slip of the program, not of its data, so it cannot go through `objects=`: r of the weight measured
    in the lamp's rest frame instead of the hit object's.  The comparison is symmetric, so the slip is given to the MODEL's side, by
    wrapping its weight function here (the model itself has no switch for it)."""
    scene = _five()
    W, H = 128, 72
    dirs = eo.pinhole_dirs(W, H)
    objs = scene.objects()
    _, rgb, rec, _ = wo.render(wlib, scene, W, H, None, dirs=dirs)
    check_frame("clean", model_frame(scene, objs, dirs), objs, rec, rgb, caps=False)
    right = pt.weight
    monkeypatch.setattr(pt, "weight", lambda cos, r_hit_frame, r_light_frame: right(cos, r_light_frame, r_hit_frame))
    assert _fails(model_frame(scene, objs, dirs), objs, rec, rgb)


def test_bites_a_window_end_moved_by_1e_3_of_its_length(wlib):
    scene = _five()
    W, H = 128, 72
    dirs = eo.pinhole_dirs(W, H)
    objs = scene.objects()
    base = model_frame(scene, objs, dirs)
    mine = np.flatnonzero((base["object"] == pc.FIVE_CUBE) & base["well_rec"])
    e0 = base["event"][mine, 0]
    p = mine[np.argsort(e0)[len(e0) // 2]]                    # the cube's median pixel by emission time
    length = 4.0
    t1 = float(np.float32(base["event"][p, 0] + 0.5e-3 * length))
    windows = wo.default_windows(len(objs))
    windows[pc.FIVE_CUBE] = (t1 - length, t1)
    moved = windows.copy()
    moved[pc.FIVE_CUBE, 1] = np.float32(t1 - 1e-3 * length)
    assert _pair(wlib, scene, windows=windows, corrupted_windows=moved)


def test_bites_a_flash_duration_off_by_one_percent(wlib):
    scene = _five()
    W, H = 128, 72
    dirs = eo.pinhole_dirs(W, H)
    objs = scene.objects()
    base = model_frame(scene, objs, dirs)
    mine = np.flatnonzero((base["object"] == pc.FIVE_SPHERE) & base["well_rec"])
    period = float(objs[pc.FIVE_SPHERE]["flashPeriod"])
    e0 = base["event"][mine, 0]
    phase = e0 - period * np.floor(e0 / period)
    k = np.argsort(phase)[len(phase) // 2]
    clean = objs.copy()
    clean["flashDuration"][pc.FIVE_SPHERE] = np.float32(phase[k] * 1.005)      # the median pixel flashes ...
    bad = clean.copy()
    bad["flashDuration"][pc.FIVE_SPHERE] = np.float32(clean["flashDuration"][pc.FIVE_SPHERE] * 0.99)      # ... and with 1 % less does not
    model = model_frame(scene, clean, dirs)
    _, rgb, rec, _ = wo.render(wlib, scene, W, H, None, dirs=dirs, objects=clean)
    check_frame("clean", model, clean, rec, rgb, caps=False)
    _, rgb, rec, _ = wo.render(wlib, scene, W, H, None, dirs=dirs, objects=bad)
    assert _fails(model, clean, rec, rgb)


@pytest.mark.parametrize("which", [pc.FIVE_SPHERE, pc.FIVE_CUBE])
def test_bites_an_object_space_translation_of_1e_4(wlib, which):
    """A thin bite, on purpose at the issue's size: 1e-4 object units is 1.4 x the derived bound on `dist` (sphere and cube alike; the
    cube's colour does not notice, the sphere's is at the colour bound).  A looser ROUNDINGS or intersector slack in primitive_truth
    would make it vacuous — this test is what says so."""
    clean = _five()
    bad = clean.objects().copy()
    bad["InvM"][which][0, 3] += np.float32(1e-4)
    assert _pair(wlib, clean, corrupted_objects=bad)


def test_bites_a_mesh_moved_in_a_corrupted_copy_of_the_arrays(wlib):
    """mesh_truth.arrays takes a corrupted COPY the same way: the pear of Scenes/shadows.txt with its vertices moved by 1e-3 of the
    mesh's size in the MODEL's copy — the oracle, on the scene as it is, must then fail the comparison."""
    scene = eo.load_scene("shadows", "rest", -1)
    W, H = 64, 36
    dirs = eo.pinhole_dirs(W, H)
    objs, p = scene.objects(), scene.params
    _, rgb, rec, _ = wo.render(wlib, scene, W, H, None, dirs=dirs)
    arrays = mesh_truth.arrays(scene)
    check_frame("clean", pt.frame(objs, dirs, -1, p["ambient"], p["white_point"], mesh_arrays=arrays), objs, rec, rgb, caps=False)
    moved = dict(arrays)
    moved["vertices"] = arrays["vertices"].copy()
    span = float(np.ptp(arrays["vertices"][:, :3], axis=0).max())
    moved["vertices"][:, 2] += np.float32(1e-3 * span)
    assert _fails(pt.frame(objs, dirs, -1, p["ambient"], p["white_point"], mesh_arrays=moved), objs, rec, rgb)


# ---- 2a. textures and mesh attributes must bite --------------------------------------------------------------------------------------------
# (One corruption asked of this list is not here: the 0.001 offset of the shadow segment taken along a mesh hit's FACE normal instead of
# the interpolated one.  Given to the model's side on every committed mesh case — both pears, both bunnies, shadows.txt, extreme-8 — it
# moves no well-conditioned pixel beyond its bound: the start moves by 0.001 |dn|, far inside a mesh pixel's normal term.  Not tuned for.)
def _textured(text, W=128, H=72, t=0.0):
    scene = pc._text(text, "rest", -1, t=t, root=pc.asset_root())
    return scene, W, H, eo.pinhole_dirs(W, H)


def _clean_frame(wlib, scene, W, H, dirs):
    objs = scene.objects()
    _, rgb, rec, _ = wo.render(wlib, scene, W, H, None, dirs=dirs)
    check_frame("clean", model_frame(scene, objs, dirs), objs, rec, rgb, caps=False)
    return objs, rec, rgb


def _oracle_on_corrupted_objects_fails(wlib, scene, W, H, dirs, bad):
    """The model of the CLEAN objects, the oracle handed `bad`."""
    objs, _, _ = _clean_frame(wlib, scene, W, H, dirs)
    _, rgb, rec, _ = wo.render(wlib, scene, W, H, None, dirs=dirs, objects=bad)
    return _fails(model_frame(scene, objs, dirs), objs, rec, rgb)


def test_bites_texture_width_and_height_swapped_on_the_3x5(wlib):
    scene, W, H, dirs = _textured(pc.TEX_FIVE, t=2.0)
    bad = scene.objects().copy()
    assert (int(bad["textureWidth"][pc.FIVE_FLOOR]), int(bad["textureHeight"][pc.FIVE_FLOOR])) == pc.TEXTURES["t3x5"]
    bad["textureWidth"][pc.FIVE_FLOOR], bad["textureHeight"][pc.FIVE_FLOOR] = pc.TEXTURES["t3x5"][::-1]
    assert _oracle_on_corrupted_objects_fails(wlib, scene, W, H, dirs, bad)


@pytest.mark.parametrize("which", [pc.FIVE_FLOOR, pc.FIVE_SPHERE])
def test_bites_a_texture_index_off_by_3_bytes(wlib, which):
    """One texel along the row: on the 3 x 5 floor (second in the pool) and on the 16 x 16 sphere (first)."""
    scene, W, H, dirs = _textured(pc.TEX_FIVE, t=2.0)
    bad = scene.objects().copy()
    bad["textureIndex"][which] += 3
    assert _oracle_on_corrupted_objects_fails(wlib, scene, W, H, dirs, bad)


@pytest.mark.parametrize("slip", ["v not flipped", "half-texel offset", "channel order reversed"])
def test_bites_a_slip_of_the_texture_fetch(wlib, monkeypatch, slip):
    """Slips of the program, not of its data: given to the MODEL's side by wrapping its own functions, as the falloff's frame is above."""
    scene, W, H, dirs = _textured(pc.TEX_FIVE, t=2.0)
    objs, rec, rgb = _clean_frame(wlib, scene, W, H, dirs)
    if slip == "v not flipped":
        monkeypatch.setattr(pt, "texel_coords", lambda u, v, Wt, Ht: (Wt * u, Ht * v))
    elif slip == "half-texel offset":
        right = pt.texel_coords
        monkeypatch.setattr(pt, "texel_coords", lambda u, v, Wt, Ht: tuple(x - 0.5 for x in right(u, v, Wt, Ht)))
    else:
        right_texels = pt.texels
        monkeypatch.setattr(pt, "texels", lambda pool, index, Wt, x, y: right_texels(pool, index, Wt, x, y)[..., ::-1])
    assert _fails(model_frame(scene, objs, dirs), objs, rec, rgb)


def _pear_frames(wlib):
    scene, W, H, _ = _textured(pc.TEX_PEAR, 64, 36)
    dirs = eo.pinhole_dirs(W, H, eo.lens_scale(pc.LENS_HALF))
    objs, p = scene.objects(), scene.params
    _, rgb, rec, _ = wo.render(wlib, scene, W, H, None, dirs=dirs)
    arrays = mesh_truth.arrays(scene)
    model = lambda a: pt.frame(objs, dirs, -1, p["ambient"], p["white_point"], mesh_arrays=a)      # noqa: E731
    check_frame("clean", model(arrays), objs, rec, rgb, caps=False)
    return arrays, model, objs, rec, rgb


def test_bites_a_meshs_vertex_normals_replaced_by_its_face_normals(wlib):
    """In the MODEL's copy of the arrays every corner of a triangle reads that triangle's own normal (on the side of its vertex normals)."""
    arrays, model, objs, rec, rgb = _pear_frames(wlib)
    words = arrays["triangles"].astype(np.int64)
    T = len(words) // 9
    v, n = arrays["vertices"][:, :3].astype(np.float64), arrays["normals"]
    A, B, C = (v[words[9 * np.arange(T) + k]] for k in (0, 3, 6))
    face = np.cross(B - A, C - A)
    face /= np.maximum(np.linalg.norm(face, axis=1, keepdims=True), 1e-300)
    face *= np.where(np.einsum("ij,ij->i", face, n[words[9 * np.arange(T) + 2], :3].astype(np.float64)) < 0, -1.0, 1.0)[:, None]
    flat = dict(arrays)
    extra = np.zeros((T, n.shape[1]), dtype=n.dtype)
    extra[:, :3] = face
    flat["normals"] = np.vstack([n, extra])
    tri = arrays["triangles"].copy()
    for k in (2, 5, 8):
        tri[9 * np.arange(T) + k] = len(n) + np.arange(T)
    flat["triangles"] = tri
    assert _fails(model(flat), objs, rec, rgb)


def test_bites_a_meshs_uv_corners_b_and_c_exchanged(wlib):
    arrays, model, objs, rec, rgb = _pear_frames(wlib)
    T = len(arrays["triangles"]) // 9
    swapped = dict(arrays)
    tri = arrays["triangles"].copy()
    tri[9 * np.arange(T) + 4], tri[9 * np.arange(T) + 7] = arrays["triangles"][9 * np.arange(T) + 7], arrays["triangles"][9 * np.arange(T) + 4]
    swapped["triangles"] = tri
    assert _fails(model(swapped), objs, rec, rgb)


# ---- 3. the front end's per-frame matrices ------------------------------------------------------------------------------------------------
U = 2.0 ** -24
FAST = ("Os\n p0,0,6,0,0,1,0,1,1,1\n v0.9999,0,0\nOc\n p1,2,9,0.3,0,1,0,1,2,1\n v0,-0.7,0.7141\nOs\n p-3,0,5,0,0,1,0,1,1,1\n v-0.57735,0.57735,-0.57730\n"
        "Oc\n p0,-2,7,0,0,1,0,3,1,3\nR\n")


def _gamma(v):
    return 1.0 / np.sqrt(1.0 - float(np.dot(v, v)))


def matrix_bounds(v_obj, v_cam):
    """(bound, Lorentz, bound, InvLorentz) in float64: the entrywise bound on Lorentz = boost(v_obj) . boost(-v_cam) formed in float32 from float32 velocities.  One float boost: gamma =
    1 / sqrt(1 - |v|^2) — the float 1 - |v|^2 is off by up to 3u absolute (three products, two sums, the subtraction), which is
    3u gamma^2 RELATIVE to it, half of that in gamma after the root, plus 2u for root and divide; the entries are products of gamma,
    (gamma - 1) / |v|^2 and v's components, 4 more roundings: every entry of a boost is off by at most e(gamma) = (1.5 gamma^2 + 6) u
    relative to the matrix of absolute values |B|.  The product of two such, a 4-term float dot per entry (4u more):
        |dL|  <=  (e(gamma_obj) + e(gamma_cam) + 4u) |B_obj| |B_cam|      entrywise.
    It grows with gamma_obj^2 + gamma_cam^2 relative to |B_obj| |B_cam|, whose entries grow with gamma_obj gamma_cam.  The inverse is boost(v_cam) . boost(-v_obj): the same bound with
    the factors in the other order (boosts are symmetric matrices)."""
    e = lambda g: (1.5 * g * g + 6.0) * U      # noqa: E731
    Bo, Bc = pt.boost(v_obj), pt.boost(-np.asarray(v_cam, dtype=np.float64))
    rel = e(_gamma(v_obj)) + e(_gamma(v_cam)) + 4 * U
    return rel * (np.abs(Bo) @ np.abs(Bc)), Bo @ Bc, rel * (np.abs(Bc.T) @ np.abs(Bo.T)), pt.boost(v_cam) @ pt.boost(-np.asarray(v_obj, dtype=np.float64))


@pytest.mark.parametrize("camera", sorted(pc.CAMERAS))
@pytest.mark.parametrize("text", ["five", "fast"])
def test_front_end_matrices_against_float64_boosts(camera, text):
    """Scene.objects() after update_objects against float64 boost(v_i) . boost(-v_c) from Scene.velocities() and get_camera(): Lorentz,
    InvLorentz (the boosts with the velocities negated, in the other order), stationaryCam = Lorentz . camera event, InvM . M = I."""
    v_cam = pc.CAMERAS[camera][0]
    scene = eo.scene_from_text(pc.FIVE if text == "five" else FAST, t=1.5)
    scene.set_camera(v_cam, 1.5, (0.25, -0.5, 1.0))
    scene.update_objects()
    objs, vel = scene.objects(), scene.velocities().astype(np.float64)[:, :3]
    vc, cam = (np.asarray(x, dtype=np.float64) for x in scene.get_camera())
    worst = 0.0
    for i in range(len(objs)):
        tol, L, tol_inv, Linv = matrix_bounds(vel[i], vc)
        for got, want, bound, what in ((objs["Lorentz"][i], L, tol, "Lorentz"), (objs["InvLorentz"][i], Linv, tol_inv, "InvLorentz")):
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= bound).all(), (i, what, float(err.max()), _gamma(vel[i]), _gamma(vc))
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        sc_bound = tol @ np.abs(cam) + 4 * U * np.abs(L) @ np.abs(cam)
        err = np.abs(objs["stationaryCam"][i].astype(np.float64) - L @ cam)
        assert (err <= sc_bound).all(), (i, "stationaryCam", err, sc_bound)
        M, InvM = objs["M"][i].astype(np.float64), objs["InvM"][i].astype(np.float64)
        eye_err = np.abs(InvM @ M - np.eye(4))
        eye_bound = 16 * U * (np.abs(InvM) @ np.abs(M))
        assert (eye_err <= eye_bound).all(), (i, "InvM . M", eye_err.max())
    print(f"{text} {camera}: gamma_cam {_gamma(vc):.2f}, largest gamma_obj {max(_gamma(v) for v in vel):.1f}; largest observed error / bound {worst:.3f}")
