"""The ballistic pass without a device: tests/native/ballistics_oracle.c, the C restatement of the rules and the reference
of tests/test_gpu_ballistics.py, against relativitypathtracer_amd.ballistics.project, the float64 model; u = 0 against the particle
oracle, byte for byte; the model against the particle model under a change of frame, and against special relativity's closed forms; the
emission window; and the non-vacuity of tests/ballistics_cases.py on CPU event frames.

The float32 bound (DESIGN.md §24 "How far float32 may put a record from the float64 model"; MEASURED on the crafted sets of this file,
times four — the dust pass's convention —, not derived: pos + beta cam.x - cam.yzw rounds at the scale of its terms, not of its result,
so a bound in eps alone does not exist).  With eps = 2^-24, gamma = sqrt(1 + u.u) of the record and A = the 2-norm of its object's
InvLorentz, e = gamma A^2 eps:
    the camera directions differ by dn <= K_N e, which goes through §20's projection steps as its dn does;
    |d dist| / dist <= K_DIST e;   |d D| / D <= K_D e;
    and on the approach set (u up to 300 towards the camera, identity frames: A = 1) |d D| / D <= K_APPROACH gamma eps."""
import math

import numpy as np
import pytest

import ballistics_cases as bc
import events_oracle as eo
import particles_cases as pc
import stars_cases as sc
from relativitypathtracer_amd import ballistics, particles
from relativitypathtracer_amd.events import _objects_array
from relativitypathtracer_amd.scene import OBJECT_DTYPE

EPS = 2.0 ** -24
# four times the largest figure measured on the 32 cases of test_the_c_oracle_puts_every_record_where_the_float64_model_does (0.647,
# 8.309, 3.123) and on test_the_approach_case (1.763): see DESIGN.md §24
K_N, K_DIST, K_D, K_APPROACH = 2.6, 33.3, 12.5, 7.1


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return bc.build_library(tmp_path_factory.mktemp("ballistics"))


@pytest.fixture(scope="module")
def particles_lib(tmp_path_factory):
    return pc.build_library(tmp_path_factory.mktemp("ballistics_particles"))


@pytest.fixture(scope="module")
def events_lib(tmp_path_factory):
    return eo.build_library(tmp_path_factory.mktemp("ballistics_events"))


_FRAMES = {}


def _frame(events_lib, scene_name, motion, interval, name, turned, W, H):
    """(scene, Object[] of the view, (H * W) records, camera) of tests/native/event_oracle.c, computed once per view."""
    key = (scene_name, motion, interval, name, turned, W, H)
    if key not in _FRAMES:
        scene = eo.load_scene(scene_name, motion, interval)
        cam = dict({k: v for k, v in bc.CAMERAS[name].items() if k != "orientation"}, orientation=sc.YPR if turned else None)
        _FRAMES[key] = (scene, pc.scene_objects(scene, cam), sc.cpu_events(events_lib, scene, W, H, cam).reshape(-1), cam)
    return _FRAMES[key]


def identity_frame(cam_t=0.0, cam=(0.0, 0.0, 0.0)):
    """One Object at rest with the camera, the camera event at (cam_t, cam) of its clock and axes."""
    o = np.zeros(1, dtype=OBJECT_DTYPE)
    o["InvLorentz"][0] = np.eye(4)
    o["Lorentz"][0] = np.eye(4)
    o["stationaryCam"][0] = (cam_t,) + tuple(cam)
    return o


# ---- the C oracle against the model ---------------------------------------------------------------------------------------------
def _position_ratios(got, want, camera, W, H, e):
    """(|dX| over §20's bound with dn = e, |dY| likewise, the records compared) — the bound's shape is tests/test_particles_model.py's."""
    n = want["n"]
    both = got["visible"] & want["visible"]
    if camera["mode"] == "pinhole":
        s = float(eo.lens_scale(camera["v_fov"])) if camera.get("v_fov") else 1.0
        both &= n[:, 2] >= 0.05
        with np.errstate(all="ignore"):
            tol_x = 1.01 * W / (2 * s * (W / H)) * (1 / n[:, 2] + np.abs(n[:, 0]) / n[:, 2] ** 2) * e + 5 * EPS * (np.abs(want["X"]) + W)
            tol_y = 1.01 * H / (2 * s) * (1 / n[:, 2] + np.abs(n[:, 1]) / n[:, 2] ** 2) * e + 5 * EPS * (np.abs(want["Y"]) + H)
        dx = got["X"] - want["X"]
    else:
        h_fov, v_fov = float(np.float32(camera.get("h_fov", 2 * math.pi))), float(np.float32(camera.get("v_fov", math.pi)))
        h = np.hypot(n[:, 0], n[:, 2])
        with np.errstate(all="ignore"):
            tol_x = W / h_fov * (np.minimum(1.01 * e / h, 2 * math.pi) + 100 * EPS) + 4 * EPS * (np.abs(want["X"]) + W)
            tol_y = H / v_fov * (np.minimum(1.01 * e / h, 1.01 * np.sqrt(2 * e)) + 20 * EPS) + 4 * EPS * (np.abs(want["Y"]) + H)
        turn = W * 2 * math.pi / h_fov
        dx = (got["X"] - want["X"] + turn / 2) % turn - turn / 2
    dy = got["Y"] - want["Y"]
    with np.errstate(all="ignore"):
        return np.abs(dx) / tol_x, np.abs(dy) / tol_y, both


@pytest.mark.parametrize("interval", bc.INTERVALS)
@pytest.mark.parametrize("motion", bc.MOTIONS)
@pytest.mark.parametrize("turned", [False, True], ids=["straight", "turned"])
@pytest.mark.parametrize("name", ["pinhole", "lens", "sphere", "partial"])
def test_the_c_oracle_puts_every_record_where_the_float64_model_does(lib, events_lib, name, turned, motion, interval):
    W, H = 128, 72
    scene, objects, records, camera = _frame(events_lib, "cubes", motion, interval, name, turned, W, H)
    bs, groups, _ = bc.crafted(records, objects, camera, W, H, interval)
    bs = bs[np.r_[groups["surface"], groups["near"], groups["far"], groups["on pixels"], groups["edges and corners"], groups["lattice"], groups["pile"]][:1200]]
    got = bc.oracle_place(lib, bc.view(camera, W, H, interval, 3), objects, bs)
    want = ballistics.project(bs, objects, camera, W, H, interval, 3)
    assert np.array_equal(got["a"] > 0, want["a"] > 0) or interval == 0
    A = np.linalg.norm(_objects_array(objects)["InvLorentz"].astype(np.float64), ord=2, axis=(1, 2))[bs["object"]]
    gamma = np.sqrt(1.0 + (bs["u"].astype(np.float64) ** 2).sum(axis=1))
    e = gamma * A * A * EPS
    rx, ry, both = _position_ratios(got, want, camera, W, H, K_N * e)
    assert both.sum() >= 100, both.sum()
    measured = _position_ratios(got, want, camera, W, H, e)
    rel_dist = np.abs(got["dist"][both] / want["dist"][both] - 1.0) / e[both]
    line = f"{name} turned={turned} {motion} interval={interval}: {both.sum()} records, |dX| / bound(K_N = 1) {measured[0][both].max():.3f}, " \
           f"|dY| {measured[1][both].max():.3f}, |d dist| / (dist e) {rel_dist.max():.3f}"
    assert rx[both].max() <= 1.0 and ry[both].max() <= 1.0, line
    assert rel_dist.max() <= K_DIST, line
    if interval == -1:
        rel_D = np.abs(got["D"][both] / want["D"][both] - 1.0) / e[both]
        line += f", |d D| / (D e) {rel_D.max():.3f}"
        assert rel_D.max() <= K_D, line
        assert (want["a"][both] > 0).any() and (want["a"][both] <= 0).any()
    print(line)
    # the colours: rule 6 in float32 against float64, every Doppler setting, with and without the inverse square
    for flags in bc.FLAGS:
        for inverse_square in (False, True):
            g = bc.oracle_place(lib, bc.view(camera, W, H, interval, flags, inverse_square=inverse_square), objects, bs)
            w = ballistics.project(bs, objects, camera, W, H, interval, flags, dict(inverse_square=inverse_square))
            ok = g["visible"] & w["visible"]
            amp = np.maximum(1.0, w["D"][ok] ** 2) / (w["r"][ok] ** 2 if inverse_square else 1.0)
            scale = (bs["rgb"][ok].astype(np.float64).max(axis=1) * amp)[:, None]
            # the spectrum's slope is at most 4.6 per unit of nu (tests/test_particles_model.py); D's error is K_D e
            assert np.max(np.abs(g["rgb"][ok] - w["rgb"][ok]) / scale) <= max(1e-4, 10.0 * K_D * e[ok].max()), (flags, inverse_square)


def _approach_set():
    """Records that come at the camera, head on and obliquely, u from 0.1 to 300, seen at distances 1 to 1000."""
    rng = np.random.default_rng(24)
    n = 600
    u = 10.0 ** rng.uniform(-1.0, math.log10(300.0), n)
    where = rng.normal(size=(n, 3))
    where[:, 2] = np.abs(where[:, 2]) + 0.2
    where = where / np.linalg.norm(where, axis=1, keepdims=True) * (10.0 ** rng.uniform(0.0, 3.0, n))[:, None]
    heading = -where / np.linalg.norm(where, axis=1, keepdims=True) + rng.normal(scale=0.2, size=(n, 3)) * (np.arange(n) % 2)[:, None]
    heading /= np.linalg.norm(heading, axis=1, keepdims=True)
    return ballistics.from_arrays(where, 0, (1.0, 0.8, 0.6), u=u[:, None] * heading)


def test_the_approach_case(lib):
    """a <= 0: tau = g (a - r') adds two terms of one sign, so D's error grows with gamma only because dist and r' each carry gamma eps."""
    bs = _approach_set()
    obj, camera = identity_frame(), dict(mode="equirect")
    got = bc.oracle_place(lib, bc.view(camera, 128, 72, -1, 3), obj, bs)
    want = ballistics.project(bs, obj, camera, 128, 72, -1, 3)
    assert want["visible"].all() and got["visible"].all() and (want["a"] < 0).all() and (got["a"] < 0).all()
    gamma = np.sqrt(1.0 + (bs["u"].astype(np.float64) ** 2).sum(axis=1))
    assert gamma.max() > 250 and want["D"].max() > 400
    rel = np.abs(got["D"] / want["D"] - 1.0) / (gamma * EPS)
    print(f"approach: largest |d D| / (D gamma eps) {rel.max():.3f} at gamma {gamma[rel.argmax()]:.1f}; |d dist| / (dist gamma eps) "
          f"{(np.abs(got['dist'] / want['dist'] - 1.0) / (gamma * EPS)).max():.3f}")
    assert rel.max() <= K_APPROACH
    assert (np.abs(got["dist"] / want["dist"] - 1.0) / (gamma * EPS)).max() <= K_DIST


# ---- u = 0 is the particle pass ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interval", bc.INTERVALS)
@pytest.mark.parametrize("motion", bc.MOTIONS)
@pytest.mark.parametrize("scene_name", bc.SCENES)
def test_at_rest_and_always_shining_the_pass_is_the_particle_pass(lib, particles_lib, events_lib, scene_name, motion, interval):
    W, H = 128, 72
    pixels = np.zeros(W * H, dtype=[("x", "<f4"), ("y", "<f4"), ("rgba", "u1", (4,)), ("unspecified", "<u4")])
    pixels["rgba"] = (40, 50, 60, 1)
    for name in ("pinhole", "sphere"):
        scene, objects, records, camera = _frame(events_lib, scene_name, motion, interval, name, False, W, H)
        ps, _, bias = pc.crafted(records, objects, camera, W, H, interval)
        ps = bc.without_negative_zero(ps)
        bs = bc.from_particles(ps)
        assert not bs["u"].any() and np.isneginf(bs["t0"]).all() and np.isposinf(bs["t1"]).all()
        for flags in bc.FLAGS:
            for inverse_square in (False, True):
                v = bc.view(camera, W, H, interval, flags, inverse_square=inverse_square, depth_bias=bias if inverse_square else 0.0)
                want, want_counts = pc.oracle_pass(particles_lib, v, objects, ps, pixels, records)
                got, got_counts = bc.oracle_pass(lib, v, objects, bs, pixels, records)
                assert want_counts[0] > 0 and (want_counts[1] > 0 or flags & 1 or inverse_square)      # (a shift or 1 / r^2 may leave every byte as it was)
                assert got.tobytes() == want.tobytes() and got_counts == want_counts, (scene_name, motion, interval, name, flags, inverse_square)
        a, b = pc.oracle_place(particles_lib, bc.view(camera, W, H, interval, 3), objects, ps), bc.oracle_place(lib, bc.view(camera, W, H, interval, 3), objects, bs)
        for key in ("visible", "X", "Y", "dist", "D", "te", "r", "rgb"):
            assert a[key].tobytes() == b[key].tobytes(), key


# ---- covariance: the particle model is the reference -----------------------------------------------------------------------------
def _boost(v):
    """The boost into the frame that moves at v (units of c), rows and columns t, x, y, z, float64."""
    v = np.asarray(v, dtype=np.float64)
    b2 = float(v @ v)
    L = np.eye(4)
    if b2 == 0.0:
        return L
    g = 1.0 / math.sqrt(1.0 - b2)
    L[0, 0] = g
    L[0, 1:] = L[1:, 0] = -g * v
    L[1:, 1:] += (g - 1.0) * np.outer(v, v) / b2
    return L


FRAMES64 = np.dtype([("InvLorentz", "<f8", (16,)), ("stationaryCam", "<f8", (4,))])


@pytest.mark.parametrize("camera", [dict(mode="pinhole"), dict(mode="equirect")], ids=["pinhole", "panorama"])
@pytest.mark.parametrize("camera_v", [(0.0, 0.0, 0.0), (0.0, 0.0, 0.9)], ids=["rest", "0.9c"])
def test_a_worldline_written_in_another_frame_is_seen_the_same(monkeypatch, camera_v, camera):
    W, H = 128, 72
    vB = np.float32([0.4, 0.4, -0.565685]).astype(np.float64)        # 0.8 c, obliquely
    text = "Os p0,0,8,0,0,1,0,1,1,1 c0.5,0.5,0.5\nOs p2,1,9,0,0,1,0,1,1,1 c0.5,0.5,0.5 v0.4,0.4,-0.565685\nR\n"
    scene = eo.scene_from_text(text, v=camera_v, t=2.0)
    o32 = scene.objects()
    assert abs(np.linalg.norm(vB) - 0.8) < 1e-6
    # the matrices as the scene forms them (object boost times the camera's inverse boost), rebuilt in float64 from the velocities: the
    # float32 ones are these to rounding, and are no inverses of one another beyond it
    vc = np.float32(camera_v).astype(np.float64)
    lor = [_boost((0.0, 0.0, 0.0)) @ _boost(-vc), _boost(vB) @ _boost(-vc)]
    inv = [_boost(vc) @ _boost((0.0, 0.0, 0.0)), _boost(vc) @ _boost(-vB)]
    for j in range(2):
        assert np.max(np.abs(lor[j] - o32["Lorentz"][j].astype(np.float64).reshape(4, 4))) < 2e-6
        assert np.max(np.abs(inv[j] - o32["InvLorentz"][j].astype(np.float64).reshape(4, 4))) < 2e-6
        assert np.max(np.abs(lor[j] @ inv[j] - np.eye(4))) < 1e-14
    cam_pos = inv[0] @ o32["stationaryCam"][0].astype(np.float64).reshape(4)       # the camera event in the camera's frame
    frames = np.zeros(2, dtype=FRAMES64)
    for j in range(2):
        frames["InvLorentz"][j] = inv[j].reshape(-1)
        frames["stationaryCam"][j] = lor[j] @ cam_pos
    # a lattice at rest in B, ahead of the camera event as B sees it
    grid = particles.lattice(1, (-2.0, -1.5, 4.0), (2.0, 1.5, 9.0), 4, (0.9, 0.6, 0.3))
    posB = grid["pos"].astype(np.float64) + frames["stationaryCam"][1][1:]
    monkeypatch.setattr(particles, "_objects_array", lambda objects: objects)
    for flags in (0, 3):
        for inverse_square in (False, True):
            options = dict(inverse_square=inverse_square)
            want = particles.project_columns(posB, np.ones(len(posB), dtype=np.int64), grid["rgb"].astype(np.float64), frames, camera, W, H, -1, flags, options)
            # two events of each worldline, B's times 0 and 1, taken into A's frame: there the line is pos + beta t
            toA = lor[0] @ inv[1]
            e0 = np.concatenate([np.zeros((len(posB), 1)), posB], axis=1) @ toA.T
            e1 = np.concatenate([np.ones((len(posB), 1)), posB], axis=1) @ toA.T
            beta = (e1[:, 1:] - e0[:, 1:]) / (e1[:, :1] - e0[:, :1])
            pos0 = e0[:, 1:] - beta * e0[:, :1]
            u = beta / np.sqrt(1.0 - (beta * beta).sum(axis=1))[:, None]
            n = len(posB)
            got = ballistics.project_columns(pos0, np.zeros(n, dtype=np.int64), grid["rgb"].astype(np.float64), u, np.full(n, -np.inf), np.full(n, np.inf),
                                             {"InvLorentz": frames["InvLorentz"], "stationaryCam": frames["stationaryCam"]}, camera, W, H, -1, flags, options)
            assert np.array_equal(got["visible"], want["visible"]) and want["visible"].sum() >= 16, int(want["visible"].sum())
            assert np.max(np.abs(np.linalg.norm(beta, axis=1) - 0.8)) < 1e-6
            ok = want["visible"]
            for key in ("X", "Y", "dist", "D", "r"):
                assert np.max(np.abs(got[key][ok] - want[key][ok]) / np.maximum(1.0, np.abs(want[key][ok]))) <= 1e-9, (key, flags, inverse_square)
            scale = np.maximum(np.abs(want["rgb"][ok]).max(axis=1, keepdims=True), 1e-300)
            assert np.max(np.abs(got["rgb"][ok] - want["rgb"][ok]) / scale) <= 1e-9, (flags, inverse_square)
            if flags:
                assert np.ptp(want["D"][ok]) > 0.05


# ---- closed forms on the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.1, 0.6, 0.95, 0.999])
def test_head_on_the_doppler_factor_is_the_longitudinal_one(beta):
    camera = dict(mode="equirect")
    coming = ballistics.from_arrays([(0.0, 0.0, 50.0)], 0, (1.0, 1.0, 1.0), beta=(0.0, 0.0, -beta))
    going = ballistics.from_arrays([(0.0, 0.0, 50.0)], 0, (1.0, 1.0, 1.0), beta=(0.0, 0.0, beta))
    a, b = (ballistics.project(s, identity_frame(3.0), camera, 64, 32, -1, 3) for s in (coming, going))
    u_error = 4e-7 * (1.0 + beta) / (1.0 - beta)        # u is a float32 number: d D / D = gamma^2 d beta / beta-ish, bounded generously
    assert abs(a["D"][0] / math.sqrt((1.0 + beta) / (1.0 - beta)) - 1.0) <= u_error and a["a"][0] < 0
    assert abs(b["D"][0] / math.sqrt((1.0 - beta) / (1.0 + beta)) - 1.0) <= u_error and b["a"][0] > 0
    assert abs(a["D"][0] * b["D"][0] - 1.0) <= 1e-12
    # the retarded position: the light left where the particle was, -tau ago
    for p in (a, b):
        assert abs(np.linalg.norm(p["pos_e"][0]) + p["tau"][0]) <= 1e-12 * abs(p["tau"][0])


def test_a_jet_blob_crosses_the_sky_faster_than_light():
    beta, theta, far = 0.95, math.radians(20.0), 1.0e6
    records = ballistics.jet(0, (0.0, 0.0, far), (math.sin(theta), 0.0, -math.cos(theta)), beta, [0.0], (1.0, 1.0, 1.0))
    camera = dict(mode="pinhole")
    frames = lambda t: {"InvLorentz": np.eye(4)[None], "stationaryCam": np.array([[t, 0.0, 0.0, 0.0]])}
    t = far + 0.5          # soon after the blob's first light: it has moved some ten units of the 10^6, the finite-distance term
    x = []
    for when in (t, t + 1.0):
        p = ballistics.project_columns(records["pos"].astype(np.float64), np.zeros(1, dtype=np.int64), np.ones((1, 3)), records["u"].astype(np.float64),
                                       records["t0"].astype(np.float64), records["t1"].astype(np.float64), frames(when), camera, 128, 72, -1)
        assert p["visible"][0]
        x.append(far * p["n"][0, 0] / p["n"][0, 2])
    speed = (x[1] - x[0]) / 1.0
    want = ballistics.apparent_velocity(float(np.linalg.norm(records["u"][0].astype(np.float64)) / math.sqrt(1.0 + float((records["u"][0].astype(np.float64) ** 2).sum()))), theta)
    assert abs(want - 3.0283) < 2e-3 and want > 1.0
    assert abs(speed / want - 1.0) <= 1e-4, (speed, want)
    assert speed > 1.0
    # before its light arrives the blob is not seen: its window opens when it leaves
    early = ballistics.project(records, identity_frame(far - 10.0), camera, 128, 72, -1)
    assert not early["visible"][0] and early["te"][0] < 0.0


def test_the_receding_branch_is_needed(lib):
    """u = 300 straight away from the camera: a > 0, and g (a - r') loses what -g w0.w0 / (a + r') keeps."""
    rng = np.random.default_rng(300)
    n = 200
    where = rng.normal(size=(n, 3))
    where[:, 2] = np.abs(where[:, 2]) + 0.2
    where = where / np.linalg.norm(where, axis=1, keepdims=True) * rng.uniform(2.0, 50.0, n)[:, None]
    bs = ballistics.from_arrays(where, 0, (1.0, 1.0, 1.0), u=300.0 * where / np.linalg.norm(where, axis=1, keepdims=True))
    obj, camera = identity_frame(), dict(mode="equirect")
    want = ballistics.project(bs, obj, camera, 128, 72, -1, 3)
    assert (want["a"] > 0).all() and want["visible"].all()
    # float64: the two forms are one root
    g = np.sqrt(1.0 + (bs["u"].astype(np.float64) ** 2).sum(axis=1))
    assert np.max(np.abs(g * (want["a"] - want["r"]) / want["tau"] - 1.0)) <= 1e-9
    # float32: the oracle stays within the table's bound
    got = bc.oracle_place(lib, bc.view(camera, 128, 72, -1, 3), obj, bs)
    e = g * EPS
    assert got["visible"].all() and (got["a"] > 0).all()
    assert np.max(np.abs(got["dist"] / want["dist"] - 1.0) / e) <= K_DIST
    assert np.max(np.abs(got["D"] / want["D"] - 1.0) / e) <= K_D
    # ... and the other form, in float32, does not: with identity frames dist = -tau
    naive = bc.oracle_naive_tau(lib, obj, bs).astype(np.float64)
    rel = np.abs(-naive / want["dist"] - 1.0) / e
    print(f"receding at u = 300: |d dist| / (dist gamma eps) {np.max(np.abs(got['dist'] / want['dist'] - 1.0) / e):.3f} with the branch, {np.median(rel):.0f} (median) without")
    assert np.median(rel) > K_DIST, "more than half of the records leave the bound"


# ---- the window ---------------------------------------------------------------------------------------------------------------------
def test_an_exploding_shell_lights_up_near_side_first(lib):
    centre, t_emit, beta = np.array([0.0, 0.0, 20.0]), 5.0, 0.5
    bs = ballistics.shell(0, centre, t_emit, beta, 600, (1.0, 0.9, 0.8))
    assert (bs["t0"] == np.float32(t_emit)).all() and np.isposinf(bs["t1"]).all()
    assert np.max(np.abs(bs["pos"].astype(np.float64) + (bs["u"] / np.sqrt(1.0 + (bs["u"].astype(np.float64) ** 2).sum(axis=1))[:, None]) * t_emit - centre)) < 1e-5
    camera = dict(mode="equirect")
    first = t_emit + 20.0           # the light of the explosion itself arrives

    def counts(records, times, t_on):
        seen = []
        for when in times:
            got = bc.oracle_place(lib, bc.view(camera, 128, 72, -1, 0), identity_frame(when), records)
            want = ballistics.project(records, identity_frame(when), camera, 128, 72, -1)
            differ = got["visible"] != want["visible"]      # (only on the window's edge, within float32's rounding of the times)
            assert differ.sum() <= 3 and (np.abs(want["te"][differ] - t_on) <= 8.0 * EPS * when).all()
            seen.append(int(want["visible"].sum()))
            if 0 < seen[-1] < len(records):      # the near side first: what shows was emitted after t_on, what is dark would have been before
                free = records.copy()
                free["t0"] = -np.inf
                along = ballistics.project(free, identity_frame(when), camera, 128, 72, -1)["te"]
                assert along[want["visible"]].min() >= t_on > along[~want["visible"]].max()
                towards = -(records["u"][:, 2])
                assert towards[want["visible"]].min() > towards[~want["visible"]].max()
        assert seen == sorted(seen), seen
        return seen

    # every worldline passes through the explosion: its light reaches the camera at `first`, and from then on all of the shell shows
    seen = counts(bs, (first - 0.5, first + 0.5, first + 2.0, first + 30.0, first + 200.0), t_emit)
    assert seen == [0, len(bs), len(bs), len(bs), len(bs)], seen
    # a shell that starts to shine when its radius is 5: the near pole's first light comes at t_on + 15, the far pole's at t_on + 25
    t_on = t_emit + 10.0
    glowing = bs.copy()
    glowing["t0"] = t_on
    seen = counts(glowing, (t_on + 14.0, t_on + 16.0, t_on + 18.0, t_on + 20.0, t_on + 22.0, t_on + 24.0, t_on + 26.0), t_on)
    assert seen[0] == 0 and all(0 < k < len(bs) for k in seen[1:-1]) and seen[-1] == len(bs) and len(set(seen)) == len(seen), seen
    # seen from the side it is prolate along the line of sight, and brighter on the near side
    late = ballistics.project(bs, identity_frame(first + 30.0), camera, 128, 72, -1, 2)
    shape = late["pos_e"] - centre
    assert np.ptp(shape[:, 2]) > 1.1 * np.ptp(shape[:, 0])
    assert late["rgb"][shape[:, 2] < 0].mean() > late["rgb"][shape[:, 2] > 0].mean()


def test_the_objects_own_window_is_not_applied(lib, particles_lib):
    """Lamps riding the three legs of tests/particles_cases.py's body: as particles two legs at least are windowed out, as ballistic
    records at rest in the same frames all of them show — the object is only the frame the worldline is written in."""
    W, H = 128, 72
    wl, scene, ps = pc.turnaround()
    camera, windows = pc.CAMERAS["pinhole"], scene.windows()
    objects = pc.scene_objects(scene, camera)
    v = bc.view(camera, W, H, -1, 0)
    held = pc.oracle_place(particles_lib, v, objects, ps, windows)
    free = pc.oracle_place(particles_lib, v, objects, ps)
    got = bc.oracle_place(lib, v, objects, bc.from_particles(bc.without_negative_zero(ps)))
    assert (free["visible"] & ~held["visible"]).any()
    assert np.array_equal(got["visible"], free["visible"]) and got["X"].tobytes() == free["X"].tobytes()


# ---- the front end ------------------------------------------------------------------------------------------------------------------
def test_from_arrays_jet_shell_save_and_load(tmp_path):
    one = ballistics.from_arrays([(1.0, 2.0, 3.0)], 2, (0.5, 0.25, 1.0), beta=(0.6, 0.0, 0.0), t0=1.0, t1=4.0, epoch=10.0)
    assert one["object"][0] == 2 and one["u"][0].tolist() == [0.75, 0.0, 0.0] and one["pos"][0].tolist() == [-5.0, 2.0, 3.0]
    assert one["t0"][0] == 1.0 and one["t1"][0] == 4.0
    same = ballistics.from_arrays([(1.0, 2.0, 3.0)], 2, (0.5, 0.25, 1.0), u=(0.75, 0.0, 0.0), epoch=10.0)
    assert same["pos"].tobytes() == one["pos"].tobytes() and np.isneginf(same["t0"][0]) and np.isposinf(same["t1"][0])
    still = ballistics.from_arrays(np.zeros((3, 3)), [0, 1, 2], (1.0, 1.0, 1.0))
    assert not still["u"].any() and still["object"].tolist() == [0, 1, 2]
    with pytest.raises(ValueError):
        ballistics.from_arrays([(0.0, 0.0, 0.0)], 0, (1.0, 1.0, 1.0), beta=(1.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        ballistics.from_arrays([(0.0, 0.0, 0.0)], 0, (1.0, 1.0, 1.0), beta=(0.1, 0.0, 0.0), u=(0.1, 0.0, 0.0))
    j = ballistics.jet(1, (0.0, 0.0, 5.0), (0.0, 0.0, -2.0), 0.8, [0.0, 1.0, 2.0], (1.0, 0.0, 0.0))
    assert len(j) == 3 and j["t0"].tolist() == [0.0, 1.0, 2.0] and np.allclose(j["pos"][:, 2], [5.0, 5.8, 6.6]) and (j["object"] == 1).all()
    s = ballistics.shell(0, (1.0, 1.0, 1.0), 0.0, 0.5, 1000, (1.0, 1.0, 1.0))
    b = s["u"].astype(np.float64) / np.sqrt(1.0 + (s["u"].astype(np.float64) ** 2).sum(axis=1))[:, None]
    assert np.allclose(np.linalg.norm(b, axis=1), 0.5, atol=1e-6) and np.abs(b.mean(axis=0)).max() < 2e-3      # evenly spread
    assert ballistics.apparent_velocity(0.95, math.radians(20.0)) == pytest.approx(3.02836, abs=1e-4)
    path = tmp_path / "set.bin"
    ballistics.save(path, j)
    assert path.stat().st_size == 48 * 3 and ballistics.load(path).tobytes() == j.tobytes()
    path.write_bytes(b"\0" * 49)
    with pytest.raises(ValueError):
        ballistics.load(path)
    with pytest.raises(ValueError):
        ballistics.project(j, identity_frame(), dict(mode="pinhole"), 64, 32, 2)


# ---- the non-vacuity of the GPU cases, on CPU event frames ------------------------------------------------------------------------
@pytest.mark.parametrize("size", bc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(bc.CAMERAS))
@pytest.mark.parametrize("motion", bc.MOTIONS)
@pytest.mark.parametrize("scene_name", bc.SCENES)
def test_the_shared_cases_show_something(lib, events_lib, scene_name, motion, name, size):
    W, H = size
    camera = bc.CAMERAS[name]
    pixels = np.zeros(W * H, dtype=[("x", "<f4"), ("y", "<f4"), ("rgba", "u1", (4,)), ("unspecified", "<u4")])
    pixels["rgba"] = (40, 50, 60, 1)
    for interval in bc.INTERVALS:
        what = f"{scene_name} {motion} {name} {W}x{H} interval {interval}"
        scene = eo.load_scene(scene_name, motion, interval)
        objects = pc.scene_objects(scene, camera)
        records = sc.cpu_events(events_lib, scene, W, H, camera).reshape(-1)
        bs, groups, bias = bc.crafted(records, objects, camera, W, H, interval)
        place, t0, tb = bc.check_shows_something(lib, records, objects, camera, W, H, interval, bs, groups, bias, what)
        for flags in bc.FLAGS:
            after, (seen, changed) = bc.oracle_pass(lib, bc.view(camera, W, H, interval, flags), objects, bs, pixels, records)
            assert 0 < seen < len(bs) and changed > 0, what
            assert seen == int((t0[:, 1] > 0).sum()), f"{what}: the oracle saw {seen} records, the taps in numpy {int((t0[:, 1] > 0).sum())}"
            assert (after["rgba"][:, 3] == 1).all() and np.array_equal(after["x"], pixels["x"]) and np.array_equal(after["unspecified"], pixels["unspecified"])
        biased, (seen_biased, _) = bc.oracle_pass(lib, bc.view(camera, W, H, interval, 0, depth_bias=bias), objects, bs, pixels, records)
        assert seen_biased == int((tb[:, 1] > 0).sum()) >= seen
