"""bench.py's command line: `python bench.py --gpus N` works BARE (it starts its own ranks through torch.distributed.run
before touching a device and relays rank 0's line), the N > 1 plumbing — rendezvous on 127.0.0.1, barriers, max over
ranks, one JSON line — is exercised without a device by --dry-run, and without a GPU the real run fails loudly."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data", "config"}


def run_bench(*args, env=None, timeout=600):
    clean = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, cwd=ROOT,
                          env={**clean, **(env or {})}, timeout=timeout)


@pytest.mark.parametrize("n", [2, 3])
def test_bare_gpus_n_launches_its_own_ranks(n):
    p = run_bench("--gpus", str(n), "--steps", "4", "--warmup", "1", "--dry-run", "--full")
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout                      # rank 0 alone prints, once
    out = json.loads(lines[0])
    assert CONTRACT_KEYS <= set(out)
    assert out["n_gpus"] == n and out["steps"] == 4 and out["warmup"] == 1 and out["dry_run"] is True
    assert out["comm"]["ranks_in_group"] == n and out["comm"]["world_size"] == n
    assert "7680x4320" in out["comm"]["config5"]["workload"]          # the N > 1 --full line carries config 5 (timed in a real run)
    assert out["config"]["workload"].startswith("Scenes/bunny.txt 3840x2160") and "model" not in out["config"]


def test_dry_run_accepts_config_5():
    p = run_bench("--gpus", "2", "--dry-run", "--width", "7680", "--height", "4320")
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert "7680x4320" in out["config"]["workload"]


def test_plain_dry_run_leaves_config_5_to_full():
    """A plain run does only what the headline needs: config 5 is timed (and announced) only with --full."""
    p = run_bench("--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run")
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert CONTRACT_KEYS <= set(out) and out["steps"] == 3 and out["comm"]["config5"] is None


def test_steps_must_be_positive():
    p = run_bench("--gpus", "1", "--steps", "0", "--dry-run")
    assert p.returncode != 0 and "--steps" in p.stderr


def test_real_run_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    for n in ("1", "2"):
        p = run_bench("--gpus", n, "--steps", "2", "--warmup", "1", "--no-cpu-baseline")
        assert p.returncode != 0
        assert "needs a GPU" in (p.stderr + p.stdout)
        assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]      # no line, no silent CPU fallback


@pytest.mark.gpu
def test_bare_single_gpu_line():
    """The driver's own N = 1 command form on the GPU box: one line, the contract's keys, roofline + regimes."""
    p = run_bench("--gpus", "1", "--steps", "10", "--warmup", "2", "--full", "--no-cpu-baseline", "--workload", "shadows", "--width", "1280", "--height", "720",
                  "--check")
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert CONTRACT_KEYS <= set(out) and out["n_gpus"] == 1
    assert out["check"] == "framebuffer rows identical to the oracle"
    r = out["roofline"]
    assert r["bound"] == "hbm" and 0 < r["frac"] < 1 and 0 < r["frac_blocking"] < 1
    # roofline.frac is the dominant kernel's own fraction (a launch that has the device to itself); the device-level figure with
    # four launches overlapping is reported under a name that says so
    assert r["frac"] == r["frac_kernel_alone"] and r["launches_overlapped"] == 1.0 and "ballot_first" in r["kernel"]
    assert 0 < r["frac_device_4_in_flight"] < 1 and r["device_in_flight"]["launches_overlapped"] >= 1.0
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["launch_ms"] * 1e-3) / 1e9) < 0.02 * r["achieved"]
    assert out["ms_per_frame_blocking"] > 0 and out["frame_ms_blocking"]["median"] > 0 and out["launch_ms_in_flight"]["frames"] == 10
    assert "traffic" in r       # null unless a PMC summary of this very build is committed


@pytest.mark.gpu
def test_plain_line_times_exactly_the_steps_and_dumps_the_last_frame(tmp_path):
    """The plain form: --steps timed steps and nothing after them (no animated, one-at-a-time or CPU legs); --dump-outputs writes the
    last timed frame, which is the oracle's frame."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_ffi
    from conftest import load_config
    W, H, steps = 1280, 720, 7
    p = run_bench("--gpus", "1", "--steps", str(steps), "--warmup", "2", "--workload", "shadows", "--width", str(W), "--height", str(H),
                  "--dump-outputs", str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert CONTRACT_KEYS <= set(out) and out["steps"] == steps and out["launch_ms_in_flight"]["frames"] == steps
    assert out["ms_per_step"] > 0 and abs(out["value"] - W * H / out["ms_per_step"] / 1e3) < 0.02 * out["value"]
    assert out["animated"] is None and out["one_frame_at_a_time"] is None and "cpu_baseline" not in out
    assert out["roofline"]["frac_kernel_alone"] is None and out["roofline"]["traffic"] is None
    idx, xy = np.load(tmp_path / "pixel_index.npy"), np.load(tmp_path / "xy.npy")
    rgba, sums = np.load(tmp_path / "rgba.npy"), np.load(tmp_path / "rgba_row_sums.npy")
    assert (idx.dtype, xy.dtype, rgba.dtype, sums.dtype) == (np.float64, np.float32, np.float32, np.float64)
    assert np.array_equal(idx, np.arange(W * H))                      # a frame this small is dumped whole
    assert np.array_equal(xy[:, 0], idx % W) and np.array_equal(xy[:, 1], idx // W)
    assert np.array_equal(sums, rgba.reshape(H, W, 4).sum(axis=1))
    scene = load_config("shadows")
    for r0, r1 in ((0, 8), (H * 2 // 5, H * 2 // 5 + 16), (H - 8, H)):
        opx, _, _ = oracle_ffi.render(scene, W, H, rows=(r0, r1), want_rgb=False)
        assert np.array_equal(rgba.reshape(H, W, 4)[r0:r1], opx["rgba"].reshape(H, W, 4)[r0:r1].astype(np.float32)), (r0, r1)


# ---- figures quoted from committed counter summaries --------------------------------------------------------------

def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_counter_figures_are_quoted_only_for_the_build_they_were_taken_on(monkeypatch):
    """roofline.traffic / roofline.valu come from profiles/*_pmc_summary.json, per kernel, and only when the summary's recorded
    library hash is the running library's: a number from another build is stale and the line then says null."""
    import json
    bench = _load_bench()
    summary = json.load(open(os.path.join(ROOT, "profiles", "r04_bunny_3840x2160_pmc_summary.json")))
    recorded = summary["build"]["librpt_hip_sha256"]
    k43, k41 = "rpt_render_kernel_ballot_first_w5", "rpt_render_kernel_ballot_w5"

    monkeypatch.setattr(bench, "library_sha256", lambda: recorded)
    t43, src = bench.measured_traffic("bunny", 3840, 2160, k43)
    t41, _ = bench.measured_traffic("bunny", 3840, 2160, k41)
    assert src == os.path.join("profiles", "r04_bunny_3840x2160_pmc_summary.json")
    d43, d41 = summary["kernels"][k43]["derived"], summary["kernels"][k41]["derived"]
    assert t43 == int(sum(v for k, v in d43.items() if k.startswith("hbm_"))) and t41 == int(sum(v for k, v in d41.items() if k.startswith("hbm_")))
    assert t43 != t41                                              # one block per kernel, not a blend
    assert 3840 * 2160 * 16 <= t41 < 1.5 * 3840 * 2160 * 16         # the frame is written once and little else moves

    v = bench.measured_valu("bunny", 3840, 2160, k41, 0.1e-3)
    n = summary["kernels"][k41]["SQ_INSTS_VALU"]["mean"]
    assert v["wave_instructions_per_launch"] == int(n) and v["kernel"] == k41
    assert v["peak_wave_instructions_per_s"] == 256 * 4 * 2.4e9 / 2          # a wave64 instruction holds its SIMD-32 for two cycles
    assert abs(v["frac"] - n / (v["peak_wave_instructions_per_s"] * 0.1e-3)) < 1e-4
    assert 1.0 <= v["lanes_active_of_64"] <= 65.0
    assert bench.measured_valu("bunny", 3840, 2160, k41, None) is None
    assert bench.measured_traffic("bunny", 3840, 2160, "rpt_render_kernel_nonexistent") == (None, None)

    monkeypatch.setattr(bench, "library_sha256", lambda: "0" * 64)          # another build: nothing is quoted
    assert bench.measured_traffic("bunny", 3840, 2160, k43) == (None, None)
    assert bench.measured_valu("bunny", 3840, 2160, k43, 0.1e-3) is None
    monkeypatch.setattr(bench, "library_sha256", lambda: None)              # no library at all
    assert bench.measured_traffic("bunny", 3840, 2160, k43) == (None, None)


def test_dump_outputs_samples_a_large_frame_reproducibly(tmp_path):
    """dump_outputs() on a synthetic frame above DUMP_MAX_PIXELS (the branch a 3840x2160 run takes): a fixed, sorted, duplicate-free
    sample of pixels whose x / y / colour bytes are those of the frame, identical from call to call, row sums over EVERY pixel, and
    the 4K dump within 64 MB."""
    import numpy as np
    import torch
    bench = _load_bench()
    for W, H in ((1536, 768), (3840, 2160)):
        n = W * H
        assert n > bench.DUMP_MAX_PIXELS
        pix = np.zeros(n, dtype=[("x", "<f4"), ("y", "<f4"), ("rgba", "u1", (4,)), ("unspecified", "<u4")])
        pix["x"], pix["y"] = np.tile(np.arange(W), H), np.repeat(np.arange(H), W)
        pix["rgba"] = np.random.default_rng(W).integers(0, 256, (n, 4))
        fb = torch.from_numpy(pix.view(np.int32).copy())
        a, b = tmp_path / f"a{W}", tmp_path / f"b{W}"
        bench.dump_outputs(fb, W, H, str(a))
        bench.dump_outputs(fb, W, H, str(b))
        names = ("pixel_index.npy", "xy.npy", "rgba.npy", "rgba_row_sums.npy")
        for name in names:
            assert np.array_equal(np.load(a / name), np.load(b / name)), name
        idx, xy, rgba, sums = (np.load(a / name) for name in names)
        assert (idx.dtype, xy.dtype, rgba.dtype, sums.dtype) == (np.float64, np.float32, np.float32, np.float64)
        k = idx.astype(np.int64)
        assert len(k) == bench.DUMP_MAX_PIXELS and np.array_equal(k, idx) and (np.diff(k) > 0).all() and 0 <= k[0] and k[-1] < n
        assert np.array_equal(xy[:, 0], k % W) and np.array_equal(xy[:, 1], k // W)
        assert np.array_equal(rgba, pix["rgba"][k].astype(np.float32))
        assert sums.shape == (H, 4) and np.array_equal(sums, pix["rgba"].reshape(H, W, 4).sum(axis=1).astype(np.float64))
        assert sum(os.path.getsize(a / name) for name in names) <= 64 << 20
