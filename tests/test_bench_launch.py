"""bench.py --gpus N launches N ranks however it is started (no GPU: the ranks run tests/helpers/cpu_rig.py, crt_amd's
renderer API over the oracle, with gloo).  The launch decision, the shard plan, the framebuffer reduce, the per-rank
timings and the statistical parity field are bench.py's own code; only the per-rank render is the rig's."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
LAUNCH_ENV = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID")
SMALL = ["--rig", "cpu_rig", "--scene", "cornell", "--width", "96", "--height", "54", "--spp", "16", "--bounces", "8",
         "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--host-build"]


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in LAUNCH_ENV}
    env.update(PYTHONPATH=os.pathsep.join([str(REPO / "tests" / "helpers"), env.get("PYTHONPATH", "")]),
               OMP_NUM_THREADS="2", **extra)
    return env


def _bench(args, env, timeout=300):
    return subprocess.run([sys.executable, str(REPO / "bench.py"), *args], capture_output=True, text=True,
                          timeout=timeout, env=env)


def test_gpus_2_without_a_launcher_starts_two_ranks():
    p = _bench(["--gpus", "2", "--dist-backend", "gloo", *SMALL], _env())
    assert p.returncode == 0, p.stderr[-3000:]
    assert "[launch]" in p.stderr and "torch.distributed.run" in p.stderr
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["n_gpus"] == 2 and out["config"]["dist_backend"] == "gloo"
    assert "rehearsal" in out and out["data"].startswith("rehearsal")
    assert len(out["render_ms_per_rank"]) == 2 and all(v > 0 for v in out["render_ms_per_rank"])
    assert len(out["reduce_ms_per_rank"]) == 2 and out["dist_timings"]["frames"] == 2
    par = out["parity"]
    assert par["kind"].startswith("statistical")
    # rank 0's 8 samples per pixel are the 1-GPU frame's first 8: expected RMS = sqrt(2) noise sqrt(1 - 1/2)
    assert "0.5000" in par["expected_rule"]
    assert all(0.8 <= v <= 1.25 for v in par["rms_over_expected"]) and par["pass"] is True
    assert out["cpu_baseline"] is None and "N=1 only" in out["cpu_baseline_note"]


def test_world_size_mismatch_exits_nonzero():
    p = _bench(["--gpus", "2", *SMALL], _env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                                              MASTER_PORT="29999"), timeout=60)
    assert p.returncode == 2 and "WORLD_SIZE=1" in p.stderr
    assert not p.stdout.strip()


def test_one_gpu_without_a_launcher_stays_in_process():
    p = _bench(SMALL + ["--no-parity"], _env())
    assert p.returncode == 0, p.stderr[-3000:]
    assert "[launch]" not in p.stderr
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["n_gpus"] == 1 and out["config"]["dist_backend"] is None and "render_ms_per_rank" not in out


def test_plain_run_times_the_steps_and_dumps_the_same_outputs_every_time(tmp_path):
    """Without --full the line holds the headline figures and nothing that takes runs of its own; --steps sets the
    number of timed frames; --dump-outputs writes the last timed frame (float32) and two runs write the same arrays."""
    import numpy as np
    plain = [a for a in SMALL if a != "--full"]
    plain[plain.index("--steps") + 1] = "3"
    dumps = []
    for k in range(2):
        p = _bench(plain + ["--dump-outputs", str(tmp_path / f"d{k}")], _env())
        assert p.returncode == 0, p.stderr[-3000:]
        out = json.loads(p.stdout.strip().splitlines()[-1])
        assert out["steps"] == 3 and p.stderr.count("[warmup ") == 1 and "[timed] 3 frames" in p.stderr
        assert out["full"] is False and out["unit"] == "Mrays/s" and out["higher_is_better"] is True
        assert out["ms_per_step"] > 0 and out["value"] > 0 and out["dtype"] == "f32"
        # value = rays per frame over the time of one step (the line rounds it to 2 decimals, ms_per_step to 3)
        assert out["value"] == pytest.approx(out["rays_per_frame"] / out["ms_per_step"] / 1e3, rel=1e-3, abs=0.006)
        for moved in ("roofline", "algorithmic", "cpu_baseline", "parity", "end_to_end", "end_to_end_s"):
            assert out[moved] is None, moved
        assert "[e2e]" not in p.stderr and "[parity]" not in p.stderr and "[cpu]" not in p.stderr
        dumps.append({f.name: np.load(f) for f in sorted((tmp_path / f"d{k}").iterdir())})
    assert sorted(dumps[0]) == ["linear.npy", "rgba8.npy"]
    assert dumps[0]["linear.npy"].shape == (54, 96, 3) and dumps[0]["rgba8.npy"].shape == (54, 96, 4)
    for name, a in dumps[0].items():
        assert a.dtype == np.float32 and np.array_equal(a, dumps[1][name])
    assert dumps[0]["linear.npy"].max() > 0 and dumps[0]["rgba8.npy"][..., 3].min() == 255


def test_dump_outputs_samples_what_exceeds_the_budget(tmp_path):
    import numpy as np
    sys.path.insert(0, str(REPO))
    import bench
    rng = np.random.default_rng(1)
    lin = rng.random((30, 50, 3), dtype=np.float32)
    rgba = rng.integers(0, 256, (30, 50, 4), dtype=np.uint8)
    budget = 25000      # the 18,000 bytes of sums fit whole; 7,000 are left for the 24,000-byte float32 RGBA frame
    for k in range(2):
        bench.dump_outputs(tmp_path / f"s{k}", [("linear", lin), ("rgba8", rgba)], budget=budget)
    a, b = np.load(tmp_path / "s0" / "linear.npy"), np.load(tmp_path / "s0" / "rgba8.npy")
    assert np.array_equal(a, lin) and b.dtype == np.float32 and b.shape == (437, 4)
    assert a.nbytes + b.nbytes <= budget
    assert np.array_equal(b, np.load(tmp_path / "s1" / "rgba8.npy"))
    # every sampled row is a pixel of the frame, taken in ascending pixel order without repeats
    idx = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(1500, size=437, replace=False))
    assert np.array_equal(b, rgba.reshape(-1, 4)[idx].astype(np.float32))
    bench.dump_outputs(tmp_path / "s2", [("linear", lin), ("rgba8", rgba)])
    assert np.load(tmp_path / "s2" / "rgba8.npy").shape == rgba.shape


def test_generated_assets_go_to_a_cache_folder_when_the_tree_is_read_only(tmp_path, monkeypatch):
    """A benchmark user who may not write assets/generated/ gets the same scene files from a cache folder."""
    sys.path.insert(0, str(REPO))
    import bench
    from crt_amd import assets
    want = [Path(f).read_bytes() for f in assets.scene_files("cornell_bunny")]
    real = assets.bunny_proxy

    def read_only_tree(out_dir=assets.GEN_DIR, *a, **kw):
        if Path(out_dir) == assets.GEN_DIR:
            raise PermissionError(13, "Permission denied", str(out_dir))
        return real(out_dir, *a, **kw)

    monkeypatch.setattr(assets, "bunny_proxy", read_only_tree)
    monkeypatch.setenv("XDG_CACHE_HOME", str(tmp_path / "cache"))
    files = bench.scene_files("cornell_bunny")
    assert assets.bunny_proxy is read_only_tree                         # the module is left as it was
    assert files[0] == str(assets.CORNELL_OBJ) and Path(files[1]).is_relative_to(tmp_path / "cache")
    assert [Path(f).read_bytes() for f in files] == want
    assert (Path(files[1]).parent / "bunny.mtl").read_text() == assets.BUNNY_MTL
    assert bench.scene_files("cornell") == [str(assets.CORNELL_OBJ)]


def test_steps_below_one_are_rejected():
    p = _bench(["--print-workload-key", "--steps", "0"], _env(), timeout=60)
    assert p.returncode == 2 and "--steps" in p.stderr


def test_share_workload_key_and_flag_checks():
    p = _bench(["--print-workload-key", "--share", "0", "8"], _env(), timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "cornell_bunny_2560x1440_250spp_20b_rebuilt4"
    p = _bench(["--print-workload-key", "--share", "3", "3"], _env(), timeout=60)
    assert p.returncode == 2
    p = _bench(["--print-workload-key", "--share", "0", "2", "--gpus", "2"], _env(), timeout=60)
    assert p.returncode == 2
