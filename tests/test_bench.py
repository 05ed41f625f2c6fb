"""bench.py's multi-rank launcher on CPU: `--gpus N` (2 and 8) without a torch.distributed environment
starts the ranks itself (a child torch.distributed.run), the ranks exchange over gloo, and the one
relayed JSON line reports the world the driver asked for, with every replica bit-identical (VERDICT r03
item 5, r04 item 4).  Also the line's self-description: the CPU-share evidence and the committed
profile the traffic figure is read from."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


@pytest.mark.parametrize("gpus", [2, 8])
def test_bench_launches_its_own_ranks_gloo(gpus):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["MASTER_ADDR"] = "127.0.0.1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--backend", "gloo",
                          "--n-gaussians", "20000", "--steps", "2", "--warmup", "1", "--full"],
                         capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == gpus
    assert rec["config"]["parallelism"] == f"view-dp{gpus}"
    ex = rec["exchange"]
    assert ex["world"] == gpus and ex["collectives_per_step"] > 0
    assert ex["grad_bytes_per_rank"] == 20000 * 59 * 4 and ex["algbw_GBps"] > 0
    assert ex["replicas_bit_identical"] is True
    bx = rec["exchange_bf16"]
    assert bx["wire_bytes_per_rank"] * 2 == bx["grad_bytes_per_rank"] and bx["collectives_per_step"] > 0
    assert bx["replicas_bit_identical"] is True
    assert rec["value"] is None and rec["headline_value"] is None  # gloo: no timed step; the headline stays unmeasured


def _run_bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["MASTER_ADDR"] = "127.0.0.1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                         timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


HEADLINE_FIELDS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("exchange", "exchange_bf16", "exchange_and_step", "dp_step", "distCUDA2", "masked_adam",
             "binning_skewed", "config2_scale", "config5_scale")


def test_plain_run_measures_nothing_beside_its_step_gloo():
    """Without --full the exchange legs (all a gloo run has) are not run; the line keeps its headline fields."""
    rec = _run_bench("--gpus", "1", "--backend", "gloo", "--n-gaussians", "20000", "--steps", "2", "--warmup", "1")
    assert all(k in rec for k in HEADLINE_FIELDS)
    assert not [k for k in FULL_ONLY if k in rec] and rec["cpu_baseline"] is None and rec["roofline"] is None


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_its_outputs(tmp_path):
    """A plain one-GPU run: `steps` timed steps, ms_per_step in the line, nothing that --full adds, and
    --dump-outputs writes the last step's scan, sorted pairs and tile ranges, which are checked against
    the pairs' definition: keys non-decreasing and each tile's range holding exactly its keys."""
    import numpy as np
    rec = _run_bench("--gpus", "1", "--n-gaussians", "20000", "--steps", "3", "--warmup", "1",
                     "--dump-outputs", str(tmp_path / "a"))
    assert all(k in rec for k in HEADLINE_FIELDS) and rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["ms_per_step"] > 0 and rec["ms_per_step"] == rec["binning_step"]["ms_per_step"]
    assert rec["value"] == rec["binning_step"]["binning_steps_per_s_all_ranks"] and 0 < rec["value"] < float("inf")
    assert rec["headline_value"] is None and rec["unit"] == "iters/s" and rec["higher_is_better"] is True
    assert rec["binning_step"]["queue_error"] == 0 and "kernels" not in rec["binning_step"]
    assert not [k for k in FULL_ONLY if k in rec] and rec["cpu_baseline"] is None and rec["roofline"] is None
    out = {n: np.load(tmp_path / "a" / f"{n}.npy")
           for n in ("point_offsets", "sorted_keys", "sorted_values", "tile_ranges")}
    assert all(a.dtype == np.float64 for a in out.values())
    K, T = rec["config"]["pairs_K"], rec["config"]["tiles"]
    keys = out["sorted_keys"].astype(np.uint64)
    assert keys.shape == (K,) and out["sorted_values"].shape == (K,) and out["tile_ranges"].shape == (T, 2)
    assert out["point_offsets"].shape == (20000,) and out["point_offsets"][-1] == K
    assert np.all(np.diff(out["point_offsets"]) >= 0) and np.all(keys[1:] >= keys[:-1])
    assert out["sorted_values"].min() >= 0 and out["sorted_values"].max() < 20000
    tiles = (keys >> np.uint64(32)).astype(np.int64)
    counts = np.bincount(tiles, minlength=T)
    ends = np.cumsum(counts)
    filled = counts > 0
    assert np.array_equal(out["tile_ranges"][filled, 1], ends[filled])
    assert np.array_equal(out["tile_ranges"][filled, 0], (ends - counts)[filled])
    assert np.all(out["tile_ranges"][~filled] == 0)


def test_dump_outputs_samples_large_arrays_at_fixed_positions(tmp_path):
    import numpy as np
    import torch
    big = torch.arange(bench.DUMP_CAP + 12345, dtype=torch.int32)
    small = torch.tensor([[0, 3], [3, 7]], dtype=torch.int32)
    keys = torch.tensor([(5 << 32) | 0xFFFFFFFF, 1 << 44], dtype=torch.int64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small, "keys": keys}, np, torch)
    a = np.load(tmp_path / "a" / "big.npy")
    assert a.dtype == np.float64 and a.shape == (bench.DUMP_CAP,) and np.all(np.diff(a) > 0)  # values = positions
    assert np.array_equal(a, np.load(tmp_path / "b" / "big.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), [[0.0, 3.0], [3.0, 7.0]])
    assert np.array_equal(np.load(tmp_path / "a" / "keys.npy"), [float((5 << 32) | 0xFFFFFFFF), float(1 << 44)])
    assert 4 * bench.DUMP_CAP * 8 <= 64 * 2 ** 20  # four arrays at the cap stay within 64 MB


def test_cpu_share_reports_its_evidence():
    share = bench.cpu_share()
    assert share["cores"] >= 1 and share["sched_getaffinity"] >= share["cores"]
    assert share["cores_source"] and "cgroup_cpu_setting" in share and share["host_cpu_count"] == os.cpu_count()
    if share["cgroup_cpu_quota"] is not None:
        assert share["cores"] <= share["cgroup_cpu_quota"]


def test_traffic_profile_key_resolves():
    """The committed PMC summary holds the bench's dominant kernels at the bench's own grid (ADVICE r04:
    a scout-count change once left segment_sort's key unresolved), and it says where it was taken."""
    table = json.load(open(bench.TRAFFIC_FILE))
    K, T = 8586682, 8160  # the bench view (BENCH_r04)
    for dom in ("radix_scatter_u64", "segment_sort"):
        key, ent = bench.traffic_entry(dom, K, T, table)
        assert key == {"radix_scatter_u64": "radix_scatter_kernel@1073664",
                       "segment_sort": f"segment_sort_kernel@{(T + bench.SCOUTS) * 256}"}[dom]
        assert ent["hbm_bytes_per_launch"] > 0
    meta = json.load(open(bench.TRAFFIC_META))
    assert meta["commit"] and len(meta["sources_sha256"]) == 64
    src = open(os.path.join(ROOT, "hidegs_amd", "csrc", "primitives.hip")).read()
    assert f"#define HIDEGS_SCOUTS {bench.SCOUTS} " in src
