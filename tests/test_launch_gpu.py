"""bench.py --gpus N through its own launcher (utils/launch.py) on a one-GPU box: two ranks on
cuda:0 over gloo run the explanation headline, the row-sharded DRSA leg, the rank-local C4 chain
(extraction + sharded optimisation) and the task-parallel DRSA grid, and rank 0 reports n_gpus = 2
(VERDICT r02 'next' 1, r04 item 7)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_plain_run_headline_only_and_dumped_outputs(tmp_path):
    """A plain run prints the headline fields and none of the --full ones, and --dump-outputs
    writes what a caller of the timed path receives: the files equal this process's own
    HeatmapGenerator run on the same seeded model and batch, bit for bit."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from drsa_audio_amd.utils.constants import LRP_NAME_MAP_GTZAN
    from drsa_audio_amd.xai.explain.explainer import HeatmapGenerator
    cmd = [sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "6", "--steps", "3",
           "--warmup", "1", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1 and out["dtype"] == "fp32"
    assert out["unit"] == "explained samples/s" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(6 / (out["ms_per_step"] * 1e-3))
    assert not {"kernels", "roofline", "whole_path", "secondary", "cpu_baseline"} & set(out)
    dev = torch.device("cuda:0")
    hg = HeatmapGenerator(bench.gtzan128().to(dev), bench.load_u(), LRP_NAME_MAP_GTZAN, "blues", num_concepts=4,
                          layer_idx=7, device=dev, standard="sum")
    hg.generate_subspace_heatmaps(bench.synthetic_logmel(6, seed=1, device=dev), to_host=False)
    torch.cuda.synchronize(dev)
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == sorted(k + ".npy" for k in hg.info_device)
    for k, v in hg.info_device.items():
        a = np.load(tmp_path / "out" / (k + ".npy"))
        assert a.dtype == (np.float32 if v.is_floating_point() else np.float64)
        assert np.array_equal(a, v.cpu().numpy()), k


@pytest.mark.gpu
def test_bench_gpus2_own_launcher_one_device():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(DRSA_BENCH_ONE_DEVICE="1", DRSA_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--batch", "16", "--steps", "2",
           "--warmup", "1", "--full", "--no-cpu-baseline", "--legs", "sharded,pipeline,grid", "--grid-steps", "4",
           "--grid-classes", "2", "--pipeline-samples", "24", "--pipeline-steps", "30"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 32
    assert out["config"]["launch"].startswith("bench.py --gpus") and out["config"]["one_device_rehearsal"]
    assert len(out["rank_ms_per_step"]) == 2 and out["ms_per_step"] == pytest.approx(max(out["rank_ms_per_step"]))
    sec = out["secondary"]
    assert sec["drsa_sharded"]["vector_steps_per_s"] > 0
    # the N > 1 line checks itself against the unsharded run of every rank's rows
    assert sec["drsa_sharded"]["traj_dev_vs_unsharded"] < 1e-5
    assert sec["drsa_sharded"]["c5_joint"]["traj_dev_vs_unsharded"] < 1e-5
    # the rank-local C4 chain (drsa_training_data(group=) -> main_sharded(local_rows=True)) against
    # the single-process chain on the whole batch
    pl = sec["drsa_rank_local_pipeline"]
    assert pl["rows_total"] == 2 * 24 * 20 and pl["extraction_rows_per_s"] > 0 and pl["optimisation_steps_per_s"] > 0
    assert pl["traj_dev_vs_unsharded"] < 1e-5
    g = sec["drsa_grid_task_parallel"]
    assert g["problems"] == 18 and g["problems_per_rank"] == [9, 9] and g["scaling"] == "strong"
    lo, hi = g["objective_final_min_max"]
    assert 0 < lo <= hi
