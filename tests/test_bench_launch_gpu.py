"""bench.py's N > 1 launch path on a 1-GPU box: `python bench.py --gpus 2 ...` outside torchrun re-launches itself under
torch.distributed.run (relaunch_under_torchrun), two ranks run the data-parallel step - packed all-gather, index-then-fetch negatives, the gradient
reducer - and rank 0 prints ONE JSON line carrying `comm.per_rank_*`; rank 1 leaves through the rank != 0 exit path.  Both ranks sit on device 0
and the process group is gloo (MICO_BENCH_ONE_DEVICE / MICO_BENCH_BACKEND: a 1-GPU box cannot host two RCCL ranks) - everything of the launch
shape the driver's SCALE run uses (the reference's: data/scripts/run_vision_captioner.sh:1-12, one process per GPU) except RCCL itself."""
import json
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("backward", ["staged", "direct"])
def test_bench_two_ranks_on_one_device(cuda, backward):
    env = dict(os.environ, MICO_BENCH_ONE_DEVICE="1", MICO_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    # (the staged run keeps the extras rank 0 runs at N > 1 - the in-run parity measurement, alone, while rank 1 waits at the final barrier: its
    # alignment steps must stay out of the collectives, distributed.local_only)
    # (--full: the `comm` object and the in-run parity are not part of a plain run)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--layers", "2", "--batch", "4", "--steps", "2", "--warmup", "1",
           "--full", "--no-cpu-baseline"] + (["--direct-backward", "--no-extras"] if backward == "direct" else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines            # exactly one line on stdout, from rank 0
    d = json.loads(lines[0])
    assert len(lines[0]) < 8192              # the whole line fits a driver's tail
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["config"]["global_batch"] == 8 and d["config"]["parallelism"] == "dp2"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert all(math.isfinite(v) for v in d["losses"].values()) and set(d["losses"]) == {"loss_itc", "loss_itm", "loss_cap"}
    c = d["comm"]
    assert c["world_size"] == 2 and len(c["per_rank_samples_per_s"]) == 2 and len(c["per_rank_exposed_reduce_ms"]) == 2
    assert c["backend"].startswith("gloo") and c["rccl_ranks"] == 0
    assert d["roofline"] is not None and "step_frac" in d["roofline"]
    assert ("staged" in d["config"]["backward"]) == (backward == "staged")
    if backward == "staged":
        assert d["parity"]["worst"] < 1e-3 and d["parity"]["tensors"] >= 12, d["parity"]      # (depth-2 goldens; the full-depth one needs the full model)
        assert "secondary" not in d and "cpu_baseline" not in d                                 # N = 1 objects


def test_bench_plain_run_and_dumped_outputs(cuda, tmp_path):
    """A plain `bench.py --gpus 1` run is the headline alone - exactly --steps timed steps, the contract fields, none of the --full objects -
    and --dump-outputs writes the last timed step's losses and gradient sample; inputs and weights come from seeds, so a second run with the
    same arguments computes the same outputs (within the rounding of the kernels' summation order)."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    runs = []
    for i in range(2):
        out = tmp_path / f"run{i}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--layers", "2", "--batch", "4", "--steps", "3", "--warmup", "1",
               "--dump-outputs", str(out)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        d = json.loads(lines[0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["unit"] == "samples/s" and d["higher_is_better"] is True
        assert abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
        assert not {"parity", "parity_config", "secondary", "droppath_ab", "comm", "cpu_baseline"} & set(d), sorted(d)
        files = sorted(os.listdir(out))
        assert files == sorted(["loss_itc.npy", "loss_itm.npy", "loss_cap.npy", "grad_sample.npy", "grad_norm.npy"]), files
        assert sum(os.path.getsize(out / f) for f in files) < 64 * 2 ** 20
        arr = {f[:-4]: np.load(out / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arr.values())
        for k, v in d["losses"].items():
            assert float(arr[k]) == v, k
        assert (arr["grad_norm"] > 0).sum() > 0.5 * arr["grad_norm"].size       # the step's gradients were captured
        runs.append(arr)
    a, b = runs
    for k in ("loss_itc", "loss_itm", "loss_cap"):
        assert abs(float(a[k]) - float(b[k])) <= 1e-5 * abs(float(a[k])), k
    assert np.abs(a["grad_norm"] - b["grad_norm"]).max() <= 1e-3 * a["grad_norm"].max()
    assert np.abs(a["grad_sample"] - b["grad_sample"]).max() <= 1e-3 * np.abs(a["grad_sample"]).max()
