"""CPU: bench.py's own launcher. `--gpus N` without a launcher around it must start N ranks itself (as a child
torch.distributed.run) or fail loudly — never report a single-GPU number under an N-GPU label. The rendezvous, the
relay of the JSON line and the band exchange are exercised over gloo with `--dry-run` (nothing rendered, value null)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(*argv, env=None, timeout=300):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GSR_FORCE_DIST"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH, *argv], capture_output=True, text=True, timeout=timeout, env=e)


def test_gpus_n_starts_n_ranks_and_relays_one_json_line():
    for n in (2, 3):
        p = _run("--gpus", str(n), "--dry-run", "--width", "200", "--height", "120")
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, p.stdout                       # exactly ONE line on stdout, the JSON
        rec = json.loads(lines[0])
        assert rec["n_gpus"] == n and rec["dry_run"] is True and rec["exchange_ok"] is True and rec["value"] is None
        assert rec["bands"][0][0] == 0 and rec["bands"][0][-1] == 8 and len(rec["bands"][0]) == n + 1
        assert rec["bands"][1] != rec["bands"][0]              # the re-cut moved a boundary towards the heavier rows


def test_gpus_n_with_fewer_devices_fails_loudly():
    p = _run("--gpus", "2")                                    # no HIP device in the CPU container
    assert p.returncode != 0 and p.stdout.strip() == ""
    assert "refusing to report" in p.stderr


def test_world_size_must_match_gpus():
    p = _run("--gpus", "2", env={"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0 and p.stdout.strip() == "" and "WORLD_SIZE=4" in p.stderr


def test_single_gpu_run_without_a_device_fails_loudly():
    p = _run("--gpus", "1", "--steps", "1")
    assert p.returncode != 0 and p.stdout.strip() == "" and "no CPU path" in p.stderr


def test_steps_below_one_are_refused():
    p = _run("--steps", "0")
    assert p.returncode != 0 and p.stdout.strip() == "" and "--steps" in p.stderr


def test_dumped_outputs_fit_the_limit_and_keep_their_positions():
    """bench.py --dump-outputs: arrays beyond their share of 64 MB are sampled at positions fixed by their size, so two
    builds run with the same arguments write comparable files; small arrays are written whole, in their shape."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(1)
    arrays = {"out_color": torch.rand((3, 1080, 1920), generator=g), "num_rendered": torch.tensor([7.0], dtype=torch.float64),
              "dL_dshs": torch.rand((1_000_000, 48), generator=g), "counts": torch.arange(10, dtype=torch.int64)}
    a, b = bench.sample_outputs(arrays), bench.sample_outputs({k: v.clone() for k, v in arrays.items()})
    assert sum(c.numel() * c.element_size() for c, _ in a.values()) <= bench.DUMP_BYTES
    assert a["num_rendered"][0].dtype == torch.float64 and a["counts"][0].dtype == torch.float64
    assert torch.equal(a["counts"][0], arrays["counts"].double()) and a["out_color"][0].dtype == torch.float32
    for k in arrays:
        assert torch.equal(a[k][0], b[k][0]), k
    c = a["dL_dshs"][0]
    assert 0 < c.numel() < arrays["dL_dshs"].numel() and bool(np.isin(c.numpy(), arrays["dL_dshs"].numpy()).all())
