"""bench.py's options around the timed steps: --dump-outputs (what the last timed step returned, as
.npy files that two builds can be compared by) and --full (the measurements beside the headline)."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _stub_trainer(n_params):
    g = torch.Generator().manual_seed(3)
    B, T = 5, 7
    ro = types.SimpleNamespace(
        resp=torch.randint(0, 32000, (B, T), generator=g), resp_len=torch.randint(1, T + 1, (B,), generator=g),
        old_logp=torch.randn(B, T, generator=g), old_values=torch.randn(B, T, generator=g).bfloat16(),
        ref_logp=torch.randn(B, T, generator=g), scores=torch.rand(B, generator=g),
        adv=torch.randn(B, T, generator=g), returns=torch.randn(B, T, generator=g))
    flat = types.SimpleNamespace(data=torch.randn(n_params, generator=g))
    return types.SimpleNamespace(last_rollout=ro, flat=flat)


def test_dump_outputs_files(tmp_path):
    metrics = {k: float(i) + 0.25 for i, k in enumerate(bench.DUMP_METRICS)}
    metrics["step_time_s"] = 4.5  # durations are not outputs
    tr = _stub_trainer(bench.DUMP_PARAM_SAMPLE + 1000)
    d1, d2 = str(tmp_path / "a" / "deep"), str(tmp_path / "b")
    bench.dump_outputs(d1, tr, metrics)
    bench.dump_outputs(d2, tr, metrics)
    names = sorted(os.listdir(d1))
    assert names == sorted(n + ".npy" for n in ("metrics", "resp_tokens", "resp_len", "old_logp", "old_values",
                                                "ref_logp", "scores", "advantages", "returns", "params_sample"))
    total = 0
    for n in names:
        a, b = np.load(os.path.join(d1, n)), np.load(os.path.join(d2, n))
        assert a.dtype in (np.float32, np.float64), (n, a.dtype)
        assert np.array_equal(a, b), n  # the sample of a large output is fixed
        total += a.nbytes
    assert total <= 64 << 20
    ro = tr.last_rollout
    assert np.array_equal(np.load(os.path.join(d1, "resp_tokens.npy")), ro.resp.numpy().astype(np.float32))
    assert np.array_equal(np.load(os.path.join(d1, "old_values.npy")), ro.old_values.float().numpy())
    assert np.array_equal(np.load(os.path.join(d1, "metrics.npy")),
                          np.arange(len(bench.DUMP_METRICS), dtype=np.float64) + 0.25)
    ps = np.load(os.path.join(d1, "params_sample.npy"))
    assert ps.shape == (bench.DUMP_PARAM_SAMPLE,)
    assert np.isin(ps, tr.flat.data.numpy()).all()
    # a small trainable set is written whole
    small = _stub_trainer(100)
    bench.dump_outputs(d2, small, metrics)
    assert np.array_equal(np.load(os.path.join(d2, "params_sample.npy")), small.flat.data.numpy())


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True,
                          text=True, timeout=300)


def test_latency_only_modes_need_full():
    """The batch-1 latency measurements live behind --full: asking for them without it is an error
    at argument parsing (before any model is built), not a silently empty result."""
    for argv in (["--steps", "0"], ["--steps", "1", "--latency-contexts", "1024"]):
        r = _bench("--gpus", "1", *argv)
        assert r.returncode == 2 and "--full" in r.stderr, r.stderr[-500:]
    r = _bench("--gpus", "1", "--steps", "0", "--full", "--dump-outputs", "x")
    assert r.returncode == 2 and "--dump-outputs" in r.stderr
