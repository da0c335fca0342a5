"""bench.py's command line on the device: a plain run is the headline alone,
``--steps`` sets the timed steps, ``--dump-outputs`` writes the timed path's
output.  One short process, shared by the tests below."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("unramped", "flash_causal", "flash_wallclock_ms", "calibration", "flash_torch_sdpa", "flash_dtypes",
             "gemv", "decode_attn", "gemm", "tp_gemm", "decode_step", "ch05_matmul_demo", "cpu_baseline",
             "cpu_other")


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench_dump")
    env = dict(os.environ, PLI_BENCH_RAMP_MS="100")  # the ramp's length is not under test
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]  # exactly the one JSON line
    return json.loads(lines[0]), d


def test_plain_run_has_the_headline_only(plain_run):
    res, _ = plain_run
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in res
    assert res["steps"] == 3 and res["warmup"] == 2 and res["n_gpus"] == 1
    assert res["unit"] == "TFLOP/s" and res["dtype"] == "bf16" and res["higher_is_better"] is True
    assert res["roofline"]["route"] == "attn_fwd_v13"
    # value is the step's 2^41 FLOP over ms_per_step
    assert res["value"] == pytest.approx(2 ** 41 / (res["ms_per_step"] * 1e-3) / 1e12, rel=1e-9)
    assert 0.5 < res["ms_per_step"] < 50
    assert not [k for k in FULL_ONLY if k in res]


def test_dump_is_the_flash_output(plain_run):
    """The dumped rows equal the library's output on the same seeded inputs
    (bitwise: same kernel, same tensors), within the size limit, in fp32."""
    import torch

    import bench
    import pli_hip
    _, d = plain_run
    assert sorted(os.listdir(d)) == ["flash_out.npy"]
    a = np.load(os.path.join(d, "flash_out.npy"))
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_ROWS, bench.D) and a.nbytes <= 64 * 10 ** 6
    gen = torch.Generator(device="cuda").manual_seed(1234)
    q, k, v = (torch.randn(bench.B, bench.H, bench.S, bench.D, device="cuda", dtype=torch.bfloat16, generator=gen)
               for _ in range(3))
    o = pli_hip.flash_attn_fwd(q, k, v)
    idx = np.sort(np.random.RandomState(bench.DUMP_SEED).choice(bench.B * bench.H * bench.S, bench.DUMP_ROWS,
                                                                 replace=False))
    ref = o.reshape(-1, bench.D)[torch.from_numpy(idx).cuda()].float().cpu().numpy()
    np.testing.assert_array_equal(a, ref)
