"""GPU: `bench.py --gpus N` with N real ranks on a box that has ONE GPU. The driver's scaling run (N = 2, 4, 8) cannot be
rehearsed here with one rank per device, so the test mode `--shared-gpu-gloo` puts the N ranks of the launch on cuda:0 and
reduces over gloo: the same launcher (torch.distributed.run on 127.0.0.1), the same barrier-bracketed regions, the REAL kernels on
the REAL strided shards — rank r decodes the trials r, r + N, ... of every Monte-Carlo round —, the native single-process driver
from rank 0 over N contexts while the other ranks wait at a host barrier, and the check the N-GPU line carries:
a 65536-trial prefix decoded by one GPU alone == the prefix sharded over the ranks == the prefix over the native driver's
contexts (PolarCode.cpp:696-775 sharded per BASELINE.json north_star). Rates of such a run mean nothing; counters do."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("world", [2, 3])
def test_n_ranks_on_one_gpu_give_the_single_gpu_counters(built_lib, world):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    total = 2 * 262144 * world
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--shared-gpu-gloo", "--steps", "1",
                        "--warmup", "1", "--batch", "4096", "--full", "--mc-trials", str(total)],
                       capture_output=True, text=True, timeout=900, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == world and line["shared_gpu_test"] is True
    assert line["bler"]["runs"] == world * 4096                     # every rank's headline shard reached the reduction
    mc = line["monte_carlo"]
    assert mc["n_gpus"] == world and mc["total_trials"] == total
    assert mc["multiprocess"]["rounds"] == 2 and mc["multiprocess"]["runs"] == [total] * 5
    assert mc["counters_equal_single_gpu_detail"] == {"multiprocess": True, "native_multi": True, "prefix_trials": 65536}
    assert mc["counters_equal_single_gpu"] is True
    nm = mc["native_multi"]
    assert "error" not in nm, nm
    assert nm["rounds"] == 2 and nm["equals_multiprocess_counters"] is True
    assert nm["block_errors"] == mc["multiprocess"]["block_errors"] and nm["block_errors"][0] > nm["block_errors"][-1] > 0


def test_the_result_line_is_the_last_line_on_stdout_with_rccl_initialised(built_lib):
    """With the RCCL process group up (every N > 1 run; forced here with one rank) RCCL writes a start-up banner through C stdio,
    which is flushed when the process exits — it used to land AFTER the JSON line, the one thing the driver reads. bench.py flushes
    the C buffers, prints the line and points stdout at stderr; ranks other than 0 never own stdout at all."""
    e = dict(os.environ, BENCH_FORCE_DIST="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--batch", "8192",
                        "--cpu-sample", "0", "--no-other-configs", "--mc-trials", "0"],
                       capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    line = json.loads(last)                                          # (fails when anything follows the line)
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["bler"]["runs"] == 8192
    assert sum(1 for l in r.stdout.splitlines() if l.startswith("{")) == 1


def test_a_native_leg_that_does_not_return_cannot_take_the_result_line_with_it(built_lib):
    """The single-process multi-GPU leg of the Monte-Carlo record runs in a thread of its own with a deadline (the library's watchdog
    covers the rounds, not a communicator set-up that never returns on some node): with the deadline set to (almost) nothing the
    launch still ends with rc 0 and ONE result line — headline, multi-process record and an error entry in place of the native one."""
    world = 2
    e = dict(os.environ, BENCH_NATIVE_DEADLINE_S="0.001")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--shared-gpu-gloo", "--steps", "1",
                        "--warmup", "1", "--batch", "4096", "--full", "--mc-trials", str(262144 * world)],
                       capture_output=True, text=True, timeout=900, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    mc = line["monte_carlo"]
    assert line["n_gpus"] == world and line["value"] > 0
    assert "deadline" in mc["native_multi"]["error"] and mc["native_multi_hung"] is True
    assert mc["counters_equal_single_gpu_detail"]["multiprocess"] is True and mc["multiprocess"]["rounds"] == 1


def test_a_plain_run_is_the_headline_alone_and_dumps_the_same_outputs_twice(built_lib, tmp_path):
    """`bench.py --steps K --warmup W` without --full: the headline record and nothing beside it, K timed steps, ms_per_step.
    --dump-outputs writes the last step's results as float .npy files, and two runs with the same arguments write the same."""
    import numpy as np
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "BENCH_FORCE_DIST"):
        e.pop(k, None)
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                            "--batch", "8192", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0 and line["bler"]["runs"] == 2 * 8192
        for k in ("monte_carlo", "cpu_baseline", "other_configs", "one_codeword_per_call", "host_batch", "p1_paths"):
            assert k not in line, k
        got = {f: np.load(d / f) for f in sorted(os.listdir(d))}
        assert set(got) == {"decoded_bits_sample.npy", "bit_errors_per_codeword.npy", "block_error_counters.npy"}
        assert all(a.dtype in (np.float32, np.float64) for a in got.values())
        assert sum(a.nbytes for a in got.values()) <= 64 << 20
        assert got["bit_errors_per_codeword.npy"].shape == (8192,)
        assert got["block_error_counters.npy"].tolist() == [line["bler"]["block_errors"], line["bler"]["runs"]]
        assert (got["block_error_counters.npy"][0] == 2 * (got["bit_errors_per_codeword.npy"] > 0).sum())
        dumps.append(got)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f
