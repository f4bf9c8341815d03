"""bench.py must never label a 1-GPU run as N GPUs (round-1 advisor finding): without WORLD_SIZE it starts the N ranks
itself, and when the ranks cannot get a GPU each the whole command fails instead of printing a line."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=300):
    env = dict(os.environ); env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, timeout=timeout)


def test_world_size_must_match_gpus():
    r = _run(["--gpus", "4", "--ne", "2", "--qsize", "1"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and b"WORLD_SIZE=2" in r.stdout and b'"n_gpus"' not in r.stdout


def test_gpus_2_without_launcher_starts_two_ranks_or_fails():
    """here (no GPU) the two self-launched ranks must refuse to run; the parent relays the failure"""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("two GPUs visible: the self-launched run would succeed")
    r = _run(["--gpus", "2", "--ne", "2", "--qsize", "1", "--steps", "3", "--warmup", "0", "--no-cpu-baseline"])
    assert r.returncode != 0, r.stdout[-2000:]
    assert b'"n_gpus"' not in r.stdout
    assert b"2 ranks but" in r.stdout      # message of the rank processes: they were really started as 2 ranks


def test_dump_sample_is_fixed_and_bounded():
    """--dump-outputs writes the same elements whatever build runs it, never more than 64 MB of them, and all of them when they fit"""
    import numpy as np
    import bench
    for ne, qsize in ((120, 35), (120, 200), (30, 35)):
        ids = bench.dump_elements(6 * ne * ne, qsize)
        assert np.array_equal(ids, bench.dump_elements(6 * ne * ne, qsize))
        assert np.all(np.diff(ids) > 0) and 0 <= ids[0] and ids[-1] < 6 * ne * ne
        assert ids.size * qsize * 72 * 16 * 8 <= 64 << 20
    assert np.array_equal(bench.dump_elements(6 * 8 * 8, 4), np.arange(6 * 8 * 8))
    # the ids themselves, so that another build or another numpy cannot pick other elements unnoticed
    ids = bench.dump_elements(6 * 120 * 120, 35)
    assert ids.size == 156 and list(ids[:3]) == [2246, 2331, 2608] and list(ids[-2:]) == [85819, 85826]
    ids = bench.dump_elements(6 * 120 * 120, 200)
    assert ids.size == 27 and list(ids[:3]) == [3101, 5072, 5842] and list(ids[-2:]) == [81473, 81953]


@pytest.mark.gpu
def test_dump_outputs_hold_the_final_state(tmp_path):
    """at ne8 the dump is the whole final Qdp: identical in two runs with the same arguments, and the time level the timed steps
    wrote last (its bit-pattern sum is the run's state_checksum)"""
    import json
    import numpy as np
    got = []
    for k in range(2):
        d = str(tmp_path / ("run%d" % k))
        r = _run(["--gpus", "1", "--ne", "8", "--qsize", "4", "--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--dump-outputs", d])
        assert r.returncode == 0, r.stdout[-2000:]
        line = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 4 and line["ms_per_step"] > 0
        q, ids = np.load(os.path.join(d, "qdp.npy")), np.load(os.path.join(d, "qdp_elements.npy"))
        assert q.dtype == np.float64 and q.shape == (384, 4, 72, 4, 4) and np.all(np.isfinite(q))
        assert np.array_equal(ids, np.arange(384))
        assert int(q.view(np.int64).sum()) & 0xFFFFFFFFFFFFFFFF == line["state_checksum"]
        got.append(q)
    assert np.array_equal(got[0], got[1])


@pytest.mark.gpu
def test_dump_rows_follow_their_element_ids_across_partitions(tmp_path):
    """the sampled dump (ne16, qsize 35: 156 of 1536 elements) of one rank against that of two ranks sharing the GPU over the
    host-staged exchange: the second rank's device rows are not its global element ids, and the result has the same bits for every
    partition, so a row put under the wrong element id, or gathered in the wrong order, shows up as a difference"""
    import json
    import numpy as np
    import bench
    got = []
    for gpus in (1, 2):
        d = str(tmp_path / ("gpus%d" % gpus))
        r = _run(["--gpus", str(gpus), "--ne", "16", "--qsize", "35", "--steps", "4", "--warmup", "2", "--no-cpu-baseline",
                  "--dump-outputs", d], {"TSE_EXCHANGE": "staged"})
        assert r.returncode == 0, r.stdout[-2000:]
        line = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1])
        assert line["n_gpus"] == gpus and line["steps"] == 4
        q, ids = np.load(os.path.join(d, "qdp.npy")), np.load(os.path.join(d, "qdp_elements.npy"))
        assert np.array_equal(ids, bench.dump_elements(1536, 35)) and q.shape == (156, 35, 72, 4, 4)
        got.append((q, line["state_checksum"]))
    assert got[0][1] == got[1][1]
    assert np.array_equal(got[0][0], got[1][0])
