"""bench.py contract guards: CLI refusals and options (no GPU), and the
plain / --full / --dump-outputs behaviour on a small corpus (GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def test_gpus_flag_refuses_single_rank_masquerade():
    """--gpus N with WORLD_SIZE unset and fewer visible GPUs must exit
    non-zero (never report n_gpus N for single-rank work)."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(
        [sys.executable, BENCH, "--gpus", "2",
         "--steps", "1", "--warmup", "0", "--rows", "1000"],
        capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert "refusing" in r.stderr


def test_cli_has_full_and_dump_outputs():
    r = subprocess.run([sys.executable, BENCH, "--help"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout


# small single-query scan: the kernels have their own parity suites; this
# checks the bench plumbing only
ROWS, STEPS, WARMUP, K = 20_000, 2, 1, 10


def _bench(outdir, *extra):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(
        [sys.executable, BENCH, "--gpus", "1", "--steps", str(STEPS),
         "--warmup", str(WARMUP), "--rows", str(ROWS),
         "--dump-outputs", str(outdir), *extra],
        capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-1000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines  # ONE JSON result line
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = tmp_path_factory.mktemp("bench")
    plain = _bench(root / "plain")
    full = _bench(root / "full", "--full")
    return root, plain, full


@pytest.mark.gpu
def test_plain_run_is_lean_and_full_adds_cpu_baseline(runs):
    _, plain, full = runs
    for line in (plain, full):
        assert line["metric"] == "knn_qps" and line["unit"] == "queries/s"
        assert line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["steps"] == STEPS and line["warmup"] == WARMUP
        assert line["ms_per_step"] > 0
        # value and ms_per_step are the same measurement (both rounded to
        # 3 decimals, hence the slack)
        assert line["value"] * line["ms_per_step"] == pytest.approx(
            1000.0, rel=1e-2)
        assert line["roofline"]["bound"] == "hbm"
    assert plain["cpu_baseline"] is None
    assert full["cpu_baseline"]["kind"] == "port"
    assert full["cpu_baseline"]["value"] > 0


@pytest.mark.gpu
def test_dump_outputs_match_oracle_and_repeat(runs):
    """The dump is what the last timed step returned: bit-exact against the
    oracle for that step's query, and identical between two runs."""
    import oracle
    root, _, _ = runs
    ids = np.load(root / "plain" / "ids.npy")
    dists = np.load(root / "plain" / "dists.npy")
    assert ids.dtype == np.float64 and dists.dtype == np.float64
    assert sorted(os.listdir(root / "plain")) == ["dists.npy", "ids.npy"]
    last = WARMUP + STEPS - 1  # query index of the last timed step
    q = oracle.gen_f32(0xBEEF, 0, last + 1, 768)[last]
    oids, odists = oracle.topk_f32(
        "cosine", oracle.gen_f32(0x5DB1, 0, ROWS, 768), q, K)
    assert np.array_equal(ids, oids.astype(np.float64)), (ids, oids)
    assert np.array_equal(dists, odists), (dists, odists)
    assert np.array_equal(ids, np.load(root / "full" / "ids.npy"))
    assert np.array_equal(dists, np.load(root / "full" / "dists.npy"))
