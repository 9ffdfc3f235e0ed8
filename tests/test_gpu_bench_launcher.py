"""bench.py through its own spawn path on the GPU box: `--gpus 1 --via-launcher` starts the same fresh
`python -m torch.distributed.run` child a `--gpus N` run starts (this pytest process stays the grandparent and the bench
parent never touches the GPU); the rank initialises RCCL, proves its communicator and prints the line the parent relays."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SMALL = ["--taxa", "224", "--trees", "6000", "--steps", "40", "--warmup", "5", "--full", "--no-cpu-baseline", "--no-e2e", "--no-score"]


def run_bench(extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    last = p.stdout.strip().splitlines()[-1]
    assert last.startswith('{"metric"'), p.stdout[-500:]
    return json.loads(last)


def test_via_launcher_reproduces_the_single_gpu_line():
    plain = run_bench(["--gpus", "1"] + SMALL)
    spawned = run_bench(["--gpus", "1", "--via-launcher"] + SMALL)
    assert "collective" not in plain and "launcher" not in plain["config"]
    col = spawned["collective"]
    assert col["ranks"] == 1 and col["proof"] == 1 and col["proof_ok"] is True and col["backend"] == "nccl"
    assert col["comm_init_ms"] > 0 and col["table_collective"] is None          # one rank: no peer to combine a table with
    assert spawned["config"]["launcher"]["ranks"] == 1
    for doc in (plain, spawned):
        assert doc["n_gpus"] == 1 and doc["steps"] == 40 and doc["config"]["parity_tuple_sums_ok"] is True
        assert doc["config"]["parity_lookup_equals_bruteforce"] is True
        assert doc["config"]["kernel_ms_source"]       # (steps below 5 ms: the mean over extra bracketed steps; else the last timed step)
    # same workload, same kernels: the two lines agree. Steps of a few ms vary by several per cent from run to run on a shared
    # box (this asserts the path, with a loose bound); configs[2] through both paths agrees within 1 %: profiles/r04_launcher/
    assert abs(spawned["ms_per_step"] / plain["ms_per_step"] - 1.0) < 0.15, (plain["ms_per_step"], spawned["ms_per_step"])


def test_config4_through_the_launcher_takes_the_table_sharded_path():
    doc = run_bench(["--gpus", "1", "--via-launcher", "--config", "4", "--taxa", "200", "--trees", "400", "--steps", "5", "--warmup", "1",
                     "--no-cpu-baseline", "--no-e2e"])
    assert doc["config"]["table_shard"] is not None and doc["config"]["collective"] is None
    assert doc["collective"]["ranks"] == 1 and doc["dtype"] == "u16"


def test_forced_collective_line_carries_its_own_scaling_figures_and_the_p2p_leg():
    """The N > 1 code path on one GPU (QS_BENCH_FORCE_DIST=1: RCCL initialised, the table collective inside every step): the line
    times the same share WITHOUT the collective in the same run (config.one_rank_same_workload: count-only ms, scaling efficiency,
    exposed collective time) and, with --p2p-leg 1, the C++ host's peer-access reduction on the same trees in a child process."""
    os.environ["QS_BENCH_FORCE_DIST"] = "1"
    try:
        doc = run_bench(["--gpus", "1", "--config", "3", "--taxa", "160", "--trees", "6000", "--steps", "10", "--warmup", "2", "--p2p-leg", "1",
                         "--full", "--no-cpu-baseline", "--no-e2e", "--no-score"])
    finally:
        del os.environ["QS_BENCH_FORCE_DIST"]
    cfg = doc["config"]
    assert doc["scaling"] == "n/a" and cfg["baseline_config"].startswith("custom") and cfg["collective"] == "scatter"
    same = cfg["one_rank_same_workload"]
    assert same["count_only_ms_per_step"] > 0 and 0.3 < same["scaling_efficiency"] < 1.2, same
    assert abs(same["collective_exposed_ms"] - (doc["ms_per_step"] - same["count_only_ms_per_step"])) < 1e-2
    leg = cfg["p2p_leg"]
    assert leg.get("counting_phase_ms", 0) > 0 and leg["counting_quartets_per_s"] > 0 and "table_reduction_ms" in leg, leg
    assert cfg["parity_reduced_tuple_sums_ok"] is True
    plain = run_bench(["--gpus", "1"] + SMALL)
    assert plain["scaling"] == "n/a" and plain["config"]["one_rank_same_workload"] is None and "p2p_leg" not in plain["config"]
    assert plain["config"]["baseline_config"].startswith("custom")


def test_table_mode_through_the_launcher_and_the_other_mode_leg():
    """`--gpus 1 --via-launcher --mode table` (the N > 1 default for configs[2], here with one rank = one shard = the whole table):
    no table collective in the step, the line says which mode ran and why, and -- with the N > 1 path forced -- it carries the
    OTHER mode (tree-sharded + RCCL reduce-scatter) as a leg measured on the same trees in the same run."""
    os.environ["QS_BENCH_FORCE_DIST"] = "1"
    try:
        doc = run_bench(["--gpus", "1", "--via-launcher", "--mode", "table"] + SMALL)
        tree = run_bench(["--gpus", "1", "--mode", "tree", "--taxa", "160", "--trees", "6000", "--steps", "10", "--warmup", "2",
                          "--full", "--no-cpu-baseline", "--no-e2e", "--no-score"])
    finally:
        del os.environ["QS_BENCH_FORCE_DIST"]
    cfg = doc["config"]
    assert cfg["mode"] == "table" and cfg["mode_decided_by"] == "--mode table" and cfg["collective"] is None
    assert cfg["parity_tuple_sums_ok"] is True and doc["collective"]["table_collective"] is None
    leg = cfg["other_mode_leg"]
    assert leg["mode"] == "tree" and leg["collective"] == "scatter" and leg["parity_tuple_sums_ok"] is True, leg
    assert leg["ms_per_step"] > 0 and 0.5 < leg["value"] / doc["value"] < 2.0, (leg["value"], doc["value"])
    cfg = tree["config"]
    assert cfg["mode"] == "tree" and cfg["collective"] == "scatter" and cfg["parity_reduced_tuple_sums_ok"] is True
    leg = cfg["other_mode_leg"]
    assert leg["mode"] == "table" and leg["collective"] is None and leg["parity_tuple_sums_ok"] is True and leg["table_shard_rank0"] == [0, 160], leg


def test_two_ranks_share_the_gpu_over_gloo_both_modes():
    """The N > 1 control flow with a REAL world size on the one-GPU box: `QS_BENCH_BACKEND=gloo python bench.py --gpus 2` -- two ranks
    started by bench.py's own launcher share cuda:0 (RCCL refuses two ranks on one device, so the collectives are staged through the
    host: quartetscores_amd/collectives.py). Table-sharded: every rank counts all trees into its cost-balanced shard, no table collective,
    sharded scoring over SUM / MIN / all-gather. Tree-sharded: 3000 trees per rank, the reduce-scatter of the one-word-per-tuple wire
    format, every rank scores the shard it received. Each line carries the other mode as a leg; all tuple-sum gates hold on every rank."""
    os.environ["QS_BENCH_BACKEND"] = "gloo"
    common = ["--gpus", "2", "--taxa", "160", "--trees", "6000", "--steps", "6", "--warmup", "1", "--p2p-leg", "0", "--full", "--no-cpu-baseline", "--no-e2e"]
    try:
        table = run_bench(common + ["--mode", "table"])
        tree = run_bench(common + ["--mode", "tree"])
    finally:
        del os.environ["QS_BENCH_BACKEND"]
    for doc in (table, tree):
        assert doc["n_gpus"] == 2 and doc["scaling"] == "strong" and doc["collective"]["backend"] == "gloo" and doc["collective"]["proof"] == 2
        assert doc["config"]["launcher"]["ranks"] == 2 and doc["config"]["parity_lookup_equals_bruteforce"] is True
    cfg = table["config"]
    assert cfg["mode"] == "table" and cfg["collective"] is None and cfg["parity_tuple_sums_ok"] is True and cfg["shard_balance"] == "cost"
    assert cfg["table_shard"][0] == 0 and 0 < cfg["table_shard"][1] < 160 and "table shards" in cfg["score_mode"]
    leg = cfg["other_mode_leg"]
    assert leg["mode"] == "tree" and leg["wire"] == "u16x2" and leg["parity_tuple_sums_ok"] is True, leg
    cfg = tree["config"]
    assert cfg["mode"] == "tree" and cfg["collective"] == "scatter" and cfg["parity_reduced_tuple_sums_ok"] is True
    assert "1 word/tuple wire" in cfg["step"] and cfg["one_rank_same_workload"]["count_only_ms_per_step"] > 0
    leg = cfg["other_mode_leg"]
    assert leg["mode"] == "table" and leg["collective"] is None and leg["parity_tuple_sums_ok"] is True, leg
    # the same units of work in both lines: all trees x all quartets per step
    assert abs(table["value"] * table["ms_per_step"] / (tree["value"] * tree["ms_per_step"]) - 1.0) < 1e-9


def test_four_ranks_share_the_gpu_table_mode_and_auto():
    """Four ranks on cuda:0 over gloo (QS_BENCH_BACKEND=gloo): the table-sharded mode with four cost-balanced shards (qs_shard_bounds), the
    tree-sharded leg with four chunks of the reduce-scatter, and `--mode auto`, which at this size (a 0.1 GB table) picks the tree cut."""
    os.environ["QS_BENCH_BACKEND"] = "gloo"
    common = ["--gpus", "4", "--taxa", "160", "--trees", "4000", "--steps", "4", "--warmup", "1", "--p2p-leg", "0", "--full", "--no-cpu-baseline", "--no-e2e"]
    try:
        table = run_bench(common + ["--mode", "table"])
        auto = run_bench(common + ["--no-score"])
    finally:
        del os.environ["QS_BENCH_BACKEND"]
    cfg = table["config"]
    assert table["n_gpus"] == 4 and table["collective"]["proof"] == 4 and cfg["mode"] == "table" and cfg["parity_tuple_sums_ok"] is True
    assert cfg["table_shard"][0] == 0 and cfg["parity_lookup_equals_bruteforce"] is True and "table shards" in cfg["score_mode"]
    assert cfg["other_mode_leg"]["mode"] == "tree" and cfg["other_mode_leg"]["parity_tuple_sums_ok"] is True
    cfg = auto["config"]
    assert cfg["mode"] == "tree" and cfg["mode_decided_by"] == "auto (model)" and cfg["mode_model"]["table_extra_ms"] > cfg["mode_model"]["tree_collective_ms_ring_bound"]
    assert cfg["parity_reduced_tuple_sums_ok"] is True and cfg["other_mode_leg"]["mode"] == "table" and cfg["other_mode_leg"]["parity_tuple_sums_ok"] is True
