"""bench.py's options (no GPU): what a plain run does besides its timed steps, and what --full adds."""
import bench


def plan(*argv, world=1):
    return bench.run_plan(bench.parse_args(list(argv)), world)


def test_plain_run_times_the_main_workload_only():
    assert plan("--gpus", "1", "--steps", "3", "--warmup", "1") == ([], False, False)
    assert plan("--dump-outputs", "out") == ([], False, False)


def test_full_run_adds_every_baseline_config_parity_and_cpu_baseline():
    assert plan("--full") == (bench.EXTRAS, True, True)
    assert plan("--full", "--no-parity") == (bench.EXTRAS, True, False)
    assert plan("--full", "--no-cpu-baseline", "--extras", "none") == ([], False, True)
    assert plan("--full", "--spp", "16") == ([], True, True)  # a changed spp is no BASELINE config
    assert plan("--full", "--workload", "final_rr") == ([], True, True)
    assert plan("--full", "--gpus", "2", world=2) == ([], False, False)


def test_explicit_extras_are_timed_with_or_without_full():
    assert plan("--extras", "final_rr,c5_shard") == (["final_rr", "c5_shard"], False, False)
    assert plan("--full", "--extras", "final_rr") == (["final_rr"], True, True)
