"""bench.py's command line without a GPU: a plain run measures the headline alone, --full adds every other measurement,
and the --no-* / --kernels-only-steps flags still narrow a --full run."""
import bench


def test_plain_run_leaves_out_everything_beside_the_headline():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.steps == 7 and a.warmup == 2
    assert a.kernels_only_steps == 0 and a.no_e2e and a.no_cpu_baseline and a.no_extra


def test_full_run_measures_what_the_plain_run_used_to():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2", "--full"])
    assert a.full and a.kernels_only_steps == 7
    assert not (a.no_e2e or a.no_cpu_baseline or a.no_extra)
    a = bench.parse_args(["--full", "--no-e2e", "--kernels-only-steps", "3"])
    assert a.no_e2e and not a.no_cpu_baseline and not a.no_extra and a.kernels_only_steps == 3


def test_preset_still_yields_to_explicit_flags():
    a = bench.parse_args(["--preset", "configs3", "--pool", "700000"])
    assert a.scaling == "strong" and a.pool == 700000 and a.workload == "150bp_w100_mixed_bins"
