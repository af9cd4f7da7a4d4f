"""bench.py's command line: a plain run times the headline alone, `--full` adds the siblings and the CPU baseline."""
import pytest

import bench


def test_plain_run_is_the_default_and_full_is_opt_in():
    plain = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not plain.full and plain.steps == 20 and plain.warmup == 5 and plain.dump_outputs is None
    full = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--no-siblings"])
    assert full.full and full.no_siblings and not full.no_extras and not full.no_cpu_baseline


def test_argument_errors_are_reported_before_any_work():
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args(["--gpus", "2", "--dump-outputs", "out"])
