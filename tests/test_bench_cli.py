"""bench.py's command line, without a GPU: a plain run leaves everything beyond the headline to `--full`."""
import importlib.util
import os


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(__file__), "..", "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_full_is_off_by_default():
    m = _bench()
    a = m.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.full is False and (a.gpus, a.steps, a.warmup) == (1, 20, 5)
    b = m.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--no-pmc", "--no-cpu-baseline"])
    assert b.full is True and b.no_pmc and b.no_cpu_baseline and not b.no_gym_loop
