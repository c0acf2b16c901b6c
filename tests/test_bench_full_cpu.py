"""CPU: what a run of bench.py does besides its steps (`bench.extras`).  A plain `bench.py --gpus 1 --steps N --warmup W`, with
or without `--dump-outputs`, does nothing besides; the self-check, the other precisions and models, the legs and the CPU
baseline belong to `--full`, where the `--no-*` options drop them one by one."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERYTHING = {"verify", "strict_f32", "config5", "pose", "legs", "cpu_baseline"}


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_full_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _extras(bench, *flags, world=1, linemod=False):
    return bench.extras(bench.parser().parse_args(["--gpus", str(world), "--steps", "5", "--warmup", "2", *flags]), world, linemod)


def test_a_plain_run_has_no_extras():
    bench = _bench()
    assert bench.parser().parse_args([]).full is False
    assert _extras(bench) == set()
    assert _extras(bench, "--dump-outputs", "somewhere") == set()
    assert _extras(bench, world=2) == set()
    assert _extras(bench, "--workload", "linemod", linemod=True) == set()
    # the options that drop parts of a --full run do not bring anything into a plain one
    assert _extras(bench, "--no-verify", "--no-strict-f32", "--no-config5", "--no-legs", "--no-cpu-baseline") == set()


def test_full_has_every_part_and_the_no_options_drop_theirs():
    bench = _bench()
    assert _extras(bench, "--full") == EVERYTHING
    for flag, gone in (("--no-verify", {"verify"}), ("--no-strict-f32", {"strict_f32"}), ("--no-config5", {"config5"}),
                       ("--no-legs", {"pose", "legs"}), ("--no-cpu-baseline", {"cpu_baseline"})):
        assert _extras(bench, "--full", flag) == EVERYTHING - gone, flag
    assert _extras(bench, "--full", "--precision", "f32") == EVERYTHING - {"strict_f32"}   # the run itself is that leg
    # more than one rank, or the pair-list workload: the self-check on every rank, none of the one-GPU legs
    assert _extras(bench, "--full", world=2) == {"verify"}
    assert _extras(bench, "--full", "--workload", "linemod", linemod=True) == {"verify", "cpu_baseline"}


def test_legs_asked_for_by_name_need_no_full():
    bench = _bench()
    assert _extras(bench, "--from-host") == {"from_host"}
    assert _extras(bench, "--only", "pose") == {"pose"}
    assert _extras(bench, "--full", "--from-host") == EVERYTHING | {"from_host"}
    assert _extras(bench, "--full", "--only", "pose") == EVERYTHING - {"legs"}
