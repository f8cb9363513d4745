"""bench.py's command line: a plain run keeps only the timed sweeps (every other leg's option is switched off,
whatever it was given), --full keeps the legs and their options, --dump-outputs names the directory."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LEGS = ("vcycles", "cpu_sweeps", "cpu_vcycles", "config5", "config2", "newton_iters")


def parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_switches_every_other_leg_off(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3", "--vcycles", "9", "--newton-iters", "4")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 3)
    assert not a.full and a.dump_outputs is None
    assert all(getattr(a, leg) == 0 for leg in LEGS) and a.cta_ab == ""


def test_full_keeps_the_legs_and_their_options(monkeypatch):
    a = parse(monkeypatch, "--full", "--steps", "7", "--vcycles", "9", "--cpu-sweeps", "0", "--dump-outputs", "d")
    assert a.full and a.steps == 7 and a.dump_outputs == "d"
    assert a.vcycles == 9 and a.cpu_sweeps == 0
    assert a.newton_iters == 2 and a.config5 == 1 and a.config2 == 1 and a.cpu_vcycles == 2 and a.cta_ab == "16,64"
