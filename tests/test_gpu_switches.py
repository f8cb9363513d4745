"""Every A/B switch of the library selects a bit-identical path: a solve under each
switch against the default build's, level 0's iterate compared byte for byte, the history to 1e-12
(paths that change the norm's block structure change its summation order only). The library reads
its switches once per process, so each run is a child process (tests/switch_probe.py), one at a time."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, rel

pytestmark = pytest.mark.gpu

PROBE = os.path.join(REPO, "tests", "switch_probe.py")
SWITCHES = ["GS_COARSE_POINTS", "GS_NEWTON_PRO_POINTS", "GS_RR_NR", "GS_RR_LDS", "GS_NO_FUSED_SWEEPS",
            "GS_NO_FUSED_RR", "GS_NO_FUSED_PROLONG", "GS_NO_SPECULATION", "GS_NO_ZERO_GUESS",
            "GS_PAIR_BIG_CHUNKS", "GS_NO_UNIT_STENCIL", "GS_PAIR_MIN_BLOCKS", "GS_FIT_ROUNDS",
            "GS_NO_PIPELINE", "GS_NO_NEWTON_FUSED_UPDATE", "GS_PAIR_ONE_ROUND", "GS_SLAB_ZC", "GS_PAIR_ZC",
            "GS_RR_REVERSE", "GS_HALO_ORDER", "GS_NO_ZERO_Q", "GS_XH_SWIZZLE",
            "GS_MID_ZC", "GS_RR_ZC", "GS_RR_ZC_BIG", "GS_RB_ZC", "GS_NEWTON_B_FUSED",
            "GS_NO_NEWTON_G", "GS_PAIR_FX"]

# (case, solve args) -> the switches whose paths that problem exercises
CASES = {
    "linear256": ((0, 256, 256, 256, 3), [("GS_NO_FUSED_SWEEPS", "1"), ("GS_NO_FUSED_RR", "1"),
                                          ("GS_NO_FUSED_PROLONG", "1"), ("GS_NO_SPECULATION", "1"),
                                          ("GS_NO_ZERO_GUESS", "1"), ("GS_NO_PIPELINE", "1"), ("GS_RR_LDS", "1"),
                                          ("GS_RR_NR", "2"), ("GS_NO_UNIT_STENCIL", "1"),
                                          ("GS_PAIR_MIN_BLOCKS", "512"), ("GS_FIT_ROUNDS", "0"),
                                          ("GS_COARSE_POINTS", "4096"), ("GS_NO_ZERO_Q", "1"),
                                          ("GS_MID_ZC", "32"), ("GS_RR_ZC", "5")]),
    "linear2e26": ((0, 512, 512, 256, 2), [("GS_RR_NR", "1"), ("GS_PAIR_BIG_CHUNKS", "0"),
                                           ("GS_RR_ZC_BIG", "7")]),
    "linear512": ((0, 512, 512, 512, 2), [("GS_PAIR_ONE_ROUND", "0"), ("GS_PAIR_ZC", "96"), ("GS_RR_REVERSE", "0"),
                                          ("GS_PAIR_FX", "0")]),
    "linear_rows700": ((0, 700, 64, 64, 3), [("GS_XH_SWIZZLE", "0")]),
    # rows of two whole 512-point column blocks: the column-block FX instances against the general column-block
    # instances. LINEAR: the plain and the prolongation pair on level 0. NEWTON: the GS_NEWTON_B prolongation pair (the
    # one NEWTON column-block FX instance), which level 0 takes from GS_NEWTON_PRO_POINTS (2^21) points on: both runs of
    # the case set it to 0 (BASE_ENV), since the thin 1024-row grid of that size, 1024 x 64 x 64, diverges in the Newton
    # iteration itself, in the CPU oracle too (residuals 1.5e5, 3.6e14, inf); 31 x 31 is the smallest y, z at
    # which the column-block pair is still level 0's smoother (128 blocks of 4-plane chunks).
    # test_rows1024_cases_run_the_column_block_fx_instances holds both claims to the schedule and the launch record
    "linear_rows1024": ((0, 1024, 64, 64, 3), [("GS_PAIR_FX", "0")]),
    "newton_rows1024": ((2, 1024, 31, 31, 2), [("GS_PAIR_FX", "0")]),
    # two loopback slabs of 512^3: the interior launches of the overlapped sweeps (z0 != 0)
    "slabs512": ((0, 512, 512, 1024, 2, 2, 2, 2), [("GS_SLAB_ZC", "16"), ("GS_HALO_ORDER", "1")]),
    "newton127": ((2, 127, 127, 127, 2), [("GS_NEWTON_PRO_POINTS", "0"), ("GS_NO_FUSED_PROLONG", "1"),
                                          ("GS_NO_PIPELINE", "1"), ("GS_NO_NEWTON_FUSED_UPDATE", "1"),
                                          ("GS_RR_REVERSE", "0"), ("GS_NO_ZERO_Q", "1")]),
    # two loopback slabs in NEWTON mode: GS_NEWTON_G's pairs on slab plane ranges (ghost planes of the factor)
    "newton_slabs": ((2, 130, 66, 128, 2, 2, 2, 2), [("GS_NO_NEWTON_G", "1")]),
    "newton_rows700": ((2, 700, 12, 10, 2), [("GS_NO_NEWTON_G", "1")]),
    # rows of whole 128-point waves: the NEWTON_B plain and prolongation pairs' FX instances
    "newton256": ((2, 256, 64, 64, 2), [("GS_PAIR_FX", "0")]),
    "newton255": ((2, 255, 127, 127, 2), [("GS_RB_ZC", "10"), ("GS_NEWTON_B_FUSED", "0"),
                                          ("GS_NO_NEWTON_G", "1")]),
}
# switches a case sets in its default run and in its switched runs alike
BASE_ENV = {"newton_rows1024": {"GS_NEWTON_PRO_POINTS": "0"}}
PARAMS = [(case, sw, val) for case, (_, sws) in CASES.items() for sw, val in sws]
_default = {}


def run(tmp_path, case, env_extra):
    args, _ = CASES[case]
    out = str(tmp_path / f"{case}_{'_'.join(env_extra) or 'default'}.npz")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(BASE_ENV.get(case, {}))
    env.update(env_extra)
    r = subprocess.run([sys.executable, PROBE, out, *map(str, args)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    d = np.load(out)
    return d["v"], list(d["hist"])


def test_switch_list_matches_integration_doc():
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for s in SWITCHES:
        assert s in doc, s
    assert {s for _, s, _ in PARAMS} == set(SWITCHES) - {"GS_ZSLAB_MIN_POINTS"}


@pytest.mark.parametrize("case,switch,value", PARAMS)
def test_switch_bit_identical(tmp_path_factory, case, switch, value):
    if case not in _default:
        _default[case] = run(tmp_path_factory.mktemp("d"), case, {})
    v0, h0 = _default[case]
    v, h = run(tmp_path_factory.mktemp("s"), case, {switch: value})
    assert v.tobytes() == v0.tobytes(), f"{switch}={value}: level-0 field differs"
    assert len(h) == len(h0)
    for a, b in zip(h, h0):
        assert rel(a, b) < 1e-12, (switch, a, b)


def level0_ops(monkeypatch, case):
    """The level-0 operations of the case's solve, from the driver's schedule (gs_zslab_schedule, one rank: no device)."""
    import ctypes as C
    import gpusolve as gsv
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for key, val in BASE_ENV.get(case, {}).items():
        monkeypatch.setenv(key, val)
    mode, nx, ny, nz, maxiter = CASES[case][0]
    q = gsv.GridParams(maxiter=maxiter, tol=0.0, gridDim=(nx, ny, nz), mode=mode).to_abi()
    d, n = gsv.driver(), C.c_int64()
    assert d.gs_zslab_schedule(C.byref(q), 1, 0, 0, None, 0, C.byref(n)) == 0
    buf = C.create_string_buffer(n.value + 1)
    assert d.gs_zslab_schedule(C.byref(q), 1, 0, 0, buf, n.value + 1, C.byref(n)) == 0
    return {line.split()[0] for line in buf.value.decode().splitlines() if "L=0" in line.split()}


@pytest.mark.parametrize("case,calls", [("linear_rows1024", [("pair", 0), ("prolong", 0)]),
                                        ("newton_rows1024", [("prolong", 3)])])
def test_rows1024_cases_run_the_column_block_fx_instances(monkeypatch, case, calls):
    """The two GS_PAIR_FX cases on 1024-point rows are not a solve compared with itself: the solve's schedule has the
    fused pair ("pair") and the prolongation pair ("pro") on level 0, and on that level the launchers select (the
    launch record, dry-run, one child process per setting) the column-block FX instance by default and the general
    column-block instance under GS_PAIR_FX=0."""
    import instance_table as IT
    ops = level0_ops(monkeypatch, case)
    assert {"pair", "pro"} <= ops, ops
    shape = CASES[case][0][1:4]
    got = {}
    for fx in ("1", "0"):
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(BASE_ENV.get(case, {}), GS_PAIR_FX=fx)
        r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "instance_probe.py"), "pairs", *map(str, shape)],
                           env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        got[fx] = [tuple(line.split(" ", 2)) for line in r.stdout.splitlines()]
    for call, mode in calls:
        for fx in ("1", "0"):
            names = [n for c, m, n in got[fx] if (c, int(m)) == (call, mode)]
            want = IT.tb2y_name(mode, False, True, True, fx == "1", call == "prolong", False)
            assert names == (["k_pro_strip<false>", want] if call == "prolong" else [want]), (case, call, mode, fx, names)
