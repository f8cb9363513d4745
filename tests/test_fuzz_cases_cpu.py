"""The fuzz draw of tests/test_gpu_fuzz.py on the CPU oracle alone: which cases can compare anything.

The GPU test compares finite points and finite history entries only, so a case whose oracle result is not finite
compares little or nothing. Among the 150 drawn cases exactly the ten named here are such (a change of the generator
shows); every sibling (the longest axis swapped into y) is wholly finite, field and history."""
import numpy as np

from test_gpu_fuzz import cases, oracle_solve, siblings

NOT_FINITE = {12, 21, 27, 28, 32, 75, 88, 97, 103, 144}


def finite(case):
    hist, field = oracle_solve(case)
    return bool(np.isfinite(field).all() and np.isfinite(hist).all())


def test_the_committed_draw(monkeypatch):
    monkeypatch.delenv("GS_FUZZ_N", raising=False)
    monkeypatch.delenv("GS_FUZZ_SEED", raising=False)
    drawn = cases()
    assert len(drawn) == 150 and sum(c[2] != 0 for c in drawn) == 95
    assert {c[0] for c in drawn if not finite(c)} == NOT_FINITE
    sib = siblings(drawn)
    # the rule is fixed: every non-LINEAR case with an axis longer than y has a sibling, the ten included
    assert {c[0] for c in sib} == {f"{c[0]}y" for c in drawn if c[2] != 0 and max(c[1][0], c[1][2]) > c[1][1]}
    assert {f"{i}y" for i in NOT_FINITE} <= {c[0] for c in sib}
    for c in sib:
        assert c[1][1] == max(c[1]) and finite(c), c
