"""The lag/origin work list has one definition in the library (amof_amd/csrc/lag_work.h, through
tests/native/lag_work_driver.cpp) and one in Python (amof_amd/lags.py): ranks split the list by index, so the two must
agree entry for entry -- exhaustively, on every cut of small lists."""

import os
import subprocess

import numpy as np
import pytest

from amof_amd import lags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FRAMES = (0, 1, 2, 3, 11, 12)
STRIDES = (1, 2, 3, 5)


def window_lists(F):
    """the lists valid for F frames (every lag in [0, max(F, 1))), one of them unsorted with a duplicate"""
    lists = [[0], [0, 2, 5], [F - 1], [F - 2], [5, 0, 5, 1], []]
    return [w for w in lists if all(0 <= m < max(F, 1) for m in w)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lw") / "lag_work_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "lag_work_driver.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_every_cut_of_the_work_list_equals_the_python_list(driver):
    cases = [(F, s, w) for F in FRAMES for s in STRIDES for w in window_lists(F)]
    assert {tuple(w) for _, _, w in cases} >= {(0,), (0, 2, 5), (5, 0, 5, 1), (), (11,), (10,)}
    text = "".join("%d %d %d %s\n" % (F, s, len(w), " ".join(str(m) for m in w)) for F, s, w in cases)
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = iter(r.stdout.splitlines())
    cuts = 0
    for F, s, w in cases:
        tag, total = next(lines).split()
        total = int(total)
        assert tag == "T" and total == lags.total_work(F, w, s) == int(lags.n_origins(F, w, s).sum())
        wl, kl = lags.work_list(F, w, s)
        assert len(wl) == len(kl) == total
        for wb in range(total + 1):
            for we in range(wb, total + 1):
                v = [int(x) for x in next(lines).split()]
                assert v[:2] == [wb, we] and len(v) == 2 + 2 * len(w)
                got_w, got_k = [], []
                for i in range(len(w)):
                    o0, o1 = v[2 + 2 * i], v[3 + 2 * i]
                    assert o0 < o1 or (o0, o1) == (0, 0)        # an empty interval is written {0, 0}: the F(q, t) kernel reads it
                    got_w += [i] * (o1 - o0)
                    got_k += [1 + s * o for o in range(o0, o1)]
                assert got_w == wl[wb:we].tolist() and got_k == kl[wb:we].tolist(), (F, s, w, wb, we)
                cuts += 1
    assert next(lines, None) is None
    assert cuts == sum((t + 1) * (t + 2) // 2 for t in (lags.total_work(F, w, s) for F, s, w in cases)) and cuts > len(cases)
    # the origin frames themselves: k = 1, 1 + s, ... <= F - m - 1
    for F, s, w in cases:
        for m in w:
            assert lags.origins(F, m, s).tolist() == [k for k in range(1, F) if (k - 1) % s == 0 and k <= F - m - 1]


def test_check_origin_stride():
    assert lags.check_origin_stride(3) == 3 and lags.check_origin_stride(2.0) == 2
    assert isinstance(lags.check_origin_stride(np.int64(4)), int)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="origin_stride must be an integer >= 1"):
            lags.check_origin_stride(bad)
