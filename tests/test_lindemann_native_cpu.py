"""amof_amd/csrc/lindemann_math.h on the CPU (tests/native/lindemann_driver.cpp, a program of its own: nothing is loaded into
Python), fed distance series of tests/lindemann_cases.py: every fixed-point term within one unit plus budget of
tests/lindemann_ref.py, every bin equal to the restatement's, the chunk traversal and the simple traversal identical to the
bit; the same program runs once more under the address and undefined-behaviour sanitizers."""

import os
import subprocess

import numpy as np
import pytest

from tests import lindemann_cases as cases
from tests import lindemann_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "lindemann_driver.cpp")
E = 40


def _build(tmp, flags, name):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags + [SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("lindemann")


@pytest.fixture(scope="module")
def driver(tmp):
    return _build(tmp, ["-O2"], "lindemann_driver")


def _run(driver, d, e=E, nbins=cases.NBINS, ddelta=cases.DDELTA):
    """(terms, bins) of the series d [B][n]; asserts that both traversals give the same bits"""
    d = np.asarray(d, dtype=np.float64)
    lines = ["%d %d %d %d %r" % (d.shape[0], d.shape[1], e, nbins, float(ddelta))]
    lines += [" ".join(float(x).hex() for x in row) for row in d]
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    rows = [line.split() for line in r.stdout.splitlines()]
    assert len(rows) == d.shape[1]
    for row in rows:
        assert row[0] == row[2] and row[1] == row[3] and row[4] == row[5], row          # chunk == simple, to the bit
    return np.array([int(row[0]) for row in rows], dtype=np.int64), np.array([int(row[1]) for row in rows], dtype=np.int64)


def _series():
    """[(name, d [B][n], delta, budget)]: walks of the cases (one chunk; three chunks, the last ragged) and the known answers"""
    out = [("class", ) + cases.driver_series("class", 20, 20), ("rect", ) + cases.driver_series("rect", 131, 131),
           ("rect65", ) + cases.driver_series("rect", 65, 65)]
    for B in (64, 130, 200):
        d, want = cases.cosine(B)
        delta, budget = ref.series_delta(d)
        assert np.all(np.abs(delta - want) <= 1e-12)
        out.append(("cosine%d" % B, d, delta, budget))
    return out


def _check(driver):
    for name, d, delta, budget in _series():
        assert d.shape[1] > 0 and float(budget.max()) < 2.0 ** -30, name
        terms, bins = _run(driver, d)
        # one unit (the rounding to the grid, generously) plus the budget, in units of 2^-E
        assert np.all(np.abs(terms - delta * 2.0 ** E) <= 1.0 + budget * 2.0 ** E), name
        assert np.array_equal(bins, np.minimum((delta / cases.DDELTA).astype(np.int64), cases.NBINS - 1)), name


def test_the_header_equals_the_restatement(driver):
    _check(driver)


def test_known_answers(driver):
    # a static pair; a pair alternating between 2 and 3 over an even block: mean 2.5, var 0.25, delta 0.2 exactly
    B = 130
    d = np.stack([np.full(B, 2.75), np.where(np.arange(B) % 2 == 0, 2.0, 3.0)], axis=1)
    terms, bins = _run(driver, d)
    assert terms.tolist() == [0, cases.ALTERNATING_TERM] and bins.tolist() == [0, 40]
    terms, bins = _run(driver, d, nbins=7)
    assert bins.tolist() == [0, 6]                      # the last bin takes everything above
    for args, want in ((("16", "64", "200"), 40), (("3000", "3000", "5000"), 62 - (3000 * 3000 * 71).bit_length()),
                       (("1000000", "1000000", "4"), 21), (("3000000", "1000000", "4"), 19), (("4000000000", "4000000000", "9"), -1)):
        r = subprocess.run([driver, "scale"] + list(args), capture_output=True, text=True)
        assert r.returncode == 0 and int(r.stdout) == want, (args, r.stdout)


def test_under_the_sanitizers(tmp):
    san = _build(tmp, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "lindemann_driver_san")
    _check(san)
