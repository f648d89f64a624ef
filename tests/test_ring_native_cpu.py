"""amof_amd/csrc/ring_search.h on the CPU (tests/native/ring_search_driver.cpp, a program of its own: nothing is loaded into
Python): the candidate enumeration, the predecessor walk, the pair enumeration and the cross-pair check that both GPU kernels
compile, on adjacency and distance tables written here.  c[v][n] must equal tests/ring_ref.py on the polygons, the 7^3 simple
cubic lattice and the ZIF-4 fixture; the path cap is met at its edge; the same program runs once more under the address and
undefined-behaviour sanitizers."""

import os
import subprocess

import numpy as np
import pytest

from tests import ring_cases as cases
from tests import ring_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ring_search_driver.cpp")
NAMES = tuple("polygon%d" % n for n in cases.POLYGONS) + ("sc7", "zif4_16", "zif4_32")


def _build(tmp, flags, name):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + [SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("ring")


@pytest.fixture(scope="module")
def driver(tmp):
    return _build(tmp, ["-O2"], "ring_search_driver")


def _run(driver, adj, nmax, cap=1024):
    rows, deg, D = ref.tables(adj, nmax // 2)
    text = "%d %d %d\n" % (len(adj), nmax, cap) + "\n".join(" ".join(map(str, r)) for r in np.maximum(rows, 0).tolist()) + "\n"
    text += " ".join(map(str, deg.tolist())) + "\n" + "\n".join(" ".join(map(str, r)) for r in D.tolist()) + "\n"
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    if lines[0] == "capacity":
        return None, None
    head = lines[0].split()
    assert head[0] == "ok" and len(lines) == 1 + len(adj)
    c = np.array([[int(x) for x in line.split()] for line in lines[1:]], dtype=np.int64).reshape(len(adj), nmax + 1)
    return c, (int(head[1]), int(head[2]))


def _check(driver, name):
    c = cases.case(name)
    for adj, (want, _) in zip(cases.graphs(name), cases.reference(name)):
        got, stats = _run(driver, adj, c.nmax)
        assert np.array_equal(got, want), name
        assert ref.rings(got) == c.known
        assert stats[0] >= stats[1] and (stats[1] > 0) == bool(c.known)


@pytest.mark.parametrize("name", NAMES)
def test_counts_equal_the_reference(driver, name):
    _check(driver, name)


def test_path_cap_at_its_edge(driver):
    # 7^3 simple cubic, nmax = 6: the antipodes at (1, 1, 1) have 3! = 6 shortest paths, every other end node fewer
    adj = cases.graphs("sc7")[0]
    assert ref.search(adj, 6)[2] == 6
    want = cases.reference("sc7")[0][0]
    got, _ = _run(driver, adj, 6, cap=6)
    assert np.array_equal(got, want)
    assert _run(driver, adj, 6, cap=5)[0] is None and _run(driver, adj, 6, cap=1)[0] is None
    # the fixture at full depth: at most 24 paths
    adj = cases.graphs("zif4_32")[0]
    assert ref.search(adj, 32)[2] == 24
    assert np.array_equal(_run(driver, adj, 32, cap=24)[0], cases.reference("zif4_32")[0][0])
    assert _run(driver, adj, 32, cap=23)[0] is None


def test_under_the_sanitizers(tmp):
    san = _build(tmp, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "ring_search_driver_san")
    for name in ("polygon3", "polygon12", "polygon13", "sc7", "zif4_32"):
        _check(san, name)
    assert _run(san, cases.graphs("sc7")[0], 6, cap=5)[0] is None
