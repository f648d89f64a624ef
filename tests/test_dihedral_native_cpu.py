"""amof_amd/csrc/dihedral_math.h on the CPU (tests/native/dihedral_driver.cpp, a program of its own: nothing is loaded into
Python): the angle / undefined decision, the fixed-point cosine term and the pattern match that both GPU kernels compile, on unit
vectors and index rows written here from the float64 bond graph.  Every integer must equal tests/dihedral_ref.py on every case
(the cosine sums within one unit per chain); the same program runs once more under the address and undefined-behaviour
sanitizers."""

import os
import subprocess

import numpy as np
import pytest

from amof_amd import dihedral as amdihedral
from tests import dihedral_cases as cases
from tests import dihedral_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "dihedral_driver.cpp")
NAMES = cases.NAMES          # every case, the planted chain in every cell form


def _build(tmp, flags, name):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags + [SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("dihedral")


@pytest.fixture(scope="module")
def driver(tmp):
    return _build(tmp, ["-O2"], "dihedral_driver")


def _run(driver, pos, cell, pbc, species, adj, chains, edges):
    inv = np.linalg.inv(cell)
    num = lambda a: " ".join(repr(float(x)) for x in np.asarray(a).reshape(-1))        # noqa: E731
    lines = ["%d %d %d" % (len(pos), len(chains), len(edges) - 1), num(edges), " ".join(str(int(x)) for c in chains for x in c),
             " ".join(str(int(s)) for s in species)]
    for i, row in enumerate(adj):
        parts = [str(len(row))]
        for j in row:
            s = (pos[j] - pos[i]) @ inv
            v = (s - np.rint(s) * np.asarray(pbc, dtype=np.float64)) @ cell
            u = v / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            parts.append("%d %s" % (j, num(u)))
        lines.append(" ".join(parts))
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = np.array([[int(x) for x in line.split()] for line in r.stdout.splitlines()], dtype=np.int64)
    return out[:, 3:], out[:, 0], out[:, 1], out[:, 2]


def _check(driver, name):
    c = cases.case(name)
    p = c.packed
    kinds = sorted(set(int(z) for z in p.numbers))
    species = [kinds.index(int(z)) for z in p.numbers]
    _, idx, edges = cases.abi_arguments(c)
    pos = p.pos_host()
    for f, fr in enumerate(cases.reference(name)):
        cell = np.asarray(p.cell[0 if p.cell.shape[0] == 1 else f], dtype=np.float64)
        hist, n, undefined, cos = _run(driver, pos[f], cell, tuple(p.pbc), species, fr.adj, idx, edges)
        assert np.array_equal(hist, fr.hist) and np.array_equal(n, fr.n) and np.array_equal(undefined, fr.undefined), (name, f)
        ref.check_cos(cos, fr.cos, fr.n)


@pytest.mark.parametrize("name", NAMES)
def test_the_header_equals_the_restatement(driver, name):
    _check(driver, name)


def test_bins_are_bads():
    edges, phi = amdihedral.bins(7.0)
    assert len(edges) == 27 and len(phi) == 26 and edges[-1] == 182.0 and phi[0] == 3.5


def test_under_the_sanitizers(tmp):
    san = _build(tmp, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "dihedral_driver_san")
    for name in NAMES:
        _check(san, name)
