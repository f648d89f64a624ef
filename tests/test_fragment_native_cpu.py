"""amof_amd/csrc/fragment_math.h on the CPU (tests/native/fragment_driver.cpp, a program of its own: nothing is loaded into
Python): the per-bond image, the relabelling round, the winding relation and the fixed-point centre of mass that both GPU kernels
compile, on positions and neighbour rows written here.  Labels, shifts (of the fragments that do not wind) and winding must equal
tests/fragment_ref.py on the crystal, the long chain and the triclinic random network; the centres lie within the derived bound of
the float64 ones; the same program runs once more under the address and undefined-behaviour sanitizers."""

import os
import subprocess

import numpy as np
import pytest

from tests import fragment_cases as cases
from tests import fragment_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "fragment_driver.cpp")
NAMES = ("crystal", "chain", "random_tri")


def _build(tmp, flags, name):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags + [SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("fragment")


@pytest.fixture(scope="module")
def driver(tmp):
    return _build(tmp, ["-O2"], "fragment_driver")


def _run(driver, pos, cell, masses, fr, ortho):
    rows, deg = ref.tables(fr)
    g = np.zeros(24)
    g[:9], g[9:18] = np.asarray(cell).reshape(9), np.linalg.inv(cell).reshape(9)
    num = lambda a: " ".join(repr(float(x)) for x in np.asarray(a).reshape(-1))        # noqa: E731
    text = "%d %d\n%s\n%s\n%s\n" % (len(pos), ortho, num(g), num(pos), num(masses))
    text += "\n".join(" ".join(map(str, r)) for r in np.maximum(rows, 0).tolist()) + "\n" + " ".join(map(str, deg.tolist())) + "\n"
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    if lines[0] == "capacity":
        return None
    head = lines[0].split()
    assert head[0] == "ok"
    N = len(pos)
    atoms = np.array([[int(x) for x in line.split()] for line in lines[1:1 + N]], dtype=np.int64).reshape(N, 5)
    roots = [line.split() for line in lines[1 + N:]]
    return int(head[1]), atoms, roots


def _check(driver, name):
    c = cases.case(name)
    p = c.packed
    for f, fr in enumerate(cases.frames(name)):
        cell = cases.cell_of(p, f)
        diagonal = not (cell - np.diag(np.diag(cell))).any()
        got = None
        for ortho in ((1, 0) if diagonal else (0,)):
            out = _run(driver, p.pos[f], cell, p.masses, fr, ortho)
            assert out is not None
            assert got is None or (out[0] == got[0] and np.array_equal(out[1], got[1]) and out[2] == got[2])     # the diagonal form: the same bits
            got = out
        rounds, atoms, roots = got
        assert np.array_equal(atoms[:, 0], fr.label), name
        winds = np.array([fr.winds[int(r)] for r in fr.label])
        assert np.array_equal(atoms[:, 4].astype(bool), winds)
        assert np.array_equal(atoms[~winds, 1:4], fr.shift[~winds])
        assert 1 <= rounds <= len(fr.label)
        want = ref.centres(p.pos[f], cell, p.masses, fr)
        X = (np.abs(p.pos[f]) + np.abs(fr.shift) @ np.abs(cell)).max()
        assert [int(r[0]) for r in roots] == sorted(fr.winds)
        for k, r in enumerate(roots):
            n, mass, centre = int(r[1]), float(r[2]), np.array([float(x) for x in r[3:6]])
            assert n == int((fr.label == int(r[0])).sum()) and abs(mass - p.masses[fr.label == int(r[0])].sum()) <= 1e-12 * mass
            if fr.winds[int(r[0])]:
                assert np.isnan(centre).all()
            else:
                assert np.all(np.abs(centre - want[k]) <= cases.centre_bound(n, mass, p.masses[fr.label == int(r[0])].max(), X)), (name, f, r[0])
    return rounds


@pytest.mark.parametrize("name", NAMES)
def test_labels_shifts_winding_and_centres_equal_the_reference(driver, name):
    rounds = _check(driver, name)
    if name == "chain":
        # the root sits at one end: the label needs a round per bond, and one more finds nothing to change
        e = cases.expected(name)
        assert rounds == 300 and e.summary.tolist() == [[1, 300, 0, 0, 0]] and np.abs(e.shift).max() >= 2


def test_a_shift_beyond_its_storage_is_refused(driver):
    # two carbon atoms bonded across 200 cells: the image does not fit an int8
    cell = np.diag([10.0, 10.0, 10.0])
    pos = np.array([[1.0, 1.0, 1.0], [2.2 + 2000.0, 1.0, 1.0]])
    fr = ref.Frame(np.zeros(2, dtype=np.int64), np.zeros((2, 3), dtype=np.int64), {0: False}, [[1], [0]], {})
    assert _run(driver, pos, cell, np.array([12.0, 12.0]), fr, 1) is None
    near = np.array([[1.0, 1.0, 1.0], [2.2 + 1000.0, 1.0, 1.0]])
    rounds, atoms, roots = _run(driver, near, cell, np.array([12.0, 12.0]), fr, 1)
    assert atoms.tolist() == [[0, 0, 0, 0, 0], [0, -100, 0, 0, 0]] and rounds == 2
    assert np.allclose([float(x) for x in roots[0][3:6]], [1.6, 1.0, 1.0], atol=1e-9)


def test_under_the_sanitizers(tmp):
    san = _build(tmp, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "fragment_driver_san")
    for name in NAMES:
        _check(san, name)
