"""The host-only headers of the surface stage through tests/native/pore_surface_driver.cpp, a program of its own (nothing is
loaded into Python): the float32 decision of amof_amd/csrc/pore_surface_math.h against long double on random neighbourhoods --
no decision may be taken in float32 that long double takes the other way -- and every surface rule of
amof_amd/csrc/pore_check.h at its edge, with the code and the message of its refusal.  The same driver runs once more under
the address and undefined-behaviour sanitizers."""

import math
import os
import subprocess

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import pore as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pore_surface_driver.cpp")
OK, EINVAL, ECAPACITY = 0, _hip.AMOF_EINVAL, _hip.AMOF_ECAPACITY
NULL = "NULL argument"
U = 2.0 ** -24

# (reach, smallest sphere radius, atoms, neighbours, samples, seed): van der Waals spheres, the cases' probes, a large reach
BOUND_LINES = [(1.7, 1.2, 40, 24, 64, 11), (3.7, 1.2, 40, 60, 64, 12), (2.59, 1.39, 40, 30, 100, 13), (7.5, 0.5, 30, 120, 64, 14),
               (3.7, 3.7, 30, 40, 64, 15)]


def _build(tmp, flags, name):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags + [SRC, "-o", out, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def _g(x):
    return "%g" % x


def _d(x):
    return float(x).hex() if math.isfinite(x) else repr(float(x))


def _norm2(u):
    return (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]


def rule_questions():
    """(line, (code, message))"""
    q = []
    for n in (-1, 0, 1, 2, 4096, 4097, 2 ** 31 - 1):
        q.append(("count %d" % n, (OK, "") if 1 <= n <= 4096 else (EINVAL, "n_dirs = %d: 1 .. 4096 directions" % n)))
    # directions: the default table passes; |u|^2 - 1 at 1e-12 passes, beyond is refused, with the row named; NaN is refused
    table = P.sphere_points(100)
    q.append(("dirs 100 " + " ".join(_d(x) for x in table.reshape(-1)), (OK, "")))
    for scale, row in ((1.0 + 4e-13, 0), (1.0 + 6e-13, 1), (1.0 - 4e-13, 2), (1.0 - 6e-13, 0), (0.0, 2), (2.0, 1)):
        rows = np.array([[0.6, 0.0, 0.8], [0.0, 1.0, 0.0], [0.48, 0.6, 0.64]])
        rows[row] = rows[row] * scale
        off = _norm2(rows[row]) - 1.0
        bad = not abs(off) <= 1e-12
        assert bad == (abs(scale - 1.0) > 5e-13)
        q.append(("dirs 3 " + " ".join(_d(x) for x in rows.reshape(-1)),
                  (EINVAL, "direction %d is no unit vector: |u|^2 - 1 = %s" % (row, _g(off))) if bad else (OK, "")))
    q.append(("dirs 1 nan 0 1", (EINVAL, "direction 0 is no unit vector: |u|^2 - 1 = nan")))
    q.append(("dirs 0", (OK, "")))
    for t in ((0.0, 1.2, 2.0), (), (-0.0,), (1.2, -1e-300), (-1.0,), (0.0, math.nan)):
        bad = [k for k, x in enumerate(t) if not x >= 0.0]
        text = "threshold %d = %s: the surface stage takes probe radii >= 0" % (bad[0], _g(t[bad[0]])) if bad else ""
        q.append(("probes %d %s" % (len(t), " ".join(_d(x) for x in t)), (EINVAL, text) if bad else (OK, "")))
    # half a height for the largest sample sphere: exactly half passes, half (1 + 1e-12) passes, the next double is refused
    for hmin in (8.0, 14.3, math.inf):
        edge = 0.5 * hmin * (1.0 + 1e-12)
        for reach in (0.5 * hmin, edge, float(np.nextafter(edge, np.inf)), 0.3 * hmin, hmin):
            for rmax in (0.0, 1.7):
                tmax = reach - rmax
                if not math.isfinite(reach) or rmax + tmax != reach:
                    continue
                text = ("the largest radius + the largest probe radius = %s exceeds half the smallest cell height %s: a sample sphere "
                        "would meet its own image" % (_g(reach), _g(hmin)))
                q.append(("hhs %s %s %s" % (_d(rmax), _d(tmax), _d(hmin)), (EINVAL, text) if reach > edge else (OK, "")))
    q.append(("hhs %s %s inf" % (_d(1.7), _d(2.0)), (OK, "")))
    for n_t, N, M in ((1, 2 ** 20, 4096), (1, 2 ** 20 + 1, 4096), (3, 5592405, 256), (3, 5592406, 256), (0, 2 ** 31 - 1, 4096), (2, 2 ** 31, 1),
                      (2, 2 ** 31 + 1, 1)):
        text = "samples of %d thresholds x %d atoms x %d directions exceed the 4 GiB a frame may take" % (n_t, N, M)
        q.append(("scap %d %d %d" % (n_t, N, M), (ECAPACITY, text) if n_t * N * M > 2 ** 32 else (OK, "")))
    for F in (0, 3):
        for n_t in (0, 2):
            for want in (0, 1):
                for bits in range(4):
                    a, b = bits & 1, bits >> 1
                    if F > 0 and n_t > 0 and not a:
                        want_answer = (EINVAL, NULL)
                    elif F > 0 and n_t > 0 and want and not b:
                        want_answer = (EINVAL, "want_access without an exposed_access array")
                    else:
                        want_answer = (OK, "")
                    q.append(("outputs %d %d %d %d %d" % (F, n_t, want, a, b), want_answer))
    return q


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("ps")


def _run(driver):
    rules = rule_questions()
    lines = ["bound %r %r %d %d %d %d" % b for b in BOUND_LINES] + [line for line, _ in rules]
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    for spec, got in zip(BOUND_LINES, out):
        eps, worst, wrong, band, buried, clear = (float(x) for x in got.split())
        reach = spec[0]
        # the arithmetic part of the bound: 1.1 x 6 u Q, Q = 3.1 reach
        assert eps == pytest.approx(1.1 * 6.0 * U * 3.1 * reach, rel=1e-12)
        assert wrong == 0, (spec, got)
        assert worst < eps, (spec, got)
        # the planted half of the samples lands in the band, and decisions of both kinds are taken in float32
        assert 0.0 < band < 0.2 and buried > 1000 and clear > 1000, (spec, got)
    seen = set()
    for (line, (code, text)), got in zip(rules, out[len(BOUND_LINES):]):
        g_code, g_value, g_text = got.split("\t")
        assert (int(g_code), g_text) == (code, text), (line, got)
        assert float(g_value) == 0.0
        seen.add((line.split()[0], code))
    return seen


def test_bound_against_long_double_and_every_rule_at_its_edge(tmp):
    seen = _run(_build(tmp, ["-O1"], "pore_surface_driver"))
    names = {"count", "dirs", "probes", "hhs", "scap", "outputs"}
    assert {r for r, code in seen if code == OK} == names and {r for r, code in seen if code != OK} == names
    assert {code for r, code in seen if r == "scap"} == {OK, ECAPACITY}


def test_under_the_sanitizers(tmp):
    _run(_build(tmp, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "pore_surface_driver_san"))


def test_the_bound_is_the_librarys():
    """amof_pore_surface_bound is the header's function: the arithmetic part and the fixed-point part of a cell"""
    cell = np.array([[14.0, 0.0, 0.0], [2.0, 15.0, 0.0], [1.0, -3.0, 16.0]])
    asum = float(np.sqrt((cell * cell).sum(axis=1)).sum())
    want = 1.1 * 6.0 * U * 3.1 * 3.7 + asum / 2.0 ** 31 + 1e-10 * asum
    assert _hip.pore_surface_bound(cell, 3.7) == pytest.approx(want, rel=1e-12)
    assert 1e-6 < _hip.pore_surface_bound(cell, 3.7) < 1e-5


def test_the_messages_are_the_headers_alone():
    csrc = os.path.join(ROOT, "amof_amd", "csrc")
    with open(os.path.join(csrc, "pore_check.h")) as fh:
        header = fh.read()
    with open(os.path.join(csrc, "pore_surface.hip")) as fh:
        kernel_file = fh.read()
    for message in ("1 .. 4096 directions", "is no unit vector", "takes probe radii >= 0", "without an exposed_access array",
                    "would meet its own image", "directions exceed the 4 GiB"):
        assert message in header and message not in kernel_file, message
    assert "amof_pore_surface " in header          # the row of the comment table
