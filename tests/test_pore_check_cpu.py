"""The argument rules of the Pore family have one definition (amof_amd/csrc/pore_check.h, here through
tests/native/pore_check_driver.cpp, a program of its own: nothing is loaded into Python): every rule at its edge against a
restatement in Python, and the code and the message of one refusal per rule -- the messages are what the GPU tests and the
callers of the library match on.  The same driver runs once more under the address and undefined-behaviour sanitizers."""

import math
import os
import re
import subprocess

import numpy as np
import pytest

from amof_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pore_check_driver.cpp")
OK, EINVAL, ECAPACITY = 0, _hip.AMOF_EINVAL, _hip.AMOF_ECAPACITY
with open(os.path.join(ROOT, "include", "amof_hip.h")) as _fh:
    MAX_WORDS = int(re.search(r"#define AMOF_PORE_MAX_WORDS (\d+)", _fh.read()).group(1))

NULL = "NULL argument"
GRID_SMALL = "grid must be at least 1 x 1 x 1"
GRID_LARGE = "the grid has more than 2^31 - 1 points"
PERIODIC = "periodic axis %d has %d grid points: a point would meet itself or one neighbour through both faces, labelling needs 3"
DR_DMAX = "dr and dmax must be finite and > 0"
NO_BIN = "dmax / dr rounds to no bin"
WORDS = "nbins + 2 + n_thresholds exceeds %d" % MAX_WORDS
RADII = "radii must be finite and >= 0"
THRESHOLDS = "thresholds must be finite"
FINITE = "the field must be finite"
WANT_FREE = "want_free without a free_sphere array"
WANT_ACCESS = "want_access without a po_access array"


def _build(tmp, flags, name):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags + [SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def _g(x):
    """C's %g"""
    return "%g" % x


def _d(x):
    return float(x).hex() if math.isfinite(x) else repr(float(x))


# ---- the rules, restated: (code, value, message) ----
def grid_rule(n, label=False, pbc=(1, 1, 1)):
    for k in range(3):
        if n[k] < 1:
            return EINVAL, 0.0, GRID_SMALL
        if label and pbc[k] and n[k] < 3:
            return EINVAL, 0.0, PERIODIC % (k, n[k])
    if n[0] * n[1] > 2 ** 31 - 1 or n[0] * n[1] * n[2] > 2 ** 31 - 1:
        return EINVAL, 0.0, GRID_LARGE
    return OK, 0.0, ""


def bins_rule(dr, dmax, n_t):
    if not (dr > 0 and math.isfinite(dr) and dmax > 0 and math.isfinite(dmax)):
        return EINVAL, 0.0, DR_DMAX
    with np.errstate(over="ignore"):
        nb = float(np.rint(np.float64(dmax) / np.float64(dr)))      # (round half to even, as rint does; 1e300 / 1e-300 = inf)
    if not nb >= 1.0:
        return EINVAL, 0.0, NO_BIN
    if nb + 2.0 + n_t > MAX_WORDS:
        return ECAPACITY, 0.0, WORDS
    return OK, nb, ""


def half_rule(reach, hmin):
    return reach > 0.5 * hmin * (1.0 + 1e-12)


def questions():
    """(line, expected answer)"""
    q = []
    # grid: the bounds, a 0 on any axis, the labelling's periodic axes
    for n in ((1, 1, 2147483647), (1, 2, 1073741824), (46341, 46341, 1), (46340, 46340, 1), (1, 1, 1), (0, 4, 4), (4, 0, 4), (4, 4, 0),
              (-1, 4, 4), (2048, 2048, 512), (2048, 2048, 511), (65536, 32768, 1), (1290, 1290, 1290), (1291, 1291, 1291)):
        q.append(("grid %d %d %d 0 0 0 0" % n, grid_rule(n)))
    assert grid_rule((1, 1, 2147483647))[0] == OK and grid_rule((1, 2, 1073741824))[0] == EINVAL and grid_rule((46341, 46341, 1))[0] == EINVAL
    for n, pbc in (((2, 5, 5), (1, 1, 1)), ((2, 5, 5), (0, 1, 1)), ((5, 5, 1), (1, 1, 1)), ((5, 5, 1), (1, 1, 0)), ((3, 3, 3), (1, 1, 1)),
                   ((5, 2, 0), (1, 1, 1)), ((0, 2, 5), (1, 1, 1)), ((2, 2, 2), (0, 0, 0)), ((5, 2, 5), (1, 1, 1))):
        q.append(("grid %d %d %d 1 %d %d %d" % (n + pbc), grid_rule(n, True, pbc)))
        q.append(("grid %d %d %d 0 %d %d %d" % (n + pbc), grid_rule(n)))         # refused only when labelling is asked for
    assert grid_rule((2, 5, 5), True)[2] == PERIODIC % (0, 2) and grid_rule((2, 5, 5))[0] == OK
    # dr, dmax, the bins and the counters
    for dr, dmax, n_t in ((1.0, 0.5, 0), (1.0, 0.51, 0), (1.0, 2.5, 0), (1.0, 3.5, 0), (0.05, 8.0, 2), (0.0, 1.0, 0), (-1.0, 1.0, 0),
                          (1.0, 0.0, 0), (math.nan, 1.0, 0), (1.0, math.inf, 0), (math.inf, 1.0, 0), (1.0, math.nan, 0), (1e-300, 1e300, 0),
                          (1.0, MAX_WORDS - 2.0, 0), (1.0, MAX_WORDS - 1.0, 0), (1.0, 100.0, MAX_WORDS - 102), (1.0, 100.0, MAX_WORDS - 101),
                          (1.0, 1.0, MAX_WORDS - 3), (1.0, 1.0, MAX_WORDS - 2)):
        q.append(("bins %s %s %d" % (_d(dr), _d(dmax), n_t), bins_rule(dr, dmax, n_t)))
    assert bins_rule(1.0, 0.5, 0)[2] == NO_BIN and bins_rule(1.0, 0.51, 0)[:2] == (OK, 1.0) and bins_rule(1.0, 2.5, 0)[:2] == (OK, 2.0)
    assert bins_rule(1.0, 100.0, MAX_WORDS - 102)[0] == OK and bins_rule(1.0, 100.0, MAX_WORDS - 101)[0] == ECAPACITY
    # radii, thresholds, a supplied field
    for r in ((1.2, 1.7), (0.0,), (), (1.0, math.nan), (math.inf,), (1.0, -1e-300), (-0.0, 2.0, 1.0)):
        bad = any(not (x >= 0 and math.isfinite(x)) for x in r)
        q.append(("radii %d %s" % (len(r), " ".join(_d(x) for x in r)), (EINVAL, 0.0, RADII) if bad else (OK, max(r + (0.0,)), "")))
    for t in ((0.0, 1.2), (), (-5.0,), (math.nan,), (0.0, math.inf), (-math.inf,)):
        bad = any(not math.isfinite(x) for x in t)
        q.append(("thr %d %s" % (len(t), " ".join(_d(x) for x in t)), (EINVAL, 0.0, THRESHOLDS) if bad else (OK, 0.0, "")))
    for f in ((-1.0, 2.5, 0.0), (-3.0, -2.0), (), (1.0, math.nan), (math.inf, 1.0), (1.0, -math.inf)):
        bad = any(not math.isfinite(x) for x in f)
        q.append(("finite %d %s" % (len(f), " ".join(_d(x) for x in f)), (EINVAL, 0.0, FINITE) if bad else (OK, max(f + (-math.inf,)), "")))
    # half a height, both forms: exactly half passes, half (1 + 1e-12) passes, the next double above that is refused
    for hmin in (8.0, 13.7, 2.0 / 3.0, math.inf):
        edge = 0.5 * hmin * (1.0 + 1e-12)
        for reach in (0.5 * hmin, edge, np.nextafter(edge, np.inf), 0.4 * hmin, hmin):
            reach = float(reach)
            refused = half_rule(reach, hmin)
            if math.isfinite(hmin):
                assert refused == (reach > edge) and not half_rule(0.5 * hmin, hmin) and not half_rule(edge, hmin)
                assert half_rule(float(np.nextafter(edge, np.inf)), hmin)
            for rmax in (0.0, 1.5):
                dmax = reach - rmax
                if dmax + rmax != reach:                # (the sum the rule forms must be the reach under test)
                    continue
                text = ("dmax + the largest radius = %s exceeds half the smallest cell height %s: one minimum image would not do"
                        % (_g(reach), _g(hmin)))
                q.append(("hha %s %s %s" % (_d(dmax), _d(rmax), _d(hmin)), (EINVAL, 0.0, text) if refused else (OK, 0.0, "")))
            text = ("the largest field value %s of frame 3 exceeds half the smallest periodic cell height %s: a sphere would reach a point "
                    "through two images" % (_g(reach), _g(hmin)))
            q.append(("hhf %s 3 %s" % (_d(reach), _d(hmin)), (EINVAL, 0.0, text) if refused else (OK, 0.0, "")))
    q.append(("hhf %s 0 %s" % (_d(-1.0), _d(math.inf)), (OK, 0.0, "")))
    # 4 GiB per frame: a per-point array, the labels
    for G in (1, 2 ** 29, 2 ** 29 + 1, 2 ** 31 - 1):
        for what in ("field", "array"):
            text = "a per-point %s of %d points per frame exceeds the 4 GiB a frame may take" % (what, G)
            q.append(("cap %d %s" % (G, what), (ECAPACITY, 0.0, text) if G * 8 > 2 ** 32 else (OK, 0.0, "")))
    for n_t, G in ((1, 2 ** 30), (1, 2 ** 30 + 1), (2, 2 ** 29), (2, 2 ** 29 + 1), (80000, 13965), (4, 2 ** 28), (3, 357913941), (3, 357913942),
                   (0, 2 ** 31 - 1), (2046, 524800), (2046, 524801)):
        text = "labels of %d thresholds x %d points exceed the 4 GiB a frame may take" % (n_t, G)
        q.append(("labels %d %d" % (n_t, G), (ECAPACITY, 0.0, text) if n_t * G * 4 > 2 ** 32 else (OK, 0.0, "")))
    # NULL arguments: every combination of given and missing
    null = (EINVAL, 0.0, NULL)

    def answer(bad, other=None):
        return null if bad else ((EINVAL, 0.0, other) if other else (OK, 0.0, ""))

    for a in range(2):
        for b in range(2):
            q.append(("null both_given %d %d" % (a, b), answer(not a or not b)))
            for n_t in (-1, 0, 2):
                if b == 0:
                    q.append(("null thresholds_given %d %d" % (a, n_t), answer(n_t < 0 or (n_t > 0 and not a))))
    for F in (0, 3):
        for n_t in (0, 2):
            for bits in range(16):
                h, c, v, m = [(bits >> k) & 1 for k in range(4)]
                q.append(("null field_outputs %d %d %d %d %d %d" % (F, n_t, h, c, v, m),
                          answer(F > 0 and (not h or not v or not m or (n_t > 0 and not c)))))
            for bits in range(4):
                a, b = bits & 1, bits >> 1
                q.append(("null psd_outputs %d %d %d %d" % (F, n_t, a, b), answer(F > 0 and (not a or (n_t > 0 and not b)))))
                for want in (0, 1):
                    q.append(("null access_outputs %d %d %d %d %d" % (F, n_t, want, a, b),
                              answer(F > 0 and n_t > 0 and not a, WANT_FREE if F > 0 and want and not b else None)))
                    q.append(("null po_access_given %d %d %d %d" % (F, n_t, want, a),
                              answer(False, WANT_ACCESS if F > 0 and n_t > 0 and want and not a else None)))
    for F in (-1, 0, 2):
        for bits in range(32):
            g, p, f, needs, c = [(bits >> k) & 1 for k in range(5)]
            q.append(("null given_field_inputs %d %d %d %d %d %d" % (g, p, F, f, needs, c),
                      answer(not g or not p or F < 0 or (F > 0 and (not f or (needs and not c))))))
    return q


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("pc")


def _run(driver):
    q = questions()
    r = subprocess.run([driver], input="\n".join(line for line, _ in q) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.splitlines()
    assert len(out) == len(q)
    seen = set()
    for (line, (code, value, text)), got in zip(q, out):
        g_code, g_value, g_text = got.split("\t")
        assert (int(g_code), g_text) == (code, text), (line, got)
        assert float(g_value) == value, (line, got)
        seen.add((line.split()[1] if line.startswith("null") else line.split()[0], code, text.split(" ")[0] if code else ""))
    return seen


def test_every_rule_at_its_edge(tmp):
    seen = _run(_build(tmp, ["-O1"], "pore_check_driver"))
    # every rule both passed and refused, each refusal with its code and text
    rules = {"grid", "bins", "radii", "thr", "finite", "hha", "hhf", "cap", "labels", "both_given", "thresholds_given",
             "field_outputs", "given_field_inputs", "access_outputs", "psd_outputs", "po_access_given"}
    assert {r for r, code, _ in seen if code == OK} == rules and {r for r, code, _ in seen if code != OK} == rules
    assert {code for r, code, _ in seen if r in ("cap", "labels")} == {OK, ECAPACITY}
    assert {(r, w) for r, code, w in seen if code == ECAPACITY} == {("cap", "a"), ("labels", "labels"), ("bins", "nbins")}
    assert {w for r, code, w in seen if r == "grid" and code} == {"grid", "the", "periodic"}
    assert {w for r, code, w in seen if r == "bins" and code} == {"dr", "dmax", "nbins"}
    assert {w for r, code, w in seen if r == "access_outputs" and code} == {"NULL", "want_free"}


def test_under_the_sanitizers(tmp):
    _run(_build(tmp, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "pore_check_driver_san"))


def test_the_messages_are_the_headers_alone():
    """the three .hip files pass the header's verdicts on: the text of no rule's message stands anywhere else"""
    csrc = os.path.join(ROOT, "amof_amd", "csrc")
    texts = {}
    for name in ("pore.hip", "pore_access.hip", "pore_cover.hip", "amof_internal.h", "pore_check.h"):
        with open(os.path.join(csrc, name)) as fh:
            texts[name] = fh.read()
    for message in (NULL, GRID_SMALL, GRID_LARGE, "labelling needs 3", DR_DMAX, NO_BIN, "n_thresholds exceeds", RADII, THRESHOLDS, FINITE,
                    WANT_FREE, WANT_ACCESS, "one minimum image would not do", "through two images", "4 GiB a frame may take"):
        assert message in texts["pore_check.h"], message
        for name in ("pore.hip", "pore_access.hip", "pore_cover.hip", "amof_internal.h"):
            assert message not in texts[name], (name, message)
