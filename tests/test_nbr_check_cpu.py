"""The argument rules of the neighbour and bond family have one definition (amof_amd/csrc/nbr_check.h, here through
tests/native/nbr_check_driver.cpp, a program of its own: nothing is loaded into Python): every rule at its edge with the code
and the literal message of its refusal -- the messages are what the GPU tests and the callers of the library match on -- the
smallest periodic height of known cells, the uniform-edge decision against numpy's own edges, and hist_bin through the step
against hist_bin through the table.  The same driver runs once more under the address and undefined-behaviour sanitizers."""

import math
import os
import subprocess

import numpy as np
import pytest

from amof_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "nbr_check_driver.cpp")
OK, EINVAL = 0, _hip.AMOF_EINVAL
PASS = (OK, 0.0, "")

SET = "set %d names a species out of range"
TRIPLE = "triple %d names a species out of range"
CHAIN = "chain %d names a species out of range"
BOND_SET = "set %d names a species outside 0..%d"
BOND_CUT = "cutoff of set %d must be finite and not negative"
FINITE = "%s must be finite and >= 0"
SYM_SETUP = "cutoff matrix must be symmetric"
SYM = "the %s matrix must be symmetric"
BAD_NB = "nb must be positive"
HIST_NB = "nb must be 1..2^24"
ORDER_NB = "nbins, nbins_tet must be 1..2^24"
EDGES = "edges must increase strictly"
N_L = "n_l must be 1..%d"
L_TOP = "l must be 1..%d"
N_CHAINS = "n_chains must be 1..%d"
CN_MAX = "cn_max must be 1..65535"
HALF = "cutoff %s exceeds half the smallest cell height %s: a pair could be bonded twice"
HALF_SET = "cutoff %s of set %d exceeds half the smallest cell height %s: %s"
TAILS = {"order": "a neighbour could be counted twice", "bond": "a pair could be bonded twice"}


def _build(tmp, flags, name):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags + [SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def _g(x):
    """C's %g"""
    return "%g" % x


def _d(x):
    return float(x).hex() if math.isfinite(x) else repr(float(x))


def _ds(v):
    return " ".join(_d(x) for x in v)


def refuse(text):
    return EINVAL, 0.0, text


def heights(cell):
    """perpendicular heights of a cell [3][3] (rows: cell vectors): volume over the area of the opposite face"""
    cell = np.asarray(cell, dtype=np.float64)
    vol = abs(np.linalg.det(cell))
    return [vol / np.linalg.norm(np.cross(cell[(k + 1) % 3], cell[(k + 2) % 3])) for k in range(3)]


def geom_rec(cells):
    """records as build_geometry lays them out: 24 doubles a cell, the heights in 18..20 (the rest is not the rule's to read)"""
    rec = np.full((len(cells), 24), 1e-3)
    for k, cell in enumerate(cells):
        rec[k, 18:21] = heights(cell)
    return rec.ravel()


ORTHO = [[8.0, 0, 0], [0, 11.0, 0], [0, 0, 9.5]]
TRICLINIC = [[10.0, 0, 0], [3.0, 9.0, 0], [-2.0, 4.0, 7.0]]
RNG = np.random.default_rng(20260115)


def bins_of(edges, x):
    """numpy.histogram's bin of every x (the last bin is closed); -1: outside"""
    edges = np.asarray(edges)
    k = np.searchsorted(edges, x, side="right") - 1
    k = np.where(x == edges[-1], len(edges) - 2, k)
    return np.where((x >= edges[0]) & (x <= edges[-1]), k, -1)


def one_ulp_off(nb, top):
    """np.linspace edges that are not k * step somewhere (they exist for these nb: asserted)"""
    e = np.linspace(0.0, top, nb + 1)
    k = np.arange(nb + 1, dtype=np.float64) * e[1]
    assert e[0] == 0.0 and np.any(e != k) and np.max(np.abs(e - k)) <= 2 * np.spacing(top)
    return e


def questions():
    """(line, expected answer)"""
    q = []
    # species named by a call: 0 .. S - 1 for a set, -1 (any) .. S - 1 for a triple or a chain; the first offender is named
    for S, sets in ((3, (0, 2, 2, 0)), (3, (0, 3)), (3, (0, 0, -1, 1)), (3, (1, 1, 2, 2, 3, 0)), (1, (0, 0)), (1, (0, 1)), (2, ())):
        bad = [k // 2 for k, x in enumerate(sets) if x < 0 or x >= S]
        q.append(("sets %d %d %s" % (S, len(sets) // 2, " ".join(map(str, sets))), refuse(SET % bad[0]) if bad else PASS))
    for S, tr in ((3, (-1, -1, 2, 0)), (3, (0, 3)), (3, (0, 0, -2, 1)), (2, (1, 1, 0, 2)), (2, ())):
        bad = [k // 2 for k, x in enumerate(tr) if x < -1 or x >= S]
        q.append(("triples %d %d %s" % (S, len(tr) // 2, " ".join(map(str, tr))), refuse(TRIPLE % bad[0]) if bad else PASS))
    for S, ch in ((3, (-1, -1, -1, -1, 0, 1, 2, 0)), (3, (0, 1, 2, 3)), (3, (0, 1, 2, 2, 0, -2, 0, 0)), (2, (1, 1, 1, 1, 1, 1, 1, 2))):
        bad = [k // 4 for k, x in enumerate(ch) if x < -1 or x >= S]
        q.append(("chains %d %d %s" % (S, len(ch) // 4, " ".join(map(str, ch))), refuse(CHAIN % bad[0]) if bad else PASS))
    for S, a, b, rc in ((3, 0, 2, 1.5), (3, 0, 3, 1.5), (3, -1, 0, 1.5), (3, 2, 2, 0.0), (3, 2, 2, -1e-300), (3, 2, 2, math.nan),
                        (3, 2, 2, math.inf), (3, 3, 0, math.nan)):
        species = a < 0 or a >= S or b < 0 or b >= S
        cut = not (rc >= 0.0 and math.isfinite(rc))
        q.append(("bondset %d %d %d %s" % (S, a, b, _d(rc)), refuse(BOND_SET % (2, S - 1)) if species else refuse(BOND_CUT % 2) if cut else PASS))
    # cutoffs: finite and >= 0 (-0.0 is 0), symmetric; entry by entry the first offender decides the text
    for what in ("cutoff", "link"):
        for v in ((0.0, 2.5, 2.5, 0.0), (-0.0, 1.0), (), (1.0, -1e-300), (math.nan,), (1.0, math.inf), (-math.inf, 1.0)):
            bad = any(not (x >= 0.0 and math.isfinite(x)) for x in v)
            q.append(("values %s %d %s" % (what, len(v), _ds(v)), refuse(FINITE % what) if bad else PASS))
    for S, m, want in ((2, (0, 2.5, 2.5, 0), PASS), (2, (0, 2.5, float(np.nextafter(2.5, 3)), 0), refuse(SYM_SETUP)), (1, (3.0,), PASS),
                       (3, (0, 1, 2, 1, 0, 3, 2, 3, 0), PASS), (3, (0, 1, 2, 1, 0, 3, 2, 4, 0), refuse(SYM_SETUP))):
        q.append(("sym %d %s" % (S, _ds(m)), want))
    for what in ("cutoff", "link"):
        for S, m, want in ((2, (0, 2.5, 2.5, 0), PASS), (2, (0, 2.5, 2.0, 0), refuse(SYM % what)), (2, (0, 2.5, 2.5, math.nan), refuse(FINITE % what)),
                           (2, (0, 2.5, 2.0, math.nan), refuse(SYM % what)),            # (0, 1) is not symmetric before (1, 1) is not finite
                           (2, (0, math.nan, math.nan, 0), refuse(FINITE % what)),      # (a NaN is refused as not finite, not as asymmetric)
                           (2, (-1.0, 2.0, 3.0, 0), refuse(FINITE % what)), (1, (math.inf,), refuse(FINITE % what)), (0, (), PASS)):
            q.append(("matrix %s %d %s" % (what, S, _ds(m)), want))
    # bin counts and edges
    for nb in (1, 0, -1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 1):
        q.append(("badbins %d" % nb, refuse(BAD_NB) if nb <= 0 else PASS))
        q.append(("histbins %d" % nb, refuse(HIST_NB) if nb <= 0 or nb > 2 ** 24 else PASS))
    for a, b in ((1, 1), (2 ** 24, 2 ** 24), (0, 5), (5, 0), (2 ** 24 + 1, 5), (5, 2 ** 24 + 1), (-3, 5)):
        q.append(("orderbins %d %d" % (a, b), PASS if 1 <= a <= 2 ** 24 and 1 <= b <= 2 ** 24 else refuse(ORDER_NB)))
    for e in ((0.0, 1.0), (0.0, float(np.nextafter(0.0, 1))), (0.0, 0.0), (0.0, 1.0, 1.0), (0.0, 2.0, 1.0), (-5.0, 0.0, 180.0), (0.0, math.nan, 2.0),
              (0.0, 1.0, math.nan), (math.nan, 1.0), (0.0, math.inf), (math.inf, math.inf)):
        bad = any(not e[k + 1] > e[k] for k in range(len(e) - 1))
        q.append(("edges %d %s" % (len(e) - 1, _ds(e)), refuse(EDGES) if bad else PASS))
    # counts
    for n_l in (1, 4, 0, 5, -1):
        q.append(("nl %d 4" % n_l, PASS if 1 <= n_l <= 4 else refuse(N_L % 4)))
    for ls in ((1,), (12, 4, 6), (0,), (4, 13), (6, -2, 99)):
        q.append(("l 12 %d %s" % (len(ls), " ".join(map(str, ls))), PASS if all(1 <= x <= 12 for x in ls) else refuse(L_TOP % 12)))
    for T in (1, 32, 0, 33, -4):
        q.append(("nchains %d 32" % T, PASS if 1 <= T <= 32 else refuse(N_CHAINS % 32)))
    for v in (1, 65535, 0, 65536, -1):
        q.append(("cnmax %d" % v, PASS if 1 <= v <= 65535 else refuse(CN_MAX)))
    # half a height: exactly half passes (no slack, unlike the Pore family's rule), the next double above is refused; without a
    # periodic axis the height is +inf and nothing is refused
    for hmin in (8.0, 13.7, 2.0 / 3.0, math.inf):
        for rc in (0.5 * hmin, float(np.nextafter(0.5 * hmin, np.inf)), 0.4 * hmin, hmin, 0.0, 1e300):
            refused = rc > 0.5 * hmin
            assert refused == (math.isfinite(hmin) and rc not in (0.5 * hmin, 0.4 * hmin, 0.0))
            q.append(("hh %s %s" % (_d(rc), _d(hmin)), refuse(HALF % (_g(rc), _g(hmin))) if refused else PASS))
            for tail in ("order", "bond"):
                q.append(("hhs %s 3 %s %s" % (_d(rc), _d(hmin), tail), refuse(HALF_SET % (_g(rc), 3, _g(hmin), TAILS[tail])) if refused else PASS))
    # the smallest height over the periodic axes of every cell
    h_o, h_t = heights(ORTHO), heights(TRICLINIC)
    assert np.allclose(h_o, [8.0, 11.0, 9.5]) and min(h_t) < 7.5 and len({round(x, 6) for x in h_t}) == 3       # (a triclinic height is no cell length)
    for pbc, cells, want in (((1, 1, 1), [ORTHO], h_o[0]), ((1, 1, 1), [TRICLINIC], min(h_t)), ((0, 1, 1), [ORTHO], h_o[2]), ((1, 0, 1), [ORTHO], h_o[0]),
                             ((1, 1, 0), [TRICLINIC], min(h_t[:2])), ((0, 0, 0), [ORTHO, TRICLINIC], math.inf), ((1, 1, 1), [], math.inf),
                             ((1, 1, 1), [ORTHO, TRICLINIC, ORTHO], min(h_t)), ((0, 0, 1), [TRICLINIC, ORTHO], min(h_t[2], h_o[2]))):
        q.append(("hmin %d %d %d %d %s" % (pbc + (len(cells), _ds(geom_rec(cells)))), (OK, float(want), "")))
    # uniform edges: k * step exactly, each one IEEE product
    for nb, step in ((180, 1.0), (36, 5.0), (1800, 0.1), (7, 1.0 / 3.0), (1, 180.0), (1, 0.1)):
        e = np.arange(nb + 1, dtype=np.float64) * step
        q.append(("step %d %s" % (nb, _ds(e)), (OK, step, "")))
        q.append(("step %d %s" % (nb, _ds(e + 1.0)), (OK, 0.0, "")))            # edges[0] != 0
        q.append(("step %d %s" % (nb, _ds(e - e[-1])), (OK, 0.0, "")))
        if nb > 1:
            off = e.copy()
            off[nb // 2 + 1] = np.nextafter(off[nb // 2 + 1], np.inf)
            q.append(("step %d %s" % (nb, _ds(off)), (OK, 0.0, "")))
    for nb, top in ((39, 180.0), (175, 180.0), (49, 1.0), (100, math.pi)):
        q.append(("step %d %s" % (nb, _ds(one_ulp_off(nb, top))), (OK, 0.0, "")))
    # hist_bin through the step and through the table: random angles, every edge, its two neighbours
    for nb, step in ((180, 1.0), (1800, 0.1), (7, 1.0 / 3.0), (1, 180.0), (257, 0.7)):
        e = np.arange(nb + 1, dtype=np.float64) * step
        x = np.concatenate([RNG.uniform(-0.01 * e[-1], 1.01 * e[-1], 400), e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf)])
        q.append(("bins %d %s %d %s" % (nb, _ds(e), len(x), _ds(x)), (OK, 0.0, ",".join(map(str, bins_of(e, x))))))
    e = one_ulp_off(175, 180.0)         # (no step: the table alone, still numpy's bins)
    x = np.concatenate([RNG.uniform(0.0, 180.0, 400), e])
    q.append(("bins 175 %s %d %s" % (_ds(e), len(x), _ds(x)), (OK, 0.0, ",".join(map(str, bins_of(e, x))))))
    return q


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("nc")


def _run(driver):
    q = questions()
    r = subprocess.run([driver], input="\n".join(line for line, _ in q) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.splitlines()
    assert len(out) == len(q)
    seen = set()
    for (line, (code, value, text)), got in zip(q, out):
        g_code, g_value, g_text = got.split("\t")
        assert (int(g_code), g_text) == (code, text), (line[:200], got[:400])
        assert float(g_value) == value, (line[:200], got[:400])
        seen.add((line.split()[0], code))
    return seen


def test_every_rule_at_its_edge(tmp):
    seen = _run(_build(tmp, ["-O1"], "nbr_check_driver"))
    rules = {"sets", "triples", "chains", "bondset", "values", "sym", "matrix", "badbins", "histbins", "orderbins", "edges", "nl", "l", "nchains",
             "cnmax", "hh", "hhs"}
    assert {r for r, code in seen if code != OK} == rules               # every rule refused ...
    assert {r for r, code in seen if code == OK} == rules | {"hmin", "step", "bins"}       # ... and passed


def test_under_the_sanitizers(tmp):
    _run(_build(tmp, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "nbr_check_driver_san"))


def test_the_messages_are_the_headers_alone():
    """the .hip files pass the header's verdicts on: the text of no rule's message stands anywhere else"""
    csrc = os.path.join(ROOT, "amof_amd", "csrc")
    texts = {}
    for name in ("nbr.hip", "order.hip", "dihedral.hip", "ring.hip", "fragment.hip", "bond.hip", "nbr_rows.h", "nbr_check.h"):
        with open(os.path.join(csrc, name)) as fh:
            texts[name] = fh.read()
    for message in ("names a species out", "must be finite and", "matrix must be symmetric", BAD_NB, "must be 1..2^24", EDGES, "n_l must be",
                    "l must be 1..", "n_chains must be", CN_MAX, "exceeds half the smallest cell height"):
        assert message in texts["nbr_check.h"], message
        for name in texts:
            assert name == "nbr_check.h" or message not in texts[name], (name, message)
    for tail in TAILS.values():         # (the two tails are the callers' to choose)
        assert tail in texts["nbr_check.h"]
    assert TAILS["order"] in texts["order.hip"] and TAILS["bond"] in texts["bond.hip"]
