"""The host decisions of S(q), density_modes and F(q, t) have one definition (amof_amd/csrc/sq_plan.h, here through
tests/native/sq_plan_driver.cpp): the species order, the hkl order and the runs, the per-bin capacity and the fixed-point
exponents, the S(q) batch, the frames an F(q, t) call touches and its slot table, the vector chunks, the counter tiles, the
grid and the self-part batches -- each against a restatement in Python at the edges of the rule, and as invariants.  The same
driver runs once more under the address and undefined-behaviour sanitizers."""

import math
import os
import subprocess

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import structure_factor as sf
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sq_plan_driver.cpp")
SQ_RUN, SQ_THREADS, SQ_BIN_BLOCKS = 16, 256, 1024
LDS_BUDGET, SQ_RHO_BUDGET, ISF_RHO_BUDGET = 64 * 1024, 512 << 20, 1 << 30
GRID_Y = 65535
ISF_THREADS, ISF_TILE, ISF_OPW = 256, 4, 64
I32_MAX = 2 ** 31 - 1
ALL_LINES = []              # every question a test asked: once more under the sanitizers


def _build(tmp, flags, name):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags + [SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("sqp")


@pytest.fixture(scope="module")
def driver(tmp):
    return _build(tmp, ["-O1"], "sq_plan_driver")


def _ask(driver, lines, env=None, keep=True):
    if keep:
        ALL_LINES.extend(lines)
    full = dict(os.environ, **env) if env else None
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=full)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.strip().splitlines()
    assert len(out) == len(lines)
    return [l.split() for l in out]


def _ints(x):
    return " ".join(str(int(v)) for v in np.asarray(x).ravel())


def _floats(x):
    return " ".join("%.17g" % float(v) for v in np.asarray(x).ravel())


# ------------------------------------------------------------------------------------------------------- runs --
def _row(h, k, l0, n):
    return [(h, k, l0 + i) for i in range(n)]


def _run_cases():
    rng = np.random.default_rng(7)
    cases = {}
    for n in (1, 16, 17, 32, 33):
        cases["row%d" % n] = _row(2, -1, 5, n)
    cases["gap"] = _row(1, 1, 0, 5) + _row(1, 1, 7, 4)
    cases["across0"] = _row(0, 3, -20, 41)
    cases["duplicate"] = [(1, 2, 3), (1, 2, 4), (1, 2, 4), (1, 2, 5), (1, 2, 3)]
    cases["K1"] = [(0, 0, 1)]
    cases["int32_max"] = [(1, 0, I32_MAX), (1, 0, I32_MAX - 1), (1, 0, -I32_MAX - 1), (1, 0, -I32_MAX), (I32_MAX, -I32_MAX - 1, 0)]
    many = sum((_row(h, k, -9, 19 + h) for h in range(-3, 4) for k in range(-2, 3)), [])
    cases["many"] = [v for v in many if v != (0, 0, 0)]
    for name in list(cases):
        v = list(cases[name])
        cases[name + "_shuffled"] = [v[i] for i in rng.permutation(len(v))]
    return cases


def _cut_runs(hkl):
    """the rule, restated: sort by (h, k, l, caller's index); a run goes on while (h, k) stay, l is the next and n < 16"""
    order = sorted(range(len(hkl)), key=lambda i: (hkl[i][0], hkl[i][1], hkl[i][2], i))
    runs = []
    for pos, i in enumerate(order):
        h, k, l = hkl[i]
        if runs and runs[-1][3] < SQ_RUN and runs[-1][0] == h and runs[-1][1] == k and runs[-1][2] + runs[-1][3] == l:
            runs[-1][3] += 1
        else:
            runs.append([h, k, l, 1, pos])
    return runs, order


def _parse_runs(w, K):
    v = [int(x) for x in w]
    zero, n = v[0], v[1]
    runs = [v[2 + 5 * i:7 + 5 * i] for i in range(n)]
    order = v[2 + 5 * n:]
    assert len(order) == (K if zero < 0 else 0)
    return zero, runs, order


def test_runs_tile_the_sorted_list(driver):
    cases = _run_cases()
    out = _ask(driver, ["R %d %s" % (len(v), _ints(v)) for v in cases.values()])
    for (name, hkl), w in zip(cases.items(), out):
        zero, runs, order = _parse_runs(w, len(hkl))
        assert zero == -1, name
        assert sorted(order) == list(range(len(hkl))), name                  # every caller's index once
        pos = 0
        for h, k, l0, n, start in runs:                                        # contiguous tiling, one (h, k), consecutive l
            assert start == pos and 1 <= n <= SQ_RUN, name
            assert [tuple(hkl[order[start + r]]) for r in range(n)] == [(h, k, l0 + r) for r in range(n)], name
            pos += n
        assert pos == len(hkl), name
        want_runs, want_order = _cut_runs(hkl)
        assert runs == want_runs and order == want_order, name
    by = {name: _parse_runs(w, len(cases[name]))[1] for name, w in zip(cases, out)}
    assert [r[3] for r in by["row16"]] == [16] and [r[3] for r in by["row17"]] == [16, 1]
    assert [r[3] for r in by["row32"]] == [16, 16] and [r[3] for r in by["row33_shuffled"]] == [16, 16, 1]
    assert [r[3] for r in by["gap"]] == [5, 4] and [r[3] for r in by["across0"]] == [16, 16, 9]
    # a duplicated vector starts a new run; equal vectors keep the callers' order
    dup = _parse_runs(out[list(cases).index("duplicate")], 5)
    assert [r[2:4] for r in dup[1]] == [[3, 1], [3, 2], [4, 2]] and dup[2] == [0, 4, 1, 2, 3]
    # l0 + n is formed in int64: the two vectors at the top of int32 are one run, nothing wraps round to the bottom
    top = [r for r in by["int32_max"] if r[0] == 1]
    assert [r[2:4] for r in top] == [[-I32_MAX - 1, 2], [I32_MAX - 1, 2]]


def test_zero_vector_is_reported_by_index(driver):
    hkl = _row(1, 0, -3, 7) + [(0, 0, 0)] + _row(0, 0, 1, 3) + [(0, 0, 0)]
    w = _ask(driver, ["R %d %s" % (len(hkl), _ints(hkl)), "R 1 0 0 0"])
    assert [int(x) for x in w[0]] == [7, 0] and [int(x) for x in w[1]] == [0, 0]


# ---------------------------------------------------------------------------------------------- species order --
def _species_cases():
    rng = np.random.default_rng(3)
    cases = [(1, np.zeros(1, dtype=int)), (2, np.array([1, 0, 1, 1, 0])), (4, rng.integers(0, 4, 272))]
    empty = rng.integers(0, 5, 300)
    empty[empty == 2] = 4                                   # species 2 has no atom
    return cases + [(5, empty), (3, np.zeros(0, dtype=int))]


def test_species_order_against_numpy(driver):
    cases = _species_cases()
    for (S, sp), w in zip(cases, _ask(driver, ["O %d %d %s" % (S, len(sp), _ints(sp)) for S, sp in cases])):
        v = np.array([int(x) for x in w], dtype=np.int64)
        assert np.array_equal(v[:len(sp)], np.argsort(sp, kind="stable"))
        assert np.array_equal(v[len(sp):], np.concatenate([[0], np.cumsum(np.bincount(sp, minlength=S))]))


# ------------------------------------------------------------------------------------- capacity and exponents --
def _capacity(recip, hkl, dq, nbins):
    """sq_bin_capacity with its operation order (Python floats: IEEE doubles, no fma)"""
    recip = [[float(x) for x in c] for c in np.asarray(recip, dtype=np.float64).reshape(-1, 9)]
    Rm = [0.0] * 9
    for c in recip:
        for i in range(9):
            Rm[i] += c[i]
    Rm = [x / float(max(len(recip), 1)) for x in Rm]
    delta = 0.0
    for c in recip:
        f2 = 0.0
        for i in range(9):
            f2 += (c[i] - Rm[i]) * (c[i] - Rm[i])
        delta = max(delta, math.sqrt(f2))
    diff = [0] * (nbins + 1)
    for h, k, l in ((float(a), float(b), float(c)) for a, b, c in hkl):
        qx = (h * Rm[0] + k * Rm[3]) + l * Rm[6]
        qy = (h * Rm[1] + k * Rm[4]) + l * Rm[7]
        qz = (h * Rm[2] + k * Rm[5]) + l * Rm[8]
        qm, r = math.sqrt((qx * qx + qy * qy) + qz * qz), delta * math.sqrt((h * h + k * k) + l * l)
        lo, hi = (qm - r) * (1.0 - 1e-9) / dq, (qm + r) * (1.0 + 1e-9) / dq
        if not lo < float(nbins):
            continue
        diff[int(lo) if lo > 0.0 else 0] += 1
        diff[(int(hi) if hi < float(nbins) else nbins - 1) + 1] -= 1
    return max([0] + list(np.cumsum(diff[:nbins])))


def _scales(species, S, F, cap):
    """(index of the refused pair or -1, its (a, c), nsp, sexp, scale) -- filled up to the refused pair as sq_scales leaves them"""
    nsp = [int(x) for x in np.bincount(species, minlength=S)] if len(species) else [0] * S
    P = S * (S + 1) // 2
    sexp, scale, p = [0] * P, [0.0] * P, 0
    for a in range(S):
        for c in range(a, S):
            bound = float(max(F, 1)) * float(max(cap, 1)) * (float(max(nsp[a], 1)) * float(max(nsp[c], 1)) + 0.5)
            e = math.frexp(bound)[1]
            sexp[p] = min(62 - e, 60)
            scale[p] = math.ldexp(1.0, sexp[p])
            nab = math.sqrt(float(max(nsp[a], 1)) * float(max(nsp[c], 1)))
            if math.ldexp(1.0, -sexp[p]) / nab > math.ldexp(1.0, -20):
                return p, (a, c), nsp, sexp, scale
            p += 1
    return -1, (-1, -1), nsp, sexp, scale


def _scale_cases():
    """name -> (S, species, F, recip [n][9], hkl, dq, nbins)"""
    rng = np.random.default_rng(11)
    packed = H.random_walk(H.zif4_frame(), 4, 0.05, 5, cell_jitter=0.02)
    sp = H.species_of(packed.numbers)[1]
    S = len(H.species_of(packed.numbers)[0])
    recip = _hip.reciprocal(packed.cell).reshape(-1, 9)
    hkl = sf.enumerate_hkl(packed.cell, 2.5)
    one = np.array([[0, 0, 1]])
    unit = np.eye(3).reshape(1, 9) * 2 * math.pi / 10.0
    cases = {
        "constant": (S, sp, 4, recip[:1], hkl, 0.03, sf.n_bins(2.5, 0.03)),
        "varying": (S, sp, 4, recip, hkl, 0.03, sf.n_bins(2.5, 0.03)),
        "all_beyond": (S, sp, 4, recip, hkl, 0.0005, 3),
        "one_bin": (S, sp, 5000, recip, hkl, 10.0, 1),
        "sheared": (2, rng.integers(0, 2, 50), 100, rng.normal(size=(3, 9)), rng.integers(-6, 7, (400, 3)) * [1, 1, 0] + [0, 0, 1], 0.25, 40),
        # quantum 2^-s / sqrt(N_a N_b) against 2^-20, one atom, one vector: s = 20 passes, s = 19 is refused
        "limit_pass": (1, np.zeros(1, dtype=int), 2 ** 41, unit, one, 1.0, 4),
        "limit_fail": (1, np.zeros(1, dtype=int), 2 ** 42, unit, one, 1.0, 4),
        # species counts (1, 4): pair (0, 0) passes with s = 20, pair (0, 1) is the first refused
        "limit_pair": (2, np.array([1, 0, 1, 1, 1]), 2 ** 41, unit, one, 1.0, 4),
        "cap60": (1, np.zeros(1, dtype=int), 1, unit, one, 1.0, 4),
        "empty_species": (3, np.array([0, 2, 2, 0, 2]), 10, unit, np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0]]), 0.5, 8),
    }
    return cases


def test_capacity_and_exponents_follow_the_restatement(driver):
    cases = _scale_cases()
    lines = []
    for S, sp, F, recip, hkl, dq, nbins in cases.values():
        lines.append("C %d %d %d %.17g %s %s" % (len(recip), len(hkl), nbins, dq, _floats(recip), _ints(hkl)))
        lines.append("E %d %d %d %d %d %d %.17g %s %s %s" % (S, len(sp), F, len(recip), len(hkl), nbins, dq, _ints(sp), _floats(recip),
                                                              _ints(hkl)))
    out = _ask(driver, lines)
    seen = {}
    for i, (name, (S, sp, F, recip, hkl, dq, nbins)) in enumerate(cases.items()):
        cap = _capacity(recip, hkl, dq, nbins)
        assert int(out[2 * i][0]) == cap, name
        bad, (ba, bc), nsp, sexp, scale = _scales(sp, S, F, cap)
        w, P = out[2 * i + 1], S * (S + 1) // 2
        assert [int(x) for x in w[:4]] == [bad, ba, bc, cap], name
        assert [int(x) for x in w[4:4 + S]] == nsp and [int(x) for x in w[4 + S:4 + S + P]] == sexp, name
        assert [float(x) for x in w[4 + S + P:4 + S + 2 * P]] == scale, name
        rest = w[4 + S + 2 * P:]
        if bad < 0:
            sexp2, scale2 = np.array(rest[:S * S], dtype=np.int64).reshape(S, S), np.array(rest[S * S:], dtype=np.float64).reshape(S, S)
            assert np.array_equal(sexp2, sexp2.T) and np.array_equal(scale2, scale2.T), name       # symmetric
            iu = np.triu_indices(S)
            assert list(sexp2[iu]) == sexp and list(scale2[iu]) == scale, name                     # the pair's scale on both sides
            assert np.array_equal(scale2, np.ldexp(1.0, sexp2)), name
        else:
            assert not rest, name
        seen[name] = (cap, bad, ba, bc, sexp)
    hkl_n = len(cases["constant"][4])
    assert 1 < seen["constant"][0] < seen["varying"][0] < hkl_n             # the delta widening counts a vector in more bins
    assert seen["all_beyond"][0] == 0 and seen["one_bin"][0] == hkl_n
    assert seen["limit_pass"][1:] == (-1, -1, -1, [20]) and seen["limit_fail"][1:] == (0, 0, 0, [19])
    assert seen["limit_pair"][1:4] == (1, 0, 1) and seen["limit_pair"][4][:2] == [20, 18]
    assert seen["cap60"][4] == [60]                                          # bound 1.5: 62 - 1 = 61, capped


# ---------------------------------------------------------------------------------------------- S(q) batches --
def test_sq_batch_plan(driver):
    big = 4000000                   # S = 4: 256 MB of rho per frame
    cases = [(K, S, nbins, n_sel, g) for K, S, nbins, n_sel in
             [(3, 1, 8, 65600), (3, 1, 8, 65535), (3, 1, 8, 3), (big, 4, 64, 5000), (big, 4, 64, 1), (10000000, 4, 64, 9), (9375, 4, 83, 5000),
              (300, 1, 4095, 10), (300, 1, 4096, 10), (300, 2, 2047, 10), (300, 2, 2048, 10), (300, 3, 1170, 10), (300, 3, 1171, 10)]
             for g in (0, 1)]
    sides = set()
    for (K, S, nbins, n_sel, g), w in zip(cases, _ask(driver, ["B %d %d %d %d %d" % c for c in cases])):
        P = S * (S + 1) // 2
        rho_frame, n_ctr = K * S * 16, (P + 1) * nbins + 1
        nb_max = max(1, min(SQ_RHO_BUDGET // rho_frame, n_sel, GRID_Y))
        glob = n_ctr * 8 > LDS_BUDGET or bool(g)
        assert [int(x) for x in w[:5]] == [nb_max, rho_frame, n_ctr, int(glob), 0 if glob else n_ctr * 8], (K, S, nbins, n_sel, g)
        assert w[5] == ("sq_bin_global" if glob else "sq")
        assert nb_max <= GRID_Y and nb_max <= n_sel and (nb_max == 1 or nb_max * rho_frame <= SQ_RHO_BUDGET)
        if not g:
            sides.add((S, nbins, glob))
    assert {(1, 4095, False), (1, 4096, True), (2, 2047, False), (2, 2048, True), (3, 1170, False), (3, 1171, True)} <= sides
    nb = {c[:4]: int(w[0]) for c, w in zip(cases, _ask(driver, ["B %d %d %d %d %d" % c for c in cases], keep=False))}
    assert nb[(3, 1, 8, 65600)] == GRID_Y and nb[(3, 1, 8, 3)] == 3 and nb[(big, 4, 64, 5000)] == 2 and nb[(10000000, 4, 64, 9)] == 1
    blocks = [(1, 1), (1, 256), (1, 257), (1024, 256), (1025, 256), (GRID_Y, 10000000)]
    for (n, K), w in zip(blocks, _ask(driver, ["N %d %d" % b for b in blocks])):
        assert int(w[0]) == min(SQ_BIN_BLOCKS, -(-n * K // SQ_THREADS))


def test_switches_are_read_from_the_environment(driver):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("AMOF_")}

    def ask(**env):
        r = subprocess.run([driver], input="V\n", capture_output=True, text=True, timeout=60, env=dict(clean, **env))
        assert r.returncode == 0
        return [int(x) for x in r.stdout.split()]

    assert ask() == [0, 0, ISF_RHO_BUDGET]
    assert ask(AMOF_SQ_GLOBAL="1") == [1, 0, ISF_RHO_BUDGET] and ask(AMOF_ISF_GLOBAL="0") == [0, 1, ISF_RHO_BUDGET]     # "set"
    assert ask(AMOF_ISF_RHO_BUDGET=str(576 * 40)) == [0, 0, 576 * 40]
    for ignored in ("0", "-5", "abc", ""):
        assert ask(AMOF_ISF_RHO_BUDGET=ignored) == [0, 0, ISF_RHO_BUDGET]


# ------------------------------------------------------------------------------------ F(q, t): touched frames --
def _lag_ranges(windows, F, stride, wb, we):
    first, out = 0, []
    for m in windows:
        n = (F - m - 2) // stride + 1 if F - m - 2 >= 0 else 0
        o0, o1 = max(wb - first, 0), min(we - first, n)
        out.append((o0, o1) if o0 < o1 else (0, 0))
        first += n
    return out, first


def _touched_cases():
    cases = []
    for F, windows in ((12, [0, 1, 2, 5]), (10, [0, 1, 3, 4]), (30, [4]), (9, [0, 8, 3]), (40, [0, 7, 38, 39, 2])):    # (a lag without origins)
        for stride in (1, 3):
            total = _lag_ranges(windows, F, stride, 0, 0)[1]
            for wb, we in {(0, total), (0, total // 2 + 1), (total // 2 + 1, total), (1, 2), (total // 3, 2 * total // 3), (0, 0)}:
                cases.append((windows, F, stride, wb, we))
    return cases


def test_touched_frames_and_slots_against_numpy(driver):
    cases = _touched_cases()
    lines = ["T %d %d %d %d %d %s" % (len(w), F, stride, wb, we, _ints(w)) for w, F, stride, wb, we in cases]
    inside = empty_lag = 0
    for (windows, F, stride, wb, we), w in zip(cases, _ask(driver, lines)):
        v = [int(x) for x in w]
        iv, total = _lag_ranges(windows, F, stride, wb, we)
        live = [(o0, o1) for o0, o1 in iv if o0 < o1]
        n_sel = v[3]
        fsel, slot_of, rest = v[4:4 + n_sel], np.array(v[4 + n_sel:4 + n_sel + F]), v[4 + n_sel + F:]
        assert v[0] == total and v[1] == (min(o0 for o0, _ in live) if live else I32_MAX) and v[2] == (max(o1 for _, o1 in live) if live else 0)
        touched = np.zeros(F, dtype=bool)
        entries = []
        for lag, (m, (o0, o1)) in enumerate(zip(windows, iv)):
            k = 1 + stride * np.arange(o0, o1)
            touched[k] = True
            touched[k + m] = True
            entries += [(lag, int(x)) for x in k]
        want_sel = np.flatnonzero(touched)
        assert fsel == list(want_sel)                                           # ascending
        want_slot = np.full(F, -1)
        want_slot[want_sel] = np.arange(len(want_sel))                          # dense, untouched frames -1
        assert np.array_equal(slot_of, want_slot)
        assert rest[0] == len(entries) == sum(o1 - o0 for o0, o1 in iv)
        got = [tuple(rest[1 + 4 * i:5 + 4 * i]) for i in range(rest[0])]
        assert got == [(lag, k, want_slot[k], want_slot[k + windows[lag]]) for lag, k in entries]
        inside += any(0 < o0 or o1 < (F - m - 2) // stride + 1 for m, (o0, o1) in zip(windows, iv) if o0 < o1)
        empty_lag += any(o0 == o1 for o0, o1 in iv) and bool(live)
    assert inside > 5 and empty_lag > 5


# ------------------------------------------------------------------------------------------- F(q, t): chunks --
def _hkl_of_runs(lengths, rng=None):
    """a list whose sorted order has exactly these run lengths (<= 16 each): one row per run"""
    hkl = sum((_row(i - len(lengths) // 2, 3, -2, n) for i, n in enumerate(lengths)), [])
    return [hkl[i] for i in rng.permutation(len(hkl))] if rng is not None else hkl


def _chunks(run_n, kc_max):
    chunks, r0, n = [], 0, len(run_n)
    while r0 < n:
        r1 = r0
        nv = 0
        while r1 < n and (r1 == r0 or nv + run_n[r1] <= kc_max):
            nv += run_n[r1]
            r1 += 1
        if r1 < n and r1 - r0 > 64:
            while (r1 - r0) % 64:
                r1 -= 1
                nv -= run_n[r1]
        chunks.append((r0, r1, sum(run_n[:r0]), nv))
        r0 = r1
    return chunks


def _chunk_cases():
    """(name, slots, S, budget, hkl)"""
    rng = np.random.default_rng(5)
    vec = 9 * 4 * 16
    cases = [("first_run_too_big", 9, 4, vec * 5, _hkl_of_runs([16, 16, 3, 16])),
             ("on_a_boundary", 9, 4, vec * 32, _hkl_of_runs([16, 16, 16, 16, 5])),
             ("one_short_of_it", 9, 4, vec * 31, _hkl_of_runs([16, 16, 16, 16, 5]))]
    for n_runs in (64, 65, 128, 129, 200):
        lengths = [int(x) for x in rng.integers(1, 17, n_runs)]
        hkl = _hkl_of_runs(lengths, rng)
        cases.append(("all_%d" % n_runs, 9, 4, vec * len(hkl), hkl))
        cases.append(("about100_%d" % n_runs, 9, 4, vec * sum(lengths[:100]), hkl))
        cases.append(("full_runs_%d" % n_runs, 3, 2, 3 * 2 * 16 * 16 * 100, _hkl_of_runs([16] * n_runs)))
    # tests/test_gpu_isf.py::test_invariances_bit_for_bit under AMOF_ISF_RHO_BUDGET = 576 * 40
    packed = H.random_walk(H.zif4_frame(), 10, 0.05, 37, cell_jitter=0.01)
    cases.append(("gpu_test", 9, 4, 576 * 40, [tuple(int(x) for x in v) for v in sf.enumerate_hkl(packed.cell, 2.5)]))
    cases.append(("default_budget", 5000, 4, ISF_RHO_BUDGET, _hkl_of_runs([16] * 600)))
    return cases


def test_chunks_partition_the_runs(driver):
    cases = _chunk_cases()
    out = _ask(driver, ["H %d %d %d %d %s" % (slots, S, budget, len(hkl), _ints(hkl)) for _, slots, S, budget, hkl in cases])
    n_chunks = {}
    for (name, slots, S, budget, hkl), w in zip(cases, out):
        v = [int(x) for x in w]
        vec_bytes, kc_max, kc_top, n_runs = v[:4]
        run_n, rest = v[4:4 + n_runs], v[4 + n_runs:]
        chunks, order_local = [tuple(rest[1 + 4 * i:5 + 4 * i]) for i in range(rest[0])], rest[1 + 4 * rest[0]:]
        assert vec_bytes == slots * S * 16 and kc_max == max(1, budget // vec_bytes), name
        assert run_n == [r[3] for r in _cut_runs(hkl)[0]] and len(order_local) == len(hkl), name
        assert chunks == _chunks(run_n, kc_max), name
        pos = v0 = 0
        for i, (r0, r1, start, nv) in enumerate(chunks):                    # the runs in order, none left out
            assert r0 == pos and r1 > r0 and start == v0 and nv == sum(run_n[r0:r1]), name
            assert nv <= kc_max or r1 - r0 == 1, name
            if r1 - r0 > 64 and i < len(chunks) - 1:
                assert (r1 - r0) % 64 == 0, name                           # whole waves of runs
            assert order_local[start:start + nv] == list(range(nv)), name  # the chunk's vectors from 0 upward
            pos, v0 = r1, v0 + nv
        assert pos == n_runs and v0 == len(hkl) and kc_top == max(c[3] for c in chunks), name
        n_chunks[name] = len(chunks)
    assert n_chunks["first_run_too_big"] == 4 and n_chunks["on_a_boundary"] == 3 and n_chunks["one_short_of_it"] == 4
    assert all(n_chunks["all_%d" % n] == 1 for n in (64, 65, 128, 129, 200))
    # 100 full runs fit: a chunk of more than 64 runs that is not the last is trimmed to 64 (200: 64, 64, 72)
    assert [n_chunks["full_runs_%d" % n] for n in (64, 65, 128, 129, 200)] == [1, 1, 2, 2, 3]
    # the headline's frame count: 209 runs fit 1 GiB, three whole waves of runs per chunk (192, 192, 192, 24)
    assert n_chunks["gpu_test"] >= 3 and n_chunks["default_budget"] == 4


# ------------------------------------------------------------------- F(q, t): counter tiles, grid, self batch --
def test_lags_per_pass_and_the_lds_choice(driver):
    cases = [(S, nbins, W, g) for S, nbins in ((1, 4096), (1, 4097), (2, 1638), (2, 1639), (1, 100), (4, 83), (3, 819), (3, 820), (5, 200))
             for W in (1, 4, 8, 64) for g in (0, 1)]
    seen = set()
    for (S, nbins, W, g), w in zip(cases, _ask(driver, ["P %d %d %d %d" % c for c in cases])):
        tile = (1 + S * S) * nbins
        glob = tile * 8 > LDS_BUDGET or bool(g)
        lpp = W if glob else min(W, LDS_BUDGET // (tile * 8))
        assert [int(x) for x in w[:4]] == [tile, int(glob), lpp, lpp * tile * 8] and w[4] == ("isf_global" if glob else "isf"), (S, nbins, W, g)
        assert glob or (1 <= lpp <= W and lpp * tile * 8 <= LDS_BUDGET)
        if not g:
            seen.add((S, nbins, glob, lpp < W))
    assert {(1, 4096, False, True), (1, 4097, True, False), (2, 1638, False, True), (2, 1639, True, False)} <= seen
    assert (1, 100, False, False) in seen and (1, 100, False, True) in seen        # W below and above what fits (40 lags)


def test_grid_covers_the_origins_within_the_launch_limits(driver):
    ranges = [1, 3, 4, 5, 63, 64, 65, 4096, GRID_Y * 64, GRID_Y * 64 + 1, I32_MAX]
    cases = [(nv, r) for r in ranges for vb in (1, 2, 40) for nv in (256 * (vb - 1) + 1, 256 * vb)]
    beyond = 0
    for (nv, rng_), w in zip(cases, _ask(driver, ["G %d %d" % c for c in cases])):
        vblocks, opw, gy = (int(x) for x in w)
        assert vblocks == -(-nv // ISF_THREADS)
        want = min(ISF_OPW, max(ISF_TILE, rng_ * vblocks // 2048 // ISF_TILE * ISF_TILE))
        want = max(want, -(-(-(-rng_ // GRID_Y)) // ISF_TILE) * ISF_TILE)
        assert opw == want and gy == -(-rng_ // opw), (nv, rng_)
        assert opw % ISF_TILE == 0 and opw >= ISF_TILE and gy * opw >= rng_ and 1 <= gy <= GRID_Y, (nv, rng_)
        assert opw <= ISF_OPW or rng_ > GRID_Y * ISF_OPW, (nv, rng_)
        beyond += opw > ISF_OPW
    assert beyond == 12


def test_self_batch_size(driver):
    cases = [(ISF_RHO_BUDGET, 2, 3, 1, 65599), (ISF_RHO_BUDGET, 2, 3, 1, 65535), (ISF_RHO_BUDGET, 272, 9375, 4, 30000), (576 * 40, 272, 226, 4, 26),
             (1, 272, 226, 4, 26), (ISF_RHO_BUDGET, 0, 5, 2, 7), (ISF_RHO_BUDGET, 1000, 3000, 3, 2000)]
    got = [int(w[0]) for w in _ask(driver, ["F %d %d %d %d %d" % c for c in cases])]
    for (budget, N, K, S, n), nb in zip(cases, got):
        assert nb == max(1, min(budget // (max(N, 1) * 16 + K * S * 16), n, GRID_Y))
    assert got[:2] == [GRID_Y, GRID_Y] and got[3] == 1 and got[4] == 1 and got[5] == 7 and 1 < got[2] < 30000


def test_one_pass_plan_and_one_grid_rule_serve_both_correlation_kernels(driver, tmp):
    """lag_pass_plan and lag_grid (sq_plan.h), asked directly and through F(q, t)'s driver line (one sum per pair, origin tile
    ISF_TILE) and C(q, t)'s (two sums per pair, tile 1): all three against the rule restated once"""
    out = str(tmp / "current_plan_driver")
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O1", os.path.join(ROOT, "tests", "native", "current_plan_driver.cpp"),
                        "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    forms = ((driver, True, 1, ISF_TILE, "isf"), (out, False, 2, 1, "current"))

    def grid(nv, rng_, tile):
        vblocks = -(-nv // ISF_THREADS)
        opw = min(ISF_OPW, max(tile, rng_ * vblocks // 2048 // tile * tile))
        opw = max(opw, -(-(-(-rng_ // GRID_Y)) // tile) * tile)
        return [vblocks, opw, -(-rng_ // opw)]

    cases = [(nv, r) for nv in (1, 255, 256, 257, 70000) for r in (1, 3, 4, 5, 63, 64, 65, 1000, GRID_Y * 64 + 1)]
    for exe, keep, _, tile, _ in forms:
        direct = _ask(driver, ["L %d %d %d" % (c + (tile,)) for c in cases])      # lag_grid itself
        for (nv, rng_), w, d in zip(cases, _ask(exe, ["G %d %d" % c for c in cases], keep=keep), direct):
            got = [int(x) for x in w]
            assert got == grid(nv, rng_, tile) and w == d, (tile, nv, rng_)
            assert got[2] <= GRID_Y and got[2] * got[1] >= rng_ and got[1] % tile == 0, (tile, nv, rng_)

    cases = [(S, nbins, W, 0) for S in (1, 2, 4, 5) for nbins in (1, 100, 911, 912, 8192) for W in (0, 1, 7, 300)]
    seen = set()
    for exe, keep, sums, _, name in forms:
        direct = _ask(driver, ["Q %d %d %d %d %d" % ((sums,) + c) for c in cases])   # lag_pass_plan itself
        for (S, nbins, W, g), w, d in zip(cases, _ask(exe, ["P %d %d %d %d" % c for c in cases], keep=keep), direct):
            tile = (1 + sums * S * S) * nbins
            glob = tile * 8 > LDS_BUDGET
            lpp = W if glob else min(W, LDS_BUDGET // (tile * 8))
            assert [int(x) for x in w[:4]] == [tile, int(glob), lpp, lpp * tile * 8] and w[4] == (name + "_global" if glob else name), (name, S, nbins, W)
            assert w[:4] == d[:4] and d[4] == ("glob" if glob else "lds"), (name, S, nbins, W)
            assert glob or int(w[3]) <= 65536, (name, S, nbins, W)
            assert glob or W < 1 or int(w[2]) >= 1, (name, S, nbins, W)
            seen.add((name, glob, lpp < W))
    assert seen == {(n, g, c) for n in ("isf", "current") for g, c in ((False, False), (False, True), (True, False))}


def test_driver_under_sanitizers(driver, tmp):
    san = _build(tmp, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "sq_plan_driver_san")
    if not ALL_LINES:                # (run alone: the tests above have not asked their questions yet)
        for test in (test_runs_tile_the_sorted_list, test_zero_vector_is_reported_by_index, test_species_order_against_numpy,
                     test_capacity_and_exponents_follow_the_restatement, test_sq_batch_plan,
                     test_touched_frames_and_slots_against_numpy, test_chunks_partition_the_runs, test_lags_per_pass_and_the_lds_choice,
                     test_grid_covers_the_origins_within_the_launch_limits, test_self_batch_size):
            test(driver)
    lines = list(ALL_LINES) + ["V"]
    r = subprocess.run([san], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    plain = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.stdout == plain.stdout and len(r.stdout.strip().splitlines()) == len(lines)
