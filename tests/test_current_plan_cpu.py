"""The host decisions of the current correlation functions have one definition (amof_amd/csrc/current_plan.h, here through
tests/native/current_plan_driver.cpp): the runs of CUR_RUN vectors, the fixed-point scales with vmax (vmax = 0 and the extreme
included), the vector chunks, the counter tiles and the grid -- each against a restatement in Python."""

import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "current_plan_driver.cpp")
LDS_BUDGET, RHO_BUDGET, THREADS, OPW = 64 * 1024, 1 << 30, 256, 64


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("curp") / "current_plan_driver")
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O1", "-Wall", SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def _ask(driver, lines, env=None):
    full = dict(os.environ, **env) if env else None
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=full)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.strip().splitlines()
    assert len(out) == len(lines)
    return [l.split() for l in out]


def _ints(x):
    return " ".join(str(int(v)) for v in np.asarray(x).ravel())


@pytest.fixture(scope="module")
def R(driver):
    k = _ask(driver, ["K"])[0]
    assert [int(x) for x in k[1:]] == [THREADS, 4, OPW, LDS_BUDGET, RHO_BUDGET]
    return int(k[0])


def _row(h, k, l0, n):
    return [(h, k, l0 + i) for i in range(n)]


def _cut_runs(hkl, R):
    """the rule, restated: sort by (h, k, l, caller's index); a run goes on while (h, k) stay, l is the next and n < R"""
    order = sorted(range(len(hkl)), key=lambda i: (hkl[i][0], hkl[i][1], hkl[i][2], i))
    runs = []
    for pos, i in enumerate(order):
        h, k, l = hkl[i]
        if runs and runs[-1][3] < R and runs[-1][0] == h and runs[-1][1] == k and runs[-1][2] + runs[-1][3] == l:
            runs[-1][3] += 1
        else:
            runs.append([h, k, l, 1, pos])
    return runs, order


def test_constants_follow_the_register_budget(R):
    """six f32 partials and six f64 sums per vector: 18 VGPRs; the run must leave room for two waves per SIMD at least"""
    assert 1 <= R <= 8 and 18 * R <= 256 - 64


def test_runs(driver, R):
    rng = np.random.default_rng(3)
    cases = {"len1": _row(2, -1, 5, 1), "lenR": _row(2, -1, 5, R), "lenR1": _row(2, -1, 5, R + 1), "len3R2": _row(0, 1, -4, 3 * R + 2),
             "gap": _row(1, 1, 0, 3) + _row(1, 1, 5, 2), "duplicate": [(1, 2, 3), (1, 2, 4), (1, 2, 4), (1, 2, 5), (1, 2, 3)],
             "across0": _row(0, 3, -7, 15), "int32": [(1, 0, 2 ** 31 - 1), (1, 0, 2 ** 31 - 2), (1, 0, -2 ** 31)]}
    many = [v for h in range(-2, 3) for k in range(-2, 3) for v in _row(h, k, -5, 11 + h) if v != (0, 0, 0)]
    cases["many"] = many
    cases["many_shuffled"] = [many[i] for i in rng.permutation(len(many))]
    names = list(cases)
    out = _ask(driver, ["R %d %s" % (len(cases[n]), _ints(cases[n])) for n in names])
    for name, got in zip(names, out):
        hkl = cases[name]
        runs, order = _cut_runs(hkl, R)
        g = [int(x) for x in got]
        assert g[0] == -1 and g[1] == len(runs), name
        assert np.array(g[2:2 + 5 * len(runs)]).reshape(-1, 5).tolist() == runs, name
        assert g[2 + 5 * len(runs):] == order, name
        assert sum(r[3] for r in runs) == len(hkl) and max(r[3] for r in runs) <= R
    assert len(_cut_runs(cases["lenR"], R)[0]) == 1 and len(_cut_runs(cases["lenR1"], R)[0]) == 2
    zero = _ask(driver, ["R 3 1 0 0 0 0 0 2 2 2"])[0]
    assert int(zero[0]) == 1


def _scales(S, species, F, cap, vmax):
    nsp = np.bincount(species, minlength=S)
    sexp, bad = [], -1
    for a in range(S):
        for c in range(a, S):
            if not vmax > 0:
                sexp.append(0)
                continue
            na, nc = max(int(nsp[a]), 1), max(int(nsp[c]), 1)
            v2 = 3.0 * vmax * vmax
            bound = float(max(F, 1)) * float(max(cap, 1)) * (float(na) * float(nc) + 0.5) * v2
            e = math.frexp(bound)[1]
            s = min(62 - e, 1000)
            sexp.append(s)
            if bad < 0 and math.ldexp(1.0, -s) / (math.sqrt(float(na) * float(nc)) * v2) > 2.0 ** -20:
                bad = len(sexp) - 1
    return nsp, sexp, bad


@pytest.mark.parametrize("vmax", [0.0, 1e-3, 0.37, 1.0, 250.0, 1e-30])
def test_scales(driver, vmax):
    rng = np.random.default_rng(5)
    S, N, F, cap = 3, 400, 200, 17
    species = rng.integers(0, S, size=N)
    got = _ask(driver, ["E %d %d %d %d %.17g %s" % (S, N, F, cap, vmax, _ints(species))])[0]
    nsp, sexp, bad = _scales(S, species, F, cap, vmax)
    P = S * (S + 1) // 2
    assert int(got[0]) == bad == -1
    assert [int(x) for x in got[3:3 + S]] == nsp.tolist()
    assert [int(x) for x in got[3 + S:3 + S + P]] == sexp
    scale = [float(x) for x in got[3 + S + P:3 + S + 2 * P]]
    if vmax == 0.0:
        assert scale == [0.0] * P and sexp == [0] * P       # zero sums, scale 0
        return
    assert scale == [math.ldexp(1.0, s) for s in sexp]
    # no overflow at the extreme: every sample at the bound, every counter full
    p = 0
    for a in range(S):
        for c in range(a, S):
            worst = F * cap * (3.0 * vmax * vmax * float(nsp[a]) * float(nsp[c]) * scale[p] + 0.5)
            assert 2.0 ** 60 <= worst < 2.0 ** 63, (a, c)
            assert math.ldexp(1.0, -sexp[p]) <= 2.0 ** -20 * 3.0 * vmax * vmax      # the quantum follows vmax^2
            p += 1
    sexp2 = np.array([int(x) for x in got[3 + S + 2 * P:3 + S + 2 * P + S * S]]).reshape(S, S)
    assert np.array_equal(sexp2, sexp2.T) and sexp2[0, 1] == sexp[1] and sexp2[1, 1] == sexp[S]


def test_scale_refuses_a_quantum_above_the_resolution(driver):
    """F cap sqrt(N_a N_c) beyond 2^42: the quantum exceeds 2^-20 of the pair's natural size"""
    S, N = 1, 1024
    species = np.zeros(N, dtype=int)
    ok = _ask(driver, ["E %d %d %d %d 0.01 %s" % (S, N, 4200, 400000, _ints(species))])[0]
    bad = _ask(driver, ["E %d %d %d %d 0.01 %s" % (S, N, 4200, 2400000, _ints(species))])[0]
    assert int(ok[0]) == -1 and [int(x) for x in bad[:3]] == [0, 0, 0]
    assert _scales(S, species, 4200, 400000, 0.01)[2] == -1 and _scales(S, species, 4200, 2400000, 0.01)[2] == 0


def test_chunks(driver, R):
    hkl = [v for h in range(0, 4) for k in range(-3, 4) for v in _row(h, k, -6, 13) if v != (0, 0, 0)]
    runs, _ = _cut_runs(hkl, R)
    slots, S = 9, 4
    vec_bytes = slots * S * 6 * 8
    for budget in (RHO_BUDGET, vec_bytes * 40, vec_bytes * 1, vec_bytes * 7 + 3):
        got = [int(x) for x in _ask(driver, ["H %d %d %d %d %s" % (slots, S, budget, len(hkl), _ints(hkl))])[0]]
        assert got[0] == vec_bytes and got[1] == max(1, budget // vec_bytes)
        n_chunks = got[3]
        chunks = np.array(got[4:4 + 4 * n_chunks]).reshape(-1, 4)
        local = got[4 + 4 * n_chunks:]
        assert chunks[0, 0] == 0 and chunks[-1, 1] == len(runs) and (chunks[1:, 0] == chunks[:-1, 1]).all()
        for r0, r1, v0, nv in chunks:
            assert nv == sum(r[3] for r in runs[r0:r1]) and v0 == runs[r0][4]
            assert nv <= got[1] or r1 - r0 == 1                    # inside the budget, or a single run
            assert local[v0:v0 + nv] == list(range(nv))
        assert got[2] == chunks[:, 3].max()
        assert (n_chunks == 1) == (budget == RHO_BUDGET)


def test_tiles_and_grid(driver):
    lines, want = [], []
    for S, nbins, W, glob in [(1, 100, 7, 0), (4, 100, 50, 0), (4, 248, 3, 0), (4, 249, 3, 0), (5, 30, 4, 0), (2, 10, 6, 1), (1, 3000, 2, 0)]:
        tile = (1 + 2 * S * S) * nbins
        g = tile * 8 > LDS_BUDGET or bool(glob)
        lpp = W if g else min(W, LDS_BUDGET // (tile * 8))
        lines.append("P %d %d %d %d" % (S, nbins, W, glob))
        want.append([str(tile), str(int(g)), str(lpp), str(lpp * tile * 8), "current_global" if g else "current"])
        assert g or lpp >= 1
    assert _ask(driver, lines) == want
    cases = [(1, 1), (300, 5), (5000, 99), (70000, 4999), (256, 10 ** 7), (257, 64)]
    got = _ask(driver, ["G %d %d" % c for c in cases])
    for (nv, rng), g in zip(cases, got):
        vb, opw, gy = (int(x) for x in g)
        assert vb == (nv + THREADS - 1) // THREADS
        assert opw == max(min(OPW, max(1, rng * vb // 2048)), (rng + 65534) // 65535)
        assert gy == (rng + opw - 1) // opw and gy <= 65535 and gy * opw >= rng


def test_switches(driver):
    assert _ask(driver, ["V"], env={"AMOF_CURRENT_GLOBAL": "", "AMOF_CURRENT_RHO_BUDGET": ""}) [0][1] == str(RHO_BUDGET)
    env = {k: v for k, v in os.environ.items() if not k.startswith("AMOF_CURRENT")}
    r = subprocess.run([driver], input="V\n", capture_output=True, text=True, env=env)
    assert r.stdout.split() == ["0", str(RHO_BUDGET)]
    assert _ask(driver, ["V"], env={"AMOF_CURRENT_GLOBAL": "1", "AMOF_CURRENT_RHO_BUDGET": "4096"})[0] == ["1", "4096"]
    assert _ask(driver, ["V"], env={"AMOF_CURRENT_RHO_BUDGET": "-5"})[0][1] == str(RHO_BUDGET)
