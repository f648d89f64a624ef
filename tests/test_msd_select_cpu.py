"""The host decisions of the window-MSD entry point have one definition (amof_amd/csrc/msd_select.h, here through
tests/native/msd_select_driver.cpp): which form and kernel family answers a call, the template buckets, the LDS bytes --
pinned on the CPU for the very shapes whose GPU tests assert a path (tests/helpers.py: msd_path_case), at the edges of
every rule against a restatement of the rules in Python, and as invariants over a sweep; species_groups against numpy.  The
same driver runs once more under the address and undefined-behaviour sanitizers."""

import os
import subprocess

import numpy as np
import pytest

from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "msd_select_driver.cpp")
SWITCHES = ("nocomb", "nofused", "nostream", "nofold", "nodb", "fused_general")
PLAN_KEYS = ("resident", "comb_d", "fused", "fused_general", "fd_d", "fd_nq", "fd_TPC", "fd_L", "fd_threads", "fd_lds", "columns",
             "family", "stream_L", "stream_T", "regscan", "comb_WT", "db", "WREG", "Rres", "nq", "wchunks", "lds")
FOLD, THREE_PASS, UNWRAP = 0, 1, 2                              # MsdColumns
STREAM, COMB, GROUP, COMB_GLOBAL, GLOBAL = 0, 1, 2, 3, 4        # MsdFamily
SERIES, DB = 150 * 1024, 80 * 1024                              # the LDS budgets
W_EDGES = (4, 5, 8, 9, 16, 17, 24, 25, 26, 28, 29, 32, 33, 40, 64, 65, 128, 129)
D_EDGES = (15, 16, 63, 64, 128, 129, 256, 257)
VH_GROUP = 8                                                    # vanhove.hip


def _build(tmp, flags, name):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags + [SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("ms")


@pytest.fixture(scope="module")
def driver(tmp):
    return _build(tmp, ["-O1"], "msd_select_driver")


def _ask(driver, lines, timeout=300):
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.strip().splitlines()
    assert len(out) == len(lines)
    return [l.split() for l in out]


# ---- a question: one call ----
def _call(F, N, window=None, d=0, W=0, unwrap=False, remove_com=True, com_ext=False, ortho=True, a0=0, a1=None, n_groups=None,
          sw=()):
    """windows w d, w < W, that lie inside the trajectory (what WindowMsd produces), or the listed ones"""
    if window is None:
        W = min(W, -(-F // d))
        window = None if W >= 2 else [0]            # (F <= d leaves one window: no spacing)
    else:
        d, W = 0, len(window)
    a1 = N if a1 is None else a1
    n_groups = -(-(a1 - a0) // 4) if n_groups is None else n_groups
    return dict(F=F, N=N, window=window, d=d, W=W, unwrap=unwrap, remove_com=remove_com, com_ext=com_ext, ortho=ortho, a0=a0, a1=a1,
                n_groups=n_groups, sw=tuple(sw))


def _line(c):
    listed = c["window"] is not None
    return "P %d %d %d %d %d %d %d %d %d %d %d %s | %s ;" % (
        c["F"], c["N"], c["unwrap"], c["remove_com"], c["com_ext"], c["ortho"], c["a0"], c["a1"], c["n_groups"], c["W"],
        0 if listed else c["d"], " ".join(str(int(w)) for w in c["window"]) if listed else "", " ".join(c["sw"]))


def _parse(w):
    p = dict(zip(PLAN_KEYS, (int(x) for x in w[:len(PLAN_KEYS)])))
    p["path"] = w[len(PLAN_KEYS)]
    rest = [int(x) for x in w[len(PLAN_KEYS) + 1:]]
    assert len(rest) == 1 + 3 * rest[0]
    p["comb_hi"] = [tuple(rest[1 + 3 * k:4 + 3 * k]) for k in range(rest[0])]
    return p


def _plans(driver, calls):
    return [_parse(w) for w in _ask(driver, [_line(c) for c in calls])]


def _last_path(p, hands_over):
    """what amof_last_path answers; hands_over: a column comes within the centre-of-mass step of half the cell"""
    return "msd_fused" if p["fused"] and not hands_over else p["path"]


# ---- the rules of the issue, restated ----
def _spacing(c):
    if c["window"] is None:
        return c["d"]
    w = [int(x) for x in c["window"]]
    if len(w) < 2 or w[0] != 0 or w[1] <= 0 or any(w[k] != k * w[1] for k in range(len(w))):
        return 0
    return w[1]


def _rules(c):
    F, N, W, sw = c["F"], c["N"], c["W"], c["sw"]
    Fp = -(-F // 32) * 32
    p = dict.fromkeys(PLAN_KEYS, 0)
    p["comb_hi"] = []
    resident = (F + W) * 8 <= SERIES
    d = _spacing(c) if W <= (128 if resident else 256) and "nocomb" not in sw else 0
    raw_com = not c["unwrap"] and c["remove_com"] and not c["com_ext"] and c["ortho"] and c["a0"] == 0 and c["a1"] == N
    nq = -(-F // d) if d else 0
    fused = raw_com and "nofused" not in sw and d >= 16 and 2 <= W <= 32 and F >= 64 and -(-nq // 5) <= 21
    p.update(resident=int(resident), comb_d=d, fused=int(fused))
    if fused:
        TPC = -(-nq // 5)
        L = 7 if W <= 8 else 15 if W <= 16 else 24 if W <= 25 else 31
        p.update(fused_general=int(nq % 5 != 0 or F % d != 0 or "fused_general" in sw), fd_d=d, fd_nq=nq, fd_TPC=TPC, fd_L=L,
                 fd_threads=-(-TPC * 24 // 64) * 64, fd_lds=2 * (L + TPC * 5) * 24 * 8)
    stream = resident and 64 <= d <= 256 and W <= 32 and Fp * 8 <= SERIES and "nostream" not in sw
    T = 128 if d <= 128 else 256
    regscan = (-(-F // T) | 1) <= 42
    fold = raw_com and resident and not (stream and not regscan) and "nofold" not in sw
    p.update(stream_T=T, regscan=int(regscan), columns=FOLD if fold else UNWRAP if c["unwrap"] else THREE_PASS)
    if stream:
        p.update(family=STREAM, stream_L=7 if W <= 8 else 15 if W <= 16 else 23 if W <= 24 else 24 if W <= 25 else 31, lds=Fp * 8,
                 path="msd_stream")
    elif resident and d > 0:
        db = 2 * Fp * 8 <= DB and "nodb" not in sw
        p.update(family=COMB, comb_WT=min(-(-W // 4) * 4, 32), db=int(db), lds=2 * Fp * 8 if db else F * 8, path="msd_comb")
        for w0 in range(32, W, 32):
            wn = min(32, W - w0)
            p["comb_hi"].append((w0, wn, 8 if wn <= 8 else 16 if wn <= 16 else 32))
    elif resident:
        p.update(family=GROUP, WREG=8 if W <= 8 else 32 if W <= 32 else 0, lds=(F + W) * 8, path="msd_group")
    else:
        Rres = min(d, 32, 16384 // nq) if d else 0
        p.update(nq=nq, Rres=Rres)
        if Rres >= 1:
            p.update(family=COMB_GLOBAL, lds=nq * Rres * 8, path="msd_comb_global")
        else:
            p.update(family=GLOBAL, wchunks=min(65535, max(1, min(W, -(-4096 // c["n_groups"])))), path="msd_global")
    return p


# ---- the shapes whose GPU tests assert a path ----
def _path_calls():
    """[(name, call, path the GPU test asserts, its trajectory hands over)]: every case of the table with every switch set its
    GPU test runs it under"""
    out = []
    for kind in ("comb", "fused", "fused_other", "long", "two_pass", "headline"):
        for key, case in H.msd_path_case(kind).items():
            a0, a1 = case["atom_range"] or (0, case["n"])
            for sw, path in case["paths"].items():
                out.append(((kind, key, sw), _call(case["F"], case["n"], window=list(case["window"]), unwrap=case["unwrap"],
                                                   ortho=case["diagonal"], a0=a0, a1=a1, sw=sw), path, case["hands_over"]))
    return out


def test_selection_takes_the_paths_the_gpu_tests_assert(driver):
    cases = _path_calls()
    assert len(cases) > 100
    for (name, call, path, hands_over), p in zip(cases, _plans(driver, [c[1] for c in cases])):
        assert _last_path(p, hands_over) == path, (name, p)
        want = _rules(call)
        assert p == want, (name, p, want)
        # each further switch, one at a time: still the rules (and the path moves only where the rules say so)
    more = [(name, dict(call, sw=call["sw"] + (s,))) for name, call, _, _ in cases for s in SWITCHES if s not in call["sw"]]
    for (name, call), p in zip(more, _plans(driver, [c for _, c in more])):
        assert p == _rules(call), (name, call["sw"], p)


def test_headline_shape_buckets(driver):
    head = H.msd_path_case("headline")["headline"]
    calls = [_call(head["F"], head["n"], window=list(head["window"]), sw=sw) for sw in ((), ("nofused",), ("nofused", "nostream"),
                                                                                          ("nofused", "nofold"), ("nocomb",))]
    fused, stream, comb, three_pass, group = _plans(driver, calls)
    assert fused["fused"] and not fused["fused_general"] and (fused["fd_L"], fused["fd_nq"], fused["fd_TPC"]) == (24, 50, 10)
    assert fused["fd_threads"] == 256 and fused["fd_lds"] == 2 * (24 + 50) * 24 * 8
    assert (stream["path"], stream["stream_L"], stream["stream_T"], stream["regscan"], stream["columns"]) == ("msd_stream", 24, 128, 1, FOLD)
    assert stream["lds"] == 5024 * 8
    assert (comb["path"], comb["comb_WT"], comb["db"], comb["columns"], comb["comb_hi"]) == ("msd_comb", 28, 1, FOLD, [])
    assert three_pass["columns"] == THREE_PASS and three_pass["path"] == "msd_stream"
    # AMOF_MSD_NOCOMB: no comb, and with it no fused form either
    assert (group["fused"], group["comb_d"], group["path"], group["WREG"]) == (0, 0, "msd_group", 32)


# ---- the bucket rules at their edges ----
def _edge_calls():
    calls = []
    for W in W_EDGES:
        for d in D_EDGES:
            for F in (63, 64, 5120, 5121, 5248, 5249, 19200 - W, 19201 - W):
                for sw in ((),) + tuple((s,) for s in SWITCHES):
                    calls.append(_call(F, 48, d=d, W=W, sw=sw))
                calls.append(_call(F, 48, d=d, W=W, ortho=False))
                calls.append(_call(F, 48, d=d, W=W, unwrap=True))
                calls.append(_call(F, 48, d=d, W=W, a0=8, a1=40))
    for F in (1680, 1681):          # nq = 105, 106 segments of 16 frames
        for W in (2, 8, 32):
            calls.append(_call(F, 48, d=16, W=W))
    # irregular windows, few and many; no centre of mass; an external one; long series with few groups and many
    for F in (330, 21000):
        for window in ([0], [0, 3, 50, 161], [5, 10, 15], list(range(0, 300)), [0, 7, 14, 22]):
            for kw in (dict(), dict(remove_com=False), dict(com_ext=True), dict(n_groups=1), dict(n_groups=5000)):
                calls.append(_call(F, 48, window=window, **kw))
    for d, W in H.MSD_LONG_COMBS + [(1, 200), (1, 300), (2, 256), (2, 257)]:
        calls.append(_call(21000, 48, d=d, W=W))
    return calls


def test_buckets_at_the_edges_follow_the_rules(driver):
    calls = _edge_calls()
    seen = set()
    for c, p in zip(calls, _plans(driver, calls)):
        want = _rules(c)
        assert p == want, (c, p, want)
        seen.add((p["family"], p["columns"], p["fused"], p["fused_general"], p["stream_L"], p["stream_T"], p["regscan"], p["comb_WT"],
                  p["db"], len(p["comb_hi"]), p["WREG"], p["fd_L"]))
    col = lambda k: {s[k] for s in seen}
    assert col(0) == {STREAM, COMB, GROUP, COMB_GLOBAL, GLOBAL} and col(1) == {FOLD, THREE_PASS, UNWRAP}
    assert col(4) == {0, 7, 15, 23, 24, 31} and col(5) == {128, 256} and col(7) == {0, 4, 8, 12, 16, 20, 24, 28, 32}
    assert col(9) >= {0, 1, 2, 3} and col(10) == {0, 8, 32} and col(11) == {0, 7, 15, 24, 31}
    assert {(s[2], s[3]) for s in seen} == {(0, 0), (1, 0), (1, 1)} and col(6) == {0, 1} and col(8) == {0, 1}
    assert any(s[0] == STREAM and not s[6] and s[1] == THREE_PASS for s in seen)        # stream without the register scan: no fold


def test_seg_shape_thresholds(driver):
    # work = atoms * nq against 4 * 64 * 1024 and 2 * 64 * 256
    cases = [(atoms, nq) for nq, edges in ((1, (262143, 262144, 262145, 32767, 32768, 32769)), (50, (5242, 5243, 655, 656)),
                                           (105, (2496, 2497, 312, 313))) for atoms in edges] + [(1, 1), (330, 100), (9792, 50)]
    for (atoms, nq), w in zip(cases, _ask(driver, ["Q %d %d" % c for c in cases])):
        tpl, U, ntiles = (int(x) for x in w)
        work = atoms * nq
        want = 4 if work >= 4 * 64 * 1024 else 2 if work >= 2 * 64 * 256 else 1
        assert (tpl, U, ntiles) == (want, 2 if want == 4 else 4, -(-atoms // (64 * want))), (atoms, nq, w)
    assert {4, 2, 1} == {4 if a * q >= 262144 else 2 if a * q >= 32768 else 1 for a, q in cases}


def test_comb_spacing_is_the_raw_progression_test(driver):
    lists = [[], [0], [0, 5], [0, 0], [5, 10], [0, 5, 10, 15], [0, 5, 10, 16], [1, 2, 3], [0, 1], list(range(0, 3000, 10)), [0, 7, 14, 22]]
    want = [0, 0, 5, 0, 0, 5, 0, 0, 1, 10, 0]
    got = [int(w[0]) for w in _ask(driver, ["C %d %s" % (len(l), " ".join(map(str, l))) for l in lists])]
    assert got == want


def test_wrap_half_lengths(driver):
    cells = np.array([np.diag([9.0, -10.5, 11.0]), np.diag([9.5, 10.0, 10.75])])
    for pbc in ((1, 1, 1), (1, 0, 1)):
        w = _ask(driver, ["H 2 %d %d %d %s" % (pbc + (" ".join("%.17g" % v for v in cells.ravel()),))])[0]
        want = [min(9.0, 9.5) * (0.5 - 1e-6), 10.0 * (0.5 - 1e-6), 10.75 * (0.5 - 1e-6)]
        for c in range(3):
            assert float(w[c]) == (want[c] if pbc[c] else 1e300)


# ---- invariants over a sweep ----
def _sweep_calls():
    frames = list(range(1, 601)) + [5120, 5121, 5248, 5249, 19000, 19136, 19200, 19201, 21000]
    return [_call(F, 48, d=d, W=W) for F in frames for W in W_EDGES for d in D_EDGES]


def test_invariants_over_a_sweep(driver):
    calls = _sweep_calls()
    families = set()
    for c, p in zip(calls, _plans(driver, calls)):
        F, W = c["F"], c["W"]
        Fp = -(-F // 32) * 32
        # exactly one family, and only its buckets are set
        assert p["family"] in (STREAM, COMB, GROUP, COMB_GLOBAL, GLOBAL), (c, p)
        assert p["path"] == ("msd_stream", "msd_comb", "msd_group", "msd_comb_global", "msd_global")[p["family"]], (c, p)
        assert (p["stream_L"] > 0) == (p["family"] == STREAM) and (p["comb_WT"] > 0) == (p["family"] == COMB), (c, p)
        assert (p["Rres"] > 0) == (p["family"] == COMB_GLOBAL) and (p["wchunks"] > 0) == (p["family"] == GLOBAL), (c, p)
        assert (p["family"] in (STREAM, COMB, GROUP)) == bool(p["resident"]), (c, p)
        assert not p["comb_hi"] or p["family"] == COMB, (c, p)
        if p["family"] == COMB:     # the passes cover [0, W) once, each within its bucket
            passes = [(0, min(W, 32), p["comb_WT"])] + p["comb_hi"]
            assert [w for w0, wn, _ in passes for w in range(w0, w0 + wn)] == list(range(W)), (c, p)
            assert all(0 < wn <= WT <= 32 for _, wn, WT in passes), (c, p)
        if p["family"] == STREAM:
            assert W <= p["stream_L"] + 1 and Fp * 8 <= SERIES and p["lds"] == Fp * 8, (c, p)
            assert 64 <= p["comb_d"] <= p["stream_T"], (c, p)
        if p["family"] == GROUP:
            assert p["WREG"] == 0 or W <= p["WREG"], (c, p)
        assert p["lds"] <= 160 * 1024, (c, p)
        if p["fused"]:
            assert 0 < p["fd_threads"] <= 512 and p["fd_threads"] % 64 == 0 and p["fd_threads"] >= p["fd_TPC"] * 24, (c, p)
            assert W <= p["fd_L"] + 1 and p["fd_lds"] <= 64 * 1024 and p["fd_TPC"] * 5 >= p["fd_nq"], (c, p)
        if p["columns"] == FOLD:
            assert p["resident"] and not (p["family"] == STREAM and not p["regscan"]), (c, p)
        families.add(p["family"])
    assert families == {STREAM, COMB, GROUP, COMB_GLOBAL}       # (msd_global needs irregular windows: the edge cases)


# ---- species_groups ----
def _group_cases():
    rng = np.random.default_rng(4)
    cases = []
    for N, S in ((1, 1), (7, 2), (40, 3), (272, 4), (1000, 5)):
        species = rng.integers(0, S, N)
        if S >= 3:
            species[species == 1] = 0           # an empty species
        for a0, a1 in ((0, N), (N // 3, N - N // 4), (N // 2, N // 2), (0, 1), (N - 1, N)):
            for gs in (4, VH_GROUP):
                cases.append((S, gs, a0, a1, species))
    return cases


def _group_line(S, gs, a0, a1, species):
    return "G %d %d %d %d %d %s" % (S, gs, a0, a1, len(species), " ".join(str(int(s)) for s in species))


def test_species_groups_against_numpy(driver):
    cases = _group_cases()
    for (S, gs, a0, a1, species), w in zip(cases, _ask(driver, [_group_line(*c) for c in cases])):
        v = [int(x) for x in w]
        n_perm, v = v[0], v[1:]
        perm, v = np.array(v[:n_perm], dtype=np.int64), v[n_perm:]
        n_groups, v = v[0], v[1:]
        groups, v = np.array(v[:3 * n_groups], dtype=np.int64).reshape(n_groups, 3), v[3 * n_groups:]
        group_first, atom_first = np.array(v[:S + 1]), np.array(v[S + 1:])
        assert len(atom_first) == S + 1
        ctx = (S, gs, a0, a1)
        # every atom of the range once, sorted by species, the order of the atoms kept within a species
        rng_atoms = np.arange(a0, a1)
        want_perm = rng_atoms[np.argsort(species[a0:a1], kind="stable")]
        assert np.array_equal(perm, want_perm), ctx
        counts = np.bincount(species[a0:a1], minlength=S) if a1 > a0 else np.zeros(S, dtype=np.int64)
        assert np.array_equal(atom_first, np.concatenate([[0], np.cumsum(counts)])), ctx
        assert np.array_equal(group_first, np.concatenate([[0], np.cumsum(-(-counts // gs))])), ctx
        # groups: in order, back to back, never across a species, full but for the last of a species
        assert n_groups == group_first[-1]
        for s in range(S):
            g = groups[group_first[s]:group_first[s + 1]]
            assert (g[:, 2] == s).all(), ctx
            assert np.array_equal(g[:, 0], atom_first[s] + gs * np.arange(len(g))), ctx
            assert (g[:-1, 1] == gs).all() and (len(g) == 0 or g[-1, 0] + g[-1, 1] == atom_first[s + 1]), ctx
            assert all((species[perm[st:st + n]] == s).all() and 0 < n <= gs for st, n, _ in g), ctx


def test_driver_under_sanitizers(tmp):
    san = _build(tmp, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "msd_select_driver_san")
    calls = [c[1] for c in _path_calls()] + _edge_calls() + _sweep_calls()
    lines = [_line(c) for c in calls] + [_group_line(*c) for c in _group_cases()]
    lines += ["Q 9792 50", "Q 1 1", "C 0", "C 1 0", "C 4 0 5 10 15", "H 1 1 1 0 9 0 0 0 10 0 0 0 11"]
    r = subprocess.run([san], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert len(r.stdout.strip().splitlines()) == len(lines)
