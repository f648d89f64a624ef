"""The partner window of a step of the slab-culled tile kernel has one definition (amof_amd/csrc/tile_plan.h, here through
tests/native/tile_plan_driver.cpp).  It is checked against brute force over the atoms' slabs: every partner whose slab
lies in the widened reach is inside a returned range; the ranges are whole quads, disjoint and inside the tile; they are
never wider than the search over sampled quads that the kernel runs without a plan; and a table of garbage still yields
in-tile ranges.  The same driver runs once more under the address and undefined-behaviour sanitizers."""

import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "tile_plan_driver.cpp")

N_SEG = 1100                                    # atoms of the species segment every table describes
COUNTS = (1, 3, 4, 5, 127, 128, 129, 512)
# centre slab ranges: both ends of the axis, one slab, a few slabs, wider than 1/16 of the axis (no f32 slab coordinates)
CENTRES = ((0, 0), (0, 3), (250, 255), (255, 255), (100, 110), (120, 140), (3, 250), (0, 255))
# cull_gap: culling off, less than a slab, reaches that wrap below 0 / above 255, the headline's share, reaches that cover
# (almost) everything
GAPS = (0, 1 << 20, 0x18000000, 0x50000000, 0x7a000000, 0x7fffffff, 0xffffffff)
M32 = 1 << 32


def _tables():
    rng = np.random.default_rng(4)
    out = {}
    out["random"] = rng.multinomial(N_SEG, np.full(256, 1 / 256.0))
    few = np.zeros(256)
    few[rng.choice(256, 20, replace=False)] = 1 / 20.0
    out["empty_slabs"] = rng.multinomial(N_SEG, few)
    one = np.zeros(256, dtype=np.int64)
    one[37] = N_SEG
    out["one_slab"] = one
    ends = np.zeros(256, dtype=np.int64)
    ends[0], ends[255] = 600, N_SEG - 600
    out["ends_only"] = ends
    lay = np.zeros(256)
    lay[[0, 1, 128, 129, 254, 255]] = 1 / 6.0
    out["layers"] = rng.multinomial(N_SEG, lay)
    return {k: np.concatenate([[0], np.cumsum(v)]).astype(np.int64) for k, v in out.items()}


def _build(tmp, flags, name):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17"] + flags + [SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("tp")


@pytest.fixture(scope="module")
def driver(tmp):
    return _build(tmp, ["-O1"], "tile_plan_driver")


def _reach(s_first, s_last, G):
    """the slabs inside the widened reach of the centres (None: no culling), and whether f32 slab coordinates hold"""
    wlo, whi = s_first << 24, (s_last << 24) | 0xffffff
    W = (whi - wlo) % M32
    if G == 0 or W + 2 * G + (2 << 24) >= M32:
        return None, False
    klo, khi = (wlo - G) % M32, (whi + G) % M32
    slo, shi = klo >> 24, khi >> 24
    s = np.arange(256)
    inside = (s >= slo) & (s <= shi) if klo <= khi else (s <= shi) | (s >= slo)
    return inside, W < (1 << 28) and G + W + (2 << 24) < (1 << 31)


def _sampled(slabs, s_first, s_last, G, own):
    """the quads the search over sampled quads visits (first / last partner of every quad, as the kernel's ballots)"""
    cnt = len(slabs)
    nq = (cnt + 3) // 4
    quads = np.arange(nq)
    wlo, whi = s_first << 24, (s_last << 24) | 0xffffff
    W = (whi - wlo) % M32
    rb0, re0, rb1, re1 = own, cnt, 0, 0
    if G != 0 and W + 2 * G + (2 << 24) < M32:
        klo, khi = (wlo - G) % M32, (whi + G) % M32
        slo, shi = klo >> 24, khi >> 24
        last, first = slabs[np.minimum(4 * quads + 3, cnt - 1)], slabs[4 * quads]
        ia, ib = np.flatnonzero(last >= slo), np.flatnonzero(first > shi)
        a_ = min(4 * int(ia[0]) if len(ia) else 4 * nq, cnt)
        b_ = min(4 * int(ib[0]) if len(ib) else 4 * nq, cnt)
        if klo <= khi:
            rb0, re0 = max(rb0, a_), b_
        elif b_ < a_:
            re0, rb1, re1 = b_, max(rb0, a_), cnt
    visit = np.zeros(nq, dtype=bool)
    if re0 > rb0:
        visit[rb0 // 4:(re0 + 3) // 4] = True
    if re1 > rb1:
        visit[rb1 // 4:(re1 + 3) // 4] = True
    return visit


def _cases():
    rng = np.random.default_rng(9)
    cases = []
    for name, start in _tables().items():
        for cnt in COUNTS:
            # a tile at the head of the segment, one at its end, and two that start and end inside a slab
            offs = {0, N_SEG - cnt, int(rng.integers(0, N_SEG - cnt + 1)), int(rng.integers(0, N_SEG - cnt + 1))}
            for toff in sorted(offs):
                for s_first, s_last in CENTRES:
                    for G in GAPS:
                        nsub = (cnt + 127) // 128
                        for diag, sub in [(0, 0)] + [(1, s) for s in range(nsub)]:
                            cases.append((name, start, toff, cnt, s_first, s_last, G, diag, sub))
    return cases


def _text(cases):
    lines, prev = [], None
    for name, start, toff, cnt, s_first, s_last, G, diag, sub in cases:
        if name != prev:
            lines.append("T " + " ".join(str(int(v) % M32) for v in start))
            prev = name
        lines.append("W %d %d %d %d %d %d %d" % (toff, cnt, s_first, s_last, G, diag, sub))
    return "\n".join(lines) + "\n"


def _ranges_ok(v, cnt):
    qb0, qe0, qb1, qe1 = v[:4]
    up4 = (cnt + 3) & ~3
    pieces = [(b, e) for b, e in ((qb0, qe0), (qb1, qe1)) if e > b]
    for b, e in pieces:
        assert b % 4 == 0 and e % 4 == 0 and 0 <= b < e <= up4, (v, cnt)
    if len(pieces) == 2:
        assert pieces[0][1] <= pieces[1][0], (v, cnt)       # disjoint, piece 0 first
    return pieces


def test_window_against_brute_force(driver):
    cases = _cases()
    assert len(cases) > 5000
    r = subprocess.run([driver], input=_text(cases), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(cases)
    seen = {"wrap_lo": 0, "wrap_hi": 0, "all": 0, "two": 0, "dead": 0, "zf": 0, "narrow": 0}
    for line, (name, start, toff, cnt, s_first, s_last, G, diag, sub) in zip(out, cases):
        v = [int(x) for x in line.split()]
        ctx = (name, toff, cnt, s_first, s_last, G, diag, sub, v)
        slabs = (np.searchsorted(start, np.arange(toff, toff + cnt), side="right") - 1).astype(np.int64)
        pieces = _ranges_ok(v, cnt)
        visit = np.zeros((cnt + 3) // 4, dtype=bool)
        for b, e in pieces:
            visit[b // 4:e // 4] = True
        inside, zf = _reach(s_first, s_last, G)
        own = sub * 128 if diag else 0
        need = np.arange(cnt) >= own
        if inside is not None:
            need &= inside[slabs]
        # every partner inside the reach (from the own block on) is inside a returned range
        assert visit[np.flatnonzero(need) // 4].all(), ctx
        # no quad in front of the own block, and nothing the search over sampled quads would not visit either
        assert not visit[:own // 4].any(), ctx
        assert not (visit & ~_sampled(slabs, s_first, s_last, G, own)).any(), ctx
        assert v[6] == int(zf), ctx
        # the record: empty pieces as zero words, the centres' slabs, the flags
        x, y, z, w = v[7:]
        live = bool(pieces)
        assert w == 0 and (x, y, z) != (0, 0, 0) if live else (x, y, z, w) == (0, 0, 0, 0), ctx
        if live:
            assert x == (v[0] | v[1] << 16 if v[1] > v[0] else 0) and y == (v[2] | v[3] << 16 if v[3] > v[2] else 0), ctx
            assert z & 0xffff == s_first | s_last << 8 and (z >> 16) & 1 == int(zf) and (z >> 19) & 1 == 1, ctx
            assert (z >> 17) & 1 == (v[4] != 0) and (z >> 18) & 1 == (v[5] != 0), ctx
        assert v[4] in (0, -1) and v[5] in (0, 1), ctx
        seen["wrap_lo"] += v[5] == 1
        seen["wrap_hi"] += v[4] == -1
        seen["all"] += inside is None or bool(inside.all())
        seen["two"] += len(pieces) == 2
        seen["dead"] += not live
        seen["zf"] += v[6]
        seen["narrow"] += live and not visit[own // 4:].all()
    assert min(seen.values()) > 0, seen


def test_slab_of_atom(driver):
    text, want = [], []
    for start in _tables().values():
        text.append("T " + " ".join(str(int(v)) for v in start))
        ks = np.unique(np.concatenate([start[:-1][np.diff(start) > 0], start[1:][np.diff(start) > 0] - 1, [0, N_SEG - 1, N_SEG // 2]]))
        text += ["S %d" % k for k in ks]
        want += (np.searchsorted(start, ks, side="right") - 1).tolist()
    r = subprocess.run([driver], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert [int(x) for x in r.stdout.split()] == want


def _garbage_text():
    rng = np.random.default_rng(12)
    tables = [rng.integers(0, M32, 257), np.full(257, M32 - 1), np.arange(257)[::-1] * 5, np.zeros(257, dtype=np.int64),
              rng.integers(0, 600, 257)]
    lines, cases = [], []
    for tab in tables:
        lines.append("T " + " ".join(str(int(v)) for v in tab))
        for cnt in COUNTS:
            for toff in (0, 300, 0x7fffff00):
                for s_first, s_last in CENTRES + ((200, 10), (1000, 70000)):
                    for G in GAPS:
                        for diag, sub in ((0, 0), (1, 0), (1, 3)):
                            lines.append("W %d %d %d %d %d %d %d" % (toff, cnt, s_first, s_last, G, diag, sub))
                            cases.append(cnt)
        lines += ["S 0", "S 5", "S %d" % (M32 - 1)]
        cases += [None] * 3
    return "\n".join(lines) + "\n", cases


def test_garbage_table_stays_inside_the_tile(driver):
    text, cases = _garbage_text()
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(cases)
    for line, cnt in zip(out, cases):
        v = [int(x) for x in line.split()]
        if cnt is None:
            assert 0 <= v[0] <= 255
        else:
            _ranges_ok(v, cnt)


def test_driver_under_sanitizers(tmp):
    san = _build(tmp, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "tile_plan_driver_san")
    for text in (_text(_cases()[::7]), _garbage_text()[0]):
        r = subprocess.run([san], input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
