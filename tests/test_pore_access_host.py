"""The accessibility analysis without a GPU: known answers of the restatement (tests/pore_access_ref.py) on the simple-cubic
frames and on the synthetic topologies of tests/pore_access_cases.py, the winding resolver of
amof_amd/csrc/pore_access_math.h through a native driver (known link lists, random masks against the restatement, once more
under the address and undefined-behaviour sanitizers), the ABI surface, the columns ``Pore`` derives from the library's
integers, and a two-rank gloo run of the class with both flags, its kernels answered by the restatements."""

import os
import re
import subprocess

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import pore as P
from tests import pore_access_cases as cases
from tests import pore_access_ref as ref
from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "pore_access_driver.cpp")


# ---- known answers of the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_over, want", [(None, [(1, 0, 3), (1, 0, 3), (0, 27, 0)]), (3.0, [(1, 0, 3), (9, 0, 1), (0, 27, 0)])])
def test_simple_cubic_known_answers(c_over, want):
    """a = 4, R = 1: the window between four atoms of a face has radius 4 / sqrt(2) - 1 = 1.83 (t*), the body centre
    2 sqrt(3) - 1 (Di / 2): probes of 1.2 and 1.6 pass everywhere, one of 2.0 is shut into the 27 cages.  With c = 3 the
    windows of the four side faces shrink to 2.5 - 1 = 1.5: a probe of 1.6 passes along z only, through nine columns."""
    field, worst = cases.simple_cubic_field(c_over)
    assert worst < 1e-12
    rows, _ = ref.access(field[0], cases.SC_PROBES)
    assert [tuple(r[1:]) for r in rows.tolist()] == want
    tstar, big = ref.free_sphere(field[0], dmax=cases.SC_DMAX)
    assert abs(tstar - (4.0 / np.sqrt(2.0) - 1.0)) <= worst
    body = 2.0 * np.sqrt(3.0) - 1.0 if c_over is None else np.sqrt(8.0 + 2.25) - 1.0
    assert abs(big - body) <= worst and big == field.max()
    # t* is a field value: V(t*) has a channel, V(nextafter(t*)) has none
    assert (field == tstar).any()
    assert ref.access(field[0], [tstar])[0][0, 1] >= 1 and ref.access(field[0], [np.nextafter(tstar, np.inf)])[0][0, 1] == 0


@pytest.mark.parametrize("name", cases.NAMES)
def test_synthetic_topologies_are_what_they_are_built_to_be(name):
    c = cases.case(name)
    rows, labels, free = cases.reference(name)
    assert set(np.unique(c.field).tolist()) <= {-1.0, 1.0, cases.T0}
    if "row" in c.known:
        assert rows[0, 0].tolist() == c.known["row"]
    if "rows" in c.known:
        assert rows[0].tolist() == c.known["rows"]
    assert np.array_equal(labels[0] >= 0, np.stack([c.field[0] >= t for t in c.thresholds]))
    if name.startswith("serpentine"):
        # one component through every tile, at least a quarter of the grid, its label in the last tile of the first layer
        lab = labels[0, 0]
        assert np.unique(lab).tolist() == [-1, c.known["label"]] and (lab >= 0).sum() >= lab.size / 4
        tiles = set(zip(*[(x // t).tolist() for x, t in zip(np.nonzero(lab >= 0), cases.TILE)]))
        per_axis = [-(-n // t) for n, t in zip(c.grid, cases.TILE)]
        assert len(tiles) == per_axis[0] * per_axis[1] * per_axis[2] >= 16
        i, j, k = np.unravel_index(c.known["label"], c.grid)
        assert (i // 8, j // 8, k // 32) == (0, per_axis[1] - 1, per_axis[2] - 1)
    if name == "inclusive":
        assert free[0].tolist() == [cases.T0, 1.0]


# ---- the resolver header ----------------------------------------------------------------------------------------------------
def _build(tmp, flags, name):
    exe = os.path.join(str(tmp), name)
    r = subprocess.run(["g++", "-std=c++17"] + flags + [SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


LINK_JOBS = [
    # (links (lo, hi, axis), {label: dimension})
    ([(3, 9, 0), (9, 3, 1), (3, 12, 0), (3, 12, 1)], {3: 2}),          # windings (1, 1, 0) and (1, -1, 0)
    ([(5, 8, 0), (5, 8, 0)], {5: 0}),                                  # there and back through the same face
    ([(4, 6, 0), (6, 4, 0)], {4: 1}),                                  # winding (2, 0, 0)
    ([(1, 2, 2), (10, 11, 2), (20, 20, 2)], {1: 0, 10: 0, 20: 1}),     # two components share a face with a third that winds
    ([(7, 7, 0), (7, 7, 1), (7, 7, 2)], {7: 3}),
    ([(2, 5, 0), (5, 2, 0), (2, 5, 1), (5, 2, 1)], {2: 2}),            # (2, 0, 0), (1, 1, 0) -> rank 2
    ([], {}),
]


def _mask_jobs():
    rng = np.random.default_rng(17)
    jobs = []
    for n, pbc, density in (((5, 4, 6), (1, 1, 1), 0.5), ((3, 3, 3), (1, 1, 1), 0.6), ((7, 5, 4), (1, 0, 1), 0.55), ((1, 9, 8), (0, 1, 1), 0.6),
                            ((6, 6, 6), (1, 1, 1), 0.35), ((4, 9, 5), (0, 0, 0), 0.6), ((8, 3, 7), (1, 1, 1), 0.7), ((5, 5, 5), (1, 1, 0), 0.45)):
        for _ in range(3):
            jobs.append((n, pbc, rng.random(n) < density))
    return jobs


def _run_driver(exe):
    text = []
    for links, _ in LINK_JOBS:
        text.append("links %d " % len(links) + " ".join("%d %d %d" % l for l in links))
    masks = _mask_jobs()
    for n, pbc, mask in masks:
        text.append("mask %d %d %d %d %d %d " % (n + pbc) + " ".join(str(int(x)) for x in mask.reshape(-1)))
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(LINK_JOBS) + len(masks)
    for (links, want), line in zip(LINK_JOBS, lines):
        got = np.array(line.split(), dtype=np.int64).reshape(-1, 2)
        assert dict(got.tolist()) == want, (links, line)
    dims = set()
    for (n, pbc, mask), line in zip(masks, lines[len(LINK_JOBS):]):
        got = [tuple(x) for x in np.array(line.split(), dtype=np.int64).reshape(-1, 3).tolist()]
        _, comps = ref.components(mask, tuple(bool(x) for x in pbc))
        assert got == comps, (n, pbc)
        dims |= set(c[2] for c in comps)
    assert dims == {0, 1, 2, 3}


def test_resolver_against_known_windings_and_the_restatement(tmp_path):
    _run_driver(_build(tmp_path, ["-O1"], "pore_access_driver"))


def test_resolver_under_the_sanitizers(tmp_path):
    _run_driver(_build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "pore_access_driver_san"))


# ---- ABI surface ------------------------------------------------------------------------------------------------------------
def test_abi_surface():
    with open(os.path.join(ROOT, "include", "amof_hip.h")) as fh:
        text = fh.read()
    assert re.search(r"\bint amof_pore_access\(", text) and re.search(r"\bint amof_pore_access_field\(", text)
    for name in ("amof_pore_access", "amof_pore_access_field"):
        assert name in _hip.EXPORTS
    comment = text[text.index("kernel family that produced"):text.index("const char *amof_last_path")]
    assert '"pore_label_tile"' in comment and '"pore_label_global"' in comment
    assert "#define AMOF_ABI_VERSION 4" in text and _hip.ABI_VERSION == 4
    for cls in (_hip.Context, _hip.MultiContext):
        assert hasattr(cls, "pore_access") and hasattr(cls, "pore_access_field")
    with open(os.path.join(ROOT, "amof_amd", "csrc", "pore_access.hip")) as fh:
        src = fh.read()
    assert "PA_TX = %d, PA_TY = %d, PA_TZ = %d;" % cases.TILE in src


# ---- the columns of the class -----------------------------------------------------------------------------------------------
def test_access_columns_from_given_integers():
    access = np.array([[[60, 1, 3, 3], [0, 0, 5, 0]], [[80, 2, 0, 1], [10, 1, 1, 2]]], dtype=np.int64)      # [F][n_probes][4]
    probe = np.array([[90, 45], [100, 10]])
    volume = np.array([1000.0, 2000.0])
    cols = P.access_columns(access, probe, volume, 120.0, [0.0, 1.2], (4, 5, 5))
    assert list(cols) == [x + "-" + rp for rp in ("0", "1.2") for x in
                          ("AV_Volume_fraction", "AV_A^3", "AV_cm^3/g", "NAV_Volume_fraction", "NAV_A^3", "NAV_cm^3/g", "Channels",
                           "Pockets", "Channel_dimension")]
    assert cols["AV_Volume_fraction-0"].tolist() == [0.6, 0.8] and cols["NAV_Volume_fraction-0"].tolist() == [0.3, 0.2]
    assert cols["AV_A^3-0"].tolist() == [600.0, 1600.0] and cols["NAV_A^3-1.2"].tolist() == [450.0, 0.0]
    assert cols["AV_cm^3/g-0"].tolist() == pytest.approx([600.0 * 0.602214076 / 120.0, 1600.0 * 0.602214076 / 120.0], rel=1e-15)
    assert cols["Channels-1.2"].tolist() == [0, 1] and cols["Pockets-0"].tolist() == [3, 0]
    assert cols["Channel_dimension-0"].tolist() == [3, 1]
    # AV + NAV == PCV in counts: the fractions are count / G of integers that add up
    G = 100
    for k, rp in enumerate(("0", "1.2")):
        av = np.rint(cols["AV_Volume_fraction-" + rp] * G).astype(np.int64)
        nav = np.rint(cols["NAV_Volume_fraction-" + rp] * G).astype(np.int64)
        assert np.array_equal(av + nav, probe[:, k]) and np.array_equal(av, access[:, k, 0])
    with pytest.raises(ValueError):
        P.access_columns(access + np.array([100, 0, 0, 0]), probe, volume, 120.0, [0.0, 1.2], (4, 5, 5))     # more accessible than void
    free = P.free_sphere_columns(np.array([[1.5, 2.0], [np.inf, np.inf], [0.0, 0.0]]))
    assert list(free) == ["Df", "Dif"] and free["Df"].tolist() == [3.0, np.inf, 0.0] and free["Dif"].tolist() == [4.0, np.inf, 0.0]


# ---- the class over two gloo ranks, the kernels answered by the restatements ----------------------------------------------
CLASS_KW = dict(probe_radius=(0.0, 1.2), grid=(7, 6, 5), dr=0.25, dmax=3.0, per_point=True, accessibility=True, free_sphere=True)


def _install(monkeypatch=None):
    """tests/oracle_context.py's stand-in, ``pore_field`` answered by tests/pore_ref.py and ``pore_access`` by
    tests/pore_access_ref.py on that field"""
    from tests import oracle_context
    from tests import pore_ref

    class AccessContext(oracle_context.OracleContext):
        def pore_field(self, packed, radii, grid, dr, dmax, thresholds=(), frame_range=None, per_point=False):
            self.calls.append("pore")
            kinds, _ = _hip.packed_species(packed)
            pos, cell = self._frames(packed, frame_range)
            res, _ = pore_ref.pore(pos, cell, packed.numbers, dict(zip(kinds, radii)), grid, dr, dmax, thresholds, pbc=tuple(packed.pbc))
            out = pore_ref.from_field(res.field, dr, dmax, thresholds)
            return out + (res.field.reshape((len(pos),) + tuple(grid)),) if per_point else out

        def pore_access(self, packed, radii, grid, dr, dmax, thresholds=(), frame_range=None, per_point=False, free_sphere=False,
                        labels=False):
            base = self.pore_field(packed, radii, grid, dr, dmax, thresholds, frame_range=frame_range, per_point=True)
            self.calls[-1] = "access"
            field, pbc = base[4], tuple(bool(x) for x in packed.pbc)
            rows = np.array([ref.access(f, thresholds, pbc)[0] for f in field], dtype=np.int64).reshape(len(field), len(thresholds), 4)
            out = base[:4] + (rows,)
            if free_sphere:
                out += (np.array([ref.free_sphere(f, pbc, dmax=dmax) for f in field], dtype=np.float64).reshape(len(field), 2),)
            if per_point:
                out += (field,)
            if labels:
                out += (np.array([ref.access(f, thresholds, pbc)[1] for f in field], dtype=np.int32).reshape((len(field), len(thresholds)) + tuple(grid)),)
            return out

    lanes = {0: AccessContext("oracle-lane-0"), 1: AccessContext("oracle-lane-1")}
    lanes[1]._follows = lanes[0]

    def lane_context(device, lane):
        from amof_amd import _lazy
        return lanes[lane if _lazy.async_enabled() else 0]

    def get_context(device=None, lane=0):
        return lanes[lane]
    if monkeypatch is not None:
        monkeypatch.setattr(_hip, "lane_context", lane_context)
        monkeypatch.setattr(_hip, "get_context", get_context)
    else:
        _hip.lane_context, _hip.get_context = lane_context, get_context
    return lanes


def _worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from tests import pore_cases
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lanes = _install()
    obj = P.Pore.from_trajectory(pore_cases.case("npt_sheared").packed, delta_Step=10, **CLASS_KW)
    data = obj.data
    assert lanes[1].calls == ["access"] and lanes[0].calls == []
    if rank == 0:
        data.to_pickle(os.path.join(out_dir, "data.pkl"))
        np.savez(os.path.join(out_dir, "raw.npz"), access=obj.access, free=obj.free_sphere, labels=obj.labels, field=obj.field)
    dist.barrier()
    dist.destroy_process_group()


def test_class_sharded_over_two_ranks_equals_one_process(tmp_path, monkeypatch):
    import pandas as pd
    import torch.multiprocessing as mp
    from tests import pore_cases
    port = 25500 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    lanes = _install(monkeypatch)
    packed = pore_cases.case("npt_sheared").packed
    one = P.Pore.from_trajectory(packed, delta_Step=10, distributed=False, **CLASS_KW)
    assert pd.read_pickle(os.path.join(str(tmp_path), "data.pkl")).equals(one.data)
    raw = np.load(os.path.join(str(tmp_path), "raw.npz"))
    for name, mine in (("access", one.access), ("free", one.free_sphere), ("labels", one.labels), ("field", one.field)):
        assert raw[name].dtype == mine.dtype and np.array_equal(raw[name], mine), name
    assert one.labels.shape == (4, 2, 7, 6, 5) and one.labels.dtype == np.int32 and one.access.shape == (4, 2, 4)
    # the columns are the helpers' on the restated integers, behind today's columns
    plain = P.Pore.from_trajectory(packed, delta_Step=10, distributed=False, **dict(CLASS_KW, accessibility=False, free_sphere=False))
    base = list(plain.data.columns)
    assert one.data[base].equals(plain.data)
    cols = P.access_columns(one.access, one.probe_counts, plain.data["Unitcell_volume"].to_numpy(),
                            float(np.asarray(packed.masses, dtype=np.float64).sum()), [0.0, 1.2], (7, 6, 5))
    cols.update(P.free_sphere_columns(one.free_sphere))
    assert list(one.data.columns) == base + list(cols)
    for name, col in cols.items():
        assert np.array_equal(one.data[name].to_numpy(), col), name
    assert np.array_equal((one.labels >= 0).sum(axis=(2, 3, 4)), one.probe_counts) and (one.access[:, :, 0] <= one.probe_counts).all()
    assert (one.access[:, 0, 1] >= 1).all()                     # the void itself percolates in every frame
    only_free = P.Pore.from_trajectory(packed, delta_Step=10, distributed=False, **dict(CLASS_KW, accessibility=False, per_point=False))
    assert list(only_free.data.columns) == base + ["Df", "Dif"] and not hasattr(only_free, "access") and not hasattr(only_free, "labels")
    for ctx in lanes.values():
        ctx.close_lane()


def test_class_walks_a_stream_batch_by_batch(tmp_path, monkeypatch):
    """an XyzStream of two-frame batches carries the extra columns, the field and the labels like the packed trajectory"""
    from amof_amd import trajectory as T
    from amof_amd.stream import XyzStream
    from tests import pore_cases
    lanes = _install(monkeypatch)
    packed = pore_cases.case("sheared").packed
    path = str(tmp_path / "s.xyz")
    T.write_xyz(path, packed, comment_lattice=False, fmt="%.17g")
    kw = dict(CLASS_KW, distributed=False)
    whole = P.Pore.from_trajectory(packed, **kw)
    walked = P.Pore.from_trajectory(XyzStream(path, cell=packed.cell[0], batch_frames=2, pinned=False), **kw)
    assert walked.data.equals(whole.data) and list(whole.data.columns)[-2:] == ["Df", "Dif"]
    for name in ("access", "free_sphere", "labels", "field", "counts"):
        assert np.array_equal(getattr(walked, name), getattr(whole, name)), name
    assert lanes[1].calls == ["access"] * 3                     # the whole trajectory once, the stream in two batches
    for ctx in lanes.values():
        ctx.close_lane()
