"""The pore analysis without a GPU: the ABI surface, the grid rule, the restatement of tests/pore_ref.py against the neighbour
oracle and a known answer, the conditions on the inputs of the GPU tests (budget cap, no grid point within the budget of a
decision, the planted ones a known delta away), the candidate arithmetic of amof_amd/csrc/pore_math.h against its bound, the
host side of ``Pore`` (defaults, refusals, ``assemble``, feather) and a two-rank gloo run of the class."""

import os
import re
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from amof_amd import _hip
from amof_amd import pore as P
from amof_amd.frames import PackedTrajectory
from tests import cell_forms
from tests import pore_cases as cases
from tests import pore_ref as ref
from tests.conftest import ROOT

ALL = cases.NAMES + cases.FORMS


def test_abi_surface():
    with open(os.path.join(ROOT, "include", "amof_hip.h")) as fh:
        text = fh.read()
    assert re.search(r"\bint amof_pore_field\(", text) and re.search(r"\bdouble amof_pore_candidate_bound\(", text)
    for name in ("amof_pore_field", "amof_pore_candidate_bound"):
        assert name in _hip.EXPORTS
    comment = text[text.index("kernel family that produced"):text.index("const char *amof_last_path")]
    assert '"pore_brick"' in comment and '"pore_exact"' in comment
    stages = text[text.index("Seconds spent inside kernels"):text.index("double amof_last_kernel_seconds")]
    assert "amof_pore_field" in stages
    assert "#define AMOF_ABI_VERSION 4" in text and _hip.ABI_VERSION == 4
    assert hasattr(_hip.Context, "pore_field") and hasattr(_hip.MultiContext, "pore_field")


def test_grid_points_match_the_elementwise_restatement():
    for cell, n in ((cases.SHEARED, (3, 5, 4)), (cell_forms.apply(cases.SHEARED, "rotmirror"), (7, 1, 2)), (cases.RECT, (1, 1, 1)),
                    (-cases.RECT, (2, 3, 9))):
        got = P.grid_points(cell, n)
        assert got.shape == tuple(n) + (3,) and np.array_equal(got.reshape(-1, 3), ref.points(cell, n))
    # the centre of a 1 x 1 x 1 grid is the body centre; positions() is the same rule for single indices
    assert np.array_equal(P.grid_points(cases.RECT, (1, 1, 1))[0, 0, 0], 0.5 * np.diag(cases.RECT))
    n = (3, 5, 4)
    idx = np.array([0, 7, 59])
    assert np.array_equal(P.positions(idx, cases.SHEARED, n), ref.points(cases.SHEARED, n)[idx])


@pytest.mark.parametrize("name", ["rect", "sheared", "planted"])
def test_inside_counts_are_the_neighbour_oracles(name):
    """v < 0 <=> sqrt(d2) < R_j: the restatement's inside points are the probe "atoms" with a neighbour, decided by the
    oracle of amof_cn_count with the grid points appended as one more species and the radii as cutoffs"""
    from oracle import clib
    c = cases.case(name)
    res, raw = cases.reference(name)
    both, rcm, sets, is_probe = cases.with_probes(c)
    kinds, sp = _hip.species_index(both.numbers)
    _, pa = clib.cn_counts(both.pos, both.cell, sp, len(kinds), rcm, sets, pbc=tuple(both.pbc), per_atom=True)
    inside = pa[:, :, is_probe].sum(axis=1) > 0
    assert np.array_equal(inside, raw < 0.0)
    assert np.array_equal(inside.sum(axis=1).astype(np.uint64), res.rows[:, 0]) and res.rows[:, 0].sum() > 0


def test_known_answer_simple_cubic():
    a, R, reps, n = 4.0, 1.0, 3, 27                 # (27 = 9 points per lattice constant: odd, the body centre is a grid point)
    sites = np.array([(i, j, k) for i in range(reps) for j in range(reps) for k in range(reps)], dtype=np.float64) * a
    res, raw = ref.pore(sites[None], np.diag([a * reps] * 3), np.full(len(sites), 30), {30: R}, (n, n, n), 0.1, 3.0, (0.0,))
    want = a * np.sqrt(3.0) / 2.0 - R
    assert raw.max() == pytest.approx(want, rel=1e-12)
    pts = ref.points(np.diag([a * reps] * 3), (n, n, n))
    at = pts[np.argmax(raw[0])] / a
    assert np.allclose(at - np.floor(at), 0.5, atol=1e-12)            # a body centre
    rows, counts, vmax, argmax = ref.from_field(res.field, 0.1, 3.0, (0.0,))
    assert vmax[0] == raw.max() and rows.sum() == n ** 3 and rows[0, -1] == 0
    assert counts[0, 0] == n ** 3 - rows[0, 0] and 0 < rows[0, 0] < n ** 3 // 8        # the spheres fill 6.5 % of the cell


@pytest.mark.parametrize("name", ALL)
def test_conditions_on_every_gpu_input(name):
    """conditions, not tolerances: the derived budget stays below 1e-10 A, and NO grid point of the restatement lies within
    its budget of a decision (0, a bin edge, dmax, a threshold), so nothing is ever excluded from the exact comparisons;
    the planted points sit delta away, delta >= 100 budgets"""
    c = cases.case(name)
    res, raw = cases.reference(name)
    assert 0.0 < res.worst < 1e-10, (name, res.worst)
    assert ref.near_decisions(raw, res.budget, c.dr, c.dmax, c.thresholds) == []
    assert np.array_equal(res.rows.sum(axis=1), np.full(len(res.rows), c.G, dtype=np.uint64))
    if not name.startswith("planted"):
        assert not c.plants
        return
    d_small, d_band = cases.plant_deltas()
    eps_c = 4.0 * d_band
    assert d_small == 2.0 ** -26 and d_small >= 100.0 * res.worst and d_band >= 100.0 * res.worst and d_small < d_band < eps_c
    kinds = {}
    for f, g, what, e, sd in c.plants:
        assert abs((raw[f, g] - e) - sd) <= 2.0 * res.budget[f, g], (f, g, what)
        assert abs(sd) in (d_small, d_band)
        kinds.setdefault(what, set()).add(sd)
    assert {k: len(v) for k, v in kinds.items()} == {"zero": 4, "edge": 4, "dmax": 4, "threshold": 4, "pair": 2}
    # the planted decisions are decisions: each sign lands in another slot
    rows_of = {}
    for f, g, what, e, sd in c.plants:
        v = res.field[f, g]
        if what == "zero":
            assert (v < 0) == (sd < 0)
        elif what == "edge":
            assert int(v / c.dr) == (3 if sd > 0 else 2)
        elif what == "dmax":
            assert (v < c.dmax) == (sd < 0) and (sd < 0 or v == c.dmax)
        elif what == "threshold":
            assert (v >= 1.2) == (sd > 0)
        else:
            # the winner is the SECOND atom of the pair: the first alone would give the decision value itself
            assert v < e and abs(v - (e + sd)) <= 2.0 * res.budget[f, g]
        rows_of[what] = True
    assert len(rows_of) == 5


def test_cases_have_the_shapes_the_gpu_tests_rely_on():
    rect = cases.case("rect")
    assert rect.packed.pos.shape == (3, 150, 3) and rect.grid == (11, 13, 17) and all(x % P_BRICK for x in rect.grid)
    assert cases.case("zif4").kinds == [1, 6, 7, 30] and cases.case("zif4").grid == P.default_grid(cases.case("zif4").packed.cell[0], 0.5)
    assert cases.case("npt_diag").packed.cell.shape == (4, 3, 3) and cases.case("npt_sheared").packed.cell.shape == (4, 3, 3)
    assert tuple(cases.case("open").packed.pbc) == (True, False, True)
    for name in ALL:
        c = cases.case(name)
        res, raw = cases.reference(name)
        assert c.G <= 6000 or name == "zif4"
        assert c.dmax + c.radii.max() <= P.half_height(c.packed.cell, c.packed.pbc)
        assert res.rows[:, 0].min() > 0 and res.rows[:, 1:-1].sum() > 0 and (res.counts[:, 0] > res.counts[:, -1]).all()
    assert cases.reference("planted")[0].rows[:, -1].min() > 0          # overflow points in every planted frame


P_BRICK = 8         # amof_amd/csrc/pore_math.h PORE_BRICK


# ---- the candidate arithmetic of the fast path ---------------------------------------------------------------------------
def test_candidate_arithmetic_stays_within_its_bound(tmp_path):
    with open(os.path.join(ROOT, "amof_amd", "csrc", "pore_math.h")) as fh:
        assert "constexpr int PORE_BRICK = %d;" % P_BRICK in fh.read()
    out = str(tmp_path / "pore_candidate_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "pore_candidate_driver.cpp"),
                        "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # (rcut, half-diagonal, radii, atoms per brick, points, seed): the cases' geometry, the headline's, a coarse brick
    lines = ["5.39 6.95 1.39 1.39 200 1500 7", "5.7 3.0 1.2 1.7 300 800 5", "9.7 1.4 1.2 2.1 500 400 3", "3.39 4.85 1.39 1.39 40 2000 11",
             "2.0 3.0 0.0 1.0 30 2000 13"]
    r = subprocess.run([out], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [np.array(l.split(), dtype=float) for l in r.stdout.strip().splitlines()]
    assert len(rows) == len(lines)
    for line, (eps, worst, missed, selected) in zip(lines, rows):
        rcut = float(line.split()[0])
        assert eps == 1.1 * 10.0 * 2.0 ** -24 * 4.0 * rcut              # the arithmetic part of the bound (no cell term)
        assert 0.0 < worst <= eps * 7.06 / 11.0, (line, worst, eps)    # the derived 7.06 u Q without the margins
        assert missed == 0 and 1.0 <= selected < 4.0, (line, missed, selected)
    # the exported bound is the header's: the arithmetic part plus 2^-31 of the summed cell-vector lengths
    cell = cases.SHEARED
    want = 1.1 * 10.0 * 2.0 ** -24 * 4.0 * 5.7 + np.sqrt((cell ** 2).sum(axis=1)).sum() / 2.0 ** 31
    assert _hip.pore_candidate_bound(cell, 5.7) == pytest.approx(want, rel=1e-14)


# ---- the host side of the class ------------------------------------------------------------------------------------------
def test_default_grid_and_dmax_rules():
    assert P.default_grid(np.diag([10.0, 10.1, 0.05]), 0.2) == (50, 51, 1)
    assert P.default_grid(cases.SHEARED, 0.5) == tuple(int(np.ceil(x / 0.5)) for x in np.sqrt((cases.SHEARED ** 2).sum(axis=1)))
    h = P.cell_heights(cases.SHEARED)[0]
    vol = abs(np.linalg.det(cases.SHEARED))
    assert h == pytest.approx([vol / np.linalg.norm(np.cross(cases.SHEARED[1], cases.SHEARED[2])),
                               vol / np.linalg.norm(np.cross(cases.SHEARED[2], cases.SHEARED[0])),
                               vol / np.linalg.norm(np.cross(cases.SHEARED[0], cases.SHEARED[1]))], rel=1e-14)
    assert P.half_height(np.diag([14.0, 30.0, 9.0]), (True, True, False)) == 7.0
    assert P.default_dmax(np.diag([40.0, 40.0, 40.0]), (True,) * 3, 1.7, 0.05) == pytest.approx(8.0, abs=1e-12)      # the 8 A cap
    got = P.default_dmax(np.diag([14.0, 30.0, 9.0]), (True, True, False), 1.7, 0.25)
    assert got == 5.25 and got + 1.7 <= 7.0                                 # 5.3 rounded down to a multiple of dr
    cells = np.stack([np.diag([14.0, 14.0, 14.0]), np.diag([12.0, 14.0, 14.0])])
    assert P.default_dmax(cells, (True,) * 3, 1.0, 0.5) == 5.0              # the smallest frame decides
    with pytest.raises(ValueError):
        P.default_dmax(np.diag([4.0, 4.0, 4.0]), (True,) * 3, 1.9, 0.25)


def test_radii_table_and_overrides():
    assert P.BONDI["Zn"] == 1.39 and P.BONDI["H"] == 1.20 and P.BONDI["U"] == 1.86 and len(P.BONDI) == 38
    assert P.species_radii([1, 6, 7, 30]).tolist() == [1.20, 1.70, 1.55, 1.39]
    assert P.species_radii([1, 26], {"Fe": 2.0, "H": 1.1}).tolist() == [1.1, 2.0]
    with pytest.raises(ValueError, match="Fe"):
        P.species_radii([1, 26])
    with pytest.raises(ValueError):
        P.species_radii([1], {"H": -1.0})


def test_arguments_refused_before_any_device_work():
    packed = PackedTrajectory(np.zeros((2, 2, 3)), np.diag([12.0, 12.0, 12.0]), np.array([30, 7]))
    iron = PackedTrajectory(np.zeros((2, 2, 3)), np.diag([12.0, 12.0, 12.0]), np.array([26, 7]))
    bad = [dict(dmax=4.5), dict(dmax=0.0), dict(dmax=0.01, dr=0.05), dict(dr=0.0), dict(dr=-1.0), dict(spacing=0.0),
           dict(grid=(4, 4)), dict(grid=(0, 4, 4)), dict(grid=(2048, 2048, 2048)), dict(probe_radius=(-0.1,)),
           dict(probe_radius=(np.nan,)), dict(radii={"Zn": np.inf}), dict(radii={"Zn": 6.5}), dict(distributed='local'),
           dict(distributed='local', grid=(4, 4, 4)), dict(distributed='local', dmax=2.0)]
    for kw in bad:
        kw.setdefault("distributed", False)
        with pytest.raises(ValueError):
            P.Pore.from_trajectory(packed, device=0, **kw)
    with pytest.raises(ValueError, match="Fe"):
        P.Pore.from_trajectory(iron, device=0, distributed=False)
    empty = P.Pore()
    assert list(empty.data.columns) == ["Step"] and len(empty.data) == 0


def test_assemble_columns_volumes_and_density():
    counts = np.array([[10, 20, 30, 40, 0], [0, 50, 25, 24, 1]], dtype=np.uint64)      # nbins = 3, G = 100
    probe = np.array([[90, 45], [100, 10]])
    vmax = np.array([1.25, 1.5])
    volume = np.array([1000.0, 2000.0])
    data, hist = P.assemble(counts, probe, vmax, np.array([5, 15]), volume, 120.0, [0.0, 1.2], (4, 5, 5), 0.5)
    assert list(data.columns) == ["Step", "Unitcell_volume", "Density", "PCV_Volume_fraction-0", "PCV_A^3-0", "PCV_cm^3/g-0",
                                  "PCV_Volume_fraction-1.2", "PCV_A^3-1.2", "PCV_cm^3/g-1.2", "Di"]
    assert data["Step"].tolist() == [5, 15] and data["Unitcell_volume"].tolist() == [1000.0, 2000.0]
    assert data["Density"].tolist() == pytest.approx([120.0 / (1000.0 * 0.602214076), 120.0 / (2000.0 * 0.602214076)], rel=1e-15)
    assert data["Density"][0] == pytest.approx(120.0 * 1.66053906660 / 1000.0, rel=1e-9)          # g/mol per A^3 in g/cm^3
    assert data["PCV_Volume_fraction-0"].tolist() == [0.9, 1.0] and data["PCV_Volume_fraction-1.2"].tolist() == [0.45, 0.1]
    assert data["PCV_A^3-1.2"].tolist() == [450.0, 200.0]
    assert data["PCV_cm^3/g-1.2"].tolist() == pytest.approx([450.0 * 0.602214076 / 120.0, 200.0 * 0.602214076 / 120.0], rel=1e-15)
    assert data["Di"].tolist() == [2.5, np.inf]                         # frame 1 has an overflow point
    assert hist["r"].tolist() == [0.25, 0.75, 1.25]
    assert hist["density"].tolist() == pytest.approx([(20 / 50 + 50 / 50) / 2, (30 / 50 + 25 / 50) / 2, (40 / 50 + 24 / 50) / 2])
    assert P.probe_label(1.0) == "1" and P.probe_label(0.25) == "0.25"


def test_feather_round_trip(tmp_path):
    obj = P.Pore()
    obj.data = P.assemble(np.array([[1, 2, 3, 0]], dtype=np.uint64), np.array([[5]]), np.array([0.7]), [3], [10.0], 12.0, [0.0],
                          (1, 2, 3), 0.5)[0]
    path = str(tmp_path / "walk")
    obj.write_to_file(path)
    assert os.path.exists(path + ".pore")
    assert P.Pore.from_file(path).data.equals(obj.data)


# ---- the class over two gloo ranks, the kernels answered by the restatement ---------------------------------------------
def _install(monkeypatch=None):
    """tests/oracle_context.py's stand-in, its ``pore_field`` answered by tests/pore_ref.py"""
    from tests import oracle_context

    class PoreContext(oracle_context.OracleContext):
        def pore_field(self, packed, radii, grid, dr, dmax, thresholds=(), frame_range=None, per_point=False):
            self.calls.append("pore")
            kinds, _ = _hip.packed_species(packed)
            pos, cell = self._frames(packed, frame_range)
            res, raw = ref.pore(pos, cell, packed.numbers, dict(zip(kinds, radii)), grid, dr, dmax, thresholds, pbc=tuple(packed.pbc))
            rows, counts, vmax, argmax = ref.from_field(res.field, dr, dmax, thresholds)
            out = (rows, counts, vmax, argmax)
            return out + (res.field.reshape((len(pos),) + tuple(grid)),) if per_point else out

    lanes = {0: PoreContext("oracle-lane-0"), 1: PoreContext("oracle-lane-1")}
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


CLASS_KW = dict(probe_radius=(0.0, 1.2), grid=(7, 6, 5), dr=0.25, dmax=3.0, per_point=True)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lanes = _install()
    packed = cases.case("npt_sheared").packed
    obj = P.Pore.from_trajectory(packed, delta_Step=10, **CLASS_KW)
    assert obj.__dict__.get("_pending") is not None
    data = obj.data
    assert lanes[1].calls == ["pore"] and lanes[0].calls == []
    if rank == 0:
        data.to_pickle(os.path.join(out_dir, "data.pkl"))
        obj.hist.to_pickle(os.path.join(out_dir, "hist.pkl"))
        np.savez(os.path.join(out_dir, "raw.npz"), counts=obj.counts, field=obj.field, where=obj.di_position)
    dist.barrier()
    dist.destroy_process_group()


def test_class_sharded_over_two_ranks_equals_one_process(tmp_path, monkeypatch):
    import torch.multiprocessing as mp
    port = 23500 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    lanes = _install(monkeypatch)
    packed = cases.case("npt_sheared").packed
    one = P.Pore.from_trajectory(packed, delta_Step=10, distributed=False, **CLASS_KW)
    assert pd.read_pickle(os.path.join(str(tmp_path), "data.pkl")).equals(one.data)
    assert pd.read_pickle(os.path.join(str(tmp_path), "hist.pkl")).equals(one.hist)
    raw = np.load(os.path.join(str(tmp_path), "raw.npz"))
    assert np.array_equal(raw["counts"], one.counts) and np.array_equal(raw["field"], one.field)
    assert np.array_equal(raw["where"], one.di_position)
    # and the class's numbers are the restatement's by the documented formulas
    assert one.data["Step"].tolist() == [0, 10, 20, 30] and one.field.shape == (4, 7, 6, 5)
    rows, counts, vmax, argmax = ref.from_field(one.field, 0.25, 3.0, (0.0, 1.2))
    assert np.array_equal(one.counts, rows)
    assert one.data["PCV_Volume_fraction-1.2"].tolist() == (counts[:, 1] / 210.0).tolist()
    assert one.data["Unitcell_volume"].tolist() == pytest.approx(np.abs(np.linalg.det(packed.cell)).tolist(), rel=1e-15)
    di = np.where(rows[:, -1] > 0, np.inf, 2.0 * vmax)
    assert one.data["Di"].tolist() == di.tolist()
    cells = np.asarray(packed.cell)
    assert np.array_equal(one.di_position, np.stack([P.grid_points(cells[f], (7, 6, 5)).reshape(-1, 3)[argmax[f]] for f in range(4)]))
    for ctx in lanes.values():
        ctx.close_lane()
