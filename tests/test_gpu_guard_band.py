"""Every fast pair path on pairs planted across its f32 guard band (tests/edge_plant.py): bit-exact against the C oracle.

The edge tests elsewhere use dyadic lattices, on which the f32 chain is exact, and random cases hold only a handful of
pairs near a decision.  Here most atoms are anchor-partner pairs within 0.01 .. 10 bands of a bin edge or a cutoff, with
anchors on cell faces, pairs shifted up to 9000 cells, non-dyadic cells, sheared and per-frame (NPT) cells.  Every case
forces its path with the switches of test_gpu_paths.py and asserts that the path ran (a silent fallback would make the
test vacuous)."""

import os

import numpy as np
import pytest

from amof_amd.frames import PackedTrajectory
from oracle import clib
from tests import edge_plant as E

pytestmark = pytest.mark.gpu

TILE = {"AMOF_RDF_NOCELL": "1", "AMOF_RDF_NORANGE": "1"}

DIAG = np.diag([17.31, 18.93, 41.77])
SHEARED = np.array([[17.31, 0.0, 0.0], [2.93, 18.11, 0.0], [-1.71, 3.37, 29.53]])
HIGH_KAPPA = np.array([[31.7, 0.0, 0.0], [0.0, 29.3, 0.0], [83.1, 79.7, 30.9]])


class _env(object):
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _numbers(n, kinds=(1, 6, 7, 30, 8), weights=(0.35, 0.3, 0.25, 0.1, 0.0)):
    """species mix; a weight of 0 is a species with a single atom"""
    w = np.asarray(weights, dtype=float)
    counts = np.floor(w / w.sum() * (n - (w == 0).sum())).astype(int)
    counts[np.argmax(w)] += n - (w == 0).sum() - counts.sum()
    counts[w == 0] = 1
    return np.repeat(kinds, counts)


def _npt(cell, F, amp, seed):
    rng = np.random.default_rng(seed)
    return np.stack([cell * (1.0 + amp * rng.uniform(-1, 1)) for _ in range(F)])


def _device(packed):
    import torch
    return PackedTrajectory(torch.as_tensor(packed.pos).cuda(), packed.cell, packed.numbers)


def _rdf_case(hip_ctx, pl, rmax, nbins, runs, device=False):
    """runs: [(env, path)]: each forced path must run and equal the oracle bit for bit"""
    packed = pl.packed
    kinds, sp = E._species(packed.numbers)
    ref, _ = clib.rdf_hist(packed.pos, packed.cell, sp, len(kinds), rmax, nbins, cell_list=True)
    assert ref.sum() > 0
    inputs = [packed, _device(packed)] if device else [packed]
    for env, path in runs:
        for inp in inputs:
            with _env(**env):
                got, _, _ = hip_ctx.rdf_accumulate(inp, rmax, nbins)
                ran = hip_ctx.last_path()
            assert ran == path, (env, ran, path)
            bad = np.argwhere(got != ref)
            assert len(bad) == 0, (path, nbins, int(np.abs(got.astype(np.int64) - ref.astype(np.int64)).sum()), bad[:8].tolist())


# ------------------------------------------------------------------------------------------------------ RDF --

@pytest.mark.parametrize("nbins", [1, 7, 999, 2310, 31744])
def test_rdf_diagonal_tile_paths(hip_ctx, nbins):
    """rdf_tile_zf (default) and rdf_tile (AMOF_RDF_NOZF), slab culling live; 3 frames, host and device input"""
    rmax = 8.0
    pl = E.plant_rdf(DIAG, _numbers(2400), rmax, nbins, seed=100 + nbins, F=3, far=nbins in (7, 2310))
    _rdf_case(hip_ctx, pl, rmax, nbins, [(TILE, "rdf_tile_zf"), (dict(TILE, AMOF_RDF_NOZF="1"), "rdf_tile")],
              device=nbins == 2310)


@pytest.mark.parametrize("cell", ["diagonal", "sheared"])
def test_rdf_species_counts_straddling_tile_sizes(hip_ctx, cell):
    """six species of 63 .. 513 atoms (one of a single atom) around the 64 / 256 / 512 tile and sub-tile sizes"""
    numbers = np.repeat([1, 6, 7, 8, 16, 30], [513, 257, 65, 1, 511, 63])
    rmax, c = (8.0, DIAG) if cell == "diagonal" else (6.5, SHEARED)
    pl = E.plant_rdf(c, numbers, rmax, 2310, seed=150, F=3, far=True)
    runs = [(TILE, "rdf_tile_zf" if cell == "diagonal" else "rdf_tile_tri"),
            (dict(TILE, AMOF_RDF_NOZF="1", AMOF_RDF_NOTRI="1"), "rdf_tile")]
    _rdf_case(hip_ctx, pl, rmax, 2310, runs)


def test_rdf_diagonal_npt_tile_paths(hip_ctx):
    rmax, nbins = 7.9, 2310
    pl = E.plant_rdf(_npt(DIAG, 5, 0.02, 3), _numbers(2000, weights=(0.5, 0.0, 0.3, 0.2, 0.0)), rmax, nbins, seed=5, far=True)
    _rdf_case(hip_ctx, pl, rmax, nbins, [(TILE, "rdf_tile_zf"), (dict(TILE, AMOF_RDF_NOZF="1"), "rdf_tile")], device=True)


@pytest.mark.parametrize("nbins", [7, 999, 2310, 31744])
def test_rdf_sheared_tile_paths(hip_ctx, nbins):
    """rdf_tile_tri (general cells) and the plain general kernel (AMOF_RDF_NOTRI) with kappa in its band"""
    rmax = 6.5
    pl = E.plant_rdf(SHEARED, _numbers(2400), rmax, nbins, seed=200 + nbins, F=3, far=nbins != 999)
    _rdf_case(hip_ctx, pl, rmax, nbins, [(TILE, "rdf_tile_tri"), (dict(TILE, AMOF_RDF_NOTRI="1"), "rdf_tile")],
              device=nbins == 999)


def test_rdf_sheared_npt_tile_paths(hip_ctx):
    rmax, nbins = 6.3, 999
    pl = E.plant_rdf(_npt(SHEARED, 3, 0.015, 4), _numbers(2400), rmax, nbins, seed=6, far=True)
    _rdf_case(hip_ctx, pl, rmax, nbins, [(TILE, "rdf_tile_tri"), (dict(TILE, AMOF_RDF_NOTRI="1"), "rdf_tile")], device=True)


@pytest.mark.parametrize("nbins", [2310, 31744])
def test_rdf_high_kappa_cell(hip_ctx, nbins):
    """a strongly sheared cell: the widest relative band of the tile paths (at 31744 bins near the guard_f < 0.25 limit)"""
    rmax = 4.2
    g = E.rdf_band(HIGH_KAPPA, rmax, nbins)
    assert g > (0.05 if nbins == 31744 else 0.003), g
    pl = E.plant_rdf(HIGH_KAPPA, _numbers(2400, weights=(0.6, 0.4, 0.0, 0.0, 0.0)), rmax, nbins, seed=300 + nbins, F=2, far=True)
    _rdf_case(hip_ctx, pl, rmax, nbins, [(TILE, "rdf_tile_tri"), (dict(TILE, AMOF_RDF_NOTRI="1"), "rdf_tile")])


@pytest.mark.parametrize("nbins", [999, 2310])
def test_rdf_image_aware_tile(hip_ctx, nbins):
    """rdf_tile_img: forced on a plain case, and selected by itself with rmax just over half the shortest height"""
    pl = E.plant_rdf(DIAG, _numbers(2400), 8.0, nbins, seed=400 + nbins, F=3, far=True)
    _rdf_case(hip_ctx, pl, 8.0, nbins, [(dict(TILE, AMOF_RDF_FORCE_IMG="1"), "rdf_tile_img")])
    rmax = 0.505 * DIAG[0, 0]
    pl = E.plant_rdf(DIAG, _numbers(2400), rmax, nbins, seed=410 + nbins, F=3, far=True)
    _rdf_case(hip_ctx, pl, rmax, nbins, [(TILE, "rdf_tile_img")])


@pytest.mark.parametrize("cell", ["diagonal", "sheared"])
def test_rdf_range_kernel(hip_ctx, cell):
    """rdf_range (2-level slab x y-bin list) on a thin long cell"""
    c = np.diag([14.73, 43.31, 52.93]) if cell == "diagonal" else np.array([[14.73, 0, 0], [1.9, 43.31, 0], [-2.2, 3.1, 52.93]])
    rmax = 5.3
    for nbins in (999, 2310):
        pl = E.plant_rdf(c, _numbers(3000), rmax, nbins, seed=500 + nbins, F=3, far=True)
        _rdf_case(hip_ctx, pl, rmax, nbins, [({"AMOF_RDF_FORCE_RANGE": "1", "AMOF_RDF_NOCELL": "1"}, "rdf_range")])


@pytest.mark.parametrize("cell", ["diagonal", "sheared", "npt"])
def test_rdf_cell_list_kernels(hip_ctx, cell):
    """rdf_cell, one wave per cell and the per-lane gather form"""
    base = np.diag([31.37, 33.71, 35.93])
    c = {"diagonal": base, "sheared": base + np.array([[0, 0, 0], [2.3, 0, 0], [-1.9, 2.7, 0]]),
         "npt": _npt(base, 3, 0.01, 7)}[cell]
    rmax = 5.5
    # (the kernel holds S (S + 1) / 2 histograms in 96 KiB of LDS: five species at 7 bins, three at 2310)
    for nbins, numbers in ((7, _numbers(4000)), (2310, _numbers(4000, kinds=(1, 6, 8), weights=(0.6, 0.4, 0.0)))):
        pl = E.plant_rdf(c, numbers, rmax, nbins, seed=600 + nbins, F=3, far=True)
        _rdf_case(hip_ctx, pl, rmax, nbins, [({"AMOF_RDF_FORCE_CELL": "1"}, "rdf_cell"),
                                             ({"AMOF_RDF_FORCE_CELL": "1", "AMOF_RDF_CELL_GATHER": "1"}, "rdf_cell")])


def test_rdf_exact_kernels(hip_ctx):
    """rdf_exact: forced (AMOF_RDF_KERNEL=v1), and the global-histogram kernel just above the LDS limit"""
    pl = E.plant_rdf(SHEARED, _numbers(2000), 6.5, 2310, seed=700, F=3, far=True)
    _rdf_case(hip_ctx, pl, 6.5, 2310, [({"AMOF_RDF_KERNEL": "v1"}, "rdf_exact")])
    nbins = 36865
    pl = E.plant_rdf(DIAG, _numbers(1500), 8.0, nbins, seed=701, F=3, far=True)
    _rdf_case(hip_ctx, pl, 8.0, nbins, [({}, "rdf_exact")])


# ----------------------------------------------------------------------------------------------- CN and BAD --

def _nbr_setup(n, seed_kinds=(30, 7, 6, 1, 8)):
    numbers = _numbers(n, kinds=seed_kinds, weights=(0.1, 0.25, 0.3, 0.35, 0.0))
    kinds, sp = E._species(numbers)
    S = len(kinds)
    zn, nn, ch, h = (kinds.index(z) for z in (30, 7, 6, 1))
    rcm = np.zeros((S, S))
    rcm[zn, nn] = rcm[nn, zn] = 2.5
    rcm[ch, h] = rcm[h, ch] = 1.31
    rcm[nn, nn] = 2.2
    rcm[ch, nn] = rcm[nn, ch] = 1.63
    sets = [(zn, nn), (nn, zn), (ch, h), (h, ch), (nn, nn), (ch, nn)]
    triples = [(zn, nn), (nn, zn), (nn, nn), (ch, h)]
    return numbers, rcm, sets, triples


EDGES_REGULAR = np.arange(int(180 // 0.5) + 2) * 0.5
EDGES_RAGGED = np.sort(np.concatenate([[0.0, 180.0], np.random.default_rng(9).uniform(0, 180, 61)]))

NBR_PATHS = [({"AMOF_NBR_NOCELL": "1"}, "fast"), ({"AMOF_NBR_FORCE_CELL": "1"}, "cell"), ({}, "frame"),
             ({"AMOF_NBR_SLABS": "1"}, "frame_slabs"), ({"AMOF_NBR_KERNEL": "v1"}, "exact")]


def _nbr_case(hip_ctx, pl, rcm, sets, triples, edges, runs, device=False, by_cn=False):
    packed = pl.packed
    kinds, sp = E._species(packed.numbers)
    S = len(kinds)
    s_ref, pa_ref = clib.cn_counts(packed.pos, packed.cell, sp, S, rcm, sets, per_atom=True)
    h_ref, a_ref = clib.bad_hist(packed.pos, packed.cell, sp, S, rcm, triples, edges)
    assert s_ref.sum() > 0 and a_ref.sum() > 0
    if by_cn:
        hc_ref, ac_ref = clib.bad_hist_by_cn(packed.pos, packed.cell, sp, S, rcm, triples, edges, 8)
    inputs = [packed, _device(packed)] if device else [packed]
    for env, path in runs:
        for inp in inputs:
            with _env(**env):
                s, pa = hip_ctx.cn_count(inp, rcm, sets, per_atom=True)
                ran = hip_ctx.last_path()
                assert ran == "cn_" + path, (env, ran)
                assert np.array_equal(s, s_ref) and np.array_equal(pa, pa_ref), \
                    (ran, int(np.abs(s - s_ref).sum()), np.argwhere(pa != pa_ref)[:8].tolist())
                hb, ab = hip_ctx.bad_hist(inp, rcm, triples, edges)
                ran = hip_ctx.last_path()
                assert ran == "bad_" + path, (env, ran)
                assert np.array_equal(ab, a_ref) and np.array_equal(hb, h_ref), \
                    (ran, int(np.abs(hb.astype(np.int64) - h_ref.astype(np.int64)).sum()))
                if by_cn:
                    hc, ac = hip_ctx.bad_hist_by_cn(inp, rcm, triples, edges, cn_max=8)
                    assert np.array_equal(ac, ac_ref) and np.array_equal(hc, hc_ref), (env, hip_ctx.last_path())


@pytest.mark.parametrize("cell", ["diagonal", "sheared", "npt"])
def test_cn_bad_paths(hip_ctx, cell):
    """cn_ / bad_ fast, cell, frame, frame_slabs, exact: pairs at rc (1 + delta) for every cutoff, triples at angle
    edges with legs at the cutoff; 3 or 5 frames; host and device input"""
    base = np.diag([21.31, 23.73, 26.91])
    c = {"diagonal": base, "sheared": base + np.array([[0, 0, 0], [3.1, 0, 0], [-2.3, 2.9, 0]]),
         "npt": _npt(base + np.array([[0, 0, 0], [1.7, 0, 0], [0, -2.1, 0]]), 5, 0.015, 8)}[cell]
    numbers, rcm, sets, triples = _nbr_setup(2400)
    for k, edges in enumerate((EDGES_REGULAR, EDGES_RAGGED)):
        pl = E.plant_nbr(c, numbers, rcm, seed=800 + k, F=None if cell == "npt" else 3, far=True, triples=triples,
                         angle_edges=edges)
        _nbr_case(hip_ctx, pl, rcm, sets, triples, edges, NBR_PATHS, device=k == 0, by_cn=k == 1 and cell != "npt")


@pytest.mark.parametrize("cell", ["diagonal", "sheared"])
def test_frame_tier_compact_records(hip_ctx, cell):
    """the frame tier's compact 16-bit records (AMOF_NBR_COMPACT=1): the coarsest band (guard_abs16)"""
    base = np.diag([21.31, 23.73, 26.91])
    c = base if cell == "diagonal" else base + np.array([[0, 0, 0], [3.1, 0, 0], [-2.3, 2.9, 0]])
    numbers, rcm, sets, triples = _nbr_setup(2400)
    pl = E.plant_nbr(c, numbers, rcm, seed=900, F=3, far=True, compact=True, triples=triples, angle_edges=EDGES_REGULAR)
    _nbr_case(hip_ctx, pl, rcm, sets, triples, EDGES_REGULAR, [({"AMOF_NBR_COMPACT": "1"}, "frame")])


def test_bad_exact_big_list(hip_ctx):
    """a dense one-species system whose centres hold more than 32 neighbours: bad_exact_biglist"""
    c = np.diag([17.93, 18.37, 19.11])
    numbers = np.full(2100, 8)
    rcm = np.array([[3.3]])
    pl = E.plant_nbr(c, numbers, rcm, seed=901, F=3, far=True, triples=[(0, 0)], angle_edges=EDGES_RAGGED)
    _, pa = clib.cn_counts(pl.packed.pos, pl.packed.cell, np.zeros(2100, np.int32), 1, rcm, [(0, 0)], per_atom=True)
    assert pa.max() > 32
    packed = pl.packed
    sp = np.zeros(len(numbers), np.int32)
    h_ref, a_ref = clib.bad_hist(packed.pos, packed.cell, sp, 1, rcm, [(0, 0)], EDGES_RAGGED)
    hb, ab = hip_ctx.bad_hist(packed, rcm, [(0, 0)], EDGES_RAGGED)
    assert hip_ctx.last_path() == "bad_exact_biglist"
    assert np.array_equal(ab, a_ref) and np.array_equal(hb, h_ref)
