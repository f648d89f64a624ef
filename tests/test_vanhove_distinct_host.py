"""DistinctVanHove host logic (no GPU): origins, the work list and its shards, the rmax clamp, assembly and normalisation
against Rdf's, the DataFrame schema and file round trip, argument checks, and the reference construction of
tests/vanhove_distinct_ref.py against a plain numpy double loop."""

import os

import numpy as np
import pytest

from amof_amd import dist
from amof_amd import lags
from amof_amd import vanhove_distinct as vd
from amof_amd.frames import PackedTrajectory
from amof_amd.lags import window_setup
from amof_amd.rdf import Rdf
from tests import vanhove_distinct_ref as ref


def test_origins_and_counts_per_lag():
    F = 11
    windows = [0, 1, 4, 9, 10]
    for s in (1, 2, 3, 7):
        n = lags.n_origins(F, windows, s)
        for w, m in enumerate(windows):
            want = [k for k in range(1, F) if k <= F - m - 1 and (k - 1) % s == 0]
            assert list(lags.origins(F, m, s)) == want
            assert n[w] == len(want)
    assert lags.n_origins(F, [10], 1)[0] == 0 and lags.n_origins(F, [9], 1)[0] == 1
    # stride 1: WindowVanHove's origins k = 1 .. F - m - 1
    assert list(lags.n_origins(F, windows)) == [F - m - 1 for m in windows]


@pytest.mark.parametrize("world", [1, 2, 3, 5, 8])
def test_work_shards_cover_every_pair_once(world):
    F = 23
    windows, _ = window_setup(F, 3)
    wl, kl = lags.work_list(F, windows, 2)
    assert len(wl) == lags.n_origins(F, windows, 2).sum()
    assert np.all(np.diff(wl) >= 0)                                    # lag-major
    seen = []
    for r in range(world):
        lo, hi = dist.shard_range(len(wl), r, world)
        seen += list(zip(wl[lo:hi], kl[lo:hi]))
    assert len(seen) == len(set(seen)) == len(wl)
    assert set(seen) == {(w, k) for w, m in enumerate(windows) for k in lags.origins(F, m, 2)}


def test_rmax_clamp_and_bins():
    lengths = np.array([[12.0, 15.0, 20.0], [11.5, 15.0, 20.0]])
    assert vd.clamp_rmax(lengths, "half_cell") == 5.75
    assert vd.clamp_rmax(lengths, 9.0) == 5.75
    assert vd.clamp_rmax(lengths, 4.0) == 4.0
    assert int(vd.clamp_rmax(lengths, "half_cell") // 0.01) == 574       # Python floor division, as Rdf
    with pytest.raises(ValueError):
        vd.clamp_rmax(lengths, "whole_cell")


def _packed(F=9, seed=3):
    rng = np.random.default_rng(seed)
    numbers = np.array([30] * 5 + [7] * 11 + [6] * 9 + [1] * 7)
    cells = np.stack([np.diag([11.0, 12.5, 13.0]) * (1 + 0.01 * rng.uniform(-1, 1)) for _ in range(F)])
    pos = rng.uniform(0, 1, (F, len(numbers), 3)) @ cells[0]
    return PackedTrajectory(pos, cells, numbers)


def test_assembly_at_t0_equals_rdf_and_schema():
    packed = _packed()
    F, N = len(packed), packed.n_atoms
    windows, time = window_setup(F, 2, timestep=1)
    kinds = sorted(set(int(z) for z in packed.numbers))
    S, W, nbins = len(kinds), len(windows), 40
    rmax = 5.0
    rng = np.random.default_rng(1)
    hist = rng.integers(0, 1000, (S, S, W, nbins)).astype(np.uint64)
    n_orig = lags.n_origins(F, windows)
    vol = vd.mean_volumes(packed.cell, F, windows)
    elements = packed.unique_numbers()
    df = vd.assemble(hist, kinds, elements, packed.species_counts(), N, n_orig, vol, time, rmax, nbins, 0.12)
    syms = {1: "H", 6: "C", 7: "N", 30: "Zn"}
    names = ["Time", "r", "X-X"] + [syms[a] + "-" + syms[b] for a in elements for b in elements] + [syms[a] + "-X" for a in elements]
    assert list(df.columns) == names and len(df) == W * nbins
    np.testing.assert_array_equal(df["Time"].values, np.repeat(time, nbins))
    np.testing.assert_array_equal(df["r"].values, np.tile(np.arange(nbins) * 0.12, W))
    # t = 0: Rdf's assembly of the same counts over frames 1 .. F-1
    r = Rdf()
    r._finish(packed, hist[:, :, 0], float(np.sum(packed.volumes()[1:])), F - 1, kinds, elements, rmax, nbins,
              np.arange(nbins) * 0.12)
    t0 = df.iloc[:nbins]
    for c in r.data.columns:
        np.testing.assert_allclose(t0[c].values, r.data[c].values, rtol=1e-12, atol=0)
    # every lag: ncount = n_origins N_a, the mean volume over its own origin frames
    w = W - 1
    a, b = kinds.index(30), kinds.index(7)
    from amof_amd.rdf import normalize_rdf
    k = lags.origins(F, windows[w])
    want = normalize_rdf(hist[a, b, w], len(k) * 5, N, np.mean(packed.volumes()[k]), rmax, nbins)
    np.testing.assert_allclose(df["Zn-N"].values[w * nbins:], want, rtol=1e-14)
    # a lag without origins: NaN volume, rows still there
    assert np.isnan(vd.mean_volumes(packed.cell, F, [F - 1])[0])


def test_feather_round_trip(tmp_path):
    packed = _packed()
    windows, time = window_setup(len(packed), 2)
    kinds = sorted(set(int(z) for z in packed.numbers))
    hist = np.ones((len(kinds), len(kinds), len(windows), 30), dtype=np.uint64)
    vh = vd.DistinctVanHove()
    vh._assemble(hist, kinds, packed, packed.unique_numbers(), lags.n_origins(len(packed), windows), windows, time, 4.0, 30, 0.13, 1)
    p = os.path.join(str(tmp_path), "gd")
    vh.write_to_file(p)
    assert os.path.exists(p + ".vanhove_distinct")
    back = vd.DistinctVanHove.from_file(p)
    assert back.data.equals(vh.data)
    assert list(vh.n_origins) == list(lags.n_origins(len(packed), windows)) and vh.rmax == 4.0 and vh.kinds == kinds


@pytest.mark.parametrize("kw", [dict(origin_stride=0), dict(origin_stride=-2), dict(origin_stride=1.5), dict(dr=0.0),
                                dict(dr=-0.01)])
def test_bad_arguments_are_rejected(kw):
    with pytest.raises(ValueError):
        vd.DistinctVanHove.from_trajectory(_packed(), delta_time=2, **kw)


@pytest.mark.parametrize("stride", [1, 2])
def test_reference_construction_equals_a_numpy_double_loop(stride):
    packed = _packed(F=7, seed=stride)
    windows, _ = window_setup(len(packed), 1)
    rmax, nbins = 5.4, 37
    # one cell for every frame here: the numpy loop takes frame k's cell like the oracle construction
    got = ref.distinct_hist(packed.pos, packed.cell, packed.numbers, windows, rmax, nbins, stride)
    want = ref.numpy_hist(packed.pos, packed.cell, packed.numbers, windows, rmax, nbins, stride)
    assert got.sum() > 0 and np.array_equal(got, want)
    # at lag 0 the counts are the oracle's RDF over frames 1 .. F-1 (no self images below half the cell)
    from oracle import clib
    kinds, sp = ref.species(packed.numbers)
    if stride == 1:
        rdf, _ = clib.rdf_hist(packed.pos[1:], packed.cell[1:], sp, len(kinds), rmax, nbins)
        assert np.array_equal(got[:, :, 0], rdf)
    # a work range is a slice of the whole
    n = int(lags.n_origins(len(packed), windows, stride).sum())
    a = ref.distinct_hist(packed.pos, packed.cell, packed.numbers, windows, rmax, nbins, stride, work_range=(0, n // 2))
    b = ref.distinct_hist(packed.pos, packed.cell, packed.numbers, windows, rmax, nbins, stride, work_range=(n // 2, n))
    assert np.array_equal(a + b, got)
