"""Bond survival on the GPU (amof_bond_survival[_dev], BondLifetime): every counter bit-exact against the restatement of
tests/bond_ref.py, every forced path asserted through last_path()."""

import os
import sys

import numpy as np
import pytest

from amof_amd.frames import PackedTrajectory
from amof_amd.lags import window_setup
from tests import bond_ref as ref
from tests import edge_plant as E
from tests import helpers as H
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

EXACT = {"AMOF_BOND_EXACT": "1"}
FRAMES = {"AMOF_BOND_LAYOUT": "frames"}
DIAG = np.diag([17.31, 18.93, 21.77])
SHEARED = np.array([[17.31, 0.0, 0.0], [2.93, 18.11, 0.0], [-1.71, 3.37, 19.53]])


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


def _device(packed):
    import torch
    return PackedTrajectory(torch.as_tensor(packed.pos).cuda(), packed.cell, packed.numbers, pbc=packed.pbc)


def _walk(cell, numbers, F, seed, sigma=0.12, pbc=(True, True, True)):
    """host random walk in any cell (or per-frame cells): fractional coordinates, wrapped"""
    rng = np.random.default_rng(seed)
    cells = np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    N = len(numbers)
    s = rng.uniform(0, 1, (N, 3))
    pos = np.empty((F, N, 3))
    for f in range(F):
        pos[f] = (s - np.floor(s)) @ cells[0 if len(cells) == 1 else f]
        s = s + rng.normal(scale=sigma, size=(N, 3)) @ np.linalg.inv(cells[0])
    return PackedTrajectory(pos, cells if len(cells) > 1 else cells[0], np.asarray(numbers), pbc=pbc)


def _abi(packed, named):
    """(cutoff matrix, sets) of the C ABI from [(A number, B number, rc)]"""
    kinds, _ = ref.species(packed.numbers)
    rcm = np.zeros((len(kinds), len(kinds)))
    sets = []
    for a, b, rc in named:
        rcm[kinds.index(a), kinds.index(b)] = rcm[kinds.index(b), kinds.index(a)] = rc
        sets.append((kinds.index(a), kinds.index(b)))
    return rcm, sets


def _case(hip_ctx, packed, named, windows, runs, stride=1, device=False):
    """runs: [(env, path)]: each forced path must run and equal the restatement bit for bit"""
    want = ref.survival(packed.pos, packed.cell, packed.numbers, named, windows, stride, pbc=tuple(packed.pbc))
    assert want[:, :, 1].sum() > 0
    rcm, sets = _abi(packed, named)
    inputs = [packed, _device(packed)] if device else [packed]
    for env, path in runs:
        for inp in inputs:
            with _env(**env):
                got = hip_ctx.bond_survival(inp, rcm, sets, windows, origin_stride=stride)
                ran = hip_ctx.last_path()
            assert ran == path, (env, ran, path)
            assert got.dtype == np.uint64 and got.shape == want.shape
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (path, env, bad[:8].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    return want


def _numbers4(n):
    return np.repeat([1, 6, 7, 30], [n - 3 * (n // 4), n // 4, n // 4 - 1, n // 4 + 1])


FAST_RUNS = [({}, "bond_series"), (EXACT, "bond_series_exact"), (FRAMES, "bond_series"),
             (dict(EXACT, **FRAMES), "bond_series_exact")]


@pytest.mark.parametrize("stride", [1, 3])
def test_rectangular_one_species(hip_ctx, stride):
    # N = 150 and F = 131: neither a multiple of 64 (ragged words and tiles); lags beyond one word
    packed = _walk(DIAG, np.full(150, 30), 131, 11)
    want = _case(hip_ctx, packed, [(30, 30, 3.1)], [0, 1, 2, 5, 63, 64, 65, 100, 129], FAST_RUNS, stride=stride, device=True)
    assert np.any((want[0, :, 2] > 0) & (want[0, :, 2] < want[0, :, 1]) & (want[0, :, 1] < want[0, :, 0]))


@pytest.mark.parametrize("stride", [1, 3])
def test_rectangular_four_species(hip_ctx, stride):
    packed = _walk(DIAG, _numbers4(203), 70, 12)
    named = [(30, 7, 3.4), (7, 30, 3.4), (6, 6, 2.9), (1, 30, 3.0), (30, 30, 0.0)]      # (a zero cutoff: never neighbours)
    want = _case(hip_ctx, packed, named, [0, 3, 7, 7, 1, 40, 68, 69], FAST_RUNS, stride=stride, device=True)
    assert np.array_equal(want[0][:, 1:], want[1][:, 1:])      # h is symmetric: A-B and B-A share the pair counts
    assert want[4].sum() == 0


def test_sheared_cell(hip_ctx):
    packed = _walk(SHEARED, _numbers4(131), 67, 13)
    _case(hip_ctx, packed, [(30, 7, 3.3), (6, 1, 3.0)], [0, 1, 4, 30, 65], [({}, "bond_series_exact"), (FRAMES, "bond_series_exact")],
          device=True)


def test_npt_cells(hip_ctx):
    rng = np.random.default_rng(14)
    F = 45
    for base in (DIAG, SHEARED):
        cells = np.stack([base * (1.0 + 0.01 * rng.normal()) for _ in range(F)])
        packed = _walk(cells, _numbers4(97), F, 15)
        _case(hip_ctx, packed, [(30, 7, 3.5), (7, 7, 3.2)], [0, 2, 9, 43], [({}, "bond_series_exact")], stride=2, device=True)


def test_open_axis(hip_ctx):
    packed = _walk(DIAG, _numbers4(120), 50, 16, pbc=(True, False, True))
    _case(hip_ctx, packed, [(30, 7, 3.5), (1, 6, 3.2)], [0, 1, 10, 48], [({}, "bond_series_exact")], device=True)
    # with the open axis the shortest cell vector limits nothing: a cutoff above half of it on that axis is accepted
    thin = _walk(np.diag([17.31, 5.0, 21.77]), _numbers4(60), 20, 17, pbc=(True, False, True))
    _case(hip_ctx, thin, [(30, 7, 3.5)], [0, 1, 5], [({}, "bond_series_exact")])


def test_zif4_walk_bonds_break_and_reform(hip_ctx):
    tr = H.random_walk(H.zif4_frame(), 80, 0.05, 5)
    named = [(30, 7, 2.5), (6, 7, 1.6)]
    windows = [0, 1, 5, 20, 40, 78]
    want = ref.survival(tr.pos, tr.cell, tr.numbers, named, windows, pbc=tuple(tr.pbc))
    assert any(0 < c[2] < c[1] < c[0] for c in want[0]), want[0].tolist()
    path = "bond_series" if E.is_diagonal(tr.cell) else "bond_series_exact"
    _case(hip_ctx, tr, named, windows, [({}, path), (EXACT, "bond_series_exact")], device=True)


def _planted(where, seed, cell=DIAG):
    """four frames (0: unused filler, 1: the origin, 2: the intermediate frame, 3: origin + 2): the pairs edge_plant puts
    on both sides of rc inside the f32 guard band sit there in frame `where`; in the two other frames the same pairs are
    bonded beyond doubt (half the planted vector), so that every counter of lag 2 hangs on the planted decision.
    cell: the cell the pairs are planted in (tests/test_gpu_cell_forms.py plants them in other forms of it)"""
    numbers = np.repeat([7, 30], [160, 140])
    rcm = np.array([[3.1, 3.4], [3.4, 2.9]])
    pl = E.plant_nbr(cell, numbers, rcm, seed, F=1, far=True)
    p0 = pl.packed.pos[0]
    vec = p0[pl.j] - p0[pl.i]
    near = p0.copy()
    near[pl.j] = p0[pl.i] + 0.5 * (vec - pl.m @ cell) + pl.m @ cell
    frames = [near.copy(), near.copy(), near.copy(), near.copy()]
    frames[where] = p0
    return PackedTrajectory(np.stack(frames), cell, numbers), pl


@pytest.mark.parametrize("where", [1, 2, 3])
def test_guard_band_pairs_at_origin_middle_and_end(hip_ctx, where):
    packed, pl = _planted(where, 40 + where)
    named = [(30, 7, 3.4), (7, 30, 3.4), (7, 7, 3.1), (30, 30, 2.9)]
    windows = [0, 1, 2]
    want = _case(hip_ctx, packed, named, windows, [({}, "bond_series"), (EXACT, "bond_series_exact"), (FRAMES, "bond_series")])
    # the planting plants: pairs on both sides of rc, inside the band and around it (Planted.check has run); the inside
    # ones are bonded in all three frames, so lag 2 has survivors, and every one of them hangs on the planted decision
    t = pl.band_units()
    assert int((t < -1e-3).sum()) >= 5 and int((t > 1e-3).sum()) >= 5 and int((np.abs(t) <= 1.0).sum()) >= 5
    assert int(want[:, 2, 2].sum()) >= 2 * int((t < -1e-3).sum())


def test_tie_to_cn_atom_ranges_and_dev(hip_ctx):
    import torch
    packed = _walk(DIAG, _numbers4(203), 70, 21)
    named = [(30, 7, 3.4), (6, 6, 2.9), (1, 30, 3.0)]
    rcm, sets = _abi(packed, named)
    windows = [0, 1, 9, 0]
    for stride in (1, 4):
        full = hip_ctx.bond_survival(packed, rcm, sets, windows, origin_stride=stride)
        # lag 0, column 0: amof_cn_count's sums added over the origin frames, as integers
        sums = hip_ctx.cn_count(packed, rcm, sets)
        tie = sums[1::stride].sum(axis=0).astype(np.uint64)
        assert np.array_equal(full[:, 0, 0], tie) and np.array_equal(full[:, 3, 0], tie)
        assert np.array_equal(full[:, 0, 0], full[:, 0, 1]) and np.array_equal(full[:, 0, 0], full[:, 0, 2])
        # three ranges of centres add up to the full call bit for bit
        parts = [hip_ctx.bond_survival(packed, rcm, sets, windows, origin_stride=stride, atom_range=r)
                 for r in ((0, 61), (61, 180), (180, 203))]
        assert np.array_equal(parts[0] + parts[1] + parts[2], full)
        want = ref.survival(packed.pos, packed.cell, packed.numbers, named, windows, stride, centres=(61, 180))
        assert np.array_equal(parts[1], want)
        # the _dev form adds into a pre-filled buffer
        out = torch.full((len(sets), len(windows), 3), 7, dtype=torch.int64, device="cuda")
        hip_ctx.bond_survival(_device(packed), rcm, sets, windows, origin_stride=stride, atom_range=(61, 203), out=out)
        hip_ctx.bond_survival(packed, rcm, sets, windows, origin_stride=stride, atom_range=(0, 61), out=out)
        assert np.array_equal(out.cpu().numpy().view(np.uint64), full + np.uint64(7))
    # the pair table in groups of centres (a budget of 100 pairs) and the words of a group in chunks: the same bits
    with _env(AMOF_BOND_PAIR_BUDGET="100"):
        assert np.array_equal(hip_ctx.bond_survival(packed, rcm, sets, windows, origin_stride=4), full)
    with _env(AMOF_BOND_PAIR_BUDGET="1"):       # one centre per group
        assert np.array_equal(hip_ctx.bond_survival(packed, rcm, sets, windows, origin_stride=4, atom_range=(150, 203)),
                              ref.survival(packed.pos, packed.cell, packed.numbers, named, windows, 4, centres=(150, 203)))
    # scratch left by one call means nothing to the next
    hip_ctx.debug_poison(0xA5)
    assert np.array_equal(hip_ctx.bond_survival(packed, rcm, sets, windows, origin_stride=4), full)


def test_stage_seconds_after_a_call_and_after_one_without_sets(hip_ctx):
    packed = _walk(DIAG, _numbers4(64), 10, 23)
    rcm, sets = _abi(packed, [(30, 7, 3.0)])
    assert hip_ctx.bond_survival(packed, rcm, sets, [0, 1]).sum() > 0
    stages = hip_ctx.last_stage_seconds()
    assert sorted(stages) == ["corr", "rho", "self"] and all(v >= 0 for v in stages.values())      # lists, series, correlations
    # without a set the call returns before it starts device work: the record of the call before it stays as it was
    assert hip_ctx.bond_survival(packed, rcm, [], [0, 1]).shape == (0, 2, 3)
    assert hip_ctx.last_stage_seconds() == stages


def test_abi_refuses_cutoff_above_half_height_and_bad_arguments(hip_ctx):
    # AMOF_EINVAL surfaces as ValueError (amof_amd/_hip.py: Context._check)
    packed = _walk(DIAG, _numbers4(64), 10, 22)
    rcm, sets = _abi(packed, [(30, 7, 8.7)])           # > 17.31 / 2
    with pytest.raises(ValueError, match="half the smallest cell height"):
        hip_ctx.bond_survival(packed, rcm, sets, [0, 1])
    rcm, sets = _abi(packed, [(30, 7, 3.0)])
    for kw in (dict(windows=[10]), dict(windows=[-1]), dict(origin_stride=0), dict(atom_range=(5, 65)), dict(atom_range=(9, 3))):
        args = dict(windows=[0, 1], origin_stride=1, atom_range=None)
        args.update(kw)
        with pytest.raises(ValueError):
            hip_ctx.bond_survival(packed, rcm, sets, args["windows"], origin_stride=args["origin_stride"], atom_range=args["atom_range"])
    assert hip_ctx.bond_survival(packed, rcm, sets, [0, 1]).shape == (1, 2, 3)       # the context still works


def test_class_data_feather_and_async(hip_ctx, tmp_path, monkeypatch):
    from amof_amd.bond_lifetime import BondLifetime
    from amof_amd.cn import CoordinationNumber
    tr = H.random_walk(H.zif4_frame(), 80, 0.05, 5)
    cut = {'Zn-N': 2.5, 'C-N': 1.6, 'Zn-Au': 3.0}
    monkeypatch.setenv("AMOF_ASYNC", "1")
    obj = BondLifetime.from_trajectory(tr, cut, delta_time=5, timestep=1, origin_stride=2, device=0, distributed=False)
    assert obj.__dict__.get("_pending") is not None         # the constructor returned before anyone looked at .data
    data = obj.data
    assert obj.__dict__.get("_pending") is None
    window, time = window_setup(len(tr), 5, "half", 1)
    want = ref.survival(tr.pos, tr.cell, tr.numbers, [(30, 7, 2.5), (6, 7, 1.6)], window, 2, pbc=tuple(tr.pbc))
    assert np.array_equal(obj.counts, want) and obj.sets == ['Zn-N', 'C-N']
    assert list(data.columns) == ["Time", "Zn-N", "Zn-N-continuous", "C-N", "C-N-continuous", "Zn-Au", "Zn-Au-continuous"]
    assert np.array_equal(data["Time"].values, time)
    for k, name in enumerate(("Zn-N", "C-N")):
        w = want[k].astype(np.float64)
        np.testing.assert_allclose(data[name].values, w[:, 1] / w[:, 0], rtol=1e-15, atol=0)
        np.testing.assert_allclose(data[name + "-continuous"].values, w[:, 2] / w[:, 0], rtol=1e-15, atol=0)
        assert data[name].values[0] == 1.0 and data[name + "-continuous"].values[0] == 1.0
        assert np.all(data[name + "-continuous"].values <= data[name].values)
    assert np.all(np.isnan(data["Zn-Au"].values))
    assert np.array_equal(obj.n_origins, [len(ref.origins(len(tr), int(m), 2)) for m in window])
    s = data["Zn-N-continuous"].values
    assert obj.lifetime()["Zn-N"] == pytest.approx(float(np.sum(0.5 * (s[1:] + s[:-1]) * np.diff(time))), rel=1e-14)
    # the tie to CoordinationNumber through the classes: bonds at the origins of lag 0 = 16 Zn x mean CN summed
    cn = CoordinationNumber.from_trajectory(tr, {'Zn-N': 2.5}, device=0, distributed=False).data
    assert int(obj.counts[0, 0, 0]) == int(round(float(cn["Zn-N"].values[1::2].sum() * 16)))
    path = str(tmp_path / "walk")
    obj.write_to_file(path)
    assert os.path.exists(path + ".bond")
    assert BondLifetime.from_file(path).data.equals(data)
    # synchronous and device-resident give the same
    monkeypatch.setenv("AMOF_ASYNC", "0")
    again = BondLifetime.from_trajectory(_device(tr), cut, delta_time=5, timestep=1, origin_stride=2, device=0, distributed=False)
    assert again.__dict__.get("_pending") is None and again.data.equals(data)
    # refusal through the class on the GPU box as well
    with pytest.raises(ValueError):
        BondLifetime.from_trajectory(tr, {'Zn-N': 9.0}, delta_time=5, timestep=1, device=0, distributed=False)


def _build():
    return H.random_walk(H.zif4_frame(), 30, 0.05, 5, cell_jitter=0.003)


def _run(packed, distributed):
    from amof_amd.bond_lifetime import BondLifetime
    obj = BondLifetime.from_trajectory(packed, {'Zn-N': 2.5, 'C-N': 1.6}, delta_time=3, timestep=1, device=0, distributed=distributed)
    return obj.data, np.asarray(obj.counts)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    data, counts = _run(_build(), None)          # None: shard the centres over the initialised group
    data.to_pickle(os.path.join(out_dir, "bond_rank%d.pkl" % rank))
    np.save(os.path.join(out_dir, "bond_rank%d.npy" % rank), counts)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_single_process(tmp_path):
    # two ranks (gloo rendezvous; both on cuda:0 where the box has one GPU, as tests/test_gpu_dist.py)
    import pandas as pd
    import torch.multiprocessing as mp
    port = 33600 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    data, counts = _run(_build(), False)
    assert counts[:, 0, 0].min() > 0
    for rank in (0, 1):
        got = pd.read_pickle(os.path.join(str(tmp_path), "bond_rank%d.pkl" % rank))
        assert got.equals(data)
        assert np.array_equal(np.load(os.path.join(str(tmp_path), "bond_rank%d.npy" % rank)), counts)


def _worker_rccl(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", AMOF_DIST_FORCE_MERGE="1")     # one rank, but every collective really runs
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    from amof_amd import dist as adist
    assert adist.merging(1) and adist.device_collectives()
    data, counts = _run(_build(), None)
    data.to_pickle(os.path.join(out_dir, "bond_rccl.pkl"))
    np.save(os.path.join(out_dir, "bond_rccl.npy"), counts)
    dist.barrier()
    dist.destroy_process_group()


def test_rccl_backend_single_rank(tmp_path):
    # the device branch of the class (amof_bond_survival_dev into a CUDA tensor, all-reduced in place, read back as u64),
    # with the one rank a single-GPU box allows (pattern of tests/test_gpu_dist.py)
    import pandas as pd
    import torch.multiprocessing as mp
    port = 35600 + os.getpid() % 2000
    mp.spawn(_worker_rccl, args=(1, port, str(tmp_path)), nprocs=1, join=True)
    data, counts = _run(_build(), False)
    assert pd.read_pickle(os.path.join(str(tmp_path), "bond_rccl.pkl")).equals(data)
    got = np.load(os.path.join(str(tmp_path), "bond_rccl.npy"))
    assert got.dtype == np.uint64 and np.array_equal(got, counts)
