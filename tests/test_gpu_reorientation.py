"""Bond reorientation on the GPU (amof_bond_reorientation[_dev], BondReorientation): the pair counter bit-exact against
amof_bond_survival's, the fixed-point sums within the derived budget of tests/reorientation_ref.py and bit-identical between
every forced path, atom range and chunking; last_path() asserted per run.  Inputs: tests/reorientation_cases.py."""

import os
import sys

import numpy as np
import pytest

from amof_amd.lags import window_setup
from tests import bond_ref
from tests import reorientation_cases as cases
from tests import reorientation_ref as ref
from tests.conftest import ROOT
from tests.test_gpu_bond import EXACT, FRAMES, _abi, _device, _env

pytestmark = pytest.mark.gpu

FAST_RUNS = [({}, "bond_reorient"), (EXACT, "bond_reorient_exact"), (FRAMES, "bond_reorient"),
             (dict(EXACT, **FRAMES), "bond_reorient_exact")]
EXACT_RUNS = [({}, "bond_reorient_exact")]


def _case(hip_ctx, name, runs, stride=1, device=False):
    """every forced path of ``runs`` on a case: the pair counter equals bond_survival's intermittent one, the sums lie within
    the restatement's budget, every run gives the same bits; returns (out, scale, Result)"""
    c = cases.case(name)
    packed = c.packed
    want = cases.reference(name, stride)
    assert want.n.sum() > 0
    rcm, sets = _abi(packed, c.sets)
    surv = hip_ctx.bond_survival(packed, rcm, sets, c.lags, origin_stride=stride)
    scale_want = ref.scales(packed.numbers, c.sets, packed.pos.shape[0], stride)
    first = None
    inputs = [packed, _device(packed)] if device else [packed]
    for env, path in runs:
        for inp in inputs:
            with _env(**env):
                got, scale = hip_ctx.bond_reorientation(inp, rcm, sets, c.lags, origin_stride=stride)
                ran = hip_ctx.last_path()
            assert ran == path, (env, ran, path)
            assert got.dtype == np.int64 and got.shape == surv.shape and scale.dtype == np.int32
            assert scale.tolist() == scale_want
            assert np.array_equal(got[:, :, 0].view(np.uint64), surv[:, :, 1]), (path, env)
            worst = ref.check(got, scale, want)
            print("%s stride %d %s: largest |difference| / budget = %.3g" % (name, stride, path, worst))
            if first is None:
                first = got
            assert np.array_equal(got, first), (path, env, np.argwhere(got != first)[:8].tolist())
    return first, scale_want, want


@pytest.mark.parametrize("stride", [1, 3])
def test_rectangular_one_species(hip_ctx, stride):
    # N = 150 and F = 131: neither a multiple of 64 (ragged words and tiles); lags beyond one word
    got, scale, want = _case(hip_ctx, "rect", FAST_RUNS, stride=stride, device=True)
    c2 = got[0, :, 2] * 2.0 ** -scale[0] / got[0, :, 0]
    assert np.any((c2 > 0.0) & (c2 < 0.9)), c2.tolist()         # the walk turns the bonds: not a trivial case


@pytest.mark.parametrize("stride", [1, 3])
def test_rectangular_four_species(hip_ctx, stride):
    got, scale, want = _case(hip_ctx, "four", FAST_RUNS, stride=stride, device=True)
    assert scale[0] == scale[1]
    assert np.array_equal(got[0], got[1])       # A-B and B-A: u -> -u at both ends, the same cosines bit for bit
    assert got[0, :, 0].sum() > 0
    assert not got[4].any()                     # zero cutoff
    assert np.array_equal(got[:, 2], got[:, 3])                 # the lag 7 given twice


def test_sheared_cell(hip_ctx):
    _case(hip_ctx, "sheared", EXACT_RUNS + [(FRAMES, "bond_reorient_exact")], device=True)


@pytest.mark.parametrize("name", ["npt_diag", "npt_sheared"])
def test_npt_cells(hip_ctx, name):
    _case(hip_ctx, name, EXACT_RUNS, stride=2, device=True)


@pytest.mark.parametrize("name", ["open", "open_thin"])
def test_open_axis(hip_ctx, name):
    _case(hip_ctx, name, EXACT_RUNS)


@pytest.mark.parametrize("name,stride", [("rect", 1), ("rect", 3), ("four", 1), ("four", 3), ("sheared", 1), ("npt_diag", 2),
                                         ("composition", 4)])
def test_lag_zero_is_exactly_one(hip_ctx, name, stride):
    c = cases.case(name)
    rcm, sets = _abi(c.packed, c.sets)
    got, scale = hip_ctx.bond_reorientation(c.packed, rcm, sets, c.lags, origin_stride=stride)
    zero = [w for w, m in enumerate(c.lags) if m == 0]
    assert zero and got[:, zero, 0].sum() > 0
    for s in range(len(sets)):
        for w in zero:
            assert got[s, w, 1] == got[s, w, 2] == int(got[s, w, 0]) << int(scale[s]), (s, w, got[s, w].tolist(), scale[s])


@pytest.mark.parametrize("where", [1, 2, 3])
def test_guard_band_pairs_at_origin_middle_and_end(hip_ctx, where):
    name = "planted%d" % where
    got, scale, want = _case(hip_ctx, name, [({}, "bond_reorient"), (EXACT, "bond_reorient_exact"), (FRAMES, "bond_reorient")])
    # the planting plants: pairs on both sides of rc, inside the band and around it; the fast and the exact decision agree
    # on every one of them (the pair counter is the survival counter on both, asserted in _case) and the sums are identical
    pl = cases.planted(where, 40 + where)[1]
    t = pl.band_units()
    assert int((t < -1e-3).sum()) >= 5 and int((t > 1e-3).sum()) >= 5 and int((np.abs(t) <= 1.0).sum()) >= 5
    assert int(got[:, 2, 0].sum()) >= 2 * int((t < -1e-3).sum())


@pytest.mark.parametrize("where", [1, 2, 3])
def test_guard_band_pairs_thousands_of_cells_apart(hip_ctx, where):
    # test_gpu_bond.py's own planting, half of its pairs shifted by up to 9000 cells: the vector kernel subtracts thousands of
    # cell vectors there.  Float64 resolves such a vector to 1e-10 only, so no restatement is held against the sums: the pair
    # counter is the survival counter on both decisions, and the sums of the two decisions and layouts are the same bits
    from tests.test_gpu_bond import _planted
    packed, pl = _planted(where, 40 + where)
    rcm, sets = _abi(packed, cases.PLANT_SETS)
    surv = hip_ctx.bond_survival(packed, rcm, sets, [0, 1, 2])
    first = None
    for env, path in [({}, "bond_reorient"), (EXACT, "bond_reorient_exact"), (FRAMES, "bond_reorient")]:
        with _env(**env):
            got, scale = hip_ctx.bond_reorientation(packed, rcm, sets, [0, 1, 2])
            assert hip_ctx.last_path() == path
        assert np.array_equal(got[:, :, 0].view(np.uint64), surv[:, :, 1]), path
        first = got if first is None else first
        assert np.array_equal(got, first), path
    assert np.all(first[:, 0, 1] == first[:, 0, 0] << scale.astype(np.int64)) and np.array_equal(first[:, 0, 1], first[:, 0, 2])
    assert np.array_equal(first[0], first[1])                   # Zn-N and N-Zn
    t = pl.band_units()
    assert int((t < -1e-3).sum()) >= 5 and int((t > 1e-3).sum()) >= 5 and int((np.abs(t) <= 1.0).sum()) >= 5
    assert int(first[:, 2, 0].sum()) >= 2 * int((t < -1e-3).sum())


def test_atom_ranges_dev_form_budgets_and_poison(hip_ctx):
    import torch
    c = cases.case("composition")
    packed = c.packed
    rcm, sets = _abi(packed, c.sets)
    windows = c.lags
    for stride in (1, 4):
        full, scale = hip_ctx.bond_reorientation(packed, rcm, sets, windows, origin_stride=stride)
        ref.check(full, scale, cases.reference("composition", stride))
        assert np.array_equal(full[:, 0], full[:, 3])
        # three ranges of centres add up to the full call bit for bit, with the scale of the full call
        parts = [hip_ctx.bond_reorientation(packed, rcm, sets, windows, origin_stride=stride, atom_range=r)
                 for r in ((0, 61), (61, 180), (180, 203))]
        assert all(p[1].tolist() == scale.tolist() for p in parts)
        assert np.array_equal(parts[0][0] + parts[1][0] + parts[2][0], full)
        ref.check(parts[1][0], scale, cases.reference("composition", stride, (61, 180)))
        # the _dev form adds into a pre-filled buffer
        out = torch.full((len(sets), len(windows), 3), 7, dtype=torch.int64, device="cuda")
        hip_ctx.bond_reorientation(_device(packed), rcm, sets, windows, origin_stride=stride, atom_range=(61, 203), out=out)
        _, sc = hip_ctx.bond_reorientation(packed, rcm, sets, windows, origin_stride=stride, atom_range=(0, 61), out=out)
        assert sc.tolist() == scale.tolist()
        assert np.array_equal(out.cpu().numpy(), full + 7)
    # the pair table in groups of centres (a budget of 100 pairs; of 1: one centre per group): the same bits
    with _env(AMOF_BOND_PAIR_BUDGET="100"):
        assert np.array_equal(hip_ctx.bond_reorientation(packed, rcm, sets, windows, origin_stride=4)[0], full)
    with _env(AMOF_BOND_PAIR_BUDGET="1"):
        assert np.array_equal(hip_ctx.bond_reorientation(packed, rcm, sets, windows, origin_stride=4)[0], full)
    # scratch left by one call means nothing to the next
    hip_ctx.debug_poison(0xA5)
    assert np.array_equal(hip_ctx.bond_reorientation(packed, rcm, sets, windows, origin_stride=4)[0], full)
    stages = hip_ctx.last_stage_seconds()
    assert all(v >= 0 for v in stages.values())      # lists, series, vectors + sums
    # two contexts of one device sharing the centres (MultiContext): the shards add up, the scale is the full call's
    from amof_amd import _hip
    multi = _hip.MultiContext([0, 0])
    try:
        m, msc = multi.bond_reorientation(packed, rcm, sets, windows, origin_stride=4)
        part, _ = multi.bond_reorientation(packed, rcm, sets, windows, origin_stride=4, atom_range=(61, 180))
    finally:
        multi.close()
    assert np.array_equal(m, full) and msc.tolist() == scale.tolist()
    assert np.array_equal(part, parts[1][0])


def test_zero_length_vector_is_an_error_return(hip_ctx):
    p = cases.coincident()
    rcm, sets = _abi(p, [(30, 7, 3.0)])
    with pytest.raises(ZeroDivisionError):
        hip_ctx.bond_reorientation(p, rcm, sets, [0, 1])
    import torch
    out = torch.full((1, 2, 3), 5, dtype=torch.int64, device="cuda")
    with pytest.raises(ZeroDivisionError):
        hip_ctx.bond_reorientation(p, rcm, sets, [0, 1], out=out)
    assert int((out.cpu() != 5).sum()) == 0                     # nothing was added
    # the context works afterwards
    good = cases.case("arguments")
    got, scale = hip_ctx.bond_reorientation(good.packed, rcm, sets, [0, 1])
    ref.check(got, scale, cases.reference("arguments", 1))


def test_abi_refuses_cutoff_above_half_height_and_bad_arguments(hip_ctx):
    packed = cases.case("arguments").packed
    rcm, sets = _abi(packed, [(30, 7, 8.7)])           # > 17.31 / 2
    with pytest.raises(ValueError, match="half the smallest cell height"):
        hip_ctx.bond_reorientation(packed, rcm, sets, [0, 1])
    rcm, sets = _abi(packed, [(30, 7, 3.0)])
    for kw in (dict(windows=[10]), dict(windows=[-1]), dict(origin_stride=0), dict(atom_range=(5, 65)), dict(atom_range=(9, 3))):
        args = dict(windows=[0, 1], origin_stride=1, atom_range=None)
        args.update(kw)
        with pytest.raises(ValueError):
            hip_ctx.bond_reorientation(packed, rcm, sets, args["windows"], origin_stride=args["origin_stride"],
                                       atom_range=args["atom_range"])
    got, scale = hip_ctx.bond_reorientation(packed, rcm, sets, [0, 1])       # the context still works
    assert got.shape == (1, 2, 3) and scale.shape == (1,)
    got, scale = hip_ctx.bond_reorientation(packed, rcm, [], [0, 1])
    assert got.shape == (0, 2, 3) and scale.shape == (0,)


def test_class_data_feather_and_async(hip_ctx, tmp_path, monkeypatch):
    from amof_amd.bond_reorientation import BondReorientation
    tr = cases.case("class").packed
    monkeypatch.setenv("AMOF_ASYNC", "1")
    obj = BondReorientation.from_trajectory(tr, cases.CLASS_CUT, delta_time=5, timestep=1, origin_stride=2, device=0,
                                            distributed=False)
    assert obj.__dict__.get("_pending") is not None         # the constructor returned before anyone looked at .data
    data = obj.data
    assert obj.__dict__.get("_pending") is None
    window, time = window_setup(len(tr), 5, "half", 1)
    want = cases.reference("class", 2)
    assert obj.sets == ['Zn-N', 'C-N'] and np.asarray(obj.counts).dtype == np.int64
    assert list(data.columns) == ["Time", "Zn-N-P1", "Zn-N-P2", "C-N-P1", "C-N-P2", "Zn-Au-P1", "Zn-Au-P2"]
    assert np.array_equal(data["Time"].values, time)
    assert list(obj.scale_log2) == ref.scales(tr.numbers, cases.CLASS_SETS, len(tr), 2)
    ref.check(obj.counts, obj.scale_log2, want)
    for k, name in enumerate(("Zn-N", "C-N")):
        p1, p2 = data[name + "-P1"].values, data[name + "-P2"].values
        assert p1[0] == 1.0 and p2[0] == 1.0
        assert np.all(p2 >= -0.5) and np.all(p2 <= 1.0) and np.all(np.abs(p1) <= 1.0)
        n = want.n[k].astype(np.float64)
        assert np.all(np.abs(p1 - want.sums[k, :, 0] / n) <= want.budget[k, :, 0] / n + 4 * ref.EPS)
        assert np.all(np.abs(p2 - want.sums[k, :, 1] / n) <= want.budget[k, :, 1] / n + 4 * ref.EPS)
    assert np.all(np.isnan(data["Zn-Au-P1"].values)) and np.all(np.isnan(data["Zn-Au-P2"].values))
    assert np.array_equal(obj.n_origins, [len(bond_ref.origins(len(tr), int(m), 2)) for m in window])
    s = data["Zn-N-P2"].values
    assert obj.relaxation_time()["Zn-N"] == pytest.approx(float(np.sum(0.5 * (s[1:] + s[:-1]) * np.diff(time))), rel=1e-14)
    path = str(tmp_path / "walk")
    obj.write_to_file(path)
    assert os.path.exists(path + ".reor")
    assert BondReorientation.from_file(path).data.equals(data)
    # synchronous and device-resident give the same
    monkeypatch.setenv("AMOF_ASYNC", "0")
    again = BondReorientation.from_trajectory(_device(tr), cases.CLASS_CUT, delta_time=5, timestep=1, origin_stride=2, device=0,
                                              distributed=False)
    assert again.__dict__.get("_pending") is None and again.data.equals(data)
    assert np.array_equal(again.counts, obj.counts)
    with pytest.raises(ValueError):
        BondReorientation.from_trajectory(tr, {'Zn-N': 9.0}, delta_time=5, timestep=1, device=0, distributed=False)


def _run(packed, distributed):
    from amof_amd.bond_reorientation import BondReorientation
    obj = BondReorientation.from_trajectory(packed, cases.RANK_CUT, delta_time=3, timestep=1, device=0, distributed=distributed)
    return obj.data, np.asarray(obj.counts)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    data, counts = _run(cases.case("ranks").packed, None)          # None: shard the centres over the initialised group
    data.to_pickle(os.path.join(out_dir, "reor_rank%d.pkl" % rank))
    np.save(os.path.join(out_dir, "reor_rank%d.npy" % rank), counts)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_single_process(tmp_path):
    # two ranks (gloo rendezvous; both on cuda:0 where the box has one GPU, as tests/test_gpu_bond.py)
    import pandas as pd
    import torch.multiprocessing as mp
    port = 37600 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    data, counts = _run(cases.case("ranks").packed, False)
    assert counts[:, 0, 0].min() > 0
    ref.check(counts, ref.scales(cases.case("ranks").packed.numbers, cases.CLASS_SETS, 30), cases.reference("ranks", 1))
    for rank in (0, 1):
        got = pd.read_pickle(os.path.join(str(tmp_path), "reor_rank%d.pkl" % rank))
        assert got.equals(data)
        assert np.array_equal(np.load(os.path.join(str(tmp_path), "reor_rank%d.npy" % rank)), counts)


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
    data, counts = _run(cases.case("ranks").packed, None)
    data.to_pickle(os.path.join(out_dir, "reor_rccl.pkl"))
    np.save(os.path.join(out_dir, "reor_rccl.npy"), counts)
    dist.barrier()
    dist.destroy_process_group()


def test_rccl_backend_single_rank(tmp_path):
    # the device branch of the class (amof_bond_reorientation_dev into a CUDA tensor, all-reduced in place, read back)
    import pandas as pd
    import torch.multiprocessing as mp
    port = 39600 + os.getpid() % 2000
    mp.spawn(_worker_rccl, args=(1, port, str(tmp_path)), nprocs=1, join=True)
    data, counts = _run(cases.case("ranks").packed, False)
    assert pd.read_pickle(os.path.join(str(tmp_path), "reor_rccl.pkl")).equals(data)
    got = np.load(os.path.join(str(tmp_path), "reor_rccl.npy"))
    assert got.dtype == np.int64 and np.array_equal(got, counts)
