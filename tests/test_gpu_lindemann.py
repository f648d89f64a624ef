"""Lindemann index on the GPU (amof_lindemann[_dev], Lindemann): pair counts and histograms bit-exact against the restatement of
tests/lindemann_ref.py, the fixed-point sums within its derived budget and bit-identical between both kernels, host and device
input, atom ranges and every chunking; last_path() asserted per run.  Inputs: tests/lindemann_cases.py (whose two conditions --
budgets below 2^-30, no delta within its budget of a bin edge -- tests/test_lindemann_host.py asserts)."""

import os
import sys

import numpy as np
import pytest

from tests import lindemann_cases as cases
from tests import lindemann_ref as ref
from tests.conftest import ROOT
from tests.test_gpu_bond import _abi, _device, _env

pytestmark = pytest.mark.gpu

SIMPLE = {"AMOF_LINDEMANN_SIMPLE": "1"}
RUNS = [({}, "lindemann_chunk"), (SIMPLE, "lindemann_simple")]
DD, NB = cases.DDELTA, cases.NBINS


def _call(ctx, packed, rcm, sets, B, S, select=0, **kw):
    return ctx.lindemann(packed, rcm, sets, B, S, NB, DD, select=select, **kw)


def _case(hip_ctx, name, device=False, selects=(0, 1)):
    """every block arithmetic of a case on both kernels (and both inputs): counts and histograms equal the restatement's, the
    sums lie within its budget, every run gives the same bits; returns {(B, S, select): (sums, hist, scale)}"""
    c = cases.case(name)
    packed = c.packed
    rcm, sets = _abi(packed, c.sets)
    inputs = [packed, _device(packed)] if device else [packed]
    out = {}
    for B, S in c.blocks:
        scale_want = ref.scales(packed.numbers, c.sets, B)
        for select in selects:
            want = cases.reference(name, B, S, select)
            first = None
            for env, path in RUNS:
                for inp in inputs:
                    with _env(**env):
                        sums, hist, scale = _call(hip_ctx, inp, rcm, sets, B, S, select)
                        ran = hip_ctx.last_path()
                    assert ran == path, (env, ran, path)
                    assert sums.dtype == np.int64 and hist.dtype == np.uint64 and scale.dtype == np.int32
                    assert sums.shape == (len(want.starts), len(sets), 2) and hist.shape == (len(want.starts), len(sets), NB)
                    assert scale.tolist() == scale_want
                    worst = ref.check(sums, scale, want)
                    print("%s B %d S %d select %d %s: largest |difference| / budget = %.3g" % (name, B, S, select, path, worst))
                    assert np.array_equal(hist, ref.hist(want, DD, NB)), (name, B, S, select, path)
                    assert np.array_equal(hist.sum(axis=2), sums[:, :, 0].astype(np.uint64))
                    if first is None:
                        first = (sums, hist)
                    assert np.array_equal(sums, first[0]) and np.array_equal(hist, first[1]), (name, B, S, select, path)
            if select == 0:
                # the pairs of a block are amof_cn_count's neighbours at the block's first frame
                cn = hip_ctx.cn_count(packed, rcm, sets)
                assert np.array_equal(first[0][:, :, 0], cn[want.starts]), (name, B, S)
            out[(B, S, select)] = first + (scale_want,)
    return out


def test_rectangular_one_species(hip_ctx):
    # N = 150 and F = 131: ragged waves, tiles and chunks; every block arithmetic of cases.RECT_BLOCKS
    got = _case(hip_ctx, "rect", device=True)
    # 'first' against 'block': the same pairs in block 0, another population later on a walk that breaks bonds
    blk, fst = got[(20, 20, 0)], got[(20, 20, 1)]
    assert np.array_equal(blk[0][0], fst[0][0]) and np.array_equal(blk[1][0], fst[1][0])
    assert np.all(fst[0][:, 0, 0] == fst[0][0, 0, 0]) and np.any(blk[0][1:, 0, 0] != fst[0][1:, 0, 0])
    assert len(got[(50, 27, 0)][0]) == 4 and len(got[(64, 67, 0)][0]) == 2


@pytest.mark.parametrize("name", ["four", "four@rot"])
def test_four_species(hip_ctx, name):
    got = _case(hip_ctx, name, device=name == "four")
    for key, (sums, hist, scale) in got.items():
        assert scale[0] == scale[1]
        assert np.array_equal(sums[:, 0], sums[:, 1]) and np.array_equal(hist[:, 0], hist[:, 1])     # A-B and B-A: d_ij = d_ji
        assert sums[:, 0, 0].min() > 0
        assert not sums[:, 4].any() and not hist[:, 4].any()                                         # zero cutoff


@pytest.mark.parametrize("name", ["sheared", "sheared@mirror", "npt_diag", "npt_sheared", "open"])
def test_general_cells(hip_ctx, name):
    _case(hip_ctx, name, device=name in ("sheared", "npt_sheared"))


def test_atom_ranges_dev_form_budgets_chunks_and_poison(hip_ctx):
    import torch
    c = cases.case("composition")
    packed = c.packed
    rcm, sets = _abi(packed, c.sets)
    B, S = c.blocks[0]
    full = _call(hip_ctx, packed, rcm, sets, B, S, per_atom=True)
    want = cases.reference("composition", B, S)
    ref.check(full[0], full[2], want)
    # per_atom: counts exact, sums within the budget, rows add up to the set sums bit for bit
    n, tot, bud = ref.per_atom(want, packed.n_atoms)
    pa = full[3]
    assert pa.dtype == np.int64 and np.array_equal(pa[..., 0], n)
    q = np.ldexp(1.0, -full[2].astype(np.int64))[None, :, None]
    assert np.all(np.abs(pa[..., 1] * q - tot) <= bud + n * 0.5 * q + n * n * ref.EPS * 8)
    assert np.array_equal(pa.sum(axis=2), full[0])
    # three ranges of centres add up to the full call bit for bit, with the scale of the full call
    parts = [_call(hip_ctx, packed, rcm, sets, B, S, atom_range=r, per_atom=True) for r in ((0, 61), (61, 180), (180, 203))]
    assert all(p[2].tolist() == full[2].tolist() for p in parts)
    for k in (0, 1, 3):
        assert np.array_equal(parts[0][k] + parts[1][k] + parts[2][k], full[k])
    ref.check(parts[1][0], full[2], cases.reference("composition", B, S, 0, (61, 180)))
    assert not parts[1][3][:, :, :61].any() and not parts[1][3][:, :, 180:].any()
    # the _dev form adds into pre-filled buffers
    nb = len(want.starts)
    out = (torch.full((nb, len(sets), 2), 7, dtype=torch.int64, device="cuda"), torch.full((nb, len(sets), NB), 3, dtype=torch.int64, device="cuda"))
    _call(hip_ctx, _device(packed), rcm, sets, B, S, atom_range=(61, 203), out=out)
    res = _call(hip_ctx, packed, rcm, sets, B, S, atom_range=(0, 61), out=out)
    assert res[2].tolist() == full[2].tolist()
    assert np.array_equal(out[0].cpu().numpy(), full[0] + 7) and np.array_equal(out[1].cpu().numpy().view(np.uint64), full[1] + np.uint64(3))
    # the pair table in groups of centres (a budget of 100 pairs; of 1: one centre per group), the partial sums in chunks of 64
    # pairs and single blocks: the same bits, on both kernels
    for env in (dict(AMOF_BOND_PAIR_BUDGET="100"), dict(AMOF_BOND_PAIR_BUDGET="1"), dict(AMOF_LINDEMANN_SCRATCH="1"),
                dict(AMOF_LINDEMANN_SCRATCH="3000"), dict(SIMPLE, AMOF_BOND_PAIR_BUDGET="100")):
        with _env(**env):
            again = _call(hip_ctx, packed, rcm, sets, B, S, per_atom=True)
        assert all(np.array_equal(again[k], full[k]) for k in range(4)), env
    # scratch left by one call means nothing to the next
    hip_ctx.debug_poison(0xA5)
    again = _call(hip_ctx, packed, rcm, sets, B, S, per_atom=True)
    assert all(np.array_equal(again[k], full[k]) for k in range(4))
    stages = hip_ctx.last_stage_seconds()
    assert all(v >= 0 for v in stages.values())      # lists, moments, reduction
    # two contexts of one device sharing the centres (MultiContext): the shards add up, the scale is the full call's
    from amof_amd import _hip
    multi = _hip.MultiContext([0, 0])
    try:
        m = multi.lindemann(packed, rcm, sets, B, S, NB, DD, per_atom=True)
        part = multi.lindemann(packed, rcm, sets, B, S, NB, DD, atom_range=(61, 180))
    finally:
        multi.close()
    assert all(np.array_equal(m[k], full[k]) for k in range(4))
    assert np.array_equal(part[0], parts[1][0]) and np.array_equal(part[1], parts[1][1])


def test_known_answers_more_bins_than_lds_and_refusals(hip_ctx):
    p = cases.alternating(8)
    rcm, sets = _abi(p, [(30, 7, 3.5)])
    for env, path in RUNS:
        with _env(**env):
            sums, hist, scale = hip_ctx.lindemann(p, rcm, sets, 4, 2, NB, DD)
            assert hip_ctx.last_path() == path
        assert scale.tolist() == [40] and sums[:, 0].tolist() == [[1, cases.ALTERNATING_TERM]] * 3
        assert np.array_equal(np.nonzero(hist[:, 0])[1], [40, 40, 40])
        with _env(**env):
            wide = hip_ctx.lindemann(p, rcm, sets, 4, 2, 20000, 2.0 ** -16)[1]     # beyond the LDS histogram: global counters
        assert wide.sum() == 3 and np.array_equal(np.nonzero(wide[:, 0])[1], [13107, 13107, 13107])
    st = cases.static()
    rcm_s, sets_s = _abi(st, cases.CLASS_SETS)
    sums, hist, _ = hip_ctx.lindemann(st, rcm_s, sets_s, 6, 6, NB, DD)
    assert sums.tolist() == [[[64, 0], [128, 0]]] and hist[0, :, 0].tolist() == [64, 128]
    packed = cases.case("arguments").packed
    rcm, sets = _abi(packed, [(30, 7, 8.7)])           # > 17.31 / 2
    with pytest.raises(ValueError, match="half the smallest cell height"):
        hip_ctx.lindemann(packed, rcm, sets, 5, 5, NB, DD)
    rcm, sets = _abi(packed, [(30, 7, 3.0)])
    for kw in (dict(block=1), dict(block=11), dict(block_stride=0), dict(nbins=0), dict(ddelta=0.0), dict(select=2),
               dict(atom_range=(5, 65)), dict(atom_range=(9, 3))):
        args = dict(block=5, block_stride=5, nbins=NB, ddelta=DD, select=0, atom_range=None)
        args.update(kw)
        with pytest.raises(ValueError):
            hip_ctx.lindemann(packed, rcm, sets, args["block"], args["block_stride"], args["nbins"], args["ddelta"],
                              select=args["select"], atom_range=args["atom_range"])
    sums, hist, scale = hip_ctx.lindemann(packed, rcm, sets, 5, 5, NB, DD)      # the context still works
    ref.check(sums, scale, cases.reference("arguments", 5, 5))
    sums, hist, scale = hip_ctx.lindemann(packed, rcm, [], 5, 5, NB, DD)
    assert sums.shape == (2, 0, 2) and hist.shape == (2, 0, NB) and scale.shape == (0,)


def test_class_data_feather_and_async(hip_ctx, tmp_path, monkeypatch):
    from amof_amd.lindemann import Lindemann
    tr = cases.case("class").packed
    monkeypatch.setenv("AMOF_ASYNC", "1")
    obj = Lindemann.from_trajectory(tr, cases.CLASS_CUT, block=20, timestep=2, per_atom=True, device=0, distributed=False)
    assert obj.__dict__.get("_pending") is not None         # the constructor returned before anyone looked at .data
    data = obj.data
    assert obj.__dict__.get("_pending") is None
    want = cases.reference("class", 20, 20)
    assert obj.sets == ['Zn-N', 'C-N'] and np.asarray(obj.counts).dtype == np.int64
    assert list(data.columns) == ["Time", "Zn-N", "Zn-N-n", "C-N", "C-N-n", "Zn-Au", "Zn-Au-n"]
    assert data["Time"].tolist() == [0.0, 40.0, 80.0, 120.0]
    assert list(obj.scale_log2) == ref.scales(tr.numbers, cases.CLASS_SETS, 20)
    ref.check(obj.counts, obj.scale_log2, want)
    assert np.array_equal(obj.hist_counts, ref.hist(want, 0.005, 100))
    for k, name in enumerate(("Zn-N", "C-N")):
        for b, row in enumerate(want.blocks):
            assert data[name + "-n"][b] == len(row[k].delta)
            assert abs(data[name][b] - row[k].delta.mean()) <= row[k].budget.mean() + 2.0 ** -40
    assert data["Zn-Au"].isna().all() and data["Zn-Au-n"].isna().all()
    assert list(obj.hist.columns) == ["delta", "Zn-N", "C-N"] and abs(obj.hist["Zn-N"].sum() * 0.005 - 1.0) < 1e-12
    n, tot, _ = ref.per_atom(want, tr.n_atoms)
    assert obj.per_atom.shape == n.shape and np.array_equal(np.isnan(obj.per_atom), n == 0)
    assert np.allclose(obj.per_atom[n > 0], (tot / np.maximum(n, 1))[n > 0], rtol=0, atol=1e-9)
    onset = obj.onset(0.0)
    assert onset["Zn-N"] == 0.0 and np.isnan(onset["Zn-Au"]) and np.isnan(obj.onset(10.0)["Zn-N"])
    path = str(tmp_path / "walk")
    obj.write_to_file(path)
    assert os.path.exists(path + ".lind")
    assert Lindemann.from_file(path).data.equals(data)
    # synchronous and device-resident give the same; the defaults take the whole trajectory as one block
    monkeypatch.setenv("AMOF_ASYNC", "0")
    again = Lindemann.from_trajectory(_device(tr), cases.CLASS_CUT, block=20, timestep=2, device=0, distributed=False)
    assert again.__dict__.get("_pending") is None and again.data.equals(data) and again.per_atom is None
    assert np.array_equal(again.counts, obj.counts) and np.array_equal(again.hist_counts, obj.hist_counts)
    whole = Lindemann.from_trajectory(tr, cases.CLASS_CUT, pairs='first', device=0, distributed=False)
    assert whole.data["Time"].tolist() == [0.0] and whole.data["Zn-N-n"][0] == 64
    static = Lindemann.from_trajectory(cases.static(), cases.CLASS_CUT, device=0, distributed=False)
    assert static.data["Zn-N"][0] == 0.0 and static.data["C-N"][0] == 0.0
    with pytest.raises(ValueError):
        Lindemann.from_trajectory(tr, {'Zn-N': 9.0}, block=20, device=0, distributed=False)


def _run(packed, distributed):
    from amof_amd.lindemann import Lindemann
    obj = Lindemann.from_trajectory(packed, cases.RANK_CUT, block=10, per_atom=True, device=0, distributed=distributed)
    return obj.data, np.asarray(obj.counts), np.asarray(obj.hist_counts), obj.per_atom


def _save(out_dir, tag, res):
    res[0].to_pickle(os.path.join(out_dir, "lind_%s.pkl" % tag))
    np.savez(os.path.join(out_dir, "lind_%s.npz" % tag), counts=res[1], hist=res[2], per_atom=res[3])


def _same(out_dir, tag, res):
    import pandas as pd
    assert pd.read_pickle(os.path.join(out_dir, "lind_%s.pkl" % tag)).equals(res[0])
    got = np.load(os.path.join(out_dir, "lind_%s.npz" % tag))
    assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], res[1]) and np.array_equal(got["hist"], res[2])
    assert np.array_equal(got["per_atom"], res[3], equal_nan=True)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _save(out_dir, "rank%d" % rank, _run(cases.case("ranks").packed, None))     # None: shard the centres over the group
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_single_process(tmp_path):
    # two ranks (gloo rendezvous; both on cuda:0 where the box has one GPU, as tests/test_gpu_bond.py)
    import torch.multiprocessing as mp
    port = 41600 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    res = _run(cases.case("ranks").packed, False)
    assert res[1][:, :, 0].min() > 0
    ref.check(res[1], ref.scales(cases.case("ranks").packed.numbers, cases.CLASS_SETS, 10), cases.reference("ranks", 10, 10))
    for rank in (0, 1):
        _same(str(tmp_path), "rank%d" % rank, res)


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
    _save(out_dir, "rccl", _run(cases.case("ranks").packed, None))
    dist.barrier()
    dist.destroy_process_group()


def test_rccl_backend_single_rank(tmp_path):
    # the device branch of the class (amof_lindemann_dev into a CUDA tensor, all-reduced in place, read back)
    import torch.multiprocessing as mp
    port = 43600 + os.getpid() % 2000
    mp.spawn(_worker_rccl, args=(1, port, str(tmp_path)), nprocs=1, join=True)
    _same(str(tmp_path), "rccl", _run(cases.case("ranks").packed, False))
