"""Fragments on the GPU (amof_fragment_stats, Fragments): every integer output, label and shift (of the fragments that do not wind)
equal tests/fragment_ref.py on every case of tests/fragment_cases.py, on both kernels, host and device-resident input, one frame per
batch, two frame ranges, two contexts and the forced fallback; last_path() asserted per run.  The centres are bit-identical across
all of these and lie within the derived bound of the float64 ones.  The bond graph is tied to amof_cn_count."""

import ctypes

import numpy as np
import pytest

from amof_amd import _hip
from tests import fragment_cases as cases
from tests import ring_cases
from tests.test_gpu_bond import _device, _env

pytestmark = pytest.mark.gpu

GLOBAL = {"AMOF_FRAGMENT_GLOBAL": "1"}
ONE_FRAME = {"AMOF_FRAGMENT_BATCH_MB": "0"}
NO_LDS = {"AMOF_FRAGMENT_LDS_KB": "0"}         # the records of no frame fit: the call takes the other kernel
RUNS = [({}, "fragment_frame"), (GLOBAL, "fragment_global"), (ONE_FRAME, "fragment_frame"), (dict(GLOBAL, **ONE_FRAME), "fragment_global"),
        (NO_LDS, "fragment_global")]
NAMES = ("summary", "size_hist", "census", "links", "label", "shift", "com", "frag_mass")


def _call(ctx, inp, name, frame_range=None):
    c, e = cases.case(name), cases.expected(name)
    lm = cases.matrix(c.packed, c.links) if c.links else None
    got = ctx.fragment_stats(inp, cases.matrix(c.packed, c.cutoff), link=lm, ref_label=e.ref_label, kinds=e.kinds, max_size=c.max_size,
                             frame_range=frame_range, per_atom=True, com=True)
    return dict(zip([n for n in NAMES if n != "links" or c.links], got))


def _same_bits(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in a)


def _check(got, name, frames=slice(None)):
    c, e = cases.case(name), cases.expected(name)
    for key, want in (("summary", e.summary), ("size_hist", e.hist), ("census", e.census), ("label", e.label)):
        assert got[key].dtype == want.dtype and np.array_equal(got[key], want[frames]), (name, key)
    if c.links:
        assert np.array_equal(got["links"], e.links[frames])
    whole = e.whole[frames]
    assert got["shift"].dtype == np.int32 and np.array_equal(got["shift"][whole], e.shift[frames][whole]), (name, "shift")
    want = e.com[frames]
    assert np.array_equal(np.isnan(got["com"]), np.isnan(want)), (name, "NaN rows")
    err = np.abs(got["com"] - want)
    print(name, "largest centre error %.3g A, bound %.3g A" % (np.nanmax(err) if not np.isnan(err).all() else 0.0, e.bound.max()))
    assert not (err > e.bound[None, :, None]).any(), (name, "centres")
    np.testing.assert_allclose(got["frag_mass"], e.mass, rtol=1e-14)


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_case_on_both_kernels(hip_ctx, name):
    c, e = cases.case(name), cases.expected(name)
    packed, F = c.packed, c.packed.n_frames
    first = None
    for env, path in RUNS:
        for inp in (packed, _device(packed)):
            with _env(**env):
                got = _call(hip_ctx, inp, name)
                ran = hip_ctx.last_path()
                rounds = hip_ctx.fragment_round_stats()
            assert ran == path, (name, env, ran)
            if first is None:
                _check(got, name)
                first = got, rounds
            assert _same_bits(got, first[0]), (name, env)
            assert rounds == first[1] and rounds["frames"] == F and 1 <= rounds["max_rounds"] <= packed.n_atoms
    if name == "chain":
        assert first[1]["max_rounds"] == 300        # a round per bond from the root at one end, and the one that changes nothing
    stages = hip_ctx.last_stage_seconds()
    assert stages["rho"] >= 0 and stages["corr"] >= 0 and stages["self"] >= 0       # adjacency, labelling, reduction
    # without a reference partition and kinds: column 3 is -1, every fragment is "other"
    rcm = cases.matrix(packed, c.cutoff)
    bare = hip_ctx.fragment_stats(packed, rcm, max_size=c.max_size)
    assert len(bare) == 3 and np.array_equal(bare[0][:, [0, 1, 2, 4]], e.summary[:, [0, 1, 2, 4]] * [1, 1, 1, 0]) and (bare[0][:, 3] == -1).all()
    assert np.array_equal(bare[1], e.hist) and np.array_equal(bare[2][:, 0], e.summary[:, 0])
    if F > 1:
        # two frame ranges concatenate; scratch left by one call means nothing to the next
        a = _call(hip_ctx, packed, name, frame_range=(0, 1))
        hip_ctx.debug_poison(0xA5)
        with _env(**GLOBAL):
            b = _call(hip_ctx, _device(packed), name, frame_range=(1, F))
        joined = {k: a[k] if k == "frag_mass" else np.concatenate([a[k], b[k]]) for k in a}
        assert _same_bits(joined, first[0])
        multi = _hip.MultiContext([0, 0])
        try:
            assert _same_bits(_call(multi, packed, name), first[0])
        finally:
            multi.close()


def test_fragments_are_tied_to_the_coordination_numbers(hip_ctx):
    c = cases.case("breaking")
    packed = c.packed
    kinds, species = _hip.species_index(packed.numbers)
    S, N, F = len(kinds), packed.n_atoms, packed.n_frames
    single = np.eye(S, dtype=np.int32)
    # (a) no bonds at all, the Zn-N pair as link: every atom is a fragment, and the ordered link bonds between the single-atom
    # kinds are the coordination numbers summed over the centres
    lm = cases.matrix(packed, cases.ZN_LINK)
    zn, n = kinds.index(30), kinds.index(7)
    _, cn = hip_ctx.cn_count(packed, lm, [(zn, n), (n, zn)], per_atom=True)             # [F][2][N], -1: not a centre of the set
    for env in ({}, GLOBAL):
        with _env(**env):
            summary, hist, census, links = hip_ctx.fragment_stats(packed, np.zeros((S, S)), link=lm, kinds=single, max_size=4)
        assert (summary[:, 0] == N).all() and (summary[:, 1] == 1).all() and not summary[:, [2, 4]].any() and (hist[:, 1] == N).all()
        assert np.array_equal(census[:, :S], np.tile(np.bincount(species, minlength=S), (F, 1))) and not census[:, S].any()
        assert np.array_equal(links[:, zn, n], np.maximum(cn[:, 0], 0).sum(axis=1)) and np.array_equal(links[:, n, zn], np.maximum(cn[:, 1], 0).sum(axis=1))
        assert links.sum() == links[:, zn, n].sum() + links[:, n, zn].sum() > 0
    # (b) the C-H pair alone, no links: no hydrogen has two carbons, so a fragment is a carbon with its hydrogens -- the size
    # histogram is the histogram of 1 + CN over the carbons, plus the atoms no such bond touches
    ch = cases.matrix(packed, {'C-H': 1.2})
    ci, hi = kinds.index(6), kinds.index(1)
    _, cn = hip_ctx.cn_count(packed, ch, [(ci, hi), (hi, ci)], per_atom=True)
    assert cn[:, 1].max() == 1
    for env in ({}, GLOBAL):
        with _env(**env):
            summary, hist, census = hip_ctx.fragment_stats(packed, ch, max_size=8)
        for f in range(F):
            want = np.bincount(1 + cn[f, 0][species == ci], minlength=10)
            want[1] += int((species != ci).sum() - (species == hi).sum()) + int((cn[f, 1][species == hi] == 0).sum())
            assert np.array_equal(hist[f], want), f
        assert (summary[:, 2] == 0).all()


def _apart(F, bad_frame, cells):
    """two carbon atoms bonded across ``cells`` cells of a 10 A box in frame ``bad_frame``, next to each other in the others"""
    from amof_amd.frames import PackedTrajectory
    pos = np.tile(np.array([[1.0, 1.0, 1.0], [2.2, 1.0, 1.0]]), (F, 1, 1))
    pos[bad_frame, 1, 0] += 10.0 * cells
    return PackedTrajectory(pos, np.diag([10.0] * 3), np.array([6, 6]))


def test_capacity_refusals_leave_zeros_and_a_usable_context(hip_ctx):
    from tests import bond_order_cases
    over, fits = bond_order_cases.cluster(counts=(17, 3), seed=6), bond_order_cases.cluster(counts=(16, 3), seed=6)
    cut = {'Zn-N': 3.0}
    far, near = _apart(3, 1, 200), _apart(3, 1, 100)
    cc = cases.matrix(far, {'C-C': 1.6})
    for env in ({}, GLOBAL):
        with _env(**env):
            with pytest.raises(_hip.AmofError, match="frame 0: an atom has more than FRAG_MAX_DEGREE = 16 neighbours") as err:
                hip_ctx.fragment_stats(over, cases.matrix(over, cut))
            assert err.value.code == _hip.AMOF_ECAPACITY
            with pytest.raises(_hip.AmofError, match="frame 0: an atom has more than FRAG_MAX_DEGREE = 16 neighbours"):
                hip_ctx.fragment_stats(over, np.zeros((2, 2)), link=cases.matrix(over, cut))
            assert hip_ctx.fragment_stats(fits, cases.matrix(fits, cut))[0][0, 1] == 17          # the Zn and its 16 N
            with pytest.raises(_hip.AmofError, match="frame 1: a shift does not fit its storage") as err:
                hip_ctx.fragment_stats(far, cc)
            assert err.value.code == _hip.AMOF_ECAPACITY
            summary, _, _, label, shift = hip_ctx.fragment_stats(near, cc, per_atom=True)
            assert summary[:, :3].tolist() == [[1, 2, 0]] * 3 and shift[:, 1, 0].tolist() == [0, -100, 0] and not label.any()
            _check(_call(hip_ctx, cases.case("crystal").packed, "crystal"), "crystal")           # the context works afterwards
    # through the C ABI: the caller's arrays hold zeros after the refusal
    th = hip_ctx._traj(far)
    summary = np.full((3, 5), 9, dtype=np.int64)
    hist = np.full((3, 6), 9, dtype=np.int64)
    census = np.full((3, 1), 9, dtype=np.int64)
    label = np.full((3, 2), 9, dtype=np.int32)
    shift = np.full((3, 2, 3), 9, dtype=np.int32)
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data)      # noqa: E731
    hip_ctx.drain()
    with hip_ctx._lock:
        rc = hip_ctx._lib.amof_fragment_stats(hip_ctx._h, ctypes.byref(th.c), ptr(np.ascontiguousarray(cc)), None, None, None, 0, 4, ptr(summary),
                                              ptr(hist), ptr(census), None, ptr(label), ptr(shift), None, None, 0)
    assert rc == _hip.AMOF_ECAPACITY and not summary.any() and not hist.any() and not census.any() and not label.any() and not shift.any()


def test_arguments(hip_ctx):
    c, e = cases.case("random_rect"), cases.expected("random_rect")
    p, m = c.packed, cases.matrix(c.packed, c.cutoff)
    with pytest.raises(ValueError, match="max_size"):
        hip_ctx.fragment_stats(p, m, max_size=0)
    with pytest.raises(ValueError, match="half the smallest cell height"):
        hip_ctx.fragment_stats(p, m * 5.0)
    with pytest.raises(ValueError, match="half the smallest cell height"):
        hip_ctx.fragment_stats(p, m * 0.0, link=m * 5.0)
    skew = m.copy()
    skew[0, 1] += 0.1
    with pytest.raises(ValueError, match="symmetric"):
        hip_ctx.fragment_stats(p, skew)
    with pytest.raises(ValueError, match="finite and >= 0"):
        hip_ctx.fragment_stats(p, -m)
    with pytest.raises(ValueError, match="named by the cutoff and by the link"):
        hip_ctx.fragment_stats(p, m, link=m)
    with pytest.raises(ValueError, match="com needs ref_label"):
        hip_ctx.fragment_stats(p, m, com=True)
    bad = e.ref_label.copy()
    bad[0] = 5
    with pytest.raises(ValueError, match="not the smallest atom of a class"):
        hip_ctx.fragment_stats(p, m, ref_label=bad)
    with pytest.raises(ValueError, match="kinds must be >= 0"):
        hip_ctx.fragment_stats(p, m, kinds=-np.ones((1, 2), dtype=np.int32))
    empty = hip_ctx.fragment_stats(p, m, ref_label=e.ref_label, kinds=e.kinds, max_size=16, frame_range=(0, 0), per_atom=True, com=True)
    assert empty[0].shape == (0, 5) and empty[3].shape == (0, 150) and empty[5].shape == (0, len(e.roots), 3)
    np.testing.assert_allclose(empty[6], e.mass, rtol=1e-14)


def _reduced_rings(frag):
    from amof_amd.ring import Ring
    table = Ring.from_trajectory(frag.reduced(), {'Zn-Fr': 4.0}, max_search_depth=16, device=0, distributed=False).table
    return {int(n): int(r) for n, r in zip(table["ring_size"], table["rings"]) if r}


def test_class_equals_the_library_call_and_feeds_the_other_analyses(hip_ctx, tmp_path, monkeypatch):
    from amof_amd.fragment import Fragments, assemble
    from amof_amd.frames import PackedTrajectory
    from amof_amd.msd import WindowMsd
    c, e = cases.case("rigid"), cases.expected("rigid")
    tr, F = c.packed, c.packed.n_frames
    want = _call(hip_ctx, tr, "rigid")
    monkeypatch.setenv("AMOF_ASYNC", "1")
    obj = Fragments.from_trajectory(tr, cases.LIGAND_CUT, links=cases.ZN_LINK, names={'C3H3N2': 'Im'}, delta_Step=5, first_frame=10,
                                    per_atom=True, device=0, distributed=False)
    data = obj.data
    assert obj.__dict__.get("_pending") is None
    step = np.arange(10, 10 + 5 * F, 5)
    tables = assemble(want["summary"], want["size_hist"], want["census"], want["links"], e.formulas, step, tr.n_atoms)
    assert data.equals(tables[0]) and obj.sizes.equals(tables[1]) and obj.links.equals(tables[2]) and obj.report_search.equals(tables[3])
    assert obj.formulas == ["C3H3N2", "Zn"] and np.array_equal(obj.label, want["label"]) and np.array_equal(obj.shift, want["shift"])
    # (the fragments move apart rigidly: the Zn-N links of frame 0 stretch and break, the partition stays)
    assert obj.links["Zn-C3H3N2"][0] == 4.0 and obj.links["C3H3N2-Zn"][0] == 2.0 and obj.report_search["in_reduced_trajectory"].all()
    red = obj.reduced()
    assert np.array_equal(red.pos, want["com"]) and red.symbols == {"Im": "Fr", "Zn": "Zn"} and red.steps.tolist() == step.tolist()
    # MSD of the centres: the imposed translations, frame 0's centres as the origin (the float64 ones)
    imposed = PackedTrajectory(e.com[0][None] + c.translation, tr.cell, red.numbers, masses=red.masses, pbc=tr.pbc)
    got = WindowMsd.from_trajectory(red, delta_time=1, timestep=1, unwrap=True, device=0, distributed=False).data
    ref = WindowMsd.from_trajectory(imposed, delta_time=1, timestep=1, unwrap=True, device=0, distributed=False).data
    assert list(got.columns) == list(ref.columns) and len(got) == F // 2 and float(ref.iloc[-1, 1:].min()) > 0.1
    np.testing.assert_allclose(got.to_numpy(dtype=np.float64), ref.to_numpy(dtype=np.float64), rtol=1e-9, atol=1e-12)
    # the crystal's reduced network: the 4-, 6- and 8-membered Zn rings
    crystal = Fragments.from_trajectory(ring_cases.zif4(), cases.LIGAND_CUT, links=cases.ZN_LINK, device=0, distributed=False)
    assert crystal.data[["C3H3N2", "Zn", "other"]].iloc[0].tolist() == [32, 16, 0]
    assert _reduced_rings(crystal) == {8: 24, 12: 32, 16: 24}
    # synchronous, device-resident, the device list and a streamed source give the same
    monkeypatch.setenv("AMOF_ASYNC", "0")
    for inp, dev in ((_device(tr), 0), (tr, [0, 0])):
        again = Fragments.from_trajectory(inp, cases.LIGAND_CUT, links=cases.ZN_LINK, delta_Step=5, first_frame=10, device=dev, distributed=False)
        assert again.data.equals(data) and np.array_equal(again.reduced().pos, red.pos)
    from amof_amd import trajectory as T
    from amof_amd.stream import XyzStream
    xyz = str(tmp_path / "rigid.xyz")
    T.write_xyz(xyz, tr, comment_lattice=False, fmt="%.17g")
    streamed = Fragments.from_trajectory(XyzStream(xyz, cell=tr.cell[0], batch_frames=5), cases.LIGAND_CUT, links=cases.ZN_LINK, delta_Step=5,
                                         first_frame=10, device=0, distributed=False)
    assert streamed.data.equals(data) and np.array_equal(streamed.reduced().pos, red.pos)
    # frames that regroup drop out of the reduced trajectory; a winding reference frame has none
    broken = Fragments.from_trajectory(cases.case("breaking").packed, cases.LIGAND_CUT, links=cases.ZN_LINK, device=0, distributed=False)
    assert broken.report_search["atoms_regrouped"].tolist() == [0, 0, 1, 2, 2, 4] and broken.reduced().steps.tolist() == [0, 1]
    net = Fragments.from_trajectory(ring_cases.zif4(), ring_cases.ZIF_CUT, device=0, distributed=False)
    assert net.data["winding"].tolist() == [1]
    with pytest.raises(ValueError, match="winds"):
        net.reduced()
    with pytest.raises(ValueError, match="reduce=False"):
        Fragments.from_trajectory(ring_cases.zif4(), cases.LIGAND_CUT, reduce=False, device=0, distributed=False).reduced()
    with pytest.raises(ValueError):
        Fragments.from_trajectory(tr, {'C-C': 9.0}, device=0, distributed=False).data


def _run(packed, distributed):
    from amof_amd.fragment import Fragments
    obj = Fragments.from_trajectory(packed, cases.LIGAND_CUT, links=cases.ZN_LINK, per_atom=True, device=0, distributed=distributed)
    return obj.data, [obj.counts[k] for k in ("summary", "size_hist", "census", "links")] + [obj.label, obj.shift, obj.com, obj.frag_mass]


def _worker(rank, world, port, out_dir):
    import os
    import sys
    from tests.conftest import ROOT
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    table, arrays = _run(cases.case("breaking").packed, None)       # None: shard the frames over the group
    table.to_pickle(os.path.join(out_dir, "fragments_rank%d.pkl" % rank))
    np.savez(os.path.join(out_dir, "fragments_rank%d.npz" % rank), *arrays)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_single_process(tmp_path):
    # the frames sharded over two ranks (gloo rendezvous; both on cuda:0 where the box has one GPU, as tests/test_gpu_ring.py)
    import os
    import pandas as pd
    import torch.multiprocessing as mp
    port = 46600 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    table, arrays = _run(cases.case("breaking").packed, False)
    assert arrays[0][:, 3].tolist() == [0, 0, 1, 2, 2, 4]
    for rank in (0, 1):
        assert pd.read_pickle(os.path.join(str(tmp_path), "fragments_rank%d.pkl" % rank)).equals(table)
        got = np.load(os.path.join(str(tmp_path), "fragments_rank%d.npz" % rank))
        for k, want in enumerate(arrays):
            assert np.array_equal(got["arr_%d" % k], want, equal_nan=want.dtype.kind == "f"), (rank, k)
