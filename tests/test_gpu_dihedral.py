"""Dihedral distributions on the GPU (amof_dihedral_hist[_dev], Dihedral): every case of tests/dihedral_cases.py on
"dihedral_frame" and on "dihedral_exact" -- equal to each other bit for bit and equal to tests/dihedral_ref.py (integers equal,
cosine sums within one unit per chain) --, the invariances (frame ranges, one frame per batch, device-resident input, a
permutation of the atoms), the slab rows of the list stage, the error paths, and BAD and the bond order parameters on rows whose
fourth word a dihedral call has just written.  last_path() asserted per run."""

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd.dihedral import Dihedral
from amof_amd.frames import PackedTrajectory
from tests import dihedral_cases as cases
from tests import dihedral_ref as ref
from tests.test_gpu_bond import _device, _env

pytestmark = pytest.mark.gpu

EXACT = {"AMOF_DIHEDRAL_EXACT": "1"}
ONE_FRAME = {"AMOF_DIHEDRAL_ROWS_MB": "0"}      # a frame per batch of neighbour rows
PATHS = (({}, "dihedral_frame"), (EXACT, "dihedral_exact"))
# every case, the planted chain in every cell form.  zif4_explicit: patterns that leave a bonded pair (C-C) unused; zif4_fine: 24 x 1801 bins, the global-memory histogram
NAMES = cases.NAMES


def _run(hip_ctx, c, env, path, packed=None, **kwargs):
    rcm, idx, edges = cases.abi_arguments(c)
    with _env(**env):
        got = hip_ctx.dihedral_hist(c.packed if packed is None else packed, rcm, idx, edges, **kwargs)
        ran = hip_ctx.last_path()
    assert ran == path, (env, ran, path)
    return got


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", NAMES)
def test_both_paths_equal_each_other_and_the_restatement(hip_ctx, name):
    c = cases.case(name)
    got = [_run(hip_ctx, c, env, path) for env, path in PATHS]
    assert _same(got[0], got[1]), "dihedral_frame and dihedral_exact differ"
    ref.check(got[0], cases.reference(name))
    stages = hip_ctx.last_stage_seconds()
    assert stages["rho"] > 0.0 and stages["corr"] > 0.0
    if name == "zif4_fine":         # more words than AMOF_MAX_LDS_BINS: both kernels counted with global atomics
        assert got[0][0].size + 24 * got[0][0].shape[0] > 36864


def test_known_answers_through_the_abi(hip_ctx):
    hist, n, undefined, sums = _run(hip_ctx, cases.case("cubic"), {}, "dihedral_frame")
    assert hist[0, [0, 12, 25]].tolist() == [1536, 3072, 1536] and int(hist.sum()) == 6144
    assert n.tolist() == [6144] and undefined.tolist() == [3456] and sums[:, 0].tolist() == [[3072, 1728, 0]] * 2
    hist, n, undefined, sums = _run(hip_ctx, cases.case("rocksalt"), {}, "dihedral_frame")
    assert n.tolist() == [6144, 6144, 0] and np.array_equal(hist[0], hist[1]) and not hist[2].any()


@pytest.mark.parametrize("name", ["zif4", "rocksalt", "planted_100_rotmirror"])
def test_through_the_class(name):
    c = cases.case(name)
    frames = cases.reference(name)
    names, _ = cases.patterns(c)
    dh = Dihedral.from_trajectory(c.packed, c.cutoff, chains=c.chains, dphi=c.dphi, device=0, distributed=False)
    assert dh.chains == names
    ref.check((dh.counts["hist"], dh.counts["n_dihedrals"], dh.counts["n_undefined"], dh.counts["frame_sums"]), frames)
    hist, n, _, _, cos = ref.totals(frames)
    assert list(dh.data.columns) == ["phi"] + [s for s, k in zip(names, n) if k]
    for s, h in zip(names, hist):
        if h.sum():
            assert np.array_equal(dh.data[s].to_numpy(), h / np.diff(np.arange(len(h) + 1) * c.dphi) / h.sum())
    assert dh.frames["Step"].tolist() == list(range(len(frames)))
    for t, s in enumerate(names):
        assert dh.frames[s + "-n"].tolist() == [int(fr.n[t]) for fr in frames]
        with np.errstate(invalid="ignore", divide="ignore"):
            want = np.array([fr.cos[t] / fr.n[t] if fr.n[t] else np.nan for fr in frames])
        assert np.allclose(dh.frames[s + "-cos"].to_numpy(), want, rtol=0, atol=1e-11, equal_nan=True)


@pytest.mark.parametrize("env, path", PATHS)
def test_frame_ranges_and_single_frame_batches_add_up(hip_ctx, env, path):
    c = cases.case("zif4")
    whole = _run(hip_ctx, c, env, path)
    parts = [_run(hip_ctx, c, env, path, frame_range=r) for r in ((0, 1), (1, 3))]
    assert all(np.array_equal(whole[k], parts[0][k] + parts[1][k]) for k in range(3))
    assert np.array_equal(whole[3], np.concatenate([parts[0][3], parts[1][3]]))
    assert _same(whole, _run(hip_ctx, c, dict(env, **ONE_FRAME), path))
    assert _same(whole, _run(hip_ctx, c, dict(env, AMOF_DIHEDRAL_NO_TABLE="1"), path))      # the loop over the patterns


def test_device_input_and_device_outputs(hip_ctx):
    import torch
    c = cases.case("zif4")
    whole = _run(hip_ctx, c, {}, "dihedral_frame")
    assert _same(whole, _run(hip_ctx, c, {}, "dihedral_frame", packed=_device(c.packed)))
    T, nb = whole[0].shape
    out = tuple(torch.full((n,), 5, dtype=torch.int64, device="cuda:0") for n in (T * nb, T, T))
    got = _run(hip_ctx, c, {}, "dihedral_frame", out=out)
    for k in range(3):
        assert np.array_equal(got[k].cpu().numpy().reshape(whole[k].shape).astype(np.uint64), whole[k] + np.uint64(5))
    assert np.array_equal(got[3], whole[3])


@pytest.mark.parametrize("env, path", PATHS)
def test_a_permutation_of_the_atoms_changes_nothing(hip_ctx, env, path):
    c = cases.case("zif4")
    whole = _run(hip_ctx, c, env, path)
    order = np.random.default_rng(3).permutation(c.packed.n_atoms)
    p = c.packed
    shuffled = PackedTrajectory(p.pos_host()[:, order], p.cell, np.asarray(p.numbers)[order], pbc=p.pbc)
    assert _same(whole, _run(hip_ctx, c, env, path, packed=shuffled))


def test_slab_rows(hip_ctx):
    """Two frames of the 9792-atom headline cell (3 x 3 x 4 ZIF-4 cells).  With the four quick-start cutoffs no species pair
    of it reaches the 8192 atoms beyond which the list stage must cut a frame into slabs (the largest, C + H, has 6912), so the
    slab items are forced (AMOF_NBR_SLABS=1): partners in the halo of several slabs then claim their slots in nondeterministic
    order.  Against dihedral_exact only; the small crystal under the same switch against the restatement too."""
    from tests import ring_cases
    c = cases.case("zif4")
    small = _run(hip_ctx, c, {"AMOF_NBR_SLABS": "1"}, "dihedral_frame")
    ref.check(small, cases.reference("zif4"))
    big = cases.Case()
    big.packed, big.cutoff, big.chains, big.dphi = ring_cases.zif4(reps=(3, 3, 4), F=2, sigma=0.05), cases.ZIF_CUT, None, 1.0
    assert big.packed.n_atoms == 9792
    slabs = _run(hip_ctx, big, {"AMOF_NBR_SLABS": "1"}, "dihedral_frame")
    assert _same(slabs, _run(hip_ctx, big, EXACT, "dihedral_exact")) and _same(slabs, _run(hip_ctx, big, {}, "dihedral_frame"))
    assert int(slabs[1].sum()) > 2 * 30000


def test_bad_and_bond_order_read_rows_a_dihedral_call_wrote(hip_ctx):
    """the partner word of the row scratch is stale after a dihedral call, and BAD's and the bond order's list kernels leave it
    alone: their integers are the oracle's / the exact kernel's as before"""
    from oracle import clib
    from tests import bond_order_cases
    from tests import helpers as H
    c = cases.case("zif4")
    _run(hip_ctx, c, {}, "dihedral_frame")
    p = c.packed
    kinds, sp = H.species_of(p.numbers)
    rcm, _, _ = cases.abi_arguments(c)
    triples = [(kinds.index(30), kinds.index(7)), (kinds.index(6), -1), (kinds.index(7), -1)]
    edges = np.arange(int(180 // 0.5) + 2) * 0.5
    hb, ab = hip_ctx.bad_hist(p, rcm, triples, edges)
    assert hip_ctx.last_path() == "bad_frame"
    hr, ar = clib.bad_hist(p.pos_host(), p.cell, sp, len(kinds), rcm, triples, edges)
    assert np.array_equal(hb, hr) and np.array_equal(ab, ar)
    _run(hip_ctx, c, {}, "dihedral_frame")
    bc = bond_order_cases.case("zif4")
    from tests.test_gpu_bond import _abi
    brcm, sets = _abi(bc.packed, bc.sets)
    frame = hip_ctx.bond_order(bc.packed, brcm, sets, bc.l, bond_order_cases.NBINS, bond_order_cases.NBINS_TET, per_atom=True)
    assert hip_ctx.last_path() == "order_frame"
    with _env(AMOF_ORDER_EXACT="1"):
        exact = hip_ctx.bond_order(bc.packed, brcm, sets, bc.l, bond_order_cases.NBINS, bond_order_cases.NBINS_TET, per_atom=True)
    assert hip_ctx.last_path() == "order_exact" and _same(frame, exact)


def _two_planted_frames(pbc=(True, True, True)):
    """the planted chains of 35 and 100 degrees as the two frames of one trajectory of four atoms"""
    a, b = cases.planted(35.0), cases.planted(100.0)
    return PackedTrajectory(np.concatenate([a.pos_host(), b.pos_host()]), a.cell, a.numbers, pbc=pbc)


def test_an_open_axis_leaves_the_call_to_the_exact_kernel(hip_ctx):
    """the list stage wants three periodic axes: with y open the frame tier does not apply and the call reaches dihedral_exact
    unforced -- the restatement's integers, the chain still bonded across the periodic face x"""
    c = cases.Case()
    c.packed, c.cutoff, c.chains, c.dphi = _two_planted_frames((True, False, True)), cases.PLANTED_CUT, cases.PLANTED_CHAINS, cases.PLANTED_DPHI
    got = _run(hip_ctx, c, {}, "dihedral_exact")
    assert _same(got, _run(hip_ctx, c, EXACT, "dihedral_exact"))
    ref.check(got, ref.trajectory(c.packed, c.cutoff, cases.patterns(c)[1], cases.abi_arguments(c)[2]))
    assert got[3][:, 0, 0].tolist() == [1, 1] and got[0][0, cases.PLANTED_BIN[35.0]] == 1 and got[0][0, cases.PLANTED_BIN[100.0]] == 1
    periodic = cases.Case()
    periodic.packed, periodic.cutoff, periodic.chains, periodic.dphi = _two_planted_frames(), c.cutoff, c.chains, c.dphi
    assert _same(got, _run(hip_ctx, periodic, {}, "dihedral_frame"))


def test_no_bonded_pair_is_nothing_to_do(hip_ctx):
    """The only cutoff belongs to a species without atoms (one species more than the kinds present, through the C ABI): the list
    stage applies and finds nothing to do, no kernel of either tier runs (the path name stays the call's before), and the
    outputs are zeros, as the exact kernel and the restatement without a bond give them.  2 frames of 4 atoms."""
    import ctypes
    c = cases.Case()
    c.packed, c.cutoff, c.chains, c.dphi = _two_planted_frames(), cases.PLANTED_CUT, ['X-X-X-X', 'H-C-N-Zn'], cases.PLANTED_DPHI
    rcm4, idx, edges = cases.abi_arguments(c)
    S, T, nb = 4, len(idx), len(edges) - 1
    rcm = np.zeros((S + 1, S + 1))
    rcm[0, S] = rcm[S, 0] = 1.3
    idx, edges = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(edges)

    def call(env):
        outs = [np.full((T, nb), 7, dtype=np.uint64), np.full(T, 7, dtype=np.uint64), np.full(T, 7, dtype=np.uint64),
                np.full((2, T, 3), 7, dtype=np.int64)]
        hip_ctx.drain()
        with _env(**env), hip_ctx._lock:
            th = hip_ctx._traj(c.packed)
            assert th.c.n_species == S
            th.c.n_species = S + 1
            rc = hip_ctx._lib.amof_dihedral_hist(hip_ctx._h, ctypes.byref(th.c), _hip._ptr(rcm), _hip._ptr(idx), T, _hip._ptr(edges), nb,
                                                 *[_hip._ptr(x) for x in outs])
        assert rc == _hip.AMOF_OK
        return outs

    hip_ctx.cn_count(c.packed, rcm4, [(1, 2)])          # (another family's path name: C-N within 1.7)
    before = hip_ctx.last_path()
    assert before.startswith("cn_")
    got = call({})
    assert hip_ctx.last_path() == before
    exact = call(EXACT)
    assert hip_ctx.last_path() == "dihedral_exact"
    assert _same(got, exact) and not any(x.any() for x in got)
    ref.check(got, ref.trajectory(c.packed, {'C-N': 0.0}, cases.patterns(c)[1], edges))


@pytest.mark.parametrize("env", [{}, EXACT])
def test_error_paths(hip_ctx, env):
    # a 17th neighbour: the capacity, naming the frame, on either path
    c = cases.Case()
    c.packed, c.cutoff, c.chains, c.dphi = cases.crowded(17), cases.CROWDED_CUT, ['X-X-X-X'], 1.0
    rcm, idx, edges = cases.abi_arguments(c)
    with _env(**env):
        with pytest.raises(_hip.AmofError, match="frame 0: an atom has more than 16 neighbours") as e:
            hip_ctx.dihedral_hist(c.packed, rcm, idx, edges)
    assert e.value.code == _hip.AMOF_ECAPACITY
    # the graph is the dictionary's, whatever the patterns name: no pattern here can use a Zn-N bond
    kinds = sorted(set(int(z) for z in c.packed.numbers))
    with _env(**env):
        with pytest.raises(_hip.AmofError, match="more than 16 neighbours"):
            hip_ctx.dihedral_hist(c.packed, rcm, [[kinds.index(1)] * 4], edges)
    # a bonded pair of coincident atoms
    pos = np.array([[5.0, 5.0, 5.0], [5.0, 5.0, 5.0], [6.4, 5.0, 5.0], [6.9, 6.2, 5.0]])
    twin = PackedTrajectory(pos[None], np.diag([20.0, 20.0, 20.0]), np.full(4, 6))
    with _env(**env):
        with pytest.raises(ZeroDivisionError):
            hip_ctx.dihedral_hist(twin, np.array([[1.7]]), [[-1, -1, -1, -1]], edges)
        # a cutoff over half the cell height
        with pytest.raises(ValueError, match="half the smallest cell height"):
            hip_ctx.dihedral_hist(twin, np.array([[10.5]]), [[-1, -1, -1, -1]], edges)
        with pytest.raises(ValueError, match="n_chains"):
            hip_ctx.dihedral_hist(twin, np.array([[1.7]]), np.full((33, 4), -1), edges)
    # and the context still works
    ref.check(_run(hip_ctx, cases.case("triangle"), env, "dihedral_exact" if env else "dihedral_frame"), cases.reference("triangle"))


@pytest.mark.parametrize("env", [{}, EXACT])
def test_a_failed_call_leaves_zeros(hip_ctx, env):
    """amof_dihedral_hist overwrites its host outputs and leaves zeros after an error: called through ctypes on arrays
    filled with a pattern, with the 17-neighbour atom"""
    import ctypes
    c = cases.Case()
    c.packed, c.cutoff, c.chains, c.dphi = cases.crowded(17), cases.CROWDED_CUT, ['X-X-X-X', 'H-N-Zn-N'], 1.0
    rcm, idx, edges = cases.abi_arguments(c)
    rcm, idx, edges = np.ascontiguousarray(rcm), np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(edges)
    T, nb = len(idx), len(edges) - 1
    outs = [np.full((T, nb), 7, dtype=np.uint64), np.full(T, 7, dtype=np.uint64), np.full(T, 7, dtype=np.uint64),
            np.full((1, T, 3), 7, dtype=np.int64)]
    hip_ctx.drain()
    with _env(**env), hip_ctx._lock:
        th = hip_ctx._traj(c.packed)
        rc = hip_ctx._lib.amof_dihedral_hist(hip_ctx._h, ctypes.byref(th.c), _hip._ptr(rcm), _hip._ptr(idx), T, _hip._ptr(edges), nb,
                                             *[_hip._ptr(x) for x in outs])
    assert rc == _hip.AMOF_ECAPACITY and not any(x.any() for x in outs)
    # a successful call overwrites the same arrays
    ok = cases.case("crowded16")
    rcm, idx, edges = cases.abi_arguments(ok)
    rcm, idx, edges = np.ascontiguousarray(rcm), np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(edges)
    for x in outs:
        x[...] = 7
    with _env(**env), hip_ctx._lock:
        th = hip_ctx._traj(ok.packed)
        rc = hip_ctx._lib.amof_dihedral_hist(hip_ctx._h, ctypes.byref(th.c), _hip._ptr(rcm), _hip._ptr(idx), T, _hip._ptr(edges), nb,
                                             *[_hip._ptr(x) for x in outs])
    assert rc == _hip.AMOF_OK
    ref.check(outs, cases.reference("crowded16"))
