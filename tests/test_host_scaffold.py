"""The host scaffolding the analysis classes share, without a GPU: ``MultiContext``'s one sharded call (driven with
stand-in contexts that answer from fixed integer tables), the one parser of a neighbour-set dictionary, and the table of
``_setup.setup`` -- which lane a class lands on, what a rank's share is, where a merged stream is refused."""
import numpy as np
import pytest

from amof_amd import _hip, _setup, lags
from amof_amd import dist as _dist
from amof_amd.bad import Bad, BadByCn
from amof_amd.bond_order import BondOrder
from amof_amd.cn import CoordinationNumber
from amof_amd.frames import PackedTrajectory
from amof_amd.msd import WindowMsd
from amof_amd.rdf import Rdf
from tests import helpers as H
from tests import oracle_context

F, N = 13, 7
TABLE = np.random.default_rng(11).integers(-(1 << 40), 1 << 40, size=(64, 3))     # one row per frame / atom / work entry
KINDS = [7, 30]
WINDOWS = [0, 1, 3]


class TableContext(object):
    """``_hip.Context``'s signatures and return shapes; every answer is a function of the shard alone: "sum" elements
    are the table's rows of the shard added up, "cat" elements those rows, "first" elements constants"""
    device = None

    def __init__(self):
        self.seen = []

    def _rows(self, shard, n, step=1):
        a, b = (0, n) if shard is None else shard
        self.seen.append((a, b))
        return TABLE[a:b:step]

    def rdf_accumulate(self, packed, rmax, nbins, frame_range=None, out=None):
        t = self._rows(frame_range, packed.n_frames)
        return t.sum(axis=0), float(t[:, 0].sum()), KINDS

    def cn_count(self, packed, cutoff, sets, frame_range=None, per_atom=False):
        t = self._rows(frame_range, packed.n_frames)
        return (t, t[:, :2]) if per_atom else t

    def bad_hist(self, packed, cutoff, triples, edges, frame_range=None, out=None):
        t = self._rows(frame_range, packed.n_frames)
        return t.sum(axis=0), t[:, 1].sum(keepdims=True)

    def bad_hist_by_cn(self, packed, cutoff, triples, edges, cn_max=16, frame_range=None):
        t = self._rows(frame_range, packed.n_frames)
        return t.sum(axis=0) * cn_max, t[:, 2].sum(keepdims=True)

    def msd_window(self, packed, windows, unwrap=False, remove_com=True, atom_range=None, com=None, out=None):
        return self._rows(atom_range, packed.n_atoms).sum(axis=0), KINDS

    def vanhove_window(self, packed, windows, dr, nbins, unwrap=False, remove_com=True, atom_range=None, com=None, out=None):
        t = self._rows(atom_range, packed.n_atoms)
        return t.sum(axis=0), t[:, 0].sum(keepdims=True), t[:, 1:].sum(axis=0), KINDS

    def vanhove_distinct(self, packed, windows, rmax, nbins, origin_stride=1, work_range=None, out=None):
        assert work_range is not None
        return self._rows(work_range, None).sum(axis=0), KINDS

    def bond_survival(self, packed, cutoff, sets, windows, origin_stride=1, atom_range=None, out=None):
        return self._rows(atom_range, packed.n_atoms).sum(axis=0)

    def bond_reorientation(self, packed, cutoff, sets, windows, origin_stride=1, atom_range=None, out=None):
        return self._rows(atom_range, packed.n_atoms).sum(axis=0), np.array([25, 26], dtype=np.int32)

    def bond_order(self, packed, cutoff, sets, l, nbins, nbins_tet, frame_range=None, per_atom=False, out=None):
        t = self._rows(frame_range, packed.n_frames)
        res = (t.sum(axis=0), t[:, :2].sum(axis=0), t)
        return res + (t[:, None, :],) if per_atom else res

    def sq_accumulate(self, packed, hkl, dq, nbins, frame_range=None, frame_stride=1, recip=None, out=None):
        assert recip.shape == (packed.cell.shape[0], 3, 3)
        t = self._rows(frame_range, packed.n_frames, frame_stride)
        return t.sum(axis=0), t[:, :2].sum(axis=0), int(t[:, 2].sum()), KINDS


def multi(n):
    mc = object.__new__(_hip.MultiContext)
    mc.ctxs = [TableContext() for _ in range(n)]
    return mc


def packed_for(cells=1):
    rng = np.random.default_rng(3)
    cell = np.diag([9.0, 9.0, 9.0]) if cells == 1 else np.stack([np.diag([9.0 + 0.1 * k, 9.0, 9.0]) for k in range(F)])
    return PackedTrajectory(rng.uniform(0, 4, (F, N, 3)), cell, np.array([30, 30, 7, 7, 7, 7, 7]))


def same(a, b):
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    return type(a) is type(b) and a == b


# (method, positional arguments after the trajectory, the keyword that carries the shard, spans to try: None = everything)
FRAMES = [None, (3, 11), (5, 7), (4, 4)]        # (5, 7) and (4, 4): fewer frames than contexts, some or all shards empty
ATOMS = [None, (1, 6), (2, 3)]
CALLS = [
    ("rdf_accumulate", (5.0, 10), {}, "frame_range", FRAMES),
    ("cn_count", (None, [(0, 1)]), {}, "frame_range", FRAMES),
    ("cn_count", (None, [(0, 1)]), {"per_atom": True}, "frame_range", FRAMES),
    ("bad_hist", (None, [(0, 1)], [0.0, 90.0, 180.0]), {}, "frame_range", FRAMES),
    ("bad_hist_by_cn", (None, [(0, 1)], [0.0, 90.0, 180.0]), {"cn_max": 5}, "frame_range", FRAMES),
    ("msd_window", (WINDOWS,), {"unwrap": True}, "atom_range", ATOMS),
    ("vanhove_window", (WINDOWS, 0.1, 10), {}, "atom_range", ATOMS),
    ("vanhove_distinct", (WINDOWS, 4.0, 10), {"origin_stride": 2}, "work_range", [None, (2, 9), (3, 4)]),
    ("bond_survival", (None, [(0, 1)], WINDOWS), {}, "atom_range", ATOMS),
    ("bond_reorientation", (None, [(0, 1)], WINDOWS), {"origin_stride": 2}, "atom_range", ATOMS),
    ("bond_order", (None, [(0, 1)], (4, 6), 10, 20), {}, "frame_range", FRAMES),
    ("bond_order", (None, [(0, 1)], (4, 6), 10, 20), {"per_atom": True}, "frame_range", FRAMES),
]


@pytest.mark.parametrize("n_ctx", [2, 3])
@pytest.mark.parametrize("name,args,kwargs,key,spans", CALLS, ids=[c[0] + ("-per_atom" if c[2].get("per_atom") else "") for c in CALLS])
def test_multicontext_shards_tile_the_span_and_merge_bit_for_bit(n_ctx, name, args, kwargs, key, spans):
    packed = packed_for()
    whole = {"frame_range": (0, F), "atom_range": (0, N), "work_range": (0, lags.total_work(F, WINDOWS, 2))}[key]
    for span in spans:
        kw = dict(kwargs) if span is None else dict(kwargs, **{key: span})
        mc = multi(n_ctx)
        got = getattr(mc, name)(packed, *args, **kw)
        one = TableContext()
        want = getattr(one, name)(packed, *args, **dict(kwargs, **{key: span or whole}))
        assert same(got, want), (name, span)
        # every context was called once, on contiguous shares that tile the span in order
        shards = [c.seen for c in mc.ctxs]
        assert all(len(s) == 1 for s in shards)
        lo, hi = span or whole
        edges = [lo] + [s[0][1] for s in shards]
        assert [s[0][0] for s in shards] == edges[:-1] and edges[-1] == hi and edges == sorted(edges)
    # the tuple lengths are Context's: per_atom adds one element (cn_count: a bare array without it)
    if "per_atom" in kwargs:
        assert len(got) == {"cn_count": 2, "bond_order": 4}[name]
    elif name in ("cn_count", "bond_survival"):
        assert isinstance(got, np.ndarray)
    elif name == "bond_order":
        assert len(got) == 3


@pytest.mark.parametrize("n_ctx", [2, 3])
@pytest.mark.parametrize("cells", [1, F])
def test_multicontext_sq_accumulate_gives_whole_strides_to_every_device(n_ctx, cells):
    packed = packed_for(cells)
    hkl = [(1, 0, 0), (0, 1, 1)]
    for span, stride in ((None, 1), (None, 3), (None, 5), ((2, 12), 4), ((1, 13), 7), ((3, 5), 2), ((6, 6), 3)):
        kw = {} if span is None else {"frame_range": span}
        mc = multi(n_ctx)
        got = mc.sq_accumulate(packed, hkl, 0.1, 10, frame_stride=stride, **kw)
        lo, hi = span or (0, F)
        want = TableContext().sq_accumulate(packed, hkl, 0.1, 10, frame_range=(lo, hi), frame_stride=stride,
                                            recip=_hip.reciprocal(packed.cell))
        assert same(got, want), (span, stride)
        # the frames the shards select are the span's selection, each once, in order; every shard starts on a stride
        shards = [c.seen[0] for c in mc.ctxs]
        assert [f for a, b in shards for f in range(a, b, stride)] == list(range(lo, hi, stride))
        assert all((a - lo) % stride == 0 and (a == b or a < b <= hi) for a, b in shards)


def test_multicontext_refuses_device_outputs_and_keeps_its_methods():
    mc, packed = multi(2), packed_for()
    for name, args in (("rdf_accumulate", (5.0, 10)), ("bad_hist", (None, [(0, 1)], [0.0, 180.0])),
                       ("bond_order", (None, [(0, 1)], (4,), 10, 20))):
        with pytest.raises(AssertionError, match="single-context"):
            getattr(mc, name)(packed, *args, out=object())
    for name in [c[0] for c in CALLS] + ["sq_accumulate", "msd_direct", "_shards", "_for_device", "_run"]:
        assert name in vars(_hip.MultiContext), name


def test_merge_results_rules():
    parts = [(np.array([1, 2], dtype=np.uint64), np.array([[1]]), "a"), (np.array([3, 4], dtype=np.uint64), np.array([[2], [3]]), "b")]
    total, rows, first = _hip.merge_results(parts, ("sum", "cat", "first"))
    assert total.dtype == np.uint64 and total.tolist() == [4, 6] and rows.tolist() == [[1], [2], [3]] and first == "a"
    assert _hip.merge_results([p[1] for p in parts], "cat").tolist() == [[1], [2], [3]]


def test_marshalling_helpers():
    a = np.arange(6, dtype=np.float64)
    assert _hip._ptr(None) is None and _hip._ptr(a).value == a.ctypes.data

    class Tensor(object):
        def data_ptr(self):
            return 4096
    assert _hip._ptr(Tensor()).value == 4096
    assert _hip._cutoff([1, 2, 3, 4], 2).dtype == np.float64 and _hip._cutoff([1, 2, 3, 4], 2).shape == (2, 2)
    assert _hip._pairs([(0, 1), (1, -1)]).dtype == np.int32 and _hip._pairs([]).shape == (0, 2)
    assert _hip._hkl([1, 0, 0, 0, 1, 1]).shape == (2, 3) and _hip._i32(np.arange(3)).dtype == np.int32
    packed = packed_for(F)
    assert np.array_equal(_hip._recip(packed, None), _hip.reciprocal(packed.cell)) and _hip._recip(packed, None).flags.c_contiguous
    with pytest.raises(AssertionError):
        _hip._recip(packed, np.zeros((1, 3, 3)))
    assert _hip._span(None, 5) == (0, 5) and _hip._span([1, 2], 5) == (1, 2)


# ------------------------------------------------------------------------------------------- the neighbour-set parser --
def test_neighbour_sets_gives_every_caller_its_fields():
    rng = np.random.default_rng(3)
    packed = PackedTrajectory(rng.uniform(0, 4, (5, 6, 3)), np.diag([9.0, 9.0, 9.0]), np.array([30, 30, 7, 7, 7, 7]))
    dic = {'Zn-N': 2.5, 'Zn-Au': 3.0, 'Au-N': 2.0, 'N-Zn': 2.5}      # both present, partner absent, centre absent, both
    ns = _setup.neighbour_sets(packed, dic)
    assert ns.names == list(dic) and ns.centres == [30, 30, 79, 7]
    assert ns.cutoff.shape == (2, 2) and ns.cutoff[0, 1] == ns.cutoff[1, 0] == 2.5
    # cn.py: a row per present set, zeros where only the centre species exists, NaN where it does not
    assert ns.present == [True, False, False, True] and ns.has_centre == [True, True, False, True]
    assert ns.live == [(1, 0), (0, 1)]
    # bond_order.py: (name, number of A centres, live) and the centre's atomic number
    assert list(zip(ns.names, ns.n_centres, ns.present)) == [('Zn-N', 2, True), ('Zn-Au', 2, False), ('Au-N', 0, False),
                                                              ('N-Zn', 4, True)]
    assert all(type(n) is int for n in ns.n_centres)
    # the bond analyses: (cutoff, [(name, present)], live), and the half-cell check stays theirs alone
    rcm, names, live = lags.neighbour_sets(packed, dic)
    assert np.array_equal(rcm, ns.cutoff) and names == list(zip(ns.names, ns.present)) and live == ns.live
    tight = PackedTrajectory(packed.pos, np.diag([4.0, 9.0, 9.0]), packed.numbers)
    assert _setup.neighbour_sets(tight, dic).live == ns.live
    with pytest.raises(ValueError, match="half the smallest"):
        lags.neighbour_sets(tight, dic)


def test_lags_keeps_its_names():
    assert lags.setup is _setup.setup and lags.pack is _setup.pack and lags.begin_local is _setup.begin_local
    assert lags.Setup is _setup.Setup


# ---------------------------------------------------------------------------------------------------- setup's table --
@pytest.fixture()
def lanes(monkeypatch):
    ls = oracle_context.install(monkeypatch)
    yield ls
    for ctx in ls.values():
        ctx.close_lane()


@pytest.fixture(scope="module")
def traj():
    return H.random_walk(H.zif4_frame(), 6, 0.05, 5)


LANDS_ON = [      # (constructor, the call it makes, its lane while the classes run asynchronously)
    (lambda t: Rdf.from_trajectory(t, dr=0.05, rmax=6.0, distributed=False), "rdf", 0),
    (lambda t: CoordinationNumber.from_trajectory(t, {'Zn-N': 2.5}, distributed=False), "cn", 1),
    (lambda t: Bad.from_trajectory(t, {'Zn-N': 2.5}, dtheta=0.5, distributed=False), "bad", 1),
    (lambda t: BadByCn.from_trajectory(t, {'Zn-N': 2.5}, dtheta=0.5, distributed=False), "bad_by_cn", 0),     # (no lane)
    (lambda t: WindowMsd.from_trajectory(t, delta_time=2, timestep=1, distributed=False), "msd", 1),
]


@pytest.mark.parametrize("asynchronous", ["1", "0"])
@pytest.mark.parametrize("make,call,lane", LANDS_ON, ids=[c[1] for c in LANDS_ON])
def test_every_class_lands_on_its_lane(lanes, traj, monkeypatch, asynchronous, make, call, lane):
    monkeypatch.setenv("AMOF_ASYNC", asynchronous)
    obj = make(traj)
    assert obj.data is not None or call == "bad_by_cn"          # (waits for the lane job)
    lane = lane if asynchronous == "1" else 0
    assert lanes[lane].calls == [call] and lanes[1 - lane].calls == []


def test_setup_states_each_choice(lanes, traj, monkeypatch):
    monkeypatch.setattr(_dist, "world", lambda group=None: (1, 3))
    monkeypatch.setattr(_dist, "merging", lambda world_size: True)
    st = _setup.setup(traj, None, None, lane=1, honour_local=True)
    assert (st.rank, st.world, st.merge, st.sharded, st.on_device) == (1, 3, True, True, False)
    assert st.ctx is lanes[1] and st.packed is traj and st.source is traj
    assert st.shard(10) == _dist.shard_range(10, 1, 3) == (4, 7)
    own = _setup.setup(traj, None, 'local', lane=1, honour_local=True)
    assert own.merge and not own.sharded and own.shard(10) == (0, 10)
    assert _setup.setup(traj, None, 'local', lane=0).sharded            # (StructureFactor, the lag family: 'local' ignored)
    alone = _setup.setup(traj, None, False, lane=None)
    assert (alone.rank, alone.world, alone.merge, alone.sharded) == (0, 1, False, False) and alone.ctx is lanes[0]
    monkeypatch.setenv("AMOF_ASYNC", "0")
    assert _setup.setup(traj, None, None, lane=1).ctx is lanes[0]


def test_a_stream_is_kept_or_read_whole_and_never_merged(lanes, traj, tmp_path, monkeypatch):
    from amof_amd import trajectory as T
    from amof_amd.stream import XyzStream
    path = str(tmp_path / "s.xyz")
    T.write_xyz(path, traj, comment_lattice=False, fmt="%.17g")

    def stream():
        return XyzStream(path, cell=traj.cell[0], batch_frames=4, pinned=False)
    kept = _setup.setup(stream(), None, False, lane=1, keep_stream=True)
    assert kept.packed.is_stream and _setup.streamed(kept)
    whole = _setup.setup(stream(), None, False, lane=1)
    assert isinstance(whole.packed, PackedTrajectory) and np.array_equal(whole.packed.pos, traj.pos) and not _setup.streamed(whole)
    # the ranks cannot merge a stream: ONE ValueError, from every class that walks batches
    monkeypatch.setattr(_dist, "merging", lambda world_size: True)
    text = r"a streamed trajectory is analysed by one process \(distributed=False\)"
    with pytest.raises(ValueError, match=text):
        _setup.streamed(_setup.setup(stream(), None, None, lane=1, keep_stream=True))
    for make in (lambda: Rdf.from_trajectory(stream(), dr=0.05, rmax=6.0),
                 lambda: CoordinationNumber.from_trajectory(stream(), {'Zn-N': 2.5}),
                 lambda: Bad.from_trajectory(stream(), {'Zn-N': 2.5}, dtheta=0.5),
                 lambda: BondOrder.from_trajectory(stream(), {'Zn-N': 2.5})):
        with pytest.raises(ValueError, match=text):
            make()
    assert lanes[0].calls == [] and lanes[1].calls == []


def test_one_layout_of_the_merged_tensor_of_the_lag_analyses():
    """``_hip.lag_layout``: counts, beyond, then the named blocks tile [0, size) without gap or overlap; ``isf_layout`` and
    ``current_layout`` are two calls of it and return what they always did"""
    for S in (1, 3):
        for W in (1, 4):
            for nbins in (1, 7):
                n = W * nbins
                for lay, blocks in ((_hip.isf_layout(S, W, nbins, True), (("coh", S * S), ("self", S))),
                                    (_hip.isf_layout(S, W, nbins, False), (("coh", S * S), ("self", 0))),
                                    (_hip.current_layout(S, W, nbins), (("long", S * S), ("trans", S * S)))):
                    assert lay == _hip.lag_layout(S, W, nbins, blocks)
                    assert set(lay) == {"counts", "beyond", "size"} | {name for name, _ in blocks}
                    spans = [(lay["counts"], n), (lay["beyond"], W)] + [(lay[name], rows * n) for name, rows in blocks]
                    at = 0
                    for start, words in spans:      # in the order of the offsets: each block starts where the last one ended
                        assert start == at
                        at += words
                    assert at == lay["size"]
    assert _hip.isf_layout(3, 4, 7, True) == {"counts": 0, "beyond": 28, "coh": 32, "self": 284, "size": 368}
    assert _hip.isf_layout(3, 4, 7, False) == {"counts": 0, "beyond": 28, "coh": 32, "self": 284, "size": 284}
    assert _hip.current_layout(3, 4, 7) == {"counts": 0, "beyond": 28, "long": 32, "trans": 284, "size": 536}
