"""What every analysis class decides before it computes: the packed trajectory, the ranks, the context of its lane, its
share of the frames / atoms / work list -- and the two things several classes make of their arguments: the neighbour sets
of ``CoordinationNumber``'s dictionary and the batch walk of a streamed trajectory.  (``lags.py`` keeps the names the
lag/origin family has always used as aliases.)
"""

import collections
import threading

from . import _hip
from . import _lazy
from . import atom as amatom
from . import data as _data
from . import dist as _dist
from .frames import pack_trajectory, resident_source


class Setup(collections.namedtuple("Setup", "packed rank world merge ctx on_device source sharded")):
    """``setup``'s answer.  ``merge``: the ranks merge their results; ``sharded``: they split one trajectory (every rank
    holds all of it) rather than each bringing its own block; ``on_device``: a merge stays in HBM (the classes that need
    more say so themselves); ``source``: what the lane job walks or waits for (``begin_local``)."""
    __slots__ = ()

    def shard(self, n):
        """this rank's contiguous share ``[lo, hi)`` of ``n`` frames, atoms or work-list entries: all of them unless sharded"""
        return _dist.shard_range(n, self.rank, self.world) if self.sharded else (0, n)


def pack(trajectory, device, keep_stream=False, upload=True):
    """the packed trajectory (one packed already passes through).  A stream is read whole unless the class walks it batch
    by batch (``keep_stream``); ``upload=False``: a host trajectory's device copy is not started here."""
    packed = pack_trajectory(trajectory, device=(device if device is not None else _hip.default_device()) if upload else None)
    if not keep_stream and getattr(packed, "is_stream", False):
        packed = packed.read_all()
    return packed


def setup(trajectory, device, distributed, lane=0, keep_stream=False, honour_local=False):
    """What every class decides before it shards its work: the packed trajectory (``pack``; one packed already -- a class
    that has checked its arguments against it, which needs no GPU -- passes through), this process's rank and world,
    whether the ranks merge, the lane's context (created here), whether the merge stays in HBM, the source
    ``begin_local`` makes resident, and whether the ranks split the trajectory.  The classes differ in three things:
      lane          0: the pair-bound analyses; 1: the memory-bound ones; None: the device's plain context, called in the
                    constructor itself (no lane job, so no device copy of a host trajectory is started either)
      keep_stream   the class walks a stream batch by batch (``streamed``, ``walk``) instead of reading it whole
      honour_local  ``distributed='local'`` -- the trajectory is this rank's own block -- merges without sharding"""
    packed = pack(trajectory, device, keep_stream, upload=lane is not None)
    rank, world = (0, 1) if distributed is False else _dist.world()
    merge = distributed is not False and _dist.merging(world)
    dev = device if device is not None else getattr(packed, "device_index", None)
    if lane is None:
        ctx, source = _hip.get_context(dev), packed
    else:
        ctx = _hip.lane_context(dev, lane)
        # a host trajectory gets ONE device copy, uploaded while its first analyses walk the part that has arrived
        source = resident_source(packed, ctx.device, allow=not merge and hasattr(ctx, "submit"))
    sharded = merge and not (honour_local and distributed == 'local')
    return Setup(packed, rank, world, merge, ctx, merge and _dist.device_collectives(), source, sharded)


def begin_local(source):
    """first thing of a ``local()`` (the lane job of amof_amd/_lazy.py): the frames are there before the kernels start"""
    if getattr(source, "is_stream", False):
        source.read_all()


def on_lane(ctx, fn):
    """``fn()`` -- a device call a CONSTRUCTOR makes on its lane's context -- in lane order: behind the jobs the context has
    queued, waited for here (what it raises is raised here).  A context is one queue of device calls and some calls come in
    pairs that nothing may split (``msd_shard_begin`` / ``_finish``): a call from the constructor's thread would land among
    the queued jobs wherever the timing puts it.  Called directly where there is no lane (a MultiContext), where the
    classes run synchronously (``AMOF_ASYNC=0``: nothing is ever queued) and from the lane's own thread."""
    if not hasattr(ctx, "submit") or not _lazy.async_enabled() or threading.get_ident() == ctx._lane_thread:
        return fn()
    return ctx.submit(fn).result()


def streamed(st):
    """whether the class walks ``st.source`` batch by batch (a file stream parses its next batch in a background thread, a
    host trajectory's next frames are on their way over PCIe, while this one is on the GPU); ValueError where the ranks
    would have to merge it"""
    if not getattr(st.source, "is_stream", False):
        return False
    if st.merge:
        raise ValueError("a streamed trajectory is analysed by one process (distributed=False)")
    return True


def walk(source, call, rules):
    """``call(batch)`` of every batch of a streamed trajectory, merged element by element (``_hip.merge_results``: frames
    are independent, so integer counts add up and per-frame rows concatenate)"""
    return _hip.merge_results([call(batch) for batch in source.batches()], rules)


NeighbourSets = collections.namedtuple("NeighbourSets", "cutoff names centres has_centre present n_centres live")


def neighbour_sets(packed, nb_set_and_cutoff):
    """``CoordinationNumber``'s dictionary (``'Zn-N': 2.5``: centre Zn, neighbour N) against a trajectory: the ``cutoff``
    matrix ``[S][S]``, and per set, in dictionary order, its name (``names``), the atomic number of the centre species
    (``centres``), whether that species is in the trajectory (``has_centre``), whether both are (``present``) and the
    number of centre atoms (``n_centres``); ``live``: the (centre, neighbour) species indices of the present sets."""
    kinds, _ = _hip.packed_species(packed)
    lut = {z: k for k, z in enumerate(kinds)}
    rcm = amatom.cutoff_matrix(amatom.format_cutoff(nb_set_and_cutoff), kinds)
    counts = packed.species_counts()
    names = list(nb_set_and_cutoff.keys())
    pairs = [tuple(_data.atomic_numbers[i] for i in name.split('-')) for name in names]
    present = [a in lut and b in lut for a, b in pairs]
    return NeighbourSets(rcm, names, [a for a, _ in pairs], [a in lut for a, _ in pairs], present,
                         [int(counts.get(a, 0)) for a, _ in pairs], [(lut[a], lut[b]) for (a, b), ok in zip(pairs, present) if ok])
