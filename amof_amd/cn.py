"""Coordination numbers on MI355X (mirror of reference amof/cn.py).

``CoordinationNumber`` keeps the reference's signatures and ``.data`` schema
(amof/cn.py:25-100).  The ASE neighbour search that takes "92% of computation
time" in the reference (amof/cn.py:65) and the per-atom counting loop
(amof/cn.py:67-73) run in the HIP kernel behind ``amof_cn_count``.
"""

import logging

import numpy as np
import pandas as pd

from ._lazy import Deferred, EmptyUntilComputed

from . import _setup
from . import dist as _dist
from . import trajectory as _trajectory
from .files import path as _path

logger = logging.getLogger(__name__)


class CoordinationNumber(Deferred):
    """
    Main class to compute CoordinationNumber

    ``from_trajectory`` enqueues the analysis on its device's second lane and returns; ``.data`` waits for it
    (amof_amd/_lazy.py; ``AMOF_ASYNC=0``: synchronous).
    """

    data = EmptyUntilComputed("Step")      # (the reference's empty first-column frame, built on first look)

    def __init__(self):
        """default constructor"""
        self.data = None

    @classmethod
    def from_trajectory(cls, trajectory, nb_set_and_cutoff, delta_Step=1, first_frame=0, parallel=False,
                        device=None, distributed=None):
        """
        constructor of CoordinationNumber class from a trajectory
        Args:
            nb_set_and_cutoff: dict, keys are str indicating pair of neighbours,
                values are cutoffs float, in Angstrom
            parallel: accepted for compatibility; frames always run in
                parallel on the GPU
        """
        cn_class = cls()
        step = _trajectory.construct_step(delta_Step=delta_Step, first_frame=first_frame,
                                          number_of_frames=len(trajectory))
        cn_class.compute_cn(trajectory, nb_set_and_cutoff, step, parallel, device=device, distributed=distributed)
        return cn_class

    def compute_cn(self, trajectory, nb_set_and_cutoff, step, parallel=False, device=None, distributed=None):
        """compute coordination numbers (reference amof/cn.py:48-82)"""
        packed = _setup.pack(trajectory, device, keep_stream=True)
        logger.info("Start computing coordination number for %s frames", len(packed))
        ns = _setup.neighbour_sets(packed, nb_set_and_cutoff)
        rcm, live = ns.cutoff, ns.live
        st = _setup.setup(packed, device, distributed, lane=1, keep_stream=True, honour_local=True)
        ctx, source = st.ctx, st.source
        frame_range = st.shard(len(packed))

        def assemble(sums):
            data = {'Step': np.asarray(step)[:len(sums)] if distributed == 'local' else step}
            k = 0
            for name, ok, has_a, n_a in zip(ns.names, ns.present, ns.has_centre, ns.n_centres):
                if ok:
                    col = sums[:, k].astype(np.float64) / n_a   # np.mean of integer counts (amof/cn.py:73)
                    k += 1
                elif has_a:
                    col = np.zeros(len(sums))                   # centres exist, partner species absent
                else:
                    col = np.full(len(sums), np.nan)            # np.mean([]) in the reference
                data[name] = col
            self.data = pd.DataFrame(data)

        def count(part, frame_range=None):
            if live:
                return ctx.cn_count(part, rcm, live, frame_range=frame_range)
            return np.zeros((len(part) if frame_range is None else frame_range[1] - frame_range[0], 0), dtype=np.int64)

        if _setup.streamed(st):
            self._defer(ctx, lambda: _setup.walk(source, count, "cat"), assemble)
            return

        def finish(sums):
            if st.sharded:
                sums = _dist.all_gather_rows(sums, device=ctx.device)
            assemble(sums)

        # (local: this rank's kernels, a lane job -- amof_amd/_lazy.py)
        self._defer(ctx, lambda: count(packed, frame_range), finish, collective=st.sharded)

    @classmethod
    def from_file(cls, filename):
        """constructor of cn class from cn file"""
        cn_class = cls()
        cn_class.read_cn_file(filename)
        return cn_class

    def read_cn_file(self, filename):
        filename = _path.append_suffix(filename, 'cn')
        self.data = pd.read_feather(filename)

    def write_to_file(self, filename):
        filename = _path.append_suffix(filename, 'cn')
        self.data.to_feather(filename)
