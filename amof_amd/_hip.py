"""ctypes binding of ``libamofhip.so`` (the C ABI declared in include/amof_hip.h).

This is the only compute back end of the package: there is no CPU fallback.
If the shared library is missing, or no GPU is visible, the analysis classes
raise -- they never silently compute somewhere else.
"""

import collections
import ctypes
import os
import threading
import time

import numpy as np

from .frames import PackedTrajectory, _is_torch_tensor

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AMOF_HIP_LIB") or os.path.join(_HERE, "csrc", "libamofhip.so")

AMOF_OK = 0
AMOF_EINVAL = -1
AMOF_ESINGULAR = -2
AMOF_EANGLE = -3
AMOF_ENOMEM = -4
AMOF_EHIP = -5
AMOF_ECAPACITY = -6
AMOF_ENODEVICE = -7
AMOF_EUNSUPPORTED = -8
ABI_VERSION = 4

EXPORTS = [
    "amof_abi_version", "amof_device_count", "amof_ctx_create", "amof_ctx_create2", "amof_ctx_destroy", "amof_last_error",
    "amof_ctx_set_stream", "amof_ctx_synchronize", "amof_ctx_wait_stream", "amof_ctx_follow", "amof_ctx_calls", "amof_ctx_debug_poison", "amof_last_kernel_seconds", "amof_last_kernel_launches",
    "amof_last_path",
    "amof_rdf_accumulate", "amof_rdf_accumulate_dev", "amof_cn_count", "amof_bad_hist", "amof_bad_hist_dev",
    "amof_bad_hist_by_cn",
    "amof_msd_window", "amof_msd_window_dev", "amof_msd_com_dev", "amof_msd_shard_begin", "amof_msd_shard_finish", "amof_msd_direct",
    "amof_vanhove_window", "amof_vanhove_window_dev", "amof_vanhove_distinct", "amof_vanhove_distinct_dev",
    "amof_vacf_window", "amof_vacf_window_dev",
    "amof_bond_survival", "amof_bond_survival_dev", "amof_bond_reorientation", "amof_bond_reorientation_dev",
    "amof_lindemann", "amof_lindemann_dev",
    "amof_bond_order", "amof_bond_order_dev", "amof_dihedral_hist", "amof_dihedral_hist_dev", "amof_ring_stats", "amof_ring_search_stats", "amof_fragment_stats", "amof_fragment_round_stats",
    "amof_pore_field", "amof_pore_candidate_bound",
    "amof_pore_access", "amof_pore_access_field", "amof_pore_psd", "amof_pore_psd_field", "amof_pore_cover_stats",
    "amof_pore_surface", "amof_pore_surface_bound", "amof_pore_surface_stats",
    "amof_sq_accumulate", "amof_sq_accumulate_dev", "amof_sq_modes", "amof_isf_accumulate", "amof_isf_accumulate_dev",
    "amof_current_modes", "amof_current_accumulate", "amof_current_accumulate_dev",
    "amof_xyz_scan", "amof_xyz_read", "amof_xyz_open", "amof_xyz_read_frames", "amof_xyz_close", "amof_cp2k_cell_read", "amof_ingest_last_error",
    "amof_pack_frames", "amof_frames_checksum",
]


class AmofError(RuntimeError):
    def __init__(self, code, message):
        RuntimeError.__init__(self, "libamofhip error %d: %s" % (code, message))
        self.code = code


class Unsupported(AmofError):
    """AMOF_EUNSUPPORTED: a specialised entry point does not take the arguments; the caller uses the general one"""


class AmofTraj(ctypes.Structure):
    """``struct amof_traj`` (include/amof_hip.h)."""
    _fields_ = [
        ("pos", ctypes.c_void_p),
        ("pos_on_device", ctypes.c_int32),
        ("n_species", ctypes.c_int32),
        ("cell", ctypes.c_void_p),
        ("n_cells", ctypes.c_int64),
        ("n_frames", ctypes.c_int64),
        ("n_atoms", ctypes.c_int64),
        ("species", ctypes.c_void_p),
        ("masses", ctypes.c_void_p),
        ("pbc", ctypes.c_uint8 * 3),
        ("_pad", ctypes.c_uint8 * 5),
    ]


_lib = None
_lib_lock = threading.Lock()
_ctx_lock = threading.Lock()


def load_library():
    """Load ``libamofhip.so`` (in-tree build) and declare the prototypes."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "amof_amd: %s not found. Build it with `make -C amof_amd/csrc` or "
                "`python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU fallback." % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.  If torch is
        # importable, let it load first so that this library binds to the same runtime (loading the
        # system runtime first makes torch.cuda report "No HIP GPUs are available" later on).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(LIB_PATH)
        P = ctypes.c_void_p
        lib.amof_abi_version.restype = ctypes.c_int
        lib.amof_device_count.restype = ctypes.c_int
        lib.amof_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(P)]
        lib.amof_ctx_create2.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(P)]
        lib.amof_ctx_destroy.argtypes = [P]
        lib.amof_ctx_destroy.restype = None
        lib.amof_last_error.argtypes = [P]
        lib.amof_last_error.restype = ctypes.c_char_p
        lib.amof_ctx_set_stream.argtypes = [P, P]
        lib.amof_ctx_synchronize.argtypes = [P]
        lib.amof_ctx_wait_stream.argtypes = [P, P]
        lib.amof_ctx_follow.argtypes = [P, P, ctypes.c_int64, ctypes.c_double]
        lib.amof_ctx_calls.argtypes = [P]
        lib.amof_ctx_calls.restype = ctypes.c_int64
        lib.amof_ctx_debug_poison.argtypes = [P, ctypes.c_int]
        lib.amof_last_kernel_seconds.argtypes = [P, ctypes.c_int]
        lib.amof_last_kernel_seconds.restype = ctypes.c_double
        lib.amof_last_kernel_launches.argtypes = [P]
        lib.amof_last_kernel_launches.restype = ctypes.c_int64
        lib.amof_last_path.argtypes = [P]
        lib.amof_last_path.restype = ctypes.c_char_p
        TP = ctypes.POINTER(AmofTraj)
        lib.amof_rdf_accumulate.argtypes = [P, TP, ctypes.c_double, ctypes.c_int32, P, ctypes.POINTER(ctypes.c_double)]
        lib.amof_rdf_accumulate_dev.argtypes = lib.amof_rdf_accumulate.argtypes
        lib.amof_cn_count.argtypes = [P, TP, P, P, ctypes.c_int32, P, P]
        lib.amof_bad_hist.argtypes = [P, TP, P, P, ctypes.c_int32, P, ctypes.c_int32, P, P]
        lib.amof_bad_hist_dev.argtypes = lib.amof_bad_hist.argtypes
        lib.amof_bad_hist_by_cn.argtypes = [P, TP, P, P, ctypes.c_int32, P, ctypes.c_int32, ctypes.c_int32, P, P]
        lib.amof_msd_window.argtypes = [P, TP, P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                        ctypes.c_int64, ctypes.c_int64, P]
        lib.amof_msd_window_dev.argtypes = [P, TP, P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                            ctypes.c_int64, ctypes.c_int64, P, P]
        lib.amof_msd_com_dev.argtypes = [P, TP, ctypes.c_int64, ctypes.c_int64, P]
        lib.amof_msd_shard_begin.argtypes = [P, TP, P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, P]
        lib.amof_msd_shard_finish.argtypes = [P, TP, P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, P, P]
        lib.amof_msd_direct.argtypes = [P, TP, P]
        lib.amof_vanhove_window.argtypes = [P, TP, P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                            ctypes.c_int64, ctypes.c_double, ctypes.c_int32, P, P, P]
        lib.amof_vanhove_window_dev.argtypes = [P, TP, P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                                ctypes.c_int64, ctypes.c_double, ctypes.c_int32, P, P, P, P]
        lib.amof_vacf_window.argtypes = [P, TP, P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                         ctypes.c_int64, P]
        lib.amof_vacf_window_dev.argtypes = [P, TP, P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                             ctypes.c_int64, P, P]
        lib.amof_vanhove_distinct.argtypes = [P, TP, P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                              ctypes.c_double, ctypes.c_int32, P]
        lib.amof_vanhove_distinct_dev.argtypes = lib.amof_vanhove_distinct.argtypes
        lib.amof_bond_survival.argtypes = [P, TP, P, P, ctypes.c_int32, P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64,
                                           ctypes.c_int64, P]
        lib.amof_bond_survival_dev.argtypes = lib.amof_bond_survival.argtypes
        lib.amof_bond_reorientation.argtypes = lib.amof_bond_survival.argtypes + [P]
        lib.amof_bond_reorientation_dev.argtypes = lib.amof_bond_reorientation.argtypes
        lib.amof_lindemann.argtypes = [P, TP, P, P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.c_double, ctypes.c_int64, ctypes.c_int64, P, P, P, P]
        lib.amof_lindemann_dev.argtypes = lib.amof_lindemann.argtypes
        lib.amof_bond_order.argtypes = [P, TP, P, P, ctypes.c_int32, P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P, P, P, P]
        lib.amof_bond_order_dev.argtypes = lib.amof_bond_order.argtypes
        lib.amof_dihedral_hist.argtypes = [P, TP, P, P, ctypes.c_int32, P, ctypes.c_int32, P, P, P, P]
        lib.amof_dihedral_hist_dev.argtypes = lib.amof_dihedral_hist.argtypes
        lib.amof_ring_stats.argtypes = [P, TP, P, ctypes.c_int32, P, P, P, P]
        lib.amof_ring_search_stats.argtypes = [P, P]
        lib.amof_fragment_stats.argtypes = [P, TP, P, P, P, P, ctypes.c_int32, ctypes.c_int32, P, P, P, P, P, P, P, P, ctypes.c_int32]
        lib.amof_fragment_round_stats.argtypes = [P, P]
        lib.amof_pore_field.argtypes = [P, TP, P, P, ctypes.c_double, ctypes.c_double, P, ctypes.c_int32, P, P, P, P, P]
        lib.amof_pore_candidate_bound.argtypes = [P, ctypes.c_double]
        lib.amof_pore_access.argtypes = [P, TP, P, P, ctypes.c_double, ctypes.c_double, P, ctypes.c_int32, ctypes.c_int32,
                                         P, P, P, P, P, P, P, P]
        lib.amof_pore_access_field.argtypes = [P, P, ctypes.c_int64, P, P, P, ctypes.c_int32, ctypes.c_int32, P, P, P]
        lib.amof_pore_psd.argtypes = [P, TP, P, P, ctypes.c_double, ctypes.c_double, P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                      P, P, P, P, P, P, P, P, P, P, P, P]
        lib.amof_pore_psd_field.argtypes = [P, P, P, ctypes.c_int64, P, P, ctypes.c_double, ctypes.c_double, P, ctypes.c_int32,
                                            ctypes.c_int32, P, P, P, P]
        lib.amof_pore_cover_stats.argtypes = [P, P]
        lib.amof_pore_surface.argtypes = lib.amof_pore_psd.argtypes + [ctypes.c_int32, P, ctypes.c_int32, P, P, P]
        lib.amof_pore_surface_bound.argtypes = [P, ctypes.c_double]
        lib.amof_pore_surface_bound.restype = ctypes.c_double
        lib.amof_pore_surface_stats.argtypes = [P, P]
        lib.amof_pore_candidate_bound.restype = ctypes.c_double
        lib.amof_sq_accumulate.argtypes = [P, TP, P, P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                           ctypes.c_double, ctypes.c_int32, P, P, P]
        lib.amof_sq_accumulate_dev.argtypes = [P, TP, P, P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                               ctypes.c_double, ctypes.c_int32, P, P, P, P]
        lib.amof_sq_modes.argtypes = [P, TP, ctypes.c_int64, P, ctypes.c_int32, P]
        lib.amof_isf_accumulate.argtypes = [P, TP, P, P, ctypes.c_int32, P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.c_int64, ctypes.c_double, ctypes.c_int32, P, P, P, P]
        lib.amof_isf_accumulate_dev.argtypes = [P, TP, P, P, ctypes.c_int32, P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64,
                                                ctypes.c_int64, ctypes.c_double, ctypes.c_int32, P, P, P, P, P]
        lib.amof_current_modes.argtypes = [P, TP, TP, ctypes.c_int64, ctypes.c_int32, P, ctypes.c_int32, P]
        lib.amof_current_accumulate.argtypes = [P, TP, TP, ctypes.c_int32, P, P, ctypes.c_int32, P, ctypes.c_int32, ctypes.c_int64,
                                                ctypes.c_int64, ctypes.c_int64, ctypes.c_double, ctypes.c_int32, P, P, P, P, P, P]
        lib.amof_current_accumulate_dev.argtypes = lib.amof_current_accumulate.argtypes
        lib.amof_xyz_scan.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
        lib.amof_xyz_read.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                      P, P, P, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]
        lib.amof_xyz_open.argtypes = [ctypes.c_char_p, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_int64),
                                      ctypes.POINTER(ctypes.c_int64)]
        lib.amof_xyz_read_frames.argtypes = [P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                             P, P, P, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]
        lib.amof_xyz_close.argtypes = [P]
        lib.amof_xyz_close.restype = None
        lib.amof_cp2k_cell_read.argtypes = [ctypes.c_char_p, ctypes.c_int64, P, ctypes.POINTER(ctypes.c_int64)]
        lib.amof_ingest_last_error.restype = ctypes.c_char_p
        lib.amof_pack_frames.argtypes = [P, ctypes.c_int64, ctypes.c_int64, P, P, ctypes.c_int32]
        lib.amof_frames_checksum.argtypes = [P, ctypes.c_int64, ctypes.c_int64, P, ctypes.c_int32]
        if lib.amof_abi_version() != ABI_VERSION:
            raise RuntimeError("libamofhip.so ABI version %d, expected %d" % (lib.amof_abi_version(), ABI_VERSION))
        _lib = lib
        return lib


def pore_surface_bound(cell, reach):
    """``amof_pore_surface_bound``: the bound (Angstrom) of the float32 compare of the "pore_surface_list" path for one cell
    ``[3][3]`` and ``reach = the largest radius + the largest probe radius``"""
    cell = np.ascontiguousarray(cell, dtype=np.float64).reshape(9)
    return float(load_library().amof_pore_surface_bound(_ptr(cell), float(reach)))


def lag_layout(S, W, nbins, blocks):
    """word offsets of the one int64 tensor a lag analysis adds into: ``counts [W][nbins]``, ``beyond [W]``, then every
    ``(name, rows)`` of ``blocks`` as ``[rows][W][nbins]`` in order (rows = 0: the name keeps its place and takes no word),
    and its ``size``"""
    n = W * nbins
    lay = {"counts": 0, "beyond": n}
    at = n + W
    for name, rows in blocks:
        lay[name] = at
        at += rows * n
    lay["size"] = at
    return lay


def isf_layout(S, W, nbins, self_part=True):
    """``lag_layout`` of ``Context.isf_accumulate(out=...)``: ``coh [S][S][W][nbins]``, ``self [S][W][nbins]`` (absent without
    ``self_part``)"""
    return lag_layout(S, W, nbins, (("coh", S * S), ("self", S if self_part else 0)))


def current_layout(S, W, nbins):
    """``lag_layout`` of ``Context.current_accumulate(out=...)``: ``long [S][S][W][nbins]``, ``trans [S][S][W][nbins]``"""
    return lag_layout(S, W, nbins, (("long", S * S), ("trans", S * S)))


def reciprocal(cell):
    """``2 pi inv(cell).T`` of every cell (``[..][3][3]``, rows = cell vectors): rows = reciprocal vectors (amof_sq_*)"""
    cell = np.asarray(cell, dtype=np.float64)
    return 2.0 * np.pi * np.swapaxes(np.linalg.inv(cell), -1, -2)


def device_count():
    return load_library().amof_device_count()


def pore_candidate_bound(cell, rcut):
    """``amof_pore_candidate_bound``: the bound (Angstrom) of the float32 candidate of the "pore_brick" path for one cell
    ``[3][3]`` and ``rcut = dmax + the largest radius``"""
    cell = np.ascontiguousarray(cell, dtype=np.float64).reshape(9)
    return float(load_library().amof_pore_candidate_bound(_ptr(cell), float(rcut)))


def species_index(numbers):
    """Map atomic numbers to the C ABI's species indices.

    Returns ``(kinds, species)``: ``kinds`` = sorted unique atomic numbers,
    ``species[i]`` = index of atom i's number in ``kinds`` (int32)."""
    numbers = np.asarray(numbers)
    uniq, inverse = np.unique(numbers, return_inverse=True)
    return [int(z) for z in uniq], inverse.astype(np.int32).reshape(-1)


def packed_species(packed):
    """:func:`species_index` of a PackedTrajectory, computed once per trajectory (numbers never change)."""
    cached = getattr(packed, "_abi_species", None)
    if cached is None:
        cached = species_index(packed.numbers)
        packed._abi_species = cached
    return cached


class _TrajHandle(object):
    """Keeps the numpy buffers behind an ``AmofTraj`` alive."""

    def __init__(self, packed, frame_range=None):
        if getattr(packed, "is_stream", False):
            raise TypeError("this analysis does not walk a stream batch by batch: pass stream.read_all() (Rdf, "
                            "cn.CoordinationNumber and Bad accept the stream itself)")
        if not isinstance(packed, PackedTrajectory):
            raise TypeError("expected a PackedTrajectory, got %s" % type(packed).__name__)
        f0, f1 = (0, packed.n_frames) if frame_range is None else frame_range
        self.kinds, self.species = packed_species(packed)
        pos = getattr(packed, "_dev_pos", None)        # (PackedTrajectory.keep_on_device: resident copy of a host array)
        if pos is None:
            pos = packed.pos
        cell = packed.cell if packed.cell.shape[0] == 1 else packed.cell[f0:f1]
        self.cell = np.ascontiguousarray(cell, dtype=np.float64)
        self.masses = np.ascontiguousarray(packed.masses, dtype=np.float64)
        t = AmofTraj()
        if _is_torch_tensor(pos):
            sub = pos[f0:f1]
            if not sub.is_contiguous():
                sub = sub.contiguous()
            self._pos = sub
            if sub.is_cuda:
                t.pos = sub.data_ptr()
                t.pos_on_device = 1
                self.device_index = sub.device.index
            else:
                t.pos = sub.data_ptr()
                t.pos_on_device = 0
                self.device_index = None
        else:
            sub = np.ascontiguousarray(pos[f0:f1])
            self._pos = sub
            t.pos = sub.ctypes.data
            t.pos_on_device = 0
            self.device_index = None
        t.n_species = len(self.kinds)
        t.cell = self.cell.ctypes.data
        t.n_cells = self.cell.shape[0]
        t.n_frames = f1 - f0
        t.n_atoms = packed.n_atoms
        t.species = self.species.ctypes.data
        t.masses = self.masses.ctypes.data
        for k in range(3):
            t.pbc[k] = 1 if packed.pbc[k] else 0
        self.c = t
        self.n_frames = f1 - f0
        self.n_atoms = packed.n_atoms
        self.S = len(self.kinds)


def _locked(method):
    """An ``amof_ctx`` is not thread-safe (include/amof_hip.h): serialise the calls of one Context.
    ctypes drops the GIL during a call, so two Python threads could otherwise be inside the same
    context at once; distinct Context objects still run concurrently."""
    def wrapper(self, *args, **kwargs):
        with self._lock:
            return method(self, *args, **kwargs)
    wrapper.__name__ = method.__name__
    wrapper.__doc__ = method.__doc__
    return wrapper


AMOF_CTX_HIGH_PRIORITY = 1
AMOF_CTX_LOW_PRIORITY = 2

_tls = threading.local()      # .producer_stream: the stream a lane job orders itself after (see Lane.submit)


class Lane(object):
    """One worker thread that runs jobs in submission order (the analysis classes enqueue their computation here and
    return: amof_amd/_lazy.py).  Mixed into :class:`Context`; ``device`` is the GPU whose current torch stream a job is
    ordered after (None: no GPU involved -- the CPU stand-ins of the test-suite)."""

    device = None
    _lane = None
    _lane_thread = None
    _last_job = None
    _lane_name = "amof-lane"
    _follows = None         # the lane whose kernels this lane's jobs are queued behind (Context.follow_leader)
    _jobs_submitted = 0     # (plain counters, written under the GIL: submit by the callers, the other two by the worker)
    _jobs_started = 0
    _jobs_finished = 0
    _calls_at_job_start = 0

    def submit(self, fn):
        """Run ``fn()`` on the worker thread, after everything submitted before; returns the
        ``concurrent.futures.Future``.  The job orders the context's stream after the work queued so far on the
        CALLER's current torch stream of this device (captured here: what produced a device-resident trajectory)."""
        from concurrent.futures import ThreadPoolExecutor
        if self._lane is None:
            with _ctx_lock:
                if self._lane is None:
                    self._lane = ThreadPoolExecutor(1, thread_name_prefix=self._lane_name)
        producer = None
        if self.device is not None:
            try:
                import torch
                if torch.cuda.is_available():
                    producer = torch.cuda.current_stream(self.device).cuda_stream
            except ImportError:
                pass

        def job():
            self._lane_thread = threading.get_ident()
            _tls.producer_stream = producer
            self._calls_at_job_start = self.device_calls()
            self._jobs_started += 1
            try:
                if self._follows is not None:
                    self.follow_leader()
                return fn()
            finally:
                _tls.producer_stream = None
                self._jobs_finished += 1
        self._jobs_submitted += 1
        fut = self._lane.submit(job)
        self._last_job = fut
        return fut

    def device_calls(self):
        """device calls begun on this lane's context so far (0: not a GPU context)"""
        return 0

    def follow_leader(self):
        """(GPU contexts) queue this lane's next kernels behind the leader lane's"""

    def drain(self):
        """wait for every job submitted to the lane (their errors stay with their futures)"""
        fut = self._last_job
        if fut is None or threading.get_ident() == self._lane_thread:
            return
        fut.exception()         # (jobs run in submission order: the last one done = all done)

    def close_lane(self):
        self.drain()
        if self._lane is not None:
            self._lane.shutdown(wait=True)
            self._lane = None


# -- marshalling: what the entry points of include/amof_hip.h take, from what the callers hand in -------------------------
def _ptr(x):
    """``c_void_p`` of a numpy array's or a torch tensor's memory; None (an optional argument) stays None"""
    if x is None:
        return None
    return ctypes.c_void_p(x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())


def _cutoff(x, S):
    """cutoff matrix ``[S][S]`` f64"""
    return np.ascontiguousarray(x, dtype=np.float64).reshape(S, S)


def _pairs(x):
    """``sets`` / ``triples``: species index pairs ``[n][2]`` i32"""
    return np.ascontiguousarray(x, dtype=np.int32).reshape(-1, 2)


def _i32(x):
    """``windows`` (and other index lists): i32"""
    return np.ascontiguousarray(x, dtype=np.int32)


def _hkl(x):
    """reciprocal-lattice vectors ``[K][3]`` i32"""
    return np.ascontiguousarray(x, dtype=np.int32).reshape(-1, 3)


def _recip(packed, recip):
    """``[n_cells][3][3]`` f64 reciprocal cells of a trajectory (default: ``reciprocal(packed.cell)``)"""
    recip = np.ascontiguousarray(reciprocal(packed.cell) if recip is None else recip, dtype=np.float64)
    assert recip.shape == (packed.cell.shape[0], 3, 3)
    return recip


def _label_cap(labels, n_t, G):
    """the library's cap on ``labels`` (4 GiB per frame, AMOF_ECAPACITY), raised before the array is allocated"""
    if labels and 4 * n_t * G > 2 ** 32:
        raise AmofError(AMOF_ECAPACITY, "labels of %d thresholds x %d points exceed the 4 GiB a frame may take" % (n_t, G))


# the arrays of the Pore calls in the order of the tuples ``pore_field`` / ``pore_access`` / ``pore_psd`` return: name, the flag that
# asks for it (None: always), its shape behind [F] (b: nbins + 2, t: n_t, g: the grid, C-contiguous [G] to the library, s: species,
# n: atoms, m: directions), dtype
_PORE = (("hist", None, "b", np.uint64), ("counts", None, "t", np.int64), ("vmax", None, "", np.float64), ("argmax", None, "", np.int64),
         ("access", "labelled", "t4", np.int64), ("free_sphere", "free_sphere", "2", np.float64), ("field", "per_point", "g", np.float64),
         ("labels", "labels", "tg", np.int32), ("psd_hist", "psd", "b", np.uint64), ("po_counts", "psd", "t", np.int64),
         ("po_access", "po_access", "t", np.int64), ("cover", "cover", "g", np.float64), ("exposed", "surface", "ts", np.int64),
         ("exposed_access", "exposed_access", "ts", np.int64), ("samples", "samples", "tnm", np.uint8))
PoreResult = collections.namedtuple("PoreResult", [x[0] for x in _PORE], defaults=(None,) * len(_PORE))


def pore_names(per_point=False, labelled=False, free_sphere=False, labels=False, psd=False, accessibility=False, surface=False):
    """which arrays a call with these flags returns, in the tuple's order (``labelled``: ``pore_access``, or ``pore_psd`` /
    ``pore_surface`` with ``accessibility`` or ``free_sphere``; ``surface``: ``pore_surface``)"""
    flags = dict(locals(), po_access=psd and accessibility, cover=psd and per_point, exposed_access=surface and accessibility,
                 samples=surface and per_point)
    return tuple(name for name, flag, _, _ in _PORE if flag is None or flags[flag])


def _pore_alloc(names, F, n_t, nbins, shape, S=0, N=0, M=0):
    """zeroed arrays of these names as a ``PoreResult``"""
    dims = {"b": (nbins + 2,), "t": (n_t,), "4": (4,), "2": (2,), "g": tuple(shape), "s": (S,), "n": (N,), "m": (M,)}
    return PoreResult(**{name: np.zeros((F,) + sum((dims[c] for c in dim), ()), dtype=kind) for name, _, dim, kind in _PORE if name in names})


def _span(given, n):
    """a ``frame_range`` / ``atom_range`` argument as ``(lo, hi)``: all ``n`` by default"""
    return (0, n) if given is None else tuple(given)


def _whole_work_list(n_frames, windows, origin_stride):
    """``work_range`` of every (lag, origin) pair (a stride below 1 is the library's to refuse)"""
    from . import lags
    return 0, lags.total_work(n_frames, windows, max(1, int(origin_stride)))


class Context(Lane):
    """One ``amof_ctx``: a device, a stream and its scratch memory -- and, for the analysis classes, a LANE: one worker
    thread that runs the (synchronous) entry points of this context in submission order, so that a class constructor
    can enqueue its analysis and return (``submit``; amof_amd/_lazy.py).  A device has two cached contexts
    (``get_context``): lane 0 for the pair-evaluation-bound RDF, lane 1 -- a stream of the highest priority -- for the
    memory-bound MSD / BAD / CN, whose kernels and host work then run beside an RDF launch instead of behind it."""

    def __init__(self, device=0, high_priority=False, priority=None):
        self._lib = load_library()
        n = self._lib.amof_device_count()
        if n <= 0:
            raise RuntimeError("amof_amd: no GPU visible to HIP; the MI355X kernels cannot run "
                               "(there is no CPU fallback)")
        h = ctypes.c_void_p()
        if priority is None:
            priority = "high" if high_priority else "normal"
        flags = {"high": AMOF_CTX_HIGH_PRIORITY, "low": AMOF_CTX_LOW_PRIORITY, "normal": 0}[priority]
        rc = self._lib.amof_ctx_create2(int(device), flags, ctypes.byref(h))
        if rc != AMOF_OK:
            raise AmofError(rc, "amof_ctx_create2(device=%d) failed" % device)
        self._h = h
        self.device = int(device)
        self.priority = priority
        self.high_priority = priority == "high"
        self._lane_name = "amof-lane-%d%s" % (self.device, "h" if high_priority else "")
        self._lock = threading.RLock()

    def close(self):
        self.close_lane()
        if getattr(self, "_h", None):
            self._lib.amof_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc == AMOF_OK:
            return
        msg = self._lib.amof_last_error(self._h).decode("utf-8", "replace")
        if rc == AMOF_EANGLE:
            raise ZeroDivisionError("Undefined angle")  # what ASE raises (reference amof/bad.py:100)
        if rc == AMOF_EINVAL:
            raise ValueError(msg)
        if rc == AMOF_EUNSUPPORTED:
            raise Unsupported(rc, msg)
        raise AmofError(rc, msg)

    def device_calls(self):
        """calls of this context that have started device work (``amof_ctx_calls``; any thread may ask)"""
        return int(self._lib.amof_ctx_calls(self._h)) if getattr(self, "_h", None) else 0

    def follow_leader(self):
        """Queue this context's next kernels BEHIND the leader lane's (``amof_ctx_follow``; lane 1 follows lane 0 of its
        device).  If the leader has a job pending, wait -- on the host, a fraction of a millisecond -- until that job has
        queued its dominant kernel, then order this context's stream after the leader's: the kernels of the memory-bound
        analyses then run when the RDF tile kernel has finished, beside the RDF's read-back and DataFrame assembly, and
        this lane's host work beside the tile kernel.  Side by side the two lose: the tile kernel fills LDS and registers,
        a second stream's workgroups trickle in between (profiles/r05/stops.txt A).  Nothing to follow (leader idle):
        returns at once.  OPT-IN, ``AMOF_LANE_ORDER=1``: measured against the unordered lanes it changes nothing at N = 1
        (74.2 / 74.6 against 74.8 / 74.6 ms per step, sequential 74.6 / 74.1) and costs 0.1 - 0.2 ms for one rank of eight,
        where the followers' kernels and result assembly end up behind the RDF's instead of before it
        (profiles/r05/lane_order.txt)."""
        lead = self._follows
        if lead is None or lead is self or os.environ.get("AMOF_LANE_ORDER", "0") != "1":
            return
        target = lead._jobs_submitted
        if lead._jobs_finished >= target:
            return                                  # the leader is idle: nothing queued that this lane could be stuck behind
        while lead._jobs_finished < target:
            if lead._jobs_started >= target:
                # the job we follow is running: its first device call is number _calls_at_job_start + 1 of its context
                with self._lock:
                    rc = self._lib.amof_ctx_follow(self._h, lead._h, lead._calls_at_job_start + 1, 0.0005)
                if rc < 0:
                    self._check(rc)
                if rc == 1:
                    return
            else:
                time.sleep(2e-5)                    # (still queued behind an earlier job of its lane)
        # the leader's job ended without a dominant kernel (an empty trajectory, an error): plain stream order
        with self._lock:
            self._check(min(0, self._lib.amof_ctx_follow(self._h, lead._h, 0, 0.0)))

    @_locked
    def set_stream(self, stream_ptr):
        self._check(self._lib.amof_ctx_set_stream(self._h, ctypes.c_void_p(stream_ptr or None)))

    def use_torch_stream(self):
        import torch
        self.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def synchronize(self):
        self.drain()
        with self._lock:
            self._check(self._lib.amof_ctx_synchronize(self._h))

    def debug_poison(self, byte=0xA5):
        """Test hook: overwrite every scratch buffer the context owns (no call may rely on a previous call's scratch)."""
        self.drain()
        with self._lock:
            self._check(self._lib.amof_ctx_debug_poison(self._h, int(byte)))

    @_locked
    def wait_stream(self, stream_ptr):
        """Order this context's stream after the work queued so far on another HIP stream."""
        self._check(self._lib.amof_ctx_wait_stream(self._h, ctypes.c_void_p(stream_ptr or None)))

    def _torch_stream(self):
        """the torch stream whose queued work this call must run after: the current stream of the calling thread -- in a
        lane job, the current stream of the thread that SUBMITTED the job (and the lane thread's own, on which the job
        may have zeroed its output tensors)"""
        import torch
        own = torch.cuda.current_stream(self.device).cuda_stream
        producer = getattr(_tls, "producer_stream", None)
        if producer is not None and producer != own:
            self.wait_stream(producer)
        return own

    def _order_after_torch(self):
        """device outputs (``out=`` tensors) were zeroed / last written by torch: run after that.  The "_dev" entry
        points are synchronous like all others, so torch work queued afterwards needs no further ordering."""
        self.wait_stream(self._torch_stream())

    def _check_out(self, tensor, numel):
        """an ``out=`` / ``com=`` tensor: contiguous, on this context's GPU, ``numel`` 8-byte words"""
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.numel() == numel and tensor.element_size() == 8
        assert tensor.device.index == self.device

    def _traj(self, packed, frame_range=None):
        """``_TrajHandle`` of a trajectory this context may read.  A device-resident ``pos`` must live on this
        context's GPU, and the context's (non-blocking) stream is ordered after torch's current stream on that
        device, i.e. after whatever produced the tensor (generation kernels, a peer copy, ``.to()``)."""
        th = _TrajHandle(packed, frame_range)
        if th.device_index is not None:
            if th.device_index != self.device:
                raise ValueError("trajectory positions live on cuda:%d but this context drives cuda:%d; use "
                                 "device=%d or copy the trajectory" % (th.device_index, self.device, th.device_index))
            self.wait_stream(self._torch_stream())
        return th

    def job_stats(self):
        """the library's record of the call that just returned on this thread"""
        with self._lock:
            return {"kernel_s_all": self._lib.amof_last_kernel_seconds(self._h, 0),
                    "kernel_s_dominant": self._lib.amof_last_kernel_seconds(self._h, 1),
                    "kernel_launches": self._lib.amof_last_kernel_launches(self._h),
                    "path": self._lib.amof_last_path(self._h).decode()}

    # (diagnostics describe the last COMPLETED call: they wait for the lane first)
    def last_kernel_seconds(self, dominant=True):
        self.drain()
        with self._lock:
            return self._lib.amof_last_kernel_seconds(self._h, 1 if dominant else 0)

    def last_path(self):
        """Kernel family that produced the last result ("rdf_tile", "rdf_cell", "cn_fast", "msd_comb", ...)."""
        self.drain()
        with self._lock:
            return self._lib.amof_last_path(self._h).decode()

    def last_kernel_launches(self):
        self.drain()
        with self._lock:
            return self._lib.amof_last_kernel_launches(self._h)

    # ------------------------------------------------------------ analyses --
    @_locked
    def rdf_accumulate(self, packed, rmax, nbins, frame_range=None, out=None):
        """ordered-pair histograms ``[S][S][nbins]`` (u64) and the volume sum.

        ``out``: optional torch CUDA int64 tensor ``[S][S][nbins]`` to
        accumulate into on the device (stays resident for an RCCL merge)."""
        th = self._traj(packed, frame_range)
        vol = ctypes.c_double(0.0)
        if out is not None:
            self._check_out(out, th.S * th.S * nbins)
            self._order_after_torch()
            fn, hist = self._lib.amof_rdf_accumulate_dev, out
        else:
            fn, hist = self._lib.amof_rdf_accumulate, np.zeros((th.S, th.S, nbins), dtype=np.uint64)
        self._check(fn(self._h, ctypes.byref(th.c), float(rmax), int(nbins), _ptr(hist), ctypes.byref(vol)))
        return hist, vol.value, th.kinds

    @_locked
    def cn_count(self, packed, cutoff, sets, frame_range=None, per_atom=False):
        th = self._traj(packed, frame_range)
        cutoff, sets = _cutoff(cutoff, th.S), _pairs(sets)
        sums = np.zeros((th.n_frames, len(sets)), dtype=np.int64)
        pa = np.zeros((th.n_frames, len(sets), th.n_atoms), dtype=np.int32) if per_atom else None
        self._check(self._lib.amof_cn_count(self._h, ctypes.byref(th.c), _ptr(cutoff), _ptr(sets), len(sets), _ptr(sums), _ptr(pa)))
        return (sums, pa) if per_atom else sums

    @_locked
    def bad_hist(self, packed, cutoff, triples, edges, frame_range=None, out=None):
        th = self._traj(packed, frame_range)
        cutoff, triples = _cutoff(cutoff, th.S), _pairs(triples)
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        nb = len(edges) - 1
        if out is not None:
            hist, nang = out
            for x, n in ((hist, len(triples) * nb), (nang, len(triples))):
                self._check_out(x, n)
            self._order_after_torch()
            fn = self._lib.amof_bad_hist_dev
        else:
            hist, nang = np.zeros((len(triples), nb), dtype=np.uint64), np.zeros(len(triples), dtype=np.uint64)
            fn = self._lib.amof_bad_hist
        self._check(fn(self._h, ctypes.byref(th.c), _ptr(cutoff), _ptr(triples), len(triples), _ptr(edges), nb, _ptr(hist),
                       _ptr(nang)))
        return hist, nang

    @_locked
    def bad_hist_by_cn(self, packed, cutoff, triples, edges, cn_max=16, frame_range=None):
        """``(hist u64 [T][cn_max+1][nb], n_angles u64 [T][cn_max+1])`` keyed by neighbour count."""
        th = self._traj(packed, frame_range)
        cutoff, triples = _cutoff(cutoff, th.S), _pairs(triples)
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        nb = len(edges) - 1
        hist = np.zeros((len(triples), cn_max + 1, nb), dtype=np.uint64)
        nang = np.zeros((len(triples), cn_max + 1), dtype=np.uint64)
        self._check(self._lib.amof_bad_hist_by_cn(self._h, ctypes.byref(th.c), _ptr(cutoff), _ptr(triples), len(triples),
                                                  _ptr(edges), nb, int(cn_max), _ptr(hist), _ptr(nang)))
        return hist, nang

    @_locked
    def msd_com(self, packed, frame_range, out):
        """centre of mass of frames ``[f0, f1)`` into rows ``f0 .. f1`` of ``out`` (torch CUDA f64 ``[F][3]``); the other
        rows are left alone (an atom-sharded run: every rank its frame share, then one sum of the zero-filled tables)."""
        th = self._traj(packed)
        self._check_out(out, 3 * th.n_frames)
        self._order_after_torch()
        self._check(self._lib.amof_msd_com_dev(self._h, ctypes.byref(th.c), int(frame_range[0]), int(frame_range[1]), _ptr(out)))
        return out

    @_locked
    def msd_window(self, packed, windows, unwrap=False, remove_com=True, atom_range=None, com=None, out=None):
        """``(sumsq [S][W] f64, kinds)``: raw sums of squared displacements.

        ``out``: optional torch CUDA f64 tensor ``[S][W]`` the sums are ADDED into on the device (stays resident for
        the ranks' all-reduce); ``com``: optional torch CUDA f64 ``[F][3]`` precomputed centre of mass (``msd_com``)."""
        th = self._traj(packed)
        windows = _i32(windows)
        a0, a1 = _span(atom_range, th.n_atoms)
        args = (self._h, ctypes.byref(th.c), _ptr(windows), len(windows), 1 if unwrap else 0, 1 if remove_com else 0, int(a0), int(a1))
        if out is not None or com is not None:
            import torch
            if out is None:
                out = torch.zeros((th.S, len(windows)), dtype=torch.float64, device=torch.device("cuda", self.device))
            self._check_out(out, th.S * len(windows))
            if com is not None:
                self._check_out(com, 3 * th.n_frames)
            self._order_after_torch()
            self._check(self._lib.amof_msd_window_dev(*args, _ptr(com), _ptr(out)))
            return out, th.kinds
        out = np.zeros((th.S, len(windows)), dtype=np.float64)
        self._check(self._lib.amof_msd_window(*args, _ptr(out)))
        return out, th.kinds

    @_locked
    def vanhove_window(self, packed, windows, dr, nbins, unwrap=False, remove_com=True, atom_range=None, com=None, out=None):
        """``(counts [S][W][nbins] u64, overflow [S][W] u64, moments [S][W][2] f64, kinds)``: the raw self Van Hove
        histograms of ``amof_vanhove_window`` (moments: sum of r^2, sum of r^4 over every sample).

        ``out``: optional ``(counts, overflow, moments)`` torch CUDA tensors (int64 ``[S][W][nbins]``, int64 ``[S][W]``, f64
        ``[S][W][2]``) the results are ADDED into on the device (they stay resident for the ranks' all-reduce); ``com``:
        optional torch CUDA f64 ``[F][3]`` precomputed centre of mass (``msd_com``)."""
        th = self._traj(packed)
        windows = _i32(windows)
        a0, a1 = _span(atom_range, th.n_atoms)
        S, W, nbins = th.S, len(windows), int(nbins)
        args = (self._h, ctypes.byref(th.c), _ptr(windows), W, 1 if unwrap else 0, 1 if remove_com else 0, int(a0), int(a1),
                float(dr), nbins)
        if out is not None or com is not None:
            import torch
            dev = torch.device("cuda", self.device)
            if out is None:
                out = (torch.zeros((S, W, nbins), dtype=torch.int64, device=dev), torch.zeros((S, W), dtype=torch.int64, device=dev),
                       torch.zeros((S, W, 2), dtype=torch.float64, device=dev))
            for x, n in zip(out, (S * W * nbins, S * W, S * W * 2)):
                self._check_out(x, n)
            if com is not None:
                self._check_out(com, 3 * th.n_frames)
            self._order_after_torch()
            self._check(self._lib.amof_vanhove_window_dev(*args, _ptr(com), *[_ptr(x) for x in out]))
            return out + (th.kinds,)
        out = (np.zeros((S, W, nbins), dtype=np.uint64), np.zeros((S, W), dtype=np.uint64), np.zeros((S, W, 2), dtype=np.float64))
        self._check(self._lib.amof_vanhove_window(*args, *[_ptr(x) for x in out]))
        return out + (th.kinds,)

    @_locked
    def vacf_window(self, packed, windows, origin_stride=1, velocities=False, remove_com=True, atom_range=None, com=None, out=None):
        """``(sums [S][W] f64, kinds)``: the raw velocity-autocorrelation sums of ``amof_vacf_window`` -- over the atoms of
        ``atom_range``, the three coordinates and the origins of every lag, of x(k) x(k + m); x: the wrapped steps of
        ``msd_window`` (Angstrom), or with ``velocities`` the trajectory's own values minus the frame's mass-weighted mean.

        ``out``: optional torch CUDA f64 tensor ``[S][W]`` the sums are ADDED into on the device (stays resident for the
        ranks' all-reduce); ``com``: optional torch CUDA f64 ``[F][3]`` precomputed centre of mass (``msd_com``)."""
        th = self._traj(packed)
        windows = _i32(windows)
        a0, a1 = _span(atom_range, th.n_atoms)
        args = (self._h, ctypes.byref(th.c), _ptr(windows), len(windows), int(origin_stride), 1 if velocities else 0,
                1 if remove_com else 0, int(a0), int(a1))
        if out is not None or com is not None:
            import torch
            if out is None:
                out = torch.zeros((th.S, len(windows)), dtype=torch.float64, device=torch.device("cuda", self.device))
            self._check_out(out, th.S * len(windows))
            if com is not None:
                self._check_out(com, 3 * th.n_frames)
            self._order_after_torch()
            self._check(self._lib.amof_vacf_window_dev(*args, _ptr(com), _ptr(out)))
            return out, th.kinds
        out = np.zeros((th.S, len(windows)), dtype=np.float64)
        self._check(self._lib.amof_vacf_window(*args, _ptr(out)))
        return out, th.kinds

    @_locked
    def vanhove_distinct(self, packed, windows, rmax, nbins, origin_stride=1, work_range=None, out=None):
        """``(hist [S][S][W][nbins] u64, kinds)``: the distinct Van Hove counts of ``amof_vanhove_distinct`` for the entries
        ``work_range`` (default: all) of the lag-major (lag, origin) work list (amof_amd.lags.work_list).

        ``out``: optional torch CUDA int64 tensor ``[S][S][W][nbins]`` the counts are ADDED into on the device (stays
        resident for an RCCL merge)."""
        th = self._traj(packed)
        windows = _i32(windows)
        W, nbins = len(windows), int(nbins)
        if work_range is None:
            work_range = _whole_work_list(th.n_frames, windows, origin_stride)
        if out is not None:
            self._check_out(out, th.S * th.S * W * nbins)
            self._order_after_torch()
            fn, hist = self._lib.amof_vanhove_distinct_dev, out
        else:
            fn, hist = self._lib.amof_vanhove_distinct, np.zeros((th.S, th.S, W, nbins), dtype=np.uint64)
        self._check(fn(self._h, ctypes.byref(th.c), _ptr(windows), W, int(origin_stride), int(work_range[0]), int(work_range[1]),
                       float(rmax), nbins, _ptr(hist)))
        return hist, th.kinds

    @_locked
    def bond_survival(self, packed, cutoff, sets, windows, origin_stride=1, atom_range=None, out=None):
        """``counts [n_sets][W][3] u64`` of ``amof_bond_survival``: per set (A, B) and lag, the bonds present at the lag's
        origins, those bonded again at origin + lag (intermittent) and those bonded at every frame in between (continuous),
        for the centres ``atom_range`` (default: all).  ``cutoff``, ``sets``: as ``cn_count``.

        ``out``: optional torch CUDA int64 tensor ``[n_sets][W][3]`` the counters are ADDED into on the device (stays
        resident for an RCCL merge)."""
        th = self._traj(packed)
        cutoff, sets, windows = _cutoff(cutoff, th.S), _pairs(sets), _i32(windows)
        a0, a1 = _span(atom_range, th.n_atoms)
        n_sets, W = len(sets), len(windows)
        args = (self._h, ctypes.byref(th.c), _ptr(cutoff), _ptr(sets), n_sets, _ptr(windows), W, int(origin_stride), int(a0), int(a1))
        if out is not None:
            self._check_out(out, n_sets * W * 3)
            self._order_after_torch()
            fn, counts = self._lib.amof_bond_survival_dev, out
        else:
            fn, counts = self._lib.amof_bond_survival, np.zeros((n_sets, W, 3), dtype=np.uint64)
        self._check(fn(*args, _ptr(counts)))
        return counts

    @_locked
    def bond_reorientation(self, packed, cutoff, sets, windows, origin_stride=1, atom_range=None, out=None):
        """``(out [n_sets][W][3] int64, scale_log2 [n_sets] int32)`` of ``amof_bond_reorientation``: per set (A, B) and lag,
        the pairs bonded at the origin and at origin + lag, and the sums over them of ``rint(P1 2^e)`` and ``rint(P2 2^e)`` of
        the cosine between the pair's vectors at both ends, for the centres ``atom_range`` (default: all); e =
        ``scale_log2[set]``.  ``cutoff``, ``sets``: as ``cn_count``.  A zero-length vector raises ``ZeroDivisionError``.

        ``out``: optional torch CUDA int64 tensor ``[n_sets][W][3]`` the sums are ADDED into on the device (stays resident
        for an RCCL merge)."""
        th = self._traj(packed)
        cutoff, sets, windows = _cutoff(cutoff, th.S), _pairs(sets), _i32(windows)
        a0, a1 = _span(atom_range, th.n_atoms)
        n_sets, W = len(sets), len(windows)
        args = (self._h, ctypes.byref(th.c), _ptr(cutoff), _ptr(sets), n_sets, _ptr(windows), W, int(origin_stride), int(a0), int(a1))
        scale = np.zeros(n_sets, dtype=np.int32)
        if out is not None:
            self._check_out(out, n_sets * W * 3)
            self._order_after_torch()
            fn, sums = self._lib.amof_bond_reorientation_dev, out
        else:
            fn, sums = self._lib.amof_bond_reorientation, np.zeros((n_sets, W, 3), dtype=np.int64)
        self._check(fn(*args, _ptr(sums), _ptr(scale)))
        return sums, scale

    @_locked
    def lindemann(self, packed, cutoff, sets, block, block_stride, nbins, ddelta, select=0, atom_range=None, per_atom=False, out=None):
        """``(sums int64 [nb][n_sets][2], hist u64 [nb][n_sets][nbins], scale_log2 int32 [n_sets] [, per_atom int64
        [nb][n_sets][N][2]])`` of ``amof_lindemann``: per block of ``block`` frames (block b starts at frame ``b *
        block_stride``) and set (A, B), the pairs bonded at the block's first frame (``select=0``) or at frame 0 (``select=1``)
        and the sum over them of ``llrint(delta 2^e)``, delta = the relative root-mean-square fluctuation of the pair's
        minimum-image distance over the block; the histogram of delta in bins of ``ddelta`` (the last takes everything above);
        per centre atom the same two numbers, for the centres ``atom_range`` (default: all).  ``cutoff``, ``sets``: as
        ``cn_count``.

        ``out``: optional pair of torch CUDA int64 tensors ``([nb][n_sets][2], [nb][n_sets][nbins])`` the sums and the
        histogram are ADDED into on the device (they stay resident for an RCCL merge); they are returned in place of the
        arrays."""
        th = self._traj(packed)
        cutoff, sets = _cutoff(cutoff, th.S), _pairs(sets)
        a0, a1 = _span(atom_range, th.n_atoms)
        block, block_stride, nbins, n_sets = int(block), int(block_stride), int(nbins), len(sets)
        if block < 2 or block > th.n_frames or block_stride < 1 or nbins < 1:
            raise ValueError("lindemann: block %d outside 2..%d frames, block_stride %d < 1 or nbins %d < 1"
                             % (block, th.n_frames, block_stride, nbins))
        nb = (th.n_frames - block) // block_stride + 1
        scale = np.zeros(n_sets, dtype=np.int32)
        pa = np.zeros((nb, n_sets, th.n_atoms, 2), dtype=np.int64) if per_atom else None
        if out is not None:
            sums, hist = out
            self._check_out(sums, nb * n_sets * 2)
            self._check_out(hist, nb * n_sets * nbins)
            self._order_after_torch()
            fn = self._lib.amof_lindemann_dev
        else:
            sums = np.zeros((nb, n_sets, 2), dtype=np.int64)
            hist = np.zeros((nb, n_sets, nbins), dtype=np.uint64)
            fn = self._lib.amof_lindemann
        self._check(fn(self._h, ctypes.byref(th.c), _ptr(cutoff), _ptr(sets), n_sets, block, block_stride, int(select), nbins,
                       float(ddelta), int(a0), int(a1), _ptr(sums), _ptr(hist), _ptr(pa), _ptr(scale)))
        return (sums, hist, scale, pa) if per_atom else (sums, hist, scale)

    @_locked
    def bond_order(self, packed, cutoff, sets, l, nbins, nbins_tet, frame_range=None, per_atom=False, out=None):
        """``(hist u64 [n_sets][n_l][nbins], hist_tet u64 [n_sets][nbins_tet], frame_sums int64 [F][n_sets][4 + n_l + 1]
        [, per_atom int64 [F][n_sets][N][2 + n_l]])`` of ``amof_bond_order``: the Steinhardt q_l (``l``: up to four values in
        1 .. 12) and the tetrahedral order parameter of every centre of the sets (A, B), binned over the frames of
        ``frame_range``; per frame and set the sums of n, of the centres with n >= 1 and n == 4, of n (n - 1) / 2, of
        ``llrint(q_l 2^30)`` per l and of ``llrint(q_tet 2^30)``; per atom ``(n, T_l ..., U)`` (include/amof_hip.h).
        ``cutoff``, ``sets``: as ``cn_count``.  A zero-length bond vector raises ``ZeroDivisionError``.

        ``out``: optional pair of torch CUDA int64 tensors ``([n_sets][n_l][nbins], [n_sets][nbins_tet])`` the histograms
        are ADDED into on the device (they stay resident for an RCCL merge); they are returned in place of the arrays."""
        th = self._traj(packed, frame_range)
        cutoff, sets = _cutoff(cutoff, th.S), _pairs(sets)
        l = _i32(l).reshape(-1)
        nbins, nbins_tet = int(nbins), int(nbins_tet)
        sums = np.zeros((th.n_frames, len(sets), 4 + len(l) + 1), dtype=np.int64)
        pa = np.zeros((th.n_frames, len(sets), th.n_atoms, 2 + len(l)), dtype=np.int64) if per_atom else None
        if out is not None:
            hist, hist_tet = out
            self._check_out(hist, len(sets) * len(l) * nbins)
            self._check_out(hist_tet, len(sets) * nbins_tet)
            self._order_after_torch()
            fn = self._lib.amof_bond_order_dev
        else:
            hist = np.zeros((len(sets), len(l), nbins), dtype=np.uint64)
            hist_tet = np.zeros((len(sets), nbins_tet), dtype=np.uint64)
            fn = self._lib.amof_bond_order
        self._check(fn(self._h, ctypes.byref(th.c), _ptr(cutoff), _ptr(sets), len(sets), _ptr(l), len(l), nbins, nbins_tet,
                       _ptr(hist), _ptr(hist_tet), _ptr(sums), _ptr(pa)))
        return (hist, hist_tet, sums, pa) if per_atom else (hist, hist_tet, sums)

    @_locked
    def dihedral_hist(self, packed, cutoff, chains, edges, frame_range=None, out=None):
        """``(hist u64 [T][nb], n_dihedrals u64 [T], n_undefined u64 [T], frame_sums int64 [F][T][3])`` of
        ``amof_dihedral_hist``: the folded torsion angle (0 .. 180 degrees) of every chain a-b-c-d of bonded atoms whose
        species match a pattern of ``chains`` (``[T][4]`` species indices, -1: any; a chain counts once per pattern, in
        whichever direction it matches), binned with ``edges`` as ``bad_hist`` bins its angles; per frame and pattern the
        defined chains, the undefined ones (a bond angle within about 1e-6 rad of straight) and the sum of
        ``llrint(cos(phi) 2^40)`` (include/amof_hip.h).  ``cutoff``: the symmetric matrix ``[S][S]`` as ``ring_stats``'.

        ``out``: optional triple of torch CUDA int64 tensors ``([T][nb], [T], [T])`` the counts are ADDED into on the
        device (they stay resident for an RCCL merge); they are returned in place of the arrays."""
        th = self._traj(packed, frame_range)
        cutoff = _cutoff(cutoff, th.S)
        chains = _i32(chains).reshape(-1, 4)
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        T, nb = len(chains), len(edges) - 1
        sums = np.zeros((th.n_frames, T, 3), dtype=np.int64)
        if out is not None:
            hist, n_def, n_undef = out
            for x, n in ((hist, T * nb), (n_def, T), (n_undef, T)):
                self._check_out(x, n)
            self._order_after_torch()
            fn = self._lib.amof_dihedral_hist_dev
        else:
            hist = np.zeros((T, nb), dtype=np.uint64)
            n_def, n_undef = np.zeros(T, dtype=np.uint64), np.zeros(T, dtype=np.uint64)
            fn = self._lib.amof_dihedral_hist
        self._check(fn(self._h, ctypes.byref(th.c), _ptr(cutoff), _ptr(chains), T, _ptr(edges), nb, _ptr(hist), _ptr(n_def),
                       _ptr(n_undef), _ptr(sums)))
        return hist, n_def, n_undef, sums

    @_locked
    def ring_stats(self, packed, cutoff, max_size=32, frame_range=None, per_atom=False, neighbours=False):
        """``(counts int64 [F][4][max_size + 1], truncated int64 [F] [, per_atom u32 [F][N][max_size + 1]] [, neighbours int32
        [F][N][17]])`` of ``amof_ring_stats``: the primitive rings of up to ``max_size`` (3 .. 32) nodes of the bond graph of
        every frame of ``frame_range``.  ``cutoff``: the symmetric matrix ``[S][S]`` (``atom.cutoff_matrix`` of a sorted-pair
        dictionary; 0: never bonded).  Per frame and size n: the sum over the atoms of the rings through them (n times the
        number of rings), the atoms on such a ring, the atoms whose smallest / largest ring it is; ``truncated``: the sources
        whose search was cut off at depth ``max_size // 2`` (include/amof_hip.h)."""
        th = self._traj(packed, frame_range)
        cutoff = _cutoff(cutoff, th.S)
        max_size = int(max_size)
        W = max(max_size, 0) + 1
        counts = np.zeros((th.n_frames, 4, W), dtype=np.int64)
        truncated = np.zeros(th.n_frames, dtype=np.int64)
        pa = np.zeros((th.n_frames, th.n_atoms, W), dtype=np.uint32) if per_atom else None
        nb = np.zeros((th.n_frames, th.n_atoms, 17), dtype=np.int32) if neighbours else None
        self._check(self._lib.amof_ring_stats(self._h, ctypes.byref(th.c), _ptr(cutoff), max_size, _ptr(counts), _ptr(truncated),
                                              _ptr(pa), _ptr(nb)))
        return (counts, truncated) + ((pa,) if per_atom else ()) + ((nb,) if neighbours else ())

    def ring_search_stats(self):
        """``{"sources", "candidates", "closed"}`` of the last ``ring_stats``: the sources searched, their candidates and the
        candidates that closed at least one ring (``amof_ring_search_stats``)"""
        self.drain()
        out = np.zeros(3, dtype=np.float64)
        with self._lock:
            self._check(self._lib.amof_ring_search_stats(self._h, _ptr(out)))
        return dict(zip(("sources", "candidates", "closed"), out.tolist()))

    @_locked
    def fragment_stats(self, packed, cutoff, link=None, ref_label=None, kinds=None, max_size=64, frame_range=None, per_atom=False,
                       com=False):
        """``(summary int64 [F][5], size_hist int64 [F][max_size + 2], census int64 [F][K + 1] [, links int64 [F][K + 1][K + 1]]
        [, label int32 [F][N], shift int32 [F][N][3]] [, com f64 [F][M][3], frag_mass f64 [M]])`` of ``amof_fragment_stats``: the
        connected components of the bond graph of ``cutoff`` (``[S][S]``, symmetric, 0: never bonded) in every frame of
        ``frame_range``.  ``summary``: fragments, atoms of the largest, winding fragments, atoms whose label differs from
        ``ref_label`` (-1 without it), link bonds inside one fragment.  ``link`` (a second matrix, no pair in common with
        ``cutoff``) adds ``links``: ordered link bonds between fragments by the kinds of the two; ``kinds [K][S]``: the species-count
        vectors the census looks for; ``per_atom`` adds the labels and shifts; ``com`` (needs ``ref_label``) the centres of mass of
        the reference fragments -- NaN rows where the frame's partition differs or the fragment winds -- and their masses
        (include/amof_hip.h)."""
        th = self._traj(packed, frame_range)
        cutoff = _cutoff(cutoff, th.S)
        link = None if link is None else _cutoff(link, th.S)
        kinds = np.zeros((0, th.S), dtype=np.int32) if kinds is None else _i32(kinds).reshape(-1, th.S)
        K, max_size = len(kinds), int(max_size)
        F, N = th.n_frames, th.n_atoms
        M = 0
        if ref_label is not None:
            ref_label = _i32(ref_label).reshape(N)
            M = int((ref_label == np.arange(N)).sum())
        elif com:
            raise ValueError("com needs ref_label")
        summary = np.zeros((F, 5), dtype=np.int64)
        hist = np.zeros((F, max(max_size, 0) + 2), dtype=np.int64)
        census = np.zeros((F, K + 1), dtype=np.int64)
        links = np.zeros((F, K + 1, K + 1), dtype=np.int64) if link is not None else None
        label = np.zeros((F, N), dtype=np.int32) if per_atom else None
        shift = np.zeros((F, N, 3), dtype=np.int32) if per_atom else None
        centres = np.zeros((F, M, 3), dtype=np.float64) if com else None
        mass = np.zeros(M, dtype=np.float64) if com else None
        self._check(self._lib.amof_fragment_stats(self._h, ctypes.byref(th.c), _ptr(cutoff), _ptr(link), _ptr(ref_label),
                                                  _ptr(kinds) if K else None, K, max_size, _ptr(summary), _ptr(hist), _ptr(census),
                                                  _ptr(links), _ptr(label), _ptr(shift), _ptr(centres), _ptr(mass), M))
        return ((summary, hist, census) + ((links,) if link is not None else ()) + ((label, shift) if per_atom else ())
                + ((centres, mass) if com else ()))

    def fragment_round_stats(self):
        """``{"frames", "rounds", "max_rounds"}`` of the last ``fragment_stats``: the frames labelled, the labelling rounds summed
        over them and the most rounds of one frame (``amof_fragment_round_stats``)"""
        self.drain()
        out = np.zeros(3, dtype=np.float64)
        with self._lock:
            self._check(self._lib.amof_fragment_round_stats(self._h, _ptr(out)))
        return dict(zip(("frames", "rounds", "max_rounds"), out.tolist()))

    def _pore_atoms(self, packed, radii, grid, dr, dmax, thresholds, frame_range, dirs=None, **flags):
        """the four calls that take atoms -- ``amof_pore_field``, ``amof_pore_access`` (``labelled``), ``amof_pore_psd``
        (``psd``), ``amof_pore_surface`` (``surface``, with ``dirs [M][3]``) -- as a ``PoreResult``; ``flags``: ``pore_names``'"""
        th = self._traj(packed, frame_range)
        radii = np.ascontiguousarray(radii, dtype=np.float64).reshape(th.S)
        grid = _i32(grid).reshape(3)
        thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        dr, dmax = float(dr), float(dmax)
        if not (np.isfinite(dr) and dr > 0 and np.isfinite(dmax) and dmax > 0):
            raise ValueError("dr and dmax must be finite and > 0")
        nbins = int(np.rint(dmax / dr))
        if nbins < 1 or (grid < 1).any() or int(grid[0]) * int(grid[1]) * int(grid[2]) > 2 ** 31 - 1:
            raise ValueError("dmax / dr rounds to no bin, or a grid that is not 1 .. 2^31 - 1 points")
        shape = tuple(int(x) for x in grid)
        _label_cap(flags.get("labels"), len(thr), shape[0] * shape[1] * shape[2])
        M = 0
        if flags.get("surface"):
            dirs = np.ascontiguousarray(dirs, dtype=np.float64)
            if dirs.ndim != 2 or dirs.shape[1] != 3:
                raise ValueError("dirs must be [M][3]")
            M = dirs.shape[0]
            if flags.get("per_point") and len(thr) * int(th.n_atoms) * M > 2 ** 32:
                raise AmofError(AMOF_ECAPACITY, "samples of %d thresholds x %d atoms x %d directions exceed the 4 GiB a frame may take"
                                % (len(thr), int(th.n_atoms), M))
        r = _pore_alloc(pore_names(**flags), th.n_frames, len(thr), nbins, shape, th.S, int(th.n_atoms), M)
        head = (self._h, ctypes.byref(th.c), _ptr(radii), _ptr(grid), dr, dmax, _ptr(thr), len(thr))
        rows = (_ptr(r.hist), _ptr(r.counts), _ptr(r.vmax), _ptr(r.argmax))
        more = (_ptr(r.access), _ptr(r.free_sphere), _ptr(r.field), _ptr(r.labels))
        if flags.get("surface"):
            rc = self._lib.amof_pore_surface(*head, int(bool(flags.get("accessibility"))), int(bool(flags.get("free_sphere"))), *rows, *more,
                                             _ptr(r.psd_hist), _ptr(r.po_counts), _ptr(r.po_access), _ptr(r.cover),
                                             int(bool(flags.get("psd"))), _ptr(dirs), M, _ptr(r.exposed), _ptr(r.exposed_access),
                                             _ptr(r.samples))
        elif flags.get("psd"):
            rc = self._lib.amof_pore_psd(*head, int(bool(flags.get("accessibility"))), int(bool(flags.get("free_sphere"))), *rows, *more,
                                         _ptr(r.psd_hist), _ptr(r.po_counts), _ptr(r.po_access), _ptr(r.cover))
        elif flags.get("labelled"):
            rc = self._lib.amof_pore_access(*head, int(bool(flags.get("free_sphere"))), *rows, *more)
        else:
            rc = self._lib.amof_pore_field(*head, *rows, _ptr(r.field))
        self._check(rc)
        return r

    def _pore_given_field(self, field, pbc, thresholds):
        """what the two calls on a supplied field ``[F][nx][ny][nz]`` share: ``(field, F, shape, grid, periodic, thresholds)``"""
        field = np.ascontiguousarray(field, dtype=np.float64)
        if field.ndim != 4:
            raise ValueError("field must be [F][nx][ny][nz]")
        F, shape = field.shape[0], tuple(int(x) for x in field.shape[1:])
        if min(shape) < 1 or shape[0] * shape[1] * shape[2] > 2 ** 31 - 1:
            raise ValueError("a grid that is not 1 .. 2^31 - 1 points")
        per = _i32([1 if x else 0 for x in pbc]).reshape(3)
        return field, F, shape, _i32(shape), per, np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)

    @_locked
    def pore_field(self, packed, radii, grid, dr, dmax, thresholds=(), frame_range=None, per_point=False):
        """``(hist u64 [F][nbins + 2], counts int64 [F][n_t], vmax f64 [F], argmax int64 [F][, field f64 [F][nx][ny][nz]])``
        of ``amof_pore_field`` over the frames of ``frame_range``: per frame the histogram of the distance ``v`` of every
        point of the grid ``grid = (nx, ny, nz)`` over the cell to the nearest atomic surface (``radii [S]`` in Angstrom,
        in ``kinds`` order; row: inside an atom, ``nbins = rint(dmax / dr)`` bins of ``[0, dmax)``, overflow), the points
        with ``v >= thresholds[t]``, the largest ``v`` and its linear grid index; ``per_point``: the field itself
        (include/amof_hip.h)."""
        r = self._pore_atoms(packed, radii, grid, dr, dmax, thresholds, frame_range, per_point=bool(per_point))
        return tuple(x for x in r if x is not None)

    @_locked
    def pore_access(self, packed, radii, grid, dr, dmax, thresholds=(), frame_range=None, per_point=False, free_sphere=False,
                    labels=False):
        """``pore_field``'s results -- the same bits -- followed by ``access int64 [F][n_t][4]`` (accessible points, channels,
        pockets, largest channel dimension of the void ``v >= thresholds[t]``), then, each only if asked for, ``free_sphere
        f64 [F][2]`` (t* and Dif / 2; +inf: not resolved below dmax), ``field f64 [F][nx][ny][nz]`` (``per_point``) and
        ``labels int32 [F][n_t][nx][ny][nz]`` (the smallest linear index of a point's periodic component, -1 outside the
        void): ``amof_pore_access`` (include/amof_hip.h has the definitions)."""
        r = self._pore_atoms(packed, radii, grid, dr, dmax, thresholds, frame_range, per_point=bool(per_point), labelled=True,
                             free_sphere=bool(free_sphere), labels=bool(labels))
        return tuple(x for x in r if x is not None)

    @_locked
    def pore_access_field(self, field, pbc=(True, True, True), thresholds=(), free_sphere=False, labels=False):
        """``(access int64 [F][n_t][4], free_sphere f64 [F][2] or None, labels int32 [F][n_t][nx][ny][nz] or None)`` of
        ``amof_pore_access_field``: the periodic components of ``{field >= thresholds[t]}`` of a field ``[F][nx][ny][nz]`` the
        caller supplies (finite; ``pbc``: which grid axes are periodic) -- ``Pore(per_point=True).field`` or any other.
        Here t* (``free_sphere[:, 0]``) is the largest field value of any sign whose void has a channel, -inf without one."""
        field, F, shape, grid, per, thr = self._pore_given_field(field, pbc, thresholds)
        _label_cap(labels, len(thr), shape[0] * shape[1] * shape[2])
        r = _pore_alloc(("access",) + ("free_sphere",) * bool(free_sphere) + ("labels",) * bool(labels), F, len(thr), 0, shape)
        self._check(self._lib.amof_pore_access_field(self._h, _ptr(field), F, _ptr(grid), _ptr(per), _ptr(thr), len(thr), int(bool(free_sphere)),
                                                     _ptr(r.access), _ptr(r.free_sphere), _ptr(r.labels)))
        return r.access, r.free_sphere, r.labels

    @_locked
    def pore_psd(self, packed, radii, grid, dr, dmax, thresholds=(), frame_range=None, per_point=False, accessibility=False,
                 free_sphere=False, labels=False):
        """``amof_pore_psd``: the results of ``pore_field`` -- of ``pore_access`` with ``accessibility`` or ``free_sphere`` --
        with the same optional outputs in the same order, the same bits, followed by ``psd_hist u64 [F][nbins + 2]`` (the
        histogram of the covering radius ``w``: covered by no sphere, the bins of ``[0, dmax)``, ``w >= dmax``), ``po_counts
        int64 [F][n_t]`` (points with ``w >= thresholds[t]``: the probe-occupiable volume), with ``accessibility`` ``po_access
        int64 [F][n_t]`` (points covered from a channel of the void ``v >= thresholds[t]``) and with ``per_point`` ``cover f64
        [F][nx][ny][nz]`` (``w`` itself).  include/amof_hip.h has the definitions."""
        labelled = bool(accessibility or free_sphere)
        r = self._pore_atoms(packed, radii, grid, dr, dmax, thresholds, frame_range, per_point=bool(per_point), labelled=labelled,
                             free_sphere=bool(free_sphere), labels=bool(labels) and labelled, psd=True, accessibility=bool(accessibility))
        return tuple(x for x in r if x is not None)

    @_locked
    def pore_psd_field(self, field, cells, pbc, dr, dmax, thresholds=(), accessibility=False, per_point=False):
        """``(psd_hist u64 [F][nbins + 2], po_counts int64 [F][n_t], po_access int64 [F][n_t] or None, cover f64
        [F][nx][ny][nz] or None)`` of ``amof_pore_psd_field``: the covering radius of a field ``[F][nx][ny][nz]`` the caller
        supplies (finite; no value above half the smallest periodic perpendicular height of its frame's cell), ``cells
        [F][3][3]`` or one cell for all frames, ``pbc``: which grid axes are periodic."""
        field, F, shape, grid, per, thr = self._pore_given_field(field, pbc, thresholds)
        cells = np.asarray(cells, dtype=np.float64).reshape(-1, 9)
        if cells.shape[0] == 1:
            cells = np.broadcast_to(cells, (F, 9))
        if cells.shape[0] != F:
            raise ValueError("cells must be one cell or one per frame")
        cells = np.ascontiguousarray(cells)
        dr, dmax = float(dr), float(dmax)
        if not (np.isfinite(dr) and dr > 0 and np.isfinite(dmax) and dmax > 0) or int(np.rint(dmax / dr)) < 1:
            raise ValueError("dr and dmax must be finite and > 0, dmax at least one bin")
        names = ("psd_hist", "po_counts") + ("po_access",) * bool(accessibility) + ("cover",) * bool(per_point)
        r = _pore_alloc(names, F, len(thr), int(np.rint(dmax / dr)), shape)
        self._check(self._lib.amof_pore_psd_field(self._h, _ptr(field), _ptr(cells), F, _ptr(grid), _ptr(per), dr, dmax, _ptr(thr), len(thr),
                                                  int(bool(accessibility)), _ptr(r.psd_hist), _ptr(r.po_counts), _ptr(r.po_access), _ptr(r.cover)))
        return r.psd_hist, r.po_counts, r.po_access, r.cover

    @_locked
    def pore_surface(self, packed, radii, grid, dr, dmax, thresholds=(), dirs=None, frame_range=None, per_point=False,
                     accessibility=False, free_sphere=False, labels=False, psd=False):
        """``amof_pore_surface``: the results of ``pore_field`` -- of ``pore_access`` with ``accessibility`` or ``free_sphere``, of
        ``pore_psd`` with ``psd`` -- with the same optional outputs in the same order, the same bits, followed by ``exposed int64
        [F][n_t][S]`` (per species, the samples ``r_j + (R_j + rp) dirs[m]`` that lie in no other atom's sphere of radius
        ``R_k + rp``), with ``accessibility`` ``exposed_access int64 [F][n_t][S]`` (of those, the samples with one of their 8
        surrounding grid points in a channel of the void ``v >= rp``) and with ``per_point`` ``samples uint8 [F][n_t][N][M]`` (0
        buried, 1 exposed, 2 exposed and accessible).  ``dirs [M][3]``: unit vectors (``amof_amd.pore.sphere_points``);
        ``thresholds``: probe radii >= 0.  include/amof_hip.h has the definitions."""
        labelled = bool(accessibility or free_sphere)
        r = self._pore_atoms(packed, radii, grid, dr, dmax, thresholds, frame_range, dirs=dirs, per_point=bool(per_point),
                             labelled=labelled, free_sphere=bool(free_sphere), labels=bool(labels) and labelled, psd=bool(psd),
                             accessibility=bool(accessibility), surface=True)
        return tuple(x for x in r if x is not None)

    def pore_surface_stats(self):
        """``{"atoms", "records", "samples", "redecisions", "early_exits"}`` summed over the launches of the last ``pore_surface``
        that stayed on the "pore_surface_list" path (``amof_pore_surface_stats``)"""
        self.drain()
        out = np.zeros(5, dtype=np.float64)
        with self._lock:
            self._check(self._lib.amof_pore_surface_stats(self._h, _ptr(out)))
        return dict(zip(("atoms", "records", "samples", "redecisions", "early_exits"), out.tolist()))

    def pore_cover_stats(self):
        """``{"bricks", "source_bricks", "records"}`` summed over the full passes of the last ``pore_psd`` / ``pore_psd_field`` on
        the "pore_cover_brick" path (``amof_pore_cover_stats``): divide by ``bricks`` for the means per destination brick"""
        self.drain()
        out = np.zeros(3, dtype=np.float64)
        with self._lock:
            self._check(self._lib.amof_pore_cover_stats(self._h, _ptr(out)))
        return dict(zip(("bricks", "source_bricks", "records"), out.tolist()))

    @_locked
    def sq_accumulate(self, packed, hkl, dq, nbins, frame_range=None, frame_stride=1, recip=None, out=None):
        """``(counts [nbins] u64, sums [P][nbins] f64, beyond, kinds)`` of ``amof_sq_accumulate``: the vectors ``hkl``
        (int ``[K][3]``) of the frames ``frame_range[0], + frame_stride, ... < frame_range[1]``, P = S(S+1)/2 species
        pairs a <= b in ``kinds`` order.  ``recip``: ``[n_cells][3][3]`` (default ``reciprocal(packed.cell)``).

        ``out``: optional ``(counts, sums)`` torch CUDA int64 tensors (``[nbins + 1]``: the counts, then beyond;
        ``[P][nbins]``: fixed-point sums) the results are ADDED into on the device; returns ``(counts, sums, scale_log2,
        kinds)`` then, with sums = ``sums * 2**-scale_log2[p]``."""
        th = self._traj(packed)
        hkl, recip = _hkl(hkl), _recip(packed, recip)
        f0, f1 = _span(frame_range, th.n_frames)
        S, nbins = th.S, int(nbins)
        P = S * (S + 1) // 2
        args = (self._h, ctypes.byref(th.c), _ptr(recip), _ptr(hkl), len(hkl), int(f0), int(f1), int(frame_stride), float(dq), nbins)
        if out is not None:
            counts, sums = out
            self._check_out(counts, nbins + 1)
            self._check_out(sums, P * nbins)
            scale = np.zeros(P, dtype=np.int32)
            self._order_after_torch()
            self._check(self._lib.amof_sq_accumulate_dev(*args, _ptr(counts), _ptr(sums), ctypes.c_void_p(counts.data_ptr() + 8 * nbins),
                                                         _ptr(scale)))
            return counts, sums, scale, th.kinds
        counts = np.zeros(nbins, dtype=np.uint64)
        sums = np.zeros((P, nbins), dtype=np.float64)
        beyond = np.zeros(1, dtype=np.uint64)
        self._check(self._lib.amof_sq_accumulate(*args, _ptr(counts), _ptr(sums), _ptr(beyond)))
        return counts, sums, int(beyond[0]), th.kinds

    def _lag_args(self, th, packed, hkl, windows, dq, nbins, origin_stride, work_range, recip, extra=()):
        """what ``amof_isf_accumulate`` and ``amof_current_accumulate`` take alike: ``(W, args, held)`` -- args the argument
        tuple up to ``nbins``, ``extra`` behind the trajectory; held: the arrays args points into (hkl, windows, recip)"""
        hkl, windows, recip = _hkl(hkl), _i32(windows), _recip(packed, recip)
        if work_range is None:
            work_range = _whole_work_list(th.n_frames, windows, origin_stride)
        args = (self._h, ctypes.byref(th.c)) + tuple(extra) + (
            _ptr(recip), _ptr(hkl), len(hkl), _ptr(windows), len(windows), int(origin_stride), int(work_range[0]),
            int(work_range[1]), float(dq), int(nbins))
        return len(windows), args, (hkl, windows, recip)

    @_locked
    def isf_accumulate(self, packed, hkl, windows, dq, nbins, origin_stride=1, work_range=None, self_part=True, recip=None,
                       out=None):
        """``(counts [W][nbins] u64, coh [S][S][W][nbins] f64, self [S][W][nbins] f64 or None, beyond [W] u64, kinds)`` of
        ``amof_isf_accumulate``: the vectors ``hkl`` (int ``[K][3]``) correlated over the entries ``work_range`` (default:
        all) of the lag-major (lag, origin) work list (amof_amd.lags.work_list); ``coh[a][c]``: species a at the
        origin, c at the origin + lag.  ``recip``: ``[n_cells][3][3]`` (default ``reciprocal(packed.cell)``).

        ``out``: optional torch CUDA int64 tensor of ``isf_layout(S, W, nbins, self_part)["size"]`` words (counts, beyond,
        fixed-point coh, fixed-point self) the results are ADDED into on the device; returns ``(out, scale_log2, kinds)``
        then, with coh[a][c] = ``coh * 2**-scale_log2[p]``, p the unordered pair of ``sq_accumulate``'s order."""
        th = self._traj(packed)
        W, args, held = self._lag_args(th, packed, hkl, windows, dq, nbins, origin_stride, work_range, recip)
        S, nbins = th.S, int(nbins)
        if out is not None:
            lay = isf_layout(S, W, nbins, self_part)
            self._check_out(out, lay["size"])
            scale = np.zeros(S * (S + 1) // 2, dtype=np.int32)
            part = [ctypes.c_void_p(out.data_ptr() + 8 * lay[k]) for k in ("counts", "coh", "self", "beyond")]
            self._order_after_torch()
            self._check(self._lib.amof_isf_accumulate_dev(*args, part[0], part[1], part[2] if self_part else None, part[3],
                                                          _ptr(scale)))
            return out, scale, th.kinds
        counts = np.zeros((W, nbins), dtype=np.uint64)
        coh = np.zeros((S, S, W, nbins), dtype=np.float64)
        selfs = np.zeros((S, W, nbins), dtype=np.float64) if self_part else None
        beyond = np.zeros(W, dtype=np.uint64)
        self._check(self._lib.amof_isf_accumulate(*args, _ptr(counts), _ptr(coh), _ptr(selfs), _ptr(beyond)))
        return counts, coh, selfs, beyond, th.kinds

    def _velocity_traj(self, packed, velocities):
        """``(handle or None, pointer or None)`` of the velocity trajectory of ``amof_current_*``: the same frames and atoms
        as ``packed``; only its array is read"""
        if velocities is None:
            return None, None
        if velocities.n_frames != packed.n_frames or velocities.n_atoms != packed.n_atoms:
            raise ValueError("velocities: other frames or atoms than the positions")
        vh = self._traj(velocities)
        return vh, ctypes.byref(vh.c)

    @_locked
    def current_modes(self, packed, hkl, frame=1, velocities=None, remove_com=True):
        """``(j [K][S][3] complex128, kinds)``: j_a(k) of the sample on frame ``frame`` >= 1 for the vectors ``hkl``
        (``amof_current_modes``), in Angstrom per frame (``velocities``, a PackedTrajectory of velocities: its units)"""
        th = self._traj(packed)
        vh, vp = self._velocity_traj(packed, velocities)
        hkl = _hkl(hkl)
        j = np.zeros((len(hkl), th.S, 3, 2), dtype=np.float64)
        self._check(self._lib.amof_current_modes(self._h, ctypes.byref(th.c), vp, int(frame), 1 if remove_com else 0, _ptr(hkl),
                                                 len(hkl), _ptr(j)))
        return j[..., 0] + 1j * j[..., 1], th.kinds

    @_locked
    def current_accumulate(self, packed, hkl, windows, dq, nbins, origin_stride=1, work_range=None, velocities=None,
                           remove_com=True, recip=None, out=None):
        """``(counts [W][nbins] u64, long [S][S][W][nbins] f64, trans [S][S][W][nbins] f64, beyond [W] u64, scale_log2 [P],
        vmax, kinds)`` of ``amof_current_accumulate``: the current correlations of the vectors ``hkl`` over the entries
        ``work_range`` (default: all) of the lag-major (lag, origin) work list; ``[a][c]``: species a at the origin, c at the
        origin + lag.  ``velocities``: a PackedTrajectory of velocities for the same frames (default: finite differences).

        ``out``: optional torch CUDA int64 tensor of ``current_layout(S, W, nbins)["size"]`` words (counts, beyond, fixed-point
        long and trans) the results are ADDED into on the device; returns ``(out, scale_log2, vmax, kinds)`` then."""
        th = self._traj(packed)
        vh, vp = self._velocity_traj(packed, velocities)
        W, args, held = self._lag_args(th, packed, hkl, windows, dq, nbins, origin_stride, work_range, recip,
                                       extra=(vp, 1 if remove_com else 0))
        S, nbins = th.S, int(nbins)
        scale = np.zeros(S * (S + 1) // 2, dtype=np.int32)
        vmax = np.zeros(1, dtype=np.float64)
        if out is not None:
            lay = current_layout(S, W, nbins)
            self._check_out(out, lay["size"])
            part = [ctypes.c_void_p(out.data_ptr() + 8 * lay[k]) for k in ("counts", "long", "trans", "beyond")]
            self._order_after_torch()
            self._check(self._lib.amof_current_accumulate_dev(*args, part[0], part[1], part[2], part[3], _ptr(scale), _ptr(vmax)))
            return out, scale, float(vmax[0]), th.kinds
        counts = np.zeros((W, nbins), dtype=np.uint64)
        lng = np.zeros((S, S, W, nbins), dtype=np.float64)
        trn = np.zeros((S, S, W, nbins), dtype=np.float64)
        beyond = np.zeros(W, dtype=np.uint64)
        self._check(self._lib.amof_current_accumulate(*args, _ptr(counts), _ptr(lng), _ptr(trn), _ptr(beyond), _ptr(scale), _ptr(vmax)))
        return counts, lng, trn, beyond, scale, float(vmax[0]), th.kinds

    def last_current_stage_seconds(self):
        """``{"records", "table", "corr"}``: kernel seconds of the stages of the last ``current_accumulate``
        (amof_last_kernel_seconds 2 .. 4)"""
        self.drain()
        with self._lock:
            return {name: self._lib.amof_last_kernel_seconds(self._h, 2 + i) for i, name in enumerate(("records", "table", "corr"))}

    def last_stage_seconds(self, pore=False):
        """``{"rho", "corr", "self"}``: kernel seconds of the stages of the last ``isf_accumulate`` (amof_last_kernel_seconds
        2 .. 4; negative: the last call was not one).  After ``bond_survival`` the same three slots hold the bond lists, the
        bit series and the correlations; after ``bond_reorientation`` the bond lists, the bit series, and the vector table
        with the reorientation sums; after ``lindemann`` the pair lists, the moments and the reduction; after ``bond_order``
        the list stage and the order kernels, after ``dihedral_hist`` the
        list stage (or the adjacency rows) and the dihedral kernels (the third is 0).  After the Pore
        calls the three slots hold the cell sort, the field kernels and the labelling; ``pore=True`` adds ``"cover"``, the covering
        stage, and ``"surface"``, the surface stage (amof_last_kernel_seconds 5 and 6)."""
        self.drain()
        names = ("rho", "corr", "self") + (("cover", "surface") if pore else ())
        with self._lock:
            return {name: self._lib.amof_last_kernel_seconds(self._h, 2 + i) for i, name in enumerate(names)}

    @_locked
    def sq_modes(self, packed, hkl, frame=0):
        """``(rho [K][S] complex128, kinds)``: rho_a(k) of one frame for the vectors ``hkl`` (``amof_sq_modes``)"""
        th = self._traj(packed)
        hkl = _hkl(hkl)
        rho = np.zeros((len(hkl), th.S, 2), dtype=np.float64)
        self._check(self._lib.amof_sq_modes(self._h, ctypes.byref(th.c), int(frame), _ptr(hkl), len(hkl), _ptr(rho)))
        return rho[:, :, 0] + 1j * rho[:, :, 1], th.kinds

    @_locked
    def msd_shard_begin(self, packed, windows, atom_range, csum):
        """first half of an atom-sharded window MSD (``amof_msd_shard_begin``): ``csum`` (torch CUDA f64 ``[F][3]``) receives
        the mass-weighted coordinate sums of the atoms ``[a0, a1)`` per frame -- the caller all-reduces it over the ranks.
        Raises :class:`Unsupported` where the fused form does not apply (the caller then takes ``msd_com`` + ``msd_window``)."""
        th = self._traj(packed)
        windows = _i32(windows)
        self._check_out(csum, 3 * th.n_frames)
        self._order_after_torch()
        self._check(self._lib.amof_msd_shard_begin(self._h, ctypes.byref(th.c), _ptr(windows), len(windows), int(atom_range[0]),
                                                   int(atom_range[1]), _ptr(csum)))
        return csum

    @_locked
    def msd_shard_finish(self, packed, windows, atom_range, csum, out):
        """second half (``amof_msd_shard_finish``, the next call on this context after its begin): adds the sums of the
        atoms ``[a0, a1)`` into ``out`` (torch CUDA f64 ``[S][W]``); ``csum`` = the table summed over the ranks"""
        th = self._traj(packed)
        windows = _i32(windows)
        self._check_out(csum, 3 * th.n_frames)
        self._check_out(out, th.S * len(windows))
        self._order_after_torch()
        self._check(self._lib.amof_msd_shard_finish(self._h, ctypes.byref(th.c), _ptr(windows), len(windows), int(atom_range[0]),
                                                    int(atom_range[1]), _ptr(csum), _ptr(out)))
        return out, th.kinds

    @_locked
    def msd_direct(self, packed):
        """``(msd [F][S+1] f64, kinds)``: column 0 = all atoms, then one per species."""
        th = self._traj(packed)
        out = np.zeros((th.n_frames, th.S + 1), dtype=np.float64)
        self._check(self._lib.amof_msd_direct(self._h, ctypes.byref(th.c), _ptr(out)))
        return out, th.kinds


def merge_results(results, rules):
    """One result from those of the shards of a call (the devices of a ``MultiContext``, the batches of a stream): per
    returned element ``"sum"``, ``"cat"`` (concatenate along axis 0) or ``"first"``; one rule for a bare result."""
    if isinstance(rules, str):
        return merge_results([(r,) for r in results], (rules,))[0]
    how = {"sum": sum, "cat": lambda xs: np.concatenate(xs, axis=0), "first": lambda xs: xs[0]}
    return tuple(how[rule]([r[i] for r in results]) for i, rule in enumerate(rules))


class MultiContext(object):
    """Several GPUs from ONE process: a :class:`Context` per device, a thread per context (ctypes
    drops the GIL during the calls).  Frames are sharded for RDF / CN / BAD, atoms for MSD; integer
    results are summed on the host, so they equal the single-GPU ones bit for bit.  The usual
    multi-GPU route stays one process per GPU with torch.distributed (amof_amd.dist); this is the
    convenience for scripts that are not launched with torchrun.  A device may be listed twice
    (two contexts with their own streams on one GPU)."""

    def __init__(self, devices):
        self.devices = [int(d) for d in devices]
        if not self.devices:
            raise ValueError("empty device list")
        self.ctxs = [Context(d) for d in self.devices]
        self.device = self.devices[0]

    def close(self):
        for c in self.ctxs:
            c.close()

    def _shards(self, lo, hi):
        from . import dist as _d
        n = len(self.ctxs)
        return [tuple(x + lo for x in _d.shard_range(hi - lo, k, n)) for k in range(n)]

    @staticmethod
    def _for_device(packed, ctx, frame_range=None):
        """The trajectory as device ``ctx.device`` can read it: host arrays as they are, a CUDA tensor on
        another device copied over (the needed frames only)."""
        if not packed.on_device or packed.pos.device.index == ctx.device:
            return packed, frame_range
        import torch
        f0, f1 = (0, packed.n_frames) if frame_range is None else frame_range
        pos = packed.pos[f0:f1].to(torch.device("cuda", ctx.device))
        cell = packed.cell if packed.cell.shape[0] == 1 else packed.cell[f0:f1]
        return PackedTrajectory(pos, cell, packed.numbers, packed.masses, packed.pbc), (0, f1 - f0)

    def _run(self, jobs):
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(len(jobs)) as ex:
            return [f.result() for f in [ex.submit(j) for j in jobs]]

    def _sharded(self, name, packed, span, key, rules, *args, copy_frames=False, per_shard=None, **kwargs):
        """``ctx.<name>(trajectory, *args, <key>=shard, **kwargs)`` on every context, merged by ``rules`` (``merge_results``).
        ``span``: the ``(lo, hi)`` that ``_shards`` cuts, or the shards themselves, one per context; ``key``: the keyword
        that receives a shard (``frame_range``, ``atom_range``, ``work_range``); ``copy_frames``: the shard is a frame range,
        and a trajectory on another device is copied for those frames only (``_for_device``: the call then gets the range
        within the copy); ``per_shard(trajectory, a, b)``: further keywords that depend on the shard."""
        def job(ctx, a, b):
            tr, fr = self._for_device(packed, ctx, (a, b) if copy_frames else None)
            extra = per_shard(tr, a, b) if per_shard is not None else {}
            return getattr(ctx, name)(tr, *args, **dict(kwargs, **{key: fr if copy_frames else (a, b)}), **extra)
        shards = self._shards(*span) if isinstance(span, tuple) else span
        return merge_results(self._run([lambda ctx=ctx, a=a, b=b: job(ctx, a, b) for ctx, (a, b) in zip(self.ctxs, shards)]), rules)

    def rdf_accumulate(self, packed, rmax, nbins, frame_range=None, out=None):
        assert out is None, "device-resident accumulation is a single-context feature"
        hist, vol, kinds = self._sharded("rdf_accumulate", packed, _span(frame_range, packed.n_frames), "frame_range",
                                         ("sum", "sum", "first"), rmax, nbins, copy_frames=True)
        return hist, float(vol), kinds

    def cn_count(self, packed, cutoff, sets, frame_range=None, per_atom=False):
        return self._sharded("cn_count", packed, _span(frame_range, packed.n_frames), "frame_range",
                             ("cat", "cat") if per_atom else "cat", cutoff, sets, copy_frames=True, per_atom=per_atom)

    def bad_hist(self, packed, cutoff, triples, edges, frame_range=None, out=None):
        assert out is None, "device-resident accumulation is a single-context feature"
        return self._sharded("bad_hist", packed, _span(frame_range, packed.n_frames), "frame_range", ("sum", "sum"),
                             cutoff, triples, edges, copy_frames=True)

    def bad_hist_by_cn(self, packed, cutoff, triples, edges, cn_max=16, frame_range=None):
        return self._sharded("bad_hist_by_cn", packed, _span(frame_range, packed.n_frames), "frame_range", ("sum", "sum"),
                             cutoff, triples, edges, copy_frames=True, cn_max=cn_max)

    def msd_window(self, packed, windows, unwrap=False, remove_com=True, atom_range=None):
        return self._sharded("msd_window", packed, _span(atom_range, packed.n_atoms), "atom_range", ("sum", "first"),
                             windows, unwrap=unwrap, remove_com=remove_com)

    def vanhove_window(self, packed, windows, dr, nbins, unwrap=False, remove_com=True, atom_range=None):
        """atoms sharded over the devices; the integer counts add up exactly, the moments up to float64 summation order"""
        return self._sharded("vanhove_window", packed, _span(atom_range, packed.n_atoms), "atom_range",
                             ("sum", "sum", "sum", "first"), windows, dr, nbins, unwrap=unwrap, remove_com=remove_com)

    def vacf_window(self, packed, windows, origin_stride=1, velocities=False, remove_com=True, atom_range=None):
        """atoms sharded over the devices; the sums add up to float64 summation order"""
        return self._sharded("vacf_window", packed, _span(atom_range, packed.n_atoms), "atom_range", ("sum", "first"), windows,
                             origin_stride=origin_stride, velocities=velocities, remove_com=remove_com)

    def vanhove_distinct(self, packed, windows, rmax, nbins, origin_stride=1, work_range=None):
        """the (lag, origin) work list sharded over the devices: the integer counts add up exactly"""
        windows = _i32(windows)
        if work_range is None:
            work_range = _whole_work_list(packed.n_frames, windows, origin_stride)
        return self._sharded("vanhove_distinct", packed, tuple(work_range), "work_range", ("sum", "first"), windows, rmax, nbins,
                             origin_stride=origin_stride)

    def bond_survival(self, packed, cutoff, sets, windows, origin_stride=1, atom_range=None):
        """the centre atoms sharded over the devices: the integer counters add up exactly"""
        return self._sharded("bond_survival", packed, _span(atom_range, packed.n_atoms), "atom_range", "sum", cutoff, sets,
                             windows, origin_stride=origin_stride)

    def bond_reorientation(self, packed, cutoff, sets, windows, origin_stride=1, atom_range=None):
        """the centre atoms sharded over the devices: the integer sums add up exactly; the scale is the same on all"""
        return self._sharded("bond_reorientation", packed, _span(atom_range, packed.n_atoms), "atom_range", ("sum", "first"),
                             cutoff, sets, windows, origin_stride=origin_stride)

    def lindemann(self, packed, cutoff, sets, block, block_stride, nbins, ddelta, select=0, atom_range=None, per_atom=False, out=None):
        """the centre atoms sharded over the devices: the integer sums, histograms and per-atom rows (disjoint between the
        shards) add up exactly; the scale is the same on all"""
        assert out is None, "device-resident accumulation is a single-context feature"
        return self._sharded("lindemann", packed, _span(atom_range, packed.n_atoms), "atom_range",
                             ("sum", "sum", "first", "sum")[:3 + bool(per_atom)], cutoff, sets, block, block_stride, nbins, ddelta,
                             select=select, per_atom=per_atom)

    def bond_order(self, packed, cutoff, sets, l, nbins, nbins_tet, frame_range=None, per_atom=False, out=None):
        """frames sharded over the devices as ``cn_count``'s: the rows concatenate, the histograms add up exactly"""
        assert out is None, "device-resident accumulation is a single-context feature"
        return self._sharded("bond_order", packed, _span(frame_range, packed.n_frames), "frame_range",
                             ("sum", "sum", "cat", "cat")[:3 + bool(per_atom)], cutoff, sets, l, nbins, nbins_tet,
                             copy_frames=True, per_atom=per_atom)

    def dihedral_hist(self, packed, cutoff, chains, edges, frame_range=None, out=None):
        """frames sharded over the devices as ``cn_count``'s: the rows concatenate, the counts add up exactly"""
        assert out is None, "device-resident accumulation is a single-context feature"
        return self._sharded("dihedral_hist", packed, _span(frame_range, packed.n_frames), "frame_range",
                             ("sum", "sum", "sum", "cat"), cutoff, chains, edges, copy_frames=True)

    def ring_stats(self, packed, cutoff, max_size=32, frame_range=None, per_atom=False, neighbours=False):
        """frames sharded over the devices as ``cn_count``'s: every output is per frame, the rows concatenate"""
        return self._sharded("ring_stats", packed, _span(frame_range, packed.n_frames), "frame_range",
                             ("cat",) * (2 + bool(per_atom) + bool(neighbours)), cutoff, max_size, copy_frames=True,
                             per_atom=per_atom, neighbours=neighbours)

    def fragment_stats(self, packed, cutoff, link=None, ref_label=None, kinds=None, max_size=64, frame_range=None, per_atom=False,
                       com=False):
        """frames sharded over the devices as ``ring_stats``': every output is per frame, the rows concatenate (the masses of the
        reference fragments are the same on all)"""
        rules = ("cat",) * (3 + (link is not None) + 2 * bool(per_atom)) + (("cat", "first") if com else ())
        return self._sharded("fragment_stats", packed, _span(frame_range, packed.n_frames), "frame_range", rules, cutoff,
                             copy_frames=True, link=link, ref_label=ref_label, kinds=kinds, max_size=max_size, per_atom=per_atom, com=com)

    def pore_field(self, packed, radii, grid, dr, dmax, thresholds=(), frame_range=None, per_point=False):
        """frames sharded over the devices as ``cn_count``'s: every output is per frame, the rows concatenate"""
        return self._sharded("pore_field", packed, _span(frame_range, packed.n_frames), "frame_range",
                             ("cat",) * (4 + bool(per_point)), radii, grid, dr, dmax, thresholds, copy_frames=True, per_point=per_point)

    def pore_access(self, packed, radii, grid, dr, dmax, thresholds=(), frame_range=None, per_point=False, free_sphere=False,
                    labels=False):
        """frames sharded over the devices as ``pore_field``'s: every output is per frame, the rows concatenate"""
        return self._sharded("pore_access", packed, _span(frame_range, packed.n_frames), "frame_range",
                             ("cat",) * (5 + bool(free_sphere) + bool(per_point) + bool(labels)), radii, grid, dr, dmax, thresholds,
                             copy_frames=True, per_point=per_point, free_sphere=free_sphere, labels=labels)

    def pore_access_field(self, field, pbc=(True, True, True), thresholds=(), free_sphere=False, labels=False):
        return self.ctxs[0].pore_access_field(field, pbc, thresholds, free_sphere=free_sphere, labels=labels)

    def pore_psd(self, packed, radii, grid, dr, dmax, thresholds=(), frame_range=None, per_point=False, accessibility=False,
                 free_sphere=False, labels=False):
        """frames sharded over the devices as ``pore_access``'s: every output is per frame, the rows concatenate"""
        labelled = bool(accessibility or free_sphere)
        n = len(pore_names(bool(per_point), labelled, bool(free_sphere), bool(labels) and labelled, True, bool(accessibility)))
        return self._sharded("pore_psd", packed, _span(frame_range, packed.n_frames), "frame_range", ("cat",) * n, radii, grid, dr,
                             dmax, thresholds, copy_frames=True, per_point=per_point, accessibility=accessibility,
                             free_sphere=free_sphere, labels=labels)

    def pore_surface(self, packed, radii, grid, dr, dmax, thresholds=(), dirs=None, frame_range=None, per_point=False,
                     accessibility=False, free_sphere=False, labels=False, psd=False):
        """frames sharded over the devices as ``pore_psd``'s: every output is per frame, the rows concatenate"""
        labelled = bool(accessibility or free_sphere)
        n = len(pore_names(bool(per_point), labelled, bool(free_sphere), bool(labels) and labelled, bool(psd), bool(accessibility), True))
        return self._sharded("pore_surface", packed, _span(frame_range, packed.n_frames), "frame_range", ("cat",) * n, radii, grid, dr,
                             dmax, thresholds, copy_frames=True, dirs=dirs, per_point=per_point, accessibility=accessibility,
                             free_sphere=free_sphere, labels=labels, psd=psd)

    def pore_psd_field(self, field, cells, pbc, dr, dmax, thresholds=(), accessibility=False, per_point=False):
        return self.ctxs[0].pore_psd_field(field, cells, pbc, dr, dmax, thresholds, accessibility=accessibility, per_point=per_point)

    def sq_accumulate(self, packed, hkl, dq, nbins, frame_range=None, frame_stride=1, recip=None):
        """frames sharded over the devices (whole strides per device; a device trajectory on another GPU is copied for the
        shard's frames only): counts add up exactly, the sums to float64 order"""
        lo, hi = _span(frame_range, packed.n_frames)
        stride = int(frame_stride)
        n_sel = max(0, (hi - lo + stride - 1) // stride)
        recip = reciprocal(packed.cell) if recip is None else np.asarray(recip, dtype=np.float64)
        shards = [(lo + a * stride, max(lo + a * stride, min(hi, lo + b * stride))) for a, b in self._shards(0, n_sel)]

        def shard_recip(tr, f0, f1):
            return {"recip": recip if tr.cell.shape[0] == recip.shape[0] else recip[f0:f1]}
        return self._sharded("sq_accumulate", packed, shards, "frame_range", ("sum", "sum", "sum", "first"), hkl, dq, nbins,
                             copy_frames=True, per_shard=shard_recip, frame_stride=stride)

    def msd_direct(self, packed):
        return self.ctxs[0].msd_direct(self._for_device(packed, self.ctxs[0])[0])

    def last_kernel_seconds(self, dominant=False):
        return max(c.last_kernel_seconds(dominant) for c in self.ctxs)

    def last_kernel_launches(self):
        return sum(c.last_kernel_launches() for c in self.ctxs)

    def last_path(self):
        return self.ctxs[0].last_path()

    def synchronize(self):
        for c in self.ctxs:
            c.synchronize()


_contexts = {}


def get_context(device=None, lane=0):
    """Cached :class:`Context` of a device (default: LOCAL_RANK or 0); a list / tuple of devices gives
    a cached :class:`MultiContext` (several GPUs driven from this process).  ``lane=1``: the device's second context,
    on a stream of the highest priority (the memory-bound analyses of the classes run there)."""
    if isinstance(device, (list, tuple)):
        key = tuple(int(d) for d in device)
        with _ctx_lock:
            ctx = _contexts.get(key)
            if ctx is None:
                ctx = MultiContext(key)
                _contexts[key] = ctx
            return ctx
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
        n = device_count()
        if n > 0 and device >= n:
            raise RuntimeError("LOCAL_RANK=%d but only %d GPU(s) are visible: refusing to pile every rank onto "
                               "cuda:0 (pass device= explicitly to share a GPU on purpose)" % (device, n))
    key = device if not lane else (device, "lane", int(lane))
    with _ctx_lock:
        ctx = _contexts.get(key)
        if ctx is None:
            ctx = Context(device, priority=os.environ.get("AMOF_LANE1_PRIORITY", "high") if lane else "normal")
            _contexts[key] = ctx
            if lane:
                lead = _contexts.get(device)
                if lead is None:
                    lead = _contexts[device] = Context(device, priority="normal")
                ctx._follows = lead
        return ctx


def default_device():
    """the GPU an analysis goes to when the caller names none: LOCAL_RANK (one process per GPU) or 0"""
    return int(os.environ.get("LOCAL_RANK", "0"))


def lane_context(device, lane):
    """the context an analysis class runs on: ``lane`` 1 (memory-bound analyses) only while the classes run
    asynchronously (amof_amd/_lazy.py); a device list stays one MultiContext"""
    from . import _lazy
    if isinstance(device, (list, tuple)) or not lane or not _lazy.async_enabled():
        return get_context(device)
    return get_context(device, lane=lane)
