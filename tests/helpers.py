"""Shared builders for the parity tests (seeded synthetic trajectories)."""

import os
import re

import numpy as np

from amof_amd import data as _data
from amof_amd.frames import Frame, PackedTrajectory

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# Independent, pure-Python extended-XYZ reader (float() per field) for the fixtures: the yardstick the native
# reader (amof_amd.trajectory.read_xyz) is compared with bit for bit in tests/test_ingest.py.
def read_extxyz(path, index=None):
    """Return a list of :class:`Frame` (or one frame if ``index`` is an int)."""
    frames = []
    with open(path, "r") as fh:
        lines = fh.read().splitlines()
    i = 0
    while i < len(lines):
        if not lines[i].strip():
            i += 1
            continue
        n = int(lines[i].split()[0])
        comment = lines[i + 1]
        m = re.search(r'Lattice="([^"]*)"', comment)
        if m is None:
            raise ValueError("no Lattice= in comment line of %s" % path)
        cell = np.array([float(x) for x in m.group(1).split()]).reshape(3, 3)
        pbc = (True, True, True)
        mp = re.search(r'pbc="([^"]*)"', comment)
        if mp is not None:
            pbc = tuple(t.upper().startswith("T") for t in mp.group(1).split())
        symbols, pos = [], []
        for line in lines[i + 2:i + 2 + n]:
            w = line.split()
            symbols.append(w[0])
            pos.append([float(w[1]), float(w[2]), float(w[3])])
        numbers = [_data.atomic_numbers[s] for s in symbols]
        frames.append(Frame(numbers, np.array(pos), cell, pbc))
        i += 2 + n
    if isinstance(index, int):
        return frames[index]
    return frames


def species_of(numbers):
    kinds = sorted(set(int(z) for z in numbers))
    return kinds, np.array([kinds.index(int(z)) for z in numbers], dtype=np.int32)


def zif4_frame():
    return read_extxyz(os.path.join(GOLDEN, "ZIF-4.xyz"), 0)


def replicate(frame, reps):
    """replicate a frame reps = (nx, ny, nz) times along its cell vectors"""
    pos, num = [], []
    for a in range(reps[0]):
        for b in range(reps[1]):
            for c in range(reps[2]):
                pos.append(frame.positions + a * frame.cell[0] + b * frame.cell[1] + c * frame.cell[2])
                num.append(frame.numbers)
    cell = frame.cell * np.array(reps)[:, None]
    return Frame(np.concatenate(num), np.concatenate(pos), cell, frame.pbc)


def random_walk(base, F, sigma, seed, wrap=True, cell_jitter=0.0, ortho=False):
    """PackedTrajectory: base + cumulative Gaussian steps, wrapped into the cell"""
    rng = np.random.default_rng(seed)
    cell0 = np.diag(np.diag(base.cell)) if ortho else base.cell.copy()
    pos = base.positions.copy()
    P = np.empty((F,) + pos.shape)
    C = np.empty((F, 3, 3))
    for k in range(F):
        cell = cell0 * (1.0 + cell_jitter * rng.normal()) if cell_jitter else cell0
        p = pos
        if wrap:
            s = np.linalg.solve(cell.T, p.T).T
            s -= np.floor(s)
            p = s @ cell
        P[k] = p
        C[k] = cell
        pos = pos + rng.normal(scale=sigma, size=pos.shape)
    if not cell_jitter:
        C = C[:1]
    return PackedTrajectory(P, C, base.numbers, pbc=base.pbc)


def random_gas(N, cell, numbers, seed, F=1):
    rng = np.random.default_rng(seed)
    cell = np.asarray(cell, dtype=float)
    if cell.shape == (3,):
        cell = np.diag(cell)
    # uniform in the cell, then displaced by whole lattice vectors (still uniform modulo the cell)
    P = (rng.uniform(0, 1, size=(F, N, 3)) + rng.integers(-1, 2, size=(F, N, 3))) @ cell
    return PackedTrajectory(P, cell, numbers)


def rdf_path_case(kind):
    """(PackedTrajectory, rmax, nbins) of the cases whose RDF kernel family the GPU tests assert (tests/test_gpu_paths.py)
    and the selection is pinned to on the CPU (tests/test_rdf_select_cpu.py)"""
    z = zif4_frame()
    if kind == "elongated":       # 2x1x4 supercell: slab culling along z is active (2 rmax < Lz)
        return random_walk(replicate(z, (2, 1, 4)), 3, 0.05, 31, ortho=True), 6.0, 600
    if kind == "elongated_tri":
        return random_walk(replicate(z, (1, 1, 3)), 3, 0.05, 32), 5.0, 417
    if kind == "npt":
        return random_walk(replicate(z, (1, 1, 2)), 6, 0.05, 33, cell_jitter=0.01), 7.0, 700
    if kind == "plain_img":       # the image-aware variant forced on an input that does not need it
        return random_walk(replicate(z, (2, 1, 2)), 3, 0.05, 98, ortho=True), 7.0, 700
    if kind == "cell_ortho":      # 3264 atoms, 30.8 x 30.8 x 55.3 A: cutoffs far below the cell size
        return random_walk(replicate(z, (2, 2, 3)), 3, 0.08, 73, ortho=True), 5.0, 500
    if kind == "thin_long":       # a slab: thin along x only (no 3-D cell list), many cutoffs long and wide
        rng = np.random.default_rng(12)
        cell = np.diag([19.0, 120.0, 150.0])
        N = 20000
        numbers = np.where(np.arange(N) % 3 == 0, 8, 1)
        return PackedTrajectory(rng.uniform(0, 1, (2, N, 3)) @ cell, cell, numbers), 9.0, 900
    assert kind == "cubicish"
    return random_walk(z, 4, 0.05, 34), 7.7, 770


def _msd_case(F, n, diagonal, window, paths, unwrap=False, atom_range=None, hands_over=False):
    return dict(F=F, n=n, diagonal=diagonal, window=np.asarray(window, dtype=np.int32), paths=paths, unwrap=unwrap,
                atom_range=atom_range, hands_over=hands_over)


def _comb_window(F, d, W):
    return np.array([w * d for w in range(W) if w * d < F], dtype=np.int32)


MSD_COMB_SHAPES = [(7, 1, 3), (50, 3, 16), (333, 7, 24), (333, 11, 25), (1000, 100, 5), (1000, 31, 32),
                   (257, 13, 12), (90, 100, 1), (64, 2, 29), (1201, 50, 21),
                   (333, 3, 40), (1000, 7, 64), (2000, 9, 100), (700, 5, 33), (900, 11, 70),
                   # window spacings of 64 .. 256 frames: the streaming kernel (one thread per residue
                   # class; whole blocks, ragged comb ends, combs shorter than one block, 128 / 256 threads)
                   (5000, 100, 25), (3000, 64, 20), (2000, 128, 12), (2600, 129, 9), (4100, 256, 8),
                   (999, 77, 13), (1530, 100, 15), (4999, 100, 32), (650, 65, 10), (3333, 90, 24)]
MSD_FUSED_SHAPES = [(5000, 100, 25, 40), (1000, 100, 5, 9), (999, 77, 13, 30), (1530, 100, 15, 25),
                    (4999, 100, 32, 12), (650, 65, 10, 100), (3333, 90, 24, 17), (64, 16, 4, 5),
                    (700, 16, 32, 64), (1680, 16, 8, 3), (1675, 16, 8, 5),     # nq = 44, 105: up to 21 threads per column
                    (2000, 128, 12, 65), (4100, 256, 8, 24), (330, 64, 3, 40), (2600, 129, 9, 8)]
MSD_LONG_COMBS = [(100, 105), (1000, 10), (7, 250), (333, 31)]        # (d, W at most) on 21000 frames


def msd_path_case(kind):
    """key -> case of the window-MSD shapes whose kernel family the GPU tests assert (tests/test_gpu_paths.py,
    test_gpu_msd_fused.py, test_gpu_edges.py) and the selection is pinned to on the CPU (tests/test_msd_select_cpu.py).
    A case: F frames, n atoms, diagonal cell or not, the window list, unwrap, an atom range, and paths: the switches set
    (AMOF_MSD_<NAME>, lower case here) -> amof_last_path.  "msd_fused" is the path of a call whose columns never come within
    the centre-of-mass step of half the cell; a gas is handed over to the path of the same case with "nofused".  hands_over:
    the GPU test's trajectory is such a gas, so where the selection tries the fused form first the path is the one behind it."""
    out = {}
    if kind == "comb":              # 9 atoms in a triclinic cell
        for F, d, W in MSD_COMB_SHAPES:
            window = _comb_window(F, d, W)
            streams = 64 <= d <= 256 and 2 <= len(window) <= 32
            paths = {(): "msd_stream" if streams else ("msd_comb" if len(window) >= 2 else "msd_group"), ("nocomb",): "msd_group"}
            if streams:
                paths[("nostream",)] = "msd_comb"
            out[(F, d, W)] = _msd_case(F, 9, False, window, paths)
    elif kind == "fused":           # diagonal cells, the whole system
        for F, d, W, n in MSD_FUSED_SHAPES:
            other = "msd_stream" if 64 <= d <= 256 else "msd_comb"
            out[(F, d, W, n)] = _msd_case(F, n, True, _comb_window(F, d, W), {(): "msd_fused", ("nofused",): other})
    elif kind == "fused_other":     # what the fused form does not take
        out["general_cell"] = _msd_case(300, 272, False, np.arange(4) * 64, {(): "msd_stream"})
        out["spacing_8"] = _msd_case(300, 12, True, np.arange(30) * 8, {(): "msd_comb"})
        out["irregular"] = _msd_case(300, 12, True, [0, 3, 50, 161], {(): "msd_group"})
        out["40_windows"] = _msd_case(300, 12, True, np.arange(40) * 5, {(): "msd_comb"})
        out["107_segments"] = _msd_case(1700, 6, True, np.arange(8) * 16, {(): "msd_comb"})
        out["atom_range"] = _msd_case(300, 12, True, np.arange(4) * 64, {(): "msd_stream"}, atom_range=(2, 9))
    elif kind == "long":            # F + W beyond the LDS-resident limit (19 200), 6 atoms
        for unwrap in (False, True):
            out[("irregular", unwrap)] = _msd_case(21000, 6, True, [0, 1, 7, 500, 9999, 20000, 20999], {(): "msd_global"}, unwrap=unwrap,
                                                   hands_over=True)
            for d, W in MSD_LONG_COMBS:
                out[(d, W, unwrap)] = _msd_case(21000, 6, True, _comb_window(21000, d, W),
                                                {(): "msd_comb_global", ("nocomb",): "msd_global"}, unwrap=unwrap, hands_over=True)
    elif kind == "two_pass":        # 330 frames of 40 atoms, constant or breathing diagonal cell
        both = ("nofold", "nofused")
        out["stream"] = _msd_case(330, 40, True, np.arange(0, 160, 64), {(): "msd_fused", ("nofused",): "msd_stream", both: "msd_stream"})
        out["comb"] = _msd_case(330, 40, True, np.arange(0, 160, 8), {(): "msd_comb", both: "msd_comb"})
        out["group"] = _msd_case(330, 40, True, [0, 3, 50, 161], {(): "msd_group", both: "msd_group"})
    else:
        assert kind == "headline"
        out["headline"] = _msd_case(5000, 9792, True, _comb_window(5000, 100, 25), {(): "msd_fused", ("nofused",): "msd_stream"})
    return out


def msd_switch_env(switches):
    return {"AMOF_MSD_" + s.upper(): "1" for s in switches}


def device_walk(device, reps, n_frames, sigma, seed, base=None):
    """Synthetic ZIF-4 supercell trajectory generated directly in HBM (torch, float64): Gaussian random walk,
    sigma per frame and axis, wrapped each frame into the constant orthorhombic cell.  The headline workload of
    bench.py (BASELINE.json configs[2]/[3]) and of tests/test_gpu_headline.py.  Returns a PackedTrajectory whose
    ``pos`` is a CUDA tensor; the caller synchronises (or relies on the library's stream ordering)."""
    import torch
    base = zif4_frame() if base is None else base
    rep = replicate(base, reps)
    lengths = np.diag(base.cell) * np.array(reps)          # constant orthorhombic cell
    cell = np.diag(lengths)
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    n = len(rep.numbers)
    L = torch.tensor(lengths, dtype=torch.float64, device=device)
    traj = torch.empty((n_frames, n, 3), dtype=torch.float64, device=device)
    cur = torch.tensor(rep.positions, dtype=torch.float64, device=device)   # unwrapped position of the last frame
    chunk = 250
    for f0 in range(0, n_frames, chunk):
        f1 = min(f0 + chunk, n_frames)
        steps = torch.randn((f1 - f0, n, 3), dtype=torch.float64, device=device, generator=g) * sigma
        if f0 == 0:
            steps[0] = 0.0                                  # frame 0 is the base structure
        walk = cur + torch.cumsum(steps, dim=0)
        cur = walk[-1].clone()
        traj[f0:f1] = walk - torch.floor(walk / L) * L     # wrapped into the cell
        del steps, walk
    return PackedTrajectory(traj, cell, rep.numbers)


def device_walk_cell(device, base, cells, n_frames, sigma, seed):
    """Like device_walk, for ANY cell: a Gaussian random walk in Cartesian space from the (replicated) Frame `base`,
    wrapped each frame into `cells` -- one [3][3] cell or a per-frame [F][3][3] series (NPT) -- in fractional
    coordinates.  Atoms keep their fractional coordinates when the cell breathes.  Generated in HBM (torch, float64)."""
    import torch
    cells = np.asarray(cells, dtype=np.float64)
    per_frame = cells.ndim == 3 and cells.shape[0] > 1
    if cells.ndim == 2:
        cells = cells.reshape(1, 3, 3)
    assert cells.shape[0] in (1, n_frames)
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    n = len(base.numbers)
    C = torch.tensor(cells, dtype=torch.float64, device=device)
    Cinv = torch.linalg.inv(C)
    traj = torch.empty((n_frames, n, 3), dtype=torch.float64, device=device)
    # the walk lives in the fractional coordinates of the first cell (steps of sigma Angstrom there)
    cur = torch.tensor(np.linalg.solve(np.asarray(base.cell).T, base.positions.T).T, dtype=torch.float64, device=device)
    chunk = 250
    for f0 in range(0, n_frames, chunk):
        f1 = min(f0 + chunk, n_frames)
        steps = torch.randn((f1 - f0, n, 3), dtype=torch.float64, device=device, generator=g) * sigma
        if f0 == 0:
            steps[0] = 0.0
        walk = cur + torch.cumsum(steps @ Cinv[0], dim=0)
        cur = walk[-1].clone()
        s = walk - torch.floor(walk)
        traj[f0:f1] = torch.matmul(s, C[f0:f1] if per_frame else C[0])
        del steps, walk, s
    return PackedTrajectory(traj, cells if per_frame else cells[0], base.numbers)


# ---------------------------------------------------------------------------------------------------------------
# A second, stricter stand-in for ase.Atoms (ASE itself is not installed here).  Unlike amof_amd.frames.Frame --
# written by the same hand as the code that consumes it -- this one copies the SHAPES of ASE 3.20's objects: the
# cell is a Cell object (not an ndarray: `.array`, `__array__`, `.lengths()`, `.volume`), `get_cell()` returns
# such an object, `pbc` is a bool ndarray, `positions` / `numbers` are properties over a private arrays dict,
# `symbols.formula._count` is a plain dict in order of first appearance.  Nothing here inherits from the product.
class CellLike(object):
    def __init__(self, array):
        self.array = np.array(array, dtype=float).reshape(3, 3)

    def __array__(self, dtype=None, copy=None):
        return self.array if dtype is None else self.array.astype(dtype)

    def __getitem__(self, item):
        return self.array[item]

    def __len__(self):
        return 3

    def copy(self):
        return CellLike(self.array.copy())

    def lengths(self):
        return np.linalg.norm(self.array, axis=1)

    def cellpar(self):
        ang = []
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            ang.append(np.degrees(np.arccos(np.dot(self.array[j], self.array[k]) /
                                            (np.linalg.norm(self.array[j]) * np.linalg.norm(self.array[k])))))
        return np.array(list(self.lengths()) + ang)

    @property
    def volume(self):
        return abs(np.linalg.det(self.array))


class _FormulaLike(object):
    def __init__(self, symbols):
        self._count = {}
        for s in symbols:
            self._count[s] = self._count.get(s, 0) + 1


class _SymbolsLike(object):
    def __init__(self, numbers):
        self.numbers = numbers

    def __iter__(self):
        return (_data.chemical_symbols[int(z)] for z in self.numbers)

    @property
    def formula(self):
        return _FormulaLike(list(self))


class AseLikeAtoms(object):
    def __init__(self, numbers, positions, cell, pbc=True):
        self.arrays = {"numbers": np.array(numbers, dtype=int), "positions": np.array(positions, dtype=float)}
        self._cellobj = CellLike(cell)
        self._pbc = np.zeros(3, bool)
        self._pbc[:] = pbc

    cell = property(lambda self: self._cellobj)
    pbc = property(lambda self: self._pbc)
    numbers = property(lambda self: self.arrays["numbers"])
    positions = property(lambda self: self.arrays["positions"],
                         lambda self, v: self.arrays["positions"].__setitem__(slice(None), v))
    symbols = property(lambda self: _SymbolsLike(self.arrays["numbers"]))

    def __len__(self):
        return len(self.arrays["positions"])

    def copy(self):
        return AseLikeAtoms(self.numbers.copy(), self.positions.copy(), self.cell.array.copy(), self.pbc.copy())

    def get_positions(self):
        return self.arrays["positions"].copy()

    def set_positions(self, newpositions):
        self.arrays["positions"][:] = newpositions

    def get_atomic_numbers(self):
        return self.arrays["numbers"].copy()

    def get_cell(self, complete=False):
        return self._cellobj.copy()

    def get_pbc(self):
        return self._pbc.copy()

    def get_cell_lengths_and_angles(self):
        return self._cellobj.cellpar()

    def get_volume(self):
        return self._cellobj.volume

    def get_masses(self):
        return np.array([_data.atomic_masses[int(z)] for z in self.numbers])

    def get_center_of_mass(self):
        m = self.get_masses()
        return np.dot(m, self.positions) / m.sum()

    def translate(self, displacement):
        self.arrays["positions"] += np.array(displacement)


def as_ase_like(packed):
    """the frames of a host PackedTrajectory as AseLikeAtoms objects"""
    return [AseLikeAtoms(packed.numbers, packed.pos[k], packed.cell_of(k), packed.pbc) for k in range(packed.n_frames)]
