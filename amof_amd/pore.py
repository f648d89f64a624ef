"""Pore geometry of a trajectory on MI355X: void fraction, cavity-size histogram and largest included sphere per frame.

``Pore`` lays a grid over the cell of every frame and gives each grid point its distance to the nearest atomic surface,

    v(p) = min_j |r_j - p| - R_j            (minimum image; R_j: the van der Waals radius of atom j's element)

which the HIP kernels behind ``amof_pore_field`` (amof_amd/csrc/pore.hip) evaluate in the library's canonical float64
arithmetic.  A probe of radius rp fits with its CENTRE at p where v(p) >= rp, so per frame

    probe-centre volume fraction(rp) = #{v >= rp} / G,      Di = 2 max_p v(p)   (largest included sphere)

and the histogram of v over the void is a cavity-size distribution.  The kernels return integers and the largest value;
the host keeps the divisions and the DataFrames.

The reference's ``Pore`` (amof/pore/core.py) writes one CIF per frame and starts the external Zeo++ binary on it.  This
class takes the reference's four arguments and Zeo++'s column names for the quantities it has, but it is NOT Zeo++: that
uses a Voronoi network, Monte-Carlo sampling and an accessibility test; this is the deterministic grid version of the same
geometric quantities, converging with the grid spacing.

``accessibility=True`` splits the probe-centre volume into its accessible and non-accessible part: the periodic connected
components of {v >= rp} (6-neighbourhood of the grid) are labelled on the GPU (``amof_pore_access``,
amof_amd/csrc/pore_access.hip); a component that winds around the cell is a channel and its points are accessible, one
that does not is a pocket.  ``free_sphere=True`` adds the largest free sphere Df -- twice the largest v at which the void still
has a channel -- and Dif, the largest included sphere along the channels of that void.  include/amof_hip.h has the
definitions.

``psd=True`` adds the Gelb-Gubbins pore size distribution and the probe-occupiable volume.  Both come from the covering radius

    w(p) = max { v(c) : v(c) >= 0, |c - p| <= v(c) }        (c: the grid points; v(p) where no sphere covers p)

the radius of the largest sphere that overlaps no atom and covers p (``amof_pore_psd``, amof_amd/csrc/pore_cover.hip).  The
fraction of points with w >= r is the cumulative pore volume V(r) of Gelb and Gubbins, its histogram is - dV/dr, and
#{w >= rp} / G is the volume a probe of radius rp occupies -- the whole probe sphere, the quantity helium or nitrogen pore
volumes are compared with; the probe-centre volume above understates it by a surface layer rp thick.  With
``accessibility`` the occupiable volume is split into the part covered from a channel (POAV) and the rest (PONAV).

``surface=True`` adds the surface area by deterministic Shrake-Rupley sampling: every atom carries ``surface_points`` samples
on its sphere of radius R_j + rp (``sphere_points``: a Fibonacci lattice, the same directions for every atom), a sample is
exposed when it lies in no other atom's sphere of radius R_k + rp, and

    SA(rp) = sum_s 4 pi (R_s + rp)^2 exposed_s / M          (rp = 0: the van der Waals surface)

from the integers of ``amof_pore_surface`` (amof_amd/csrc/pore_surface.hip).  With ``accessibility`` an exposed sample is
accessible when one of the 8 grid points around it lies in a channel of the void of that probe: ASA and NASA, a grid estimate
that converges with the spacing.  Zeo++ samples the same spheres at random; these are not its numbers.
"""

import logging

import numpy as np
import pandas as pd

from ._lazy import Deferred, EmptyUntilComputed

from . import _hip
from . import _setup
from . import data as _data
from . import dist as _dist
from . import trajectory as _trajectory
from .files import path as _path

logger = logging.getLogger(__name__)

# van der Waals radii in Angstrom (A. Bondi, J. Phys. Chem. 68 (1964) 441, and the later values commonly tabulated with them)
BONDI = {"H": 1.20, "He": 1.40, "Li": 1.82, "C": 1.70, "N": 1.55, "O": 1.52, "F": 1.47, "Ne": 1.54, "Na": 2.27, "Mg": 1.73,
         "Si": 2.10, "P": 1.80, "S": 1.80, "Cl": 1.75, "Ar": 1.88, "K": 2.75, "Ni": 1.63, "Cu": 1.40, "Zn": 1.39, "Ga": 1.87,
         "As": 1.85, "Se": 1.90, "Br": 1.85, "Kr": 2.02, "Pd": 1.63, "Ag": 1.72, "Cd": 1.58, "In": 1.93, "Sn": 2.17,
         "Te": 2.06, "I": 1.98, "Xe": 2.16, "Pt": 1.75, "Au": 1.66, "Hg": 1.55, "Tl": 1.96, "Pb": 2.02, "U": 1.86}
AVOGADRO_A3 = 0.602214076       # N_A * 1e-24: Angstrom^3 per atom and g/mol  ->  cm^3/g
DMAX_CAP = 8.0


def grid_points(cell, n):
    """Cartesian grid points ``[nx][ny][nz][3]`` of one cell ``[3][3]`` (rows = cell vectors): the point (i, j, k) has the
    fractional coordinates ``((i + 0.5) / nx, (j + 0.5) / ny, (k + 0.5) / nz)`` and ``p_c = (f_x C[0][c] + f_y C[1][c]) +
    f_z C[2][c]`` -- float64 products and sums in this order, the kernels' own bits.  Linear index: ``(i ny + j) nz + k``."""
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    nx, ny, nz = (int(x) for x in n)
    fx = ((np.arange(nx, dtype=np.float64) + 0.5) / np.float64(nx))[:, None, None, None]
    fy = ((np.arange(ny, dtype=np.float64) + 0.5) / np.float64(ny))[None, :, None, None]
    fz = ((np.arange(nz, dtype=np.float64) + 0.5) / np.float64(nz))[None, None, :, None]
    return (fx * cell[0] + fy * cell[1]) + fz * cell[2]


def default_grid(cell, spacing):
    """``n_k = max(1, ceil(|a_k| / spacing))`` from the lattice-vector lengths of one cell"""
    spacing = float(spacing)
    if not (np.isfinite(spacing) and spacing > 0):
        raise ValueError("spacing must be finite and > 0")
    lengths = np.sqrt((np.asarray(cell, dtype=np.float64).reshape(3, 3) ** 2).sum(axis=1))
    return tuple(max(1, int(np.ceil(x / spacing))) for x in lengths)


def cell_heights(cells):
    """perpendicular heights ``[..][3]`` of cells ``[..][3][3]``: volume / area of the face spanned by the other two vectors"""
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3, 3)
    faces = np.stack([np.cross(cells[:, 1], cells[:, 2]), np.cross(cells[:, 2], cells[:, 0]), np.cross(cells[:, 0], cells[:, 1])], axis=1)
    vol = np.abs((cells[:, 0] * faces[:, 0]).sum(axis=1))
    return vol[:, None] / np.sqrt((faces ** 2).sum(axis=2))


def half_height(cells, pbc):
    """half the smallest perpendicular height of any cell on a periodic axis (inf without one)"""
    h = cell_heights(cells)[:, np.asarray(pbc, dtype=bool)]
    return 0.5 * float(h.min()) if h.size else np.inf


def default_dmax(cells, pbc, rmax, dr):
    """the largest multiple of ``dr`` not above ``min(8 A, min over frames of h_min / 2 - rmax)``"""
    limit = min(DMAX_CAP, half_height(cells, pbc) - rmax)
    k = int(np.floor(limit / dr)) if limit > 0 else 0
    while k > 0 and k * dr > limit:
        k -= 1
    if k < 1:
        raise ValueError("no multiple of dr = %g fits below half the smallest cell height minus the largest radius (%g): the cell "
                         "is too small for these radii" % (dr, limit))
    return k * dr


def species_radii(numbers, radii=None):
    """van der Waals radius (Angstrom) per atomic number of ``numbers``: ``radii`` (element symbol -> Angstrom) over the
    built-in ``BONDI`` table; an element in neither raises ValueError"""
    table = dict(BONDI)
    for sym, r in (radii or {}).items():
        r = float(r)
        if not (np.isfinite(r) and r >= 0):
            raise ValueError("radius of %s must be finite and >= 0" % sym)
        table[str(sym).capitalize()] = r
    out = []
    for z in numbers:
        sym = _data.chemical_symbols[int(z)]
        if sym not in table:
            raise ValueError("no van der Waals radius for element %s: pass radii={'%s': ...}" % (sym, sym))
        out.append(table[sym])
    return np.array(out, dtype=np.float64)


def probe_label(rp):
    return "%g" % rp


def positions(argmax, cells, grid):
    """``[F][3]`` grid points of the linear indices ``argmax [F]`` in the cells ``[1 or F][3][3]`` (``grid_points``' rule)"""
    am = np.asarray(argmax, dtype=np.int64)
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3, 3)
    if cells.shape[0] == 1:
        cells = np.broadcast_to(cells, (len(am), 3, 3))
    nx, ny, nz = (int(x) for x in grid)
    i, j, k = am // (ny * nz), (am // nz) % ny, am % nz
    f = np.stack([(i + 0.5) / np.float64(nx), (j + 0.5) / np.float64(ny), (k + 0.5) / np.float64(nz)], axis=1)
    return (f[:, 0:1] * cells[:, 0] + f[:, 1:2] * cells[:, 1]) + f[:, 2:3] * cells[:, 2]


def assemble(counts, probe_counts, vmax, step, volume, mass, probes, grid, dr):
    """``(data, hist)`` from the library's per-frame results: ``counts`` u64 ``[F][nbins + 2]`` (inside an atom, the bins of
    [0, dmax), overflow), ``probe_counts [F][n_probes]`` (points with v >= rp), ``vmax [F]``; ``volume [F]``: the cell
    volumes (A^3), ``mass``: the sum of the atomic masses (g/mol).
      data   Step, Unitcell_volume (A^3), Density (g/cm^3) = M / (V 0.602214076), per probe rp (``%g``)
             PCV_Volume_fraction-rp = count / G, PCV_A^3-rp, PCV_cm^3/g-rp = V 0.602214076 / M (probe-centre volume:
             accessible plus non-accessible), and Di = 2 vmax (inf where the frame has an overflow point: the largest sphere
             is not resolved, raise dmax)
      hist   r (bin centres) and density: the trajectory mean of count / (G dr) over the non-negative bins"""
    counts = np.asarray(counts, dtype=np.uint64)
    F = counts.shape[0]
    nbins = counts.shape[1] - 2
    G = int(grid[0]) * int(grid[1]) * int(grid[2])
    volume = np.asarray(volume, dtype=np.float64).reshape(F)
    step = np.asarray(step)
    data = {"Step": step[:F] if len(step) >= F else np.arange(F), "Unitcell_volume": volume,
            "Density": float(mass) / (volume * AVOGADRO_A3)}
    probe_counts = np.asarray(probe_counts, dtype=np.int64).reshape(F, len(probes))
    for k, rp in enumerate(probes):
        frac = probe_counts[:, k].astype(np.float64) / G
        data["PCV_Volume_fraction-" + probe_label(rp)] = frac
        data["PCV_A^3-" + probe_label(rp)] = frac * volume
        data["PCV_cm^3/g-" + probe_label(rp)] = frac * volume * AVOGADRO_A3 / float(mass)
    overflow = counts[:, nbins + 1] > 0
    data["Di"] = np.where(overflow, np.inf, 2.0 * np.asarray(vmax, dtype=np.float64).reshape(F))
    per_frame = counts[:, 1:nbins + 1].astype(np.float64) / (G * float(dr))
    hist = pd.DataFrame({"r": (np.arange(nbins) + 0.5) * float(dr),
                         "density": per_frame.mean(axis=0) if F else np.full(nbins, np.nan)})
    return pd.DataFrame(data), hist


def access_columns(access, probe_counts, volume, mass, probes, grid):
    """the columns ``accessibility=True`` adds to ``.data``, from the library's integers: ``access [F][n_probes][4]`` (accessible
    points, channels, pockets, largest channel dimension), ``probe_counts [F][n_probes]`` (points with v >= rp).  Per probe
    rp: AV_Volume_fraction-rp = accessible / G, NAV_Volume_fraction-rp = (count - accessible) / G, each with its A^3 and cm^3/g
    as the PCV columns (AV + NAV = PCV in counts), Channels-rp, Pockets-rp, Channel_dimension-rp (0 without a channel)."""
    access = np.asarray(access, dtype=np.int64).reshape(-1, len(probes), 4)
    F = access.shape[0]
    probe_counts = np.asarray(probe_counts, dtype=np.int64).reshape(F, len(probes))
    volume = np.asarray(volume, dtype=np.float64).reshape(F)
    G = int(grid[0]) * int(grid[1]) * int(grid[2])
    if (access[:, :, 0] > probe_counts).any() or (access < 0).any():
        raise ValueError("more accessible points than points of the void")
    cols = {}
    for k, rp in enumerate(probes):
        for name, count in (("AV", access[:, k, 0]), ("NAV", probe_counts[:, k] - access[:, k, 0])):
            frac = count.astype(np.float64) / G
            cols[name + "_Volume_fraction-" + probe_label(rp)] = frac
            cols[name + "_A^3-" + probe_label(rp)] = frac * volume
            cols[name + "_cm^3/g-" + probe_label(rp)] = frac * volume * AVOGADRO_A3 / float(mass)
        cols["Channels-" + probe_label(rp)] = access[:, k, 1].copy()
        cols["Pockets-" + probe_label(rp)] = access[:, k, 2].copy()
        cols["Channel_dimension-" + probe_label(rp)] = access[:, k, 3].copy()
    return cols


def psd_columns(psd_counts, po_counts, po_access, volume, mass, probes, grid, dr):
    """``(columns, psd)`` of ``psd=True`` from the library's integers: ``psd_counts`` u64 ``[F][nbins + 2]`` (points covered by no
    sphere, the bins of the covering radius w over [0, dmax), w >= dmax), ``po_counts [F][n_probes]`` (points with w >= rp),
    ``po_access [F][n_probes]`` or None (points covered from a channel of the void v >= rp).
      columns  per probe rp POV_Volume_fraction-rp = po_count / G with its A^3 and cm^3/g as the PCV columns; with ``po_access``
               POAV_* = po_access / G and PONAV_* = (po_count - po_access) / G (POAV + PONAV = POV in counts)
      psd      r (bin centres), density: the trajectory mean of count / (G dr), - dV/dr as a fraction of the cell volume per
               Angstrom; cumulative: the trajectory mean of the fraction of points with w >= the bin's lower edge, summed from
               the integers, the points with w >= dmax included -- it starts at the covered fraction and never rises"""
    psd_counts = np.asarray(psd_counts, dtype=np.uint64)
    F = psd_counts.shape[0]
    nbins = psd_counts.shape[1] - 2
    G = int(grid[0]) * int(grid[1]) * int(grid[2])
    po_counts = np.asarray(po_counts, dtype=np.int64).reshape(F, len(probes))
    volume = np.asarray(volume, dtype=np.float64).reshape(F)
    kinds = [("POV", po_counts)]
    if po_access is not None:
        po_access = np.asarray(po_access, dtype=np.int64).reshape(F, len(probes))
        if (po_access > po_counts).any() or (po_access < 0).any():
            raise ValueError("more points covered from channels than covered at all")
        kinds += [("POAV", po_access), ("PONAV", po_counts - po_access)]
    cols = {}
    for k, rp in enumerate(probes):
        for name, count in kinds:
            frac = count[:, k].astype(np.float64) / G
            cols[name + "_Volume_fraction-" + probe_label(rp)] = frac
            cols[name + "_A^3-" + probe_label(rp)] = frac * volume
            cols[name + "_cm^3/g-" + probe_label(rp)] = frac * volume * AVOGADRO_A3 / float(mass)
    ints = psd_counts[:, 1:].astype(np.int64)                   # the bins, then w >= dmax
    above = ints[:, ::-1].cumsum(axis=1)[:, ::-1][:, :nbins]    # points with w >= the lower edge of bin b
    psd = pd.DataFrame({"r": (np.arange(nbins) + 0.5) * float(dr),
                        "density": (ints[:, :nbins].astype(np.float64) / (G * float(dr))).mean(axis=0) if F else np.full(nbins, np.nan),
                        "cumulative": (above.astype(np.float64) / G).mean(axis=0) if F else np.full(nbins, np.nan)})
    return cols, psd


def sphere_points(M):
    """``[M][3]`` unit vectors of the Fibonacci lattice: ``z_m = 1 - (2 m + 1) / M``, ``phi_m = m pi (3 - sqrt 5)``, ``u = (sqrt(1 -
    z^2) cos phi, sqrt(1 - z^2) sin phi, z)`` -- uniform in z, the default directions of ``Pore(surface=True)``"""
    M = int(M)
    if not 1 <= M <= 4096:
        raise ValueError("1 .. 4096 sphere points")
    m = np.arange(M, dtype=np.float64)
    z = 1.0 - (2.0 * m + 1.0) / M
    phi = m * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    return np.ascontiguousarray(np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1))


def surface_area(exposed, radii, rp, M):
    """``[..]`` Angstrom^2 from exposed counts ``[..][S]``: ``sum_s ((4 pi) rho_s rho_s) exposed_s / M``, ``rho_s = radii[s] + rp``,
    the species added in order"""
    exposed = np.asarray(exposed, dtype=np.int64)
    total = np.zeros(exposed.shape[:-1], dtype=np.float64)
    for k, R in enumerate(np.asarray(radii, dtype=np.float64)):
        rho = R + np.float64(rp)
        total = total + ((4.0 * np.pi) * rho * rho) * exposed[..., k].astype(np.float64) / np.float64(M)
    return total


SURFACE_PER_GRAM = 6022.14076       # 1e-20 m^2 per Angstrom^2 x N_A: A^2 per cell and g/mol per cell  ->  m^2/g


def surface_columns(exposed, exposed_access, radii, volume, mass, probes, M):
    """the columns ``surface=True`` adds to ``.data``, from the library's integers: ``exposed [F][n_probes][S]`` (exposed samples
    per species), ``exposed_access`` the same of the accessible ones, or None; ``radii [S]``, ``volume [F]`` (A^3), ``mass``
    (g/mol per cell), ``M`` samples per atom.  Per probe rp: SA_A^2-rp (``surface_area``), SA_m^2/cm^3-rp = A^2 1e4 / V,
    SA_m^2/g-rp = A^2 6022.14076 / mass; with ``exposed_access`` ASA_* of the accessible and NASA_* of exposed - accessible samples
    (ASA + NASA = SA in counts)."""
    exposed = np.asarray(exposed, dtype=np.int64)
    F = exposed.shape[0]
    exposed = exposed.reshape(F, len(probes), -1)
    volume = np.asarray(volume, dtype=np.float64).reshape(F)
    kinds = [("SA", exposed)]
    if exposed_access is not None:
        exposed_access = np.asarray(exposed_access, dtype=np.int64).reshape(exposed.shape)
        if (exposed_access > exposed).any() or (exposed_access < 0).any():
            raise ValueError("more accessible samples than exposed ones")
        kinds += [("ASA", exposed_access), ("NASA", exposed - exposed_access)]
    cols = {}
    for k, rp in enumerate(probes):
        for name, count in kinds:
            area = surface_area(count[:, k], radii, rp, M)
            cols[name + "_A^2-" + probe_label(rp)] = area
            cols[name + "_m^2/cm^3-" + probe_label(rp)] = area * 1e4 / volume
            cols[name + "_m^2/g-" + probe_label(rp)] = area * SURFACE_PER_GRAM / float(mass)
    return cols


def free_sphere_columns(free):
    """``Df = 2 t*`` and ``Dif`` from ``free [F][2]`` (t*, Dif / 2; inf: not resolved below dmax, 0: no channel at all)"""
    free = np.asarray(free, dtype=np.float64).reshape(-1, 2)
    return {"Df": 2.0 * free[:, 0], "Dif": 2.0 * free[:, 1]}


class Pore(Deferred):
    """
    Void fraction, cavity-size histogram and largest included sphere of every frame of a trajectory

    ``from_trajectory`` enqueues the analysis on its device's second lane and returns; ``.data`` (and every other result)
    waits for it (amof_amd/_lazy.py; ``AMOF_ASYNC=0``: synchronous).

      .data         per frame: Step, Unitcell_volume, Density, PCV_Volume_fraction-rp / PCV_A^3-rp / PCV_cm^3/g-rp per probe
                    radius, Di (``assemble``)
      .hist         r, density: distribution of the distance to the nearest atomic surface over the void, trajectory mean
      .counts       u64 [F][nbins + 2]: grid points inside an atom, per bin of [0, dmax), overflow
      .di_position  [F][3]: where the largest included sphere sits
      per_point=True: .field float64 [F][nx][ny][nz], the distance itself (dmax where it is not below dmax)
      accessibility=True: per probe radius AV_* / NAV_* (accessible / non-accessible probe-centre volume), Channels-rp,
                    Pockets-rp, Channel_dimension-rp (``access_columns``); .access int64 [F][n_probes][4]; with per_point
                    .labels int32 [F][n_probes][nx][ny][nz]: the smallest linear index of a point's component, -1 outside
      free_sphere=True: Df, Dif (``free_sphere_columns``); .free_sphere [F][2]: t* and Dif / 2
      psd=True:     per probe radius POV_* (probe-occupiable volume), with accessibility POAV_* / PONAV_* (``psd_columns``);
                    .psd: r, density, cumulative -- the pore size distribution - dV/dr and V(r), trajectory means;
                    .psd_counts u64 [F][nbins + 2], .po_counts int64 [F][n_probes], with accessibility .po_access; with
                    per_point .cover float64 [F][nx][ny][nz], the covering radius.  In a frame with overflow points (the
                    warning below) the covering radius is a lower bound where it reaches dmax: the POV columns stay valid for
                    rp <= dmax, the distribution above dmax is not resolved.
      surface=True: per probe radius SA_A^2-rp, SA_m^2/cm^3-rp, SA_m^2/g-rp, with accessibility ASA_* / NASA_*
                    (``surface_columns``); .exposed int64 [F][n_probes][S], with accessibility .exposed_access;
                    .surface_by_species: A^2 per element and probe radius; with per_point .surface_samples uint8
                    [F][n_probes][N][M]: 0 buried, 1 exposed, 2 exposed and accessible
    These are grid estimates of geometric quantities, not Zeo++'s numbers (see the module's docstring).
    """

    data = EmptyUntilComputed("Step")

    def __init__(self):
        """default constructor"""
        self.data = None

    @classmethod
    def from_trajectory(cls, trajectory, delta_Step=1, first_frame=0, parallel=False, *, probe_radius=(0.0, 1.2), spacing=0.2,
                        grid=None, dr=0.05, dmax=None, radii=None, per_point=False, device=None, distributed=None, accessibility=False,
                        free_sphere=False, psd=False, surface=False, surface_points=256):
        """
        Args:
            trajectory: list of ase.Atoms-like frames, a PackedTrajectory or an XyzStream
            parallel: accepted for the reference's signature and ignored
            probe_radius: probe radii in Angstrom (0: the void itself)
            spacing: grid spacing in Angstrom: ``n_k = max(1, ceil(|a_k| / spacing))`` from frame 0's cell, the same grid for
                all frames; grid: ``(nx, ny, nz)`` instead (required, as is dmax, with ``distributed='local'``)
            dr: bin width of the histogram; dmax: its upper end and the largest distance resolved (default: the largest
                multiple of dr not above min(8, half the smallest cell height - the largest radius)); dmax + the largest
                radius above half the smallest perpendicular cell height raises ValueError
            radii: dict element -> Angstrom over the built-in Bondi table; an element in neither raises ValueError
            per_point: keep the field
            accessibility: label the void of every probe radius and split its volume into accessible and non-accessible
                (every periodic grid axis then needs at least 3 points)
            free_sphere: the largest free sphere Df and Dif per frame (about log2 of the grid size labellings per frame)
            psd: the pore size distribution and the probe-occupiable volume of every probe radius (one more pass over the
                field, about as heavy as the field itself; with accessibility one more per probe radius that has a channel)
            surface: the surface area of every probe radius by Shrake-Rupley sampling, with accessibility its accessible and
                non-accessible part; surface_points: samples per atom (1 .. 4096, ``sphere_points``).  The largest radius + the
                largest probe radius above half the smallest perpendicular cell height raises ValueError
            device: GPU index or list of indices (default: LOCAL_RANK or 0)
            distributed: None -> the ranks of an initialised torch.distributed group take contiguous shares of the frames;
                False -> single process; 'local' -> the trajectory is this rank's own block of frames
        """
        pore = cls()
        step = _trajectory.construct_step(delta_Step=delta_Step, first_frame=first_frame, number_of_frames=len(trajectory))
        pore.compute_pore(trajectory, step, probe_radius, spacing, grid, dr, dmax, radii, per_point, device=device,
                          distributed=distributed, accessibility=accessibility, free_sphere=free_sphere, psd=psd, surface=surface,
                          surface_points=surface_points)
        return pore

    def compute_pore(self, trajectory, step, probe_radius=(0.0, 1.2), spacing=0.2, grid=None, dr=0.05, dmax=None, radii=None,
                     per_point=False, device=None, distributed=None, accessibility=False, free_sphere=False, psd=False, surface=False,
                     surface_points=256):
        packed = _setup.pack(trajectory, device, keep_stream=True)
        logger.info("Start pore analysis for %s frames", len(packed))
        kinds, _ = _hip.packed_species(packed)
        rs = species_radii(kinds, radii)
        probes = [float(x) for x in np.atleast_1d(np.asarray(probe_radius, dtype=np.float64))]
        if any(not (np.isfinite(x) and x >= 0) for x in probes):
            raise ValueError("probe radii must be finite and >= 0")
        dr = float(dr)
        if not (np.isfinite(dr) and dr > 0):
            raise ValueError("dr must be finite and > 0")
        cells = packed._cells_known() if hasattr(packed, "_cells_known") else packed.cell
        cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3, 3)
        if distributed == 'local' and (grid is None or dmax is None):
            # the defaults come from the cells a rank sees: ranks with blocks of their own would not agree on the grid, on
            # dmax or on the number of bins of the rows they gather
            raise ValueError("distributed='local': every rank sees its own frames only, pass grid=(nx, ny, nz) and dmax=")
        if grid is None:
            grid = default_grid(cells[0], spacing)
        grid = tuple(int(x) for x in grid)
        if len(grid) != 3 or min(grid) < 1 or grid[0] * grid[1] * grid[2] > 2 ** 31 - 1:
            raise ValueError("grid must be three counts >= 1 with at most 2^31 - 1 points")
        rmax = float(rs.max()) if len(rs) else 0.0
        F = len(packed)
        if F:
            if dmax is None:
                dmax = default_dmax(cells, packed.pbc, rmax, dr)
            dmax = float(dmax)
            if not (np.isfinite(dmax) and dmax > 0) or int(np.rint(dmax / dr)) < 1:
                raise ValueError("dmax must be finite, > 0 and at least one bin of dr")
            # (the library's own check, with its relative slack: the default dmax may land on half a height exactly)
            if dmax + rmax > half_height(cells, packed.pbc) * (1.0 + 1e-12):
                raise ValueError("dmax + the largest radius = %g exceeds half the smallest cell height %g: one minimum image "
                                 "would not do" % (dmax + rmax, 2.0 * half_height(cells, packed.pbc)))
        else:
            dmax = float(dmax) if dmax is not None else dr
        nbins, n_t = int(np.rint(dmax / dr)), len(probes)
        mass = float(np.asarray(packed.masses, dtype=np.float64).sum())

        st = _setup.setup(packed, device, distributed, lane=1, keep_stream=True, honour_local=True)
        ctx, source, sharded = st.ctx, st.source, st.sharded
        frame_range = st.shard(F)
        G = grid[0] * grid[1] * grid[2]

        accessibility, free_sphere, psd, surface = bool(accessibility), bool(free_sphere), bool(psd), bool(surface)
        dirs = sphere_points(surface_points) if surface else None
        S, N, M = len(rs), len(packed.numbers), (len(dirs) if surface else 0)
        if surface and F and rmax + max(probes + [0.0]) > half_height(cells, packed.pbc) * (1.0 + 1e-12):
            raise ValueError("the largest radius + the largest probe radius = %g exceeds half the smallest cell height %g: a sample "
                             "sphere would meet its own image" % (rmax + max(probes + [0.0]), 2.0 * half_height(cells, packed.pbc)))
        labelled = accessibility or free_sphere
        want_labels = accessibility and per_point
        if labelled and any(p and n < 3 for p, n in zip(packed.pbc, grid)):
            raise ValueError("accessibility / free_sphere: a periodic grid axis needs at least 3 points, the grid is %s" % (grid,))
        base_cols = nbins + 2 + n_t + 6
        access_cols = base_cols + (4 * n_t if labelled else 0) + (2 if free_sphere else 0)
        psd_cols = access_cols + ((nbins + 2 + n_t + (n_t if accessibility else 0)) if psd else 0)
        cols = psd_cols + (n_t * S * (2 if accessibility else 1) if surface else 0)
        want_cover = psd and per_point
        want_samples = surface and per_point

        def finish_host(raw):
            rows, field, labels, cover, samples = raw
            rows = np.asarray(rows, dtype=np.int64).reshape(-1, cols)
            tail = rows[:, nbins + 2 + n_t:base_cols].copy()
            self._assemble(rows[:, :nbins + 2].copy().view(np.uint64), rows[:, nbins + 2:nbins + 2 + n_t].copy(),
                           tail[:, 0].copy().view(np.float64), tail[:, 1].copy(), tail[:, 2].copy().view(np.float64),
                           tail[:, 3:].copy().view(np.float64), field, step, mass, probes, grid, dr, dmax, rs, kinds)
            if labelled:
                self._assemble_access(rows[:, base_cols:base_cols + 4 * n_t].copy().reshape(-1, n_t, 4),
                                      rows[:, base_cols + 4 * n_t:access_cols].copy().view(np.float64) if free_sphere else None, labels,
                                      accessibility, tail[:, 2].copy().view(np.float64), mass, probes, grid)
            if psd:
                more = rows[:, access_cols:psd_cols]
                self._assemble_psd(more[:, :nbins + 2].copy().view(np.uint64), more[:, nbins + 2:nbins + 2 + n_t].copy(),
                                   more[:, nbins + 2 + n_t:].copy() if accessibility else None, cover,
                                   tail[:, 2].copy().view(np.float64), mass, probes, grid, dr)
            if surface:
                more = rows[:, psd_cols:].copy().reshape(-1, 2 if accessibility else 1, n_t, S)
                self._assemble_surface(more[:, 0], more[:, 1] if accessibility else None, samples, rs, kinds,
                                       tail[:, 2].copy().view(np.float64), mass, probes, M)

        def call(tr, frame_range=None):
            # one int64 row per frame -- histogram, probe counts, the bits of vmax, argmax, the bits of the cell volume and of
            # the position of vmax -- so that one gather merges the ranks
            flags = dict(per_point=per_point, labelled=labelled, free_sphere=free_sphere, labels=want_labels, psd=psd,
                         accessibility=(psd or surface) and accessibility, surface=surface)
            if surface:
                res = ctx.pore_surface(tr, rs, grid, dr, dmax, probes, dirs=dirs, frame_range=frame_range, per_point=per_point,
                                       accessibility=accessibility, free_sphere=free_sphere, labels=want_labels, psd=psd)
            elif psd:
                res = ctx.pore_psd(tr, rs, grid, dr, dmax, probes, frame_range=frame_range, per_point=per_point,
                                   accessibility=accessibility, free_sphere=free_sphere, labels=want_labels)
            elif labelled:
                res = ctx.pore_access(tr, rs, grid, dr, dmax, probes, frame_range=frame_range, per_point=per_point,
                                      free_sphere=free_sphere, labels=want_labels)
            else:
                res = ctx.pore_field(tr, rs, grid, dr, dmax, probes, frame_range=frame_range, per_point=per_point)
            r = _hip.PoreResult(**dict(zip(_hip.pore_names(**flags), res, strict=True)))       # (None: not asked for)
            more = []
            if labelled:
                more += [r.access.reshape(-1, 4 * n_t)] + ([r.free_sphere.view(np.int64)] if free_sphere else [])
            if psd:
                more += [r.psd_hist.view(np.int64), r.po_counts] + ([r.po_access] if accessibility else [])
            if surface:
                more += [r.exposed.reshape(-1, n_t * S)] + ([r.exposed_access.reshape(-1, n_t * S)] if accessibility else [])
            hist, counts, vmax, argmax = r.hist, r.counts, r.vmax, r.argmax
            f0, f1 = (0, len(vmax)) if frame_range is None else frame_range
            c = np.asarray(tr.cell, dtype=np.float64).reshape(-1, 3, 3)
            c = np.broadcast_to(c, (f1 - f0, 3, 3)) if c.shape[0] == 1 else c[f0:f1]
            volume = np.ascontiguousarray(np.abs(np.linalg.det(c)), dtype=np.float64).reshape(-1)
            where = np.ascontiguousarray(positions(argmax, c, grid), dtype=np.float64).reshape(-1, 3)
            rows = np.concatenate([hist.view(np.int64), counts, vmax.view(np.int64)[:, None], argmax[:, None],
                                   volume.view(np.int64)[:, None], where.view(np.int64)] + more, axis=1)
            return rows, r.field, r.labels, r.cover, r.samples

        if _setup.streamed(st):
            def walk():
                keep = [0] + ([1] if per_point else []) + ([2] if want_labels else []) + ([3] if want_cover else []) + ([4] if want_samples else [])

                def kept(batch):
                    res = call(batch)
                    return tuple(res[k] for k in keep)
                got = _setup.walk(source, kept, ("cat",) * len(keep))
                return tuple(got[keep.index(k)] if k in keep else None for k in range(5))

            self._defer(ctx, walk, finish_host)
            return

        def local():
            # this rank's kernels (a lane job: amof_amd/_lazy.py)
            if F == 0:
                return (np.zeros((0, cols), dtype=np.int64), (np.zeros((0,) + grid) if per_point else None),
                        (np.zeros((0, n_t) + grid, dtype=np.int32) if want_labels else None),
                        (np.zeros((0,) + grid) if want_cover else None),
                        (np.zeros((0, n_t, N, M), dtype=np.uint8) if want_samples else None))
            return call(packed, frame_range)

        def finish(raw):
            rows, field, labels, cover, samples = raw
            if sharded:
                rows = _dist.all_gather_rows(rows, device=ctx.device)
                if per_point:
                    field = _dist.all_gather_rows(field.reshape(-1, G).view(np.int64), device=ctx.device).view(np.float64)
                    field = field.reshape((-1,) + grid)
                if want_labels:
                    labels = _dist.all_gather_rows(labels.reshape(-1, n_t * G).astype(np.int64), device=ctx.device)
                    labels = labels.astype(np.int32).reshape((-1, n_t) + grid)
                if want_cover:
                    cover = _dist.all_gather_rows(cover.reshape(-1, G).view(np.int64), device=ctx.device).view(np.float64)
                    cover = cover.reshape((-1,) + grid)
                if want_samples:
                    samples = _dist.all_gather_rows(samples.reshape(-1, n_t * N * M).astype(np.int64), device=ctx.device)
                    samples = samples.astype(np.uint8).reshape((-1, n_t, N, M))
            finish_host((rows, field, labels, cover, samples))

        self._defer(ctx, local, finish, collective=sharded)

    def _assemble(self, counts, probe_counts, vmax, argmax, volume, where, field, step, mass, probes, grid, dr, dmax, radii, kinds):
        self.counts = counts
        self.probe_counts = probe_counts
        self.vmax = vmax
        self.argmax = argmax
        self.di_position = where
        self.grid, self.dr, self.dmax, self.probe_radius = tuple(grid), dr, dmax, list(probes)
        self.radii = {_data.chemical_symbols[int(z)]: float(r) for z, r in zip(kinds, radii)}
        if field is not None:
            self.field = field
        self.data, self.hist = assemble(counts, probe_counts, vmax, step, volume, mass, probes, grid, dr)
        nbins = counts.shape[1] - 2
        over = np.nonzero(counts[:, nbins + 1] > 0)[0]
        if len(over):
            logger.warning("Pore: %d frame(s) have grid points farther than dmax = %g from every atomic surface (first: frame %d); "
                           "Di is inf there -- raise dmax", len(over), dmax, int(over[0]))

    def _assemble_access(self, access, free, labels, accessibility, volume, mass, probes, grid):
        """the columns of ``accessibility`` / ``free_sphere`` behind ``assemble``'s (``access_columns``, ``free_sphere_columns``)"""
        cols = {}
        if accessibility:
            self.access = access
            cols.update(access_columns(access, self.probe_counts, volume, mass, probes, grid))
            if labels is not None:
                self.labels = labels
        if free is not None:
            self.free_sphere = free
            cols.update(free_sphere_columns(free))
        self.data = pd.concat([self.data, pd.DataFrame(cols, index=self.data.index)], axis=1)

    def _assemble_psd(self, psd_counts, po_counts, po_access, cover, volume, mass, probes, grid, dr):
        """the columns and the distribution of ``psd`` behind the others (``psd_columns``)"""
        self.psd_counts, self.po_counts = psd_counts, po_counts
        if po_access is not None:
            self.po_access = po_access
        if cover is not None:
            self.cover = cover
        cols, self.psd = psd_columns(psd_counts, po_counts, po_access, volume, mass, probes, grid, dr)
        self.data = pd.concat([self.data, pd.DataFrame(cols, index=self.data.index)], axis=1)

    def _assemble_surface(self, exposed, exposed_access, samples, radii, kinds, volume, mass, probes, M):
        """the columns of ``surface`` behind the others (``surface_columns``), the areas per element"""
        self.exposed = exposed
        if exposed_access is not None:
            self.exposed_access = exposed_access
        if samples is not None:
            self.surface_samples = samples
        self.surface_points = M
        by = {}
        for s, z in enumerate(kinds):
            only = np.zeros_like(exposed)
            only[:, :, s] = exposed[:, :, s]
            for k, rp in enumerate(probes):
                by[_data.chemical_symbols[int(z)] + "-" + probe_label(rp)] = surface_area(only[:, k], radii, rp, M)
        self.surface_by_species = pd.DataFrame(by, index=self.data.index)
        cols = surface_columns(exposed, exposed_access, radii, volume, mass, probes, M)
        self.data = pd.concat([self.data, pd.DataFrame(cols, index=self.data.index)], axis=1)

    def write_to_file(self, path_to_output):
        """writes ``.data`` to ``<path>.pore`` (feather)"""
        self.data.to_feather(_path.append_suffix(path_to_output, 'pore'))

    @classmethod
    def from_file(cls, path_to_file):
        """constructor from the file ``write_to_file`` wrote"""
        pore = cls()
        pore.data = pd.read_feather(_path.append_suffix(path_to_file, 'pore'))
        return pore
