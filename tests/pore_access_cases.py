"""The inputs of tests/test_gpu_pore_access.py, importable without a GPU: fields of +-1 (no decision is near a threshold)
whose void has a known topology, handed to the labelling kernels through ``Context.pore_access_field``, and the simple-cubic
frames with known free spheres.  tests/test_pore_access_host.py asserts the topologies on the restatement
(tests/pore_access_ref.py).  Grids: at most 40 points per axis but for one of 70, 15 to 18 tiles of 8 x 8 x 32, a ragged one
(19 x 21 x 35), an axis of 3 points, an open axis of 1 point."""

import functools

import numpy as np

from tests import pore_access_ref as ref

TILE = (8, 8, 32)           # amof_amd/csrc/pore_access.hip PA_TX, PA_TY, PA_TZ
EVEN = (24, 24, 40)         # 3 x 3 x 2 tiles, every count even (the checkerboard closes through the faces), nx == ny (staircases)
RAGGED = (19, 21, 35)       # 3 x 3 x 2 tiles, none full along any axis
THIN = (3, 33, 70)          # the smallest periodic axis
SLAB = (1, 40, 70)          # one layer, open along x
PBC = (True, True, True)

Case = type("Case", (), {})


def _case(name, field, pbc=PBC, thresholds=(0.0,), **known):
    c = Case()
    c.name, c.pbc, c.thresholds, c.known = name, tuple(pbc), tuple(float(t) for t in thresholds), known
    c.field = np.ascontiguousarray(field, dtype=np.float64)[None]           # one frame
    c.grid = c.field.shape[1:]
    c.field.setflags(write=False)
    return c


def _field(n, points, inside=1.0, outside=-1.0):
    f = np.full(n, outside)
    for p in points:
        f[tuple(x % m for x, m in zip(p, n))] = inside
    return f


def lin(n, p):
    return (p[0] * n[1] + p[1]) * n[2] + p[2]


def serpentine(n):
    """one component through every tile: in every odd layer i the rows j of the parity of ny - 1, whole along k and joined
    at alternating ends; consecutive odd layers joined through one point; and the single point (0, ny - 1, nz - 1) on top of
    layer 1 -- the smallest index of the component, in the last tile of the first tile layer"""
    nx, ny, nz = n
    par = (ny - 1) % 2
    pts = [(0, ny - 1, nz - 1)]
    rows = [j for j in range(ny) if j % 2 == par]
    for i in range(1, nx, 2):
        for r, j in enumerate(rows):
            pts += [(i, j, k) for k in range(nz)]
            if r + 1 < len(rows):
                pts.append((i, j + 1, nz - 1 if r % 2 == 0 else 0))
        if i + 2 < nx:
            pts.append((i + 1, rows[0], 0))
    return _field(n, pts)


def staircase(n, k0, dj=1, j0=0):
    """(s, j0 + dj s, k0), (s + 1, j0 + dj s, k0) for s = 0 .. nx - 1 (nx == ny): closes after nx steps with winding (1, dj, 0)"""
    assert n[0] == n[1]
    return [p for s in range(n[0]) for p in ((s, j0 + dj * s, k0), (s + 1, j0 + dj * s, k0))]


def u_shape(n, j0, k0):
    """leaves through the upper x face, turns and comes back through the same face: net winding 0"""
    nx = n[0]
    return [(nx - 2, j0, k0), (nx - 1, j0, k0), (0, j0, k0), (1, j0, k0), (1, j0 + 1, k0), (1, j0 + 2, k0), (0, j0 + 2, k0),
            (nx - 1, j0 + 2, k0), (nx - 2, j0 + 2, k0)]


def helix(n, i0, j0):
    """one closed path that leaves through the upper z face twice before it closes: winding (0, 0, 2).  Column A at (i0, j0)
    lands on (i0, j0, 0), crosses to column B at (i0 + 2, j0), which moves over to (i0 + 2, j0 + 2) below the top, lands on
    (i0 + 2, j0 + 2, 0), crosses to (i0, j0 + 2), rises two points and joins the foot of column A at k = 2."""
    nz = n[2]
    assert nz >= 8
    pts = [(i0, j0, k) for k in range(2, nz)]                                   # A
    pts += [(i0, j0, 0), (i0 + 1, j0, 0)] + [(i0 + 2, j0, k) for k in range(0, nz - 2)]             # landing, bridge, B
    pts += [(i0 + 2, j0 + 1, nz - 3)] + [(i0 + 2, j0 + 2, k) for k in range(nz - 3, nz)]            # over to D, up to the face
    pts += [(i0 + 2, j0 + 2, 0), (i0 + 1, j0 + 2, 0)] + [(i0, j0 + 2, k) for k in range(0, 3)]      # landing, bridge, C
    pts += [(i0, j0 + 1, 2)]                                                    # C to the foot of A
    return pts


def box(lo, edge):
    return [(lo[0] + a, lo[1] + b, lo[2] + c) for a in range(edge) for b in range(edge) for c in range(edge)]


def _random(n, density, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n) < density, 1.0, -1.0)


T0 = 0.3


@functools.lru_cache(maxsize=None)
def case(name):
    n = EVEN
    if name == "serpentine":
        return _case(name, serpentine(n), label=lin(n, (0, n[1] - 1, n[2] - 1)))
    if name == "serpentine_ragged":
        return _case(name, serpentine(RAGGED), label=lin(RAGGED, (0, RAGGED[1] - 1, RAGGED[2] - 1)))
    if name == "staircase":
        return _case(name, _field(n, staircase(n, 5)), row=[2 * n[0], 1, 0, 1])
    if name == "two_staircases_cross":
        return _case(name, _field(n, staircase(n, 5) + staircase(n, 5, dj=-1)), row=[4 * n[0] - 4, 1, 0, 2])
    if name == "u_shape":
        return _case(name, _field(RAGGED, u_shape(RAGGED, 4, 33)), row=[0, 0, 1, 0])
    if name == "helix":
        return _case(name, _field(RAGGED, helix(RAGGED, 7, 7)), row=[2 * RAGGED[2] + 8, 1, 0, 1])
    if name == "interleaved":
        return _case(name, _field(n, staircase(n, 5) + staircase(n, 5, j0=3)), row=[4 * n[0], 2, 0, 1])
    if name == "boxes":
        return _case(name, _field(RAGGED, box((-2, -2, -2), 4) + box((9, 10, 30), 3)), row=[0, 0, 2, 0])
    if name == "checkerboard":
        i, j, k = np.indices(n)
        return _case(name, np.where((i + j + k) % 2 == 0, 1.0, -1.0), row=[0, 0, n[0] * n[1] * n[2] // 2, 0])
    if name == "all_void":
        return _case(name, np.ones(RAGGED), row=[RAGGED[0] * RAGGED[1] * RAGGED[2], 1, 0, 3])
    if name == "all_solid":
        return _case(name, -np.ones(RAGGED), row=[0, 0, 0, 0])
    if name == "inclusive":
        # a straight channel along z whose bottleneck point holds T0: a channel at T0, a pocket just above
        f = _field(RAGGED, [(5, 6, k) for k in range(RAGGED[2])])
        f[5, 6, 17] = T0
        return _case(name, f, thresholds=(T0, np.nextafter(T0, np.inf)), rows=[[RAGGED[2], 1, 0, 1], [0, 0, 1, 0]])
    if name == "thin_column":
        # winds through the axis of three points
        return _case(name, _field(THIN, [(a, 9, 40) for a in range(3)] + box((0, 20, 60), 2)), row=[3, 1, 1, 1])
    if name == "thin_random":
        return _case(name, _random(THIN, 0.45, 3))
    if name == "slab_open_axis":
        return _case(name, np.ones(SLAB), pbc=(False, True, True), row=[SLAB[1] * SLAB[2], 1, 0, 2])
    if name == "slab_random":
        return _case(name, _random(SLAB, 0.62, 5), pbc=(False, True, True))
    if name == "open_box":
        # nothing is periodic: the staircase that winds in a periodic cell is a pocket here
        return _case(name, _field(n, staircase(n, 5)), pbc=(False, False, False))
    if name == "random_sparse":
        return _case(name, _random(RAGGED, 0.3, 7))
    if name == "random_dense":
        return _case(name, _random(RAGGED, 0.7, 9), pbc=(True, False, True))
    raise KeyError(name)


NAMES = ["serpentine", "serpentine_ragged", "staircase", "two_staircases_cross", "u_shape", "helix", "interleaved", "boxes",
         "checkerboard", "all_void", "all_solid", "inclusive", "thin_column", "thin_random", "slab_open_axis", "slab_random",
         "open_box", "random_sparse", "random_dense"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """``(access [1][n_t][4], labels [1][n_t][nx][ny][nz], free_sphere [1][2])`` of the restatement, computed once per process"""
    c = case(name)
    rows, labels = ref.access(c.field[0], c.thresholds, c.pbc)
    free = np.array([ref.free_sphere(c.field[0], c.pbc)], dtype=np.float64)
    out = (rows[None], labels[None], free)
    for a in out:
        a.setflags(write=False)
    return out


# ---- simple-cubic frames with known free spheres ---------------------------------------------------------------------------
SC_A, SC_R, SC_DR, SC_DMAX = 4.0, 1.0, 0.1, 3.0
SC_PROBES = (1.2, 1.6, 2.0)


def simple_cubic(c_over=None):
    """``(positions [1][27][3], cell, grid)``: 3 x 3 x 3 sites, a = 4 (c = 3 along z with ``c_over=3.0``), two grid points
    per Angstrom, the atoms shifted by half a grid step so that they, the face centres and the body centres are grid points"""
    c = SC_A if c_over is None else float(c_over)
    sites = np.array([(i * SC_A, j * SC_A, k * c) for i in range(3) for j in range(3) for k in range(3)], dtype=np.float64) + 0.25
    cell = np.diag([3 * SC_A, 3 * SC_A, 3 * c])
    grid = (24, 24, int(round(6 * c)))
    return sites[None], cell, grid


def simple_cubic_field(c_over=None):
    """the capped field of the frame by tests/pore_ref.py"""
    from tests import pore_ref
    pos, cell, grid = simple_cubic(c_over)
    res, _ = pore_ref.pore(pos, cell, np.full(27, 30), {30: SC_R}, grid, SC_DR, SC_DMAX, SC_PROBES)
    return res.field.reshape((1,) + grid), res.worst
