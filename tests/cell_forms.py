"""Test infrastructure (the package never imports it): the forms a cell can be stored in besides the two the rest of the
suite uses (positive diagonal; lower-triangular, right-handed, positive diagonal), and the library's view of a form.

Rows are lattice vectors.  Every form describes the same lattice up to a rigid motion or a relabelling of its vectors,
so every pair distance a planting puts in it is what it would be in the base cell; what changes is which of the nine
entries are non-zero, their signs, the handedness and the order of the rows -- everything the kernels multiply by.

  rot        C Q                    full matrix, right-handed
  mirror     C diag(1, 1, -1)       left-handed; a diagonal base stays "ortho" with one negative entry
  rotmirror  C Q diag(-1, 1, 1)     full matrix, left-handed
  negrow     second row negated     left-handed, c10 = L10 / L00 of the metric's lower factor changes sign
  negall     -C                     left-handed, every entry negated
  perm       C[[1, 2, 0]]           a diagonal base: orthogonal, but not diagonal in storage

Per-frame cells ([F][3][3]) are transformed frame by frame."""

import numpy as np

# one fixed proper rotation: the Q of numpy's QR of default_rng(5).normal(size=(3, 3)) (the first seed whose Q has no entry
# below 0.15 in magnitude; det +1), written out so that it does not depend on the generator
Q = np.array([[-0.7559716855415088, -0.1834403985228726, -0.6283760266347689],
              [0.39634897110789685, -0.892242061511047, -0.21635987791692918],
              [-0.5209743791792852, -0.412618133217975, 0.7472161483657]])

FORMS = ("rot", "mirror", "rotmirror", "negrow", "negall", "perm")


def apply(cell, form):
    """the cell (3 x 3, or [F][3][3]) in the given form; None: unchanged"""
    c = np.asarray(cell, dtype=np.float64)
    if form is None:
        return c.copy()
    if form == "rot":
        return c @ Q
    if form == "mirror":
        return c @ np.diag([1.0, 1.0, -1.0])
    if form == "rotmirror":
        return c @ Q @ np.diag([-1.0, 1.0, 1.0])
    if form == "negrow":
        out = c.copy()
        out[..., 1, :] = -out[..., 1, :]
        return out
    if form == "negall":
        return -c
    if form == "perm":
        return c[..., [1, 2, 0], :].copy()
    raise ValueError("unknown cell form %r" % (form,))


def view(cell):
    """what the library sees: all_ortho (every off-diagonal entry of every frame exactly zero, as geom_one in ctx.hip
    decides it), the handedness (sign of the determinant; the same in every frame), the count of non-zero entries (the
    smallest over the frames) and whether a diagonal entry is negative"""
    c = np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    off = ~np.eye(3, dtype=bool)
    det = np.linalg.det(c)
    assert np.all(det > 0) or np.all(det < 0)
    return dict(all_ortho=bool(np.all(c[:, off] == 0.0)), hand=1 if det[0] > 0 else -1,
                nonzero=int(min(np.count_nonzero(x) for x in c)),
                neg_diag=bool(np.any(c[:, np.arange(3), np.arange(3)] < 0.0)))


def expected_view(base, form):
    """the view `form` of the cell `base` has by the table above, derived from the base's own view: what every test
    asserts it is exercising"""
    b = view(base)
    hand = b["hand"] * (1 if form in (None, "rot", "perm") else -1)
    if form in ("rot", "rotmirror"):
        return dict(all_ortho=False, hand=hand, nonzero=9)
    ortho = b["all_ortho"] and form != "perm"
    return dict(all_ortho=ortho, hand=hand, nonzero=b["nonzero"])


def check(base, form):
    """the transformed cell, after asserting that it is what the form claims"""
    c = apply(base, form)
    v, want = view(c), expected_view(base, form)
    for k, x in want.items():
        assert v[k] == x, (form, k, v, want)
    if form in ("mirror", "negrow", "negall") and want["all_ortho"]:
        assert v["neg_diag"], (form, v)
    # the same lattice: the metric is the base's (row order and row signs apart)
    b = np.asarray(base, dtype=np.float64).reshape(-1, 3, 3)
    g0 = np.abs(b @ b.transpose(0, 2, 1))
    g1 = np.abs(c.reshape(-1, 3, 3) @ c.reshape(-1, 3, 3).transpose(0, 2, 1))
    if form == "perm":
        g0 = g0[:, [1, 2, 0]][:, :, [1, 2, 0]]
    assert np.allclose(g0, g1, rtol=1e-13, atol=1e-11), form
    return c


# ------------------------------------------------- the cells of tests/test_gpu_cell_forms.py, shared with the CPU test --
# (the base cells of tests/test_gpu_guard_band.py, so that a form differs from a tested case in its storage alone)

DIAG = np.diag([17.31, 18.93, 41.77])
SHEARED = np.array([[17.31, 0.0, 0.0], [2.93, 18.11, 0.0], [-1.71, 3.37, 29.53]])
HIGH_KAPPA = np.array([[31.7, 0.0, 0.0], [0.0, 29.3, 0.0], [83.1, 79.7, 30.9]])
THIN = {"diagonal": np.diag([14.73, 43.31, 52.93]),
        "sheared": np.array([[14.73, 0, 0], [1.9, 43.31, 0], [-2.2, 3.1, 52.93]])}
WIDE = {"diagonal": np.diag([31.37, 33.71, 35.93]),
        "sheared": np.diag([31.37, 33.71, 35.93]) + np.array([[0, 0, 0], [2.3, 0, 0], [-1.9, 2.7, 0]])}
NBR_BASE = np.diag([21.31, 23.73, 26.91])
NBR_SHEAR = np.array([[0, 0, 0], [3.1, 0, 0], [-2.3, 2.9, 0]])
NBR_NPT_SHEAR = np.array([[0, 0, 0], [1.7, 0, 0], [0, -2.1, 0]])

RDF_NBINS = (999, 2310)
RDF_RMAX = {"diagonal": 8.0, "sheared": 6.5}        # tile paths and rdf_exact
RDF_RMAX_NPT = {"diagonal": 7.9, "sheared": 6.3}
RMAX_THIN, RMAX_WIDE, RMAX_HIGH_KAPPA = 5.3, 5.5, 4.2

# (base, form) of the RDF tests.  A diagonal base under `mirror` / `negall` keeps the ortho flag and takes the diagonal
# kernels (rdf_tile_zf, rdf_tile_img, ...); every other pair is a general cell to the library (rdf_tile_tri, ...).
ORTHO_FORMS = [("diagonal", "mirror"), ("diagonal", "negall")]
GENERAL_FORMS = [("diagonal", "rot"), ("diagonal", "perm")] + [("sheared", f) for f in FORMS]


def npt(cell, F, amp, seed):
    """per-frame cells: the cell breathing by up to +-amp"""
    rng = np.random.default_rng(seed)
    return np.stack([cell * (1.0 + amp * rng.uniform(-1, 1)) for _ in range(F)])


def nbr_cell(kind):
    """the three cells of test_gpu_guard_band.py::test_cn_bad_paths"""
    return {"diagonal": NBR_BASE, "sheared": NBR_BASE + NBR_SHEAR, "npt": npt(NBR_BASE + NBR_NPT_SHEAR, 5, 0.015, 8)}[kind]
