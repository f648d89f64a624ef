"""The covering radius without a GPU: known answers of the restatement (tests/pore_cover_ref.py) on single-centre fields and
on the simple-cubic frames of tests/pore_access_cases.py, the ABI surface, the columns ``Pore(psd=True)`` derives from the
library's integers, and a two-rank gloo run of the class with ``psd`` and ``accessibility``, its kernels answered by the
restatements."""

import os
import re

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import pore as P
from tests import pore_access_cases as acases
from tests import pore_access_ref as aref
from tests import pore_cover_ref as ref
from tests.conftest import ROOT

CUBE = np.diag([8.0, 8.0, 8.0])


# ---- known answers of the restatement ---------------------------------------------------------------------------------------
def test_single_centre_tie_on_the_sphere():
    """16^3 points over diag(8, 8, 8): step 0.5, and d2 of the offset (3, 4, 0) is 1.5^2 + 2^2 = 6.25 exactly.  A centre of
    v = 2.5 covers the 515 offsets with d2 <= 6.25; one ulp below, the 30 offsets on the sphere drop out."""
    A = ref.step_vectors(CUBE, (16, 16, 16))
    assert ref.offset_d2(A, 3, 4, 0) == 6.25 and ref.offset_d2(A, 0, -5, 0) == 6.25
    field = np.full((16, 16, 16), -1.0)
    field[8, 8, 8] = 2.5
    w = ref.cover(field, CUBE)
    assert (w == 2.5).sum() == 515 and ((w == 2.5) | (w == -1.0)).all()
    assert w[11, 12, 8] == 2.5 and w[11, 12, 9] == -1.0
    field[8, 8, 8] = np.nextafter(2.5, 0.0)
    w = ref.cover(field, CUBE)
    assert (w >= 0.0).sum() == 485 and w[11, 12, 8] == -1.0
    # the same centre next to an open face loses the offsets that leave the grid, and only those
    field = np.full((16, 16, 16), -1.0)
    field[0, 8, 8] = 2.5
    w = ref.cover(field, CUBE, pbc=(False, True, True))
    full = ref.cover(field, CUBE)
    assert (w[:8] == full[:8]).all() and (w[8:] == -1.0).all() and (full[11:] == 2.5).any()
    row = ref.histogram(full, 0.5, 3.0)
    assert row.tolist() == [16 ** 3 - 515, 0, 0, 0, 0, 0, 515, 0]


def test_two_centres_the_larger_wins():
    field = np.full((16, 16, 16), -1.0)
    field[8, 8, 8], field[8, 8, 10] = 1.0, 1.5
    w = ref.cover(field, CUBE)
    assert w[8, 8, 9] == 1.5 and w[8, 8, 8] == 1.5 and w[8, 8, 6] == 1.0 and w[8, 8, 13] == 1.5 and w[8, 8, 14] == -1.0


@pytest.mark.parametrize("c_over", [None, 3.0])
def test_simple_cubic_frames(c_over):
    """a = 4, R = 1 (tests/pore_access_cases.py): a probe of 2.0 is shut into the 27 cages -- it occupies volume, none of it
    reached from a channel"""
    field, _ = acases.simple_cubic_field(c_over)
    pos, cell, grid = acases.simple_cubic(c_over)
    v = field[0]
    w, row, po, acc = ref.psd(v, cell, (True, True, True), acases.SC_DR, acases.SC_DMAX, acases.SC_PROBES, access=True)
    assert (w[v >= 0.0] >= v[v >= 0.0]).all() and (w[v < 0.0] >= v[v < 0.0]).all()
    assert w.max() == v.max()
    for k, t in enumerate(acases.SC_PROBES):
        assert po[k] >= (v >= t).sum() > 0
        assert 0 <= acc[k] <= po[k]
    assert acc[2] == 0 and po[2] > 0
    assert acc[0] == po[0]                      # the void of 1.2 is one channel: whatever is covered is covered from it
    assert int(row.sum()) == v.size and row[0] == (w < 0.0).sum()


# ---- ABI surface ------------------------------------------------------------------------------------------------------------
def test_abi_surface():
    with open(os.path.join(ROOT, "include", "amof_hip.h")) as fh:
        text = fh.read()
    assert re.search(r"\bint amof_pore_psd\(", text) and re.search(r"\bint amof_pore_psd_field\(", text)
    for name in ("amof_pore_psd", "amof_pore_psd_field", "amof_pore_cover_stats"):
        assert name in _hip.EXPORTS
    comment = text[text.index("kernel family that produced"):text.index("const char *amof_last_path")]
    assert '"pore_cover_brick"' in comment and '"pore_cover_exact"' in comment
    assert "which = 5 the covering stage" in text
    assert "#define AMOF_ABI_VERSION 4" in text and _hip.ABI_VERSION == 4
    for cls in (_hip.Context, _hip.MultiContext):
        assert hasattr(cls, "pore_psd") and hasattr(cls, "pore_psd_field")
    with open(os.path.join(ROOT, "amof_amd", "csrc", "Makefile")) as fh:
        assert "pore_cover.hip" in fh.read()


# ---- the columns of the class -----------------------------------------------------------------------------------------------
def test_psd_columns_from_given_integers():
    G, dr = 100, 0.5
    psd = np.array([[40, 10, 20, 30, 0, 0], [50, 0, 10, 20, 15, 5]], dtype=np.uint64)         # [F][nbins + 2], nbins = 4
    po = np.array([[60, 30], [50, 35]])
    acc = np.array([[45, 0], [50, 20]])
    volume = np.array([1000.0, 2000.0])
    cols, dist = P.psd_columns(psd, po, acc, volume, 120.0, [0.0, 1.2], (4, 5, 5), dr)
    assert list(cols) == [x + "_" + y + "-" + rp for rp in ("0", "1.2") for x in ("POV", "POAV", "PONAV")
                          for y in ("Volume_fraction", "A^3", "cm^3/g")]
    assert cols["POV_Volume_fraction-0"].tolist() == [0.6, 0.5] and cols["PONAV_Volume_fraction-1.2"].tolist() == [0.3, 0.15]
    assert cols["POAV_A^3-0"].tolist() == [450.0, 1000.0]
    assert cols["POV_cm^3/g-1.2"].tolist() == pytest.approx([300.0 * 0.602214076 / 120.0, 700.0 * 0.602214076 / 120.0], rel=1e-15)
    for k, rp in enumerate(("0", "1.2")):       # POAV + PONAV == POV in counts
        a = np.rint(cols["POAV_Volume_fraction-" + rp] * G).astype(np.int64)
        b = np.rint(cols["PONAV_Volume_fraction-" + rp] * G).astype(np.int64)
        assert np.array_equal(a + b, po[:, k]) and np.array_equal(a, acc[:, k])
    assert list(dist.columns) == ["r", "density", "cumulative"] and dist["r"].tolist() == [0.25, 0.75, 1.25, 1.75]
    assert dist["density"].tolist() == [(10 / 50 + 0) / 2, (20 / 50 + 10 / 50) / 2, (30 / 50 + 20 / 50) / 2, (0 + 15 / 50) / 2]
    # the cumulative column starts at the covered fraction and never rises; the points with w >= dmax stay in it
    assert dist["cumulative"][0] == ((100 - 40) / 100 + (100 - 50) / 100) / 2
    assert (np.diff(dist["cumulative"].to_numpy()) <= 0).all() and dist["cumulative"].tolist()[-1] == (0.0 + 0.2) / 2
    only, _ = P.psd_columns(psd, po, None, volume, 120.0, [0.0, 1.2], (4, 5, 5), dr)
    assert list(only) == ["POV_" + y + "-" + rp for rp in ("0", "1.2") for y in ("Volume_fraction", "A^3", "cm^3/g")]
    with pytest.raises(ValueError):
        P.psd_columns(psd, po, acc + 100, volume, 120.0, [0.0, 1.2], (4, 5, 5), dr)


# ---- the class over two gloo ranks, the kernels answered by the restatements ----------------------------------------------
CLASS_KW = dict(probe_radius=(0.0, 1.2), grid=(7, 6, 5), dr=0.25, dmax=3.0, per_point=True, accessibility=True, psd=True)


def restated_rows(field, cells, pbc, dr, dmax, thresholds, access):
    """``(psd_hist, po_counts, po_access or None, cover)`` of the restatement for fields ``[F][nx][ny][nz]``"""
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3, 3)
    out = [ref.psd(field[f], cells[0 if len(cells) == 1 else f], pbc, dr, dmax, thresholds, access=access) for f in range(len(field))]
    return (np.array([o[1] for o in out], dtype=np.uint64).reshape(len(field), -1),
            np.array([o[2] for o in out], dtype=np.int64).reshape(len(field), len(thresholds)),
            np.array([o[3] for o in out], dtype=np.int64).reshape(len(field), len(thresholds)) if access else None,
            np.array([o[0] for o in out], dtype=np.float64).reshape(field.shape))


def _install(monkeypatch=None):
    """tests/test_pore_access_host.py's stand-in with ``pore_psd`` answered by tests/pore_cover_ref.py on its field"""
    from tests import test_pore_access_host as H
    lanes = H._install(monkeypatch)
    base = type(lanes[0])

    def pore_psd(self, packed, radii, grid, dr, dmax, thresholds=(), frame_range=None, per_point=False, accessibility=False,
                 free_sphere=False, labels=False):
        labelled = accessibility or free_sphere
        if labelled:
            res = base.pore_access(self, packed, radii, grid, dr, dmax, thresholds, frame_range=frame_range, per_point=True,
                                   free_sphere=free_sphere, labels=labels)
            field = res[5 + bool(free_sphere)]
        else:
            res = base.pore_field(self, packed, radii, grid, dr, dmax, thresholds, frame_range=frame_range, per_point=True)
            field = res[4]
        self.calls[-1] = "psd"
        if not per_point:
            res = tuple(x for x in res if x is not field)
        _, cell = self._frames(packed, frame_range)
        hist, po, acc, cover = restated_rows(field, cell, tuple(bool(x) for x in packed.pbc), dr, dmax, thresholds, accessibility)
        return res + (hist, po) + ((acc,) if accessibility else ()) + ((cover,) if per_point else ())

    if monkeypatch is not None:
        monkeypatch.setattr(base, "pore_psd", pore_psd, raising=False)
    else:
        base.pore_psd = pore_psd            # (a spawned worker: the process ends with it)
    return lanes


def _worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from tests import pore_cases
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lanes = _install()
    obj = P.Pore.from_trajectory(pore_cases.case("npt_sheared").packed, delta_Step=10, **CLASS_KW)
    data = obj.data
    assert lanes[1].calls == ["psd"] and lanes[0].calls == []
    if rank == 0:
        data.to_pickle(os.path.join(out_dir, "data.pkl"))
        obj.psd.to_pickle(os.path.join(out_dir, "psd.pkl"))
        np.savez(os.path.join(out_dir, "raw.npz"), psd_counts=obj.psd_counts, po_counts=obj.po_counts, po_access=obj.po_access,
                 cover=obj.cover, field=obj.field, labels=obj.labels)
    dist.barrier()
    dist.destroy_process_group()


def test_class_sharded_over_two_ranks_equals_one_process(tmp_path, monkeypatch):
    import pandas as pd
    import torch.multiprocessing as mp
    from tests import pore_cases
    port = 27500 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    lanes = _install(monkeypatch)
    packed = pore_cases.case("npt_sheared").packed
    one = P.Pore.from_trajectory(packed, delta_Step=10, distributed=False, **CLASS_KW)
    assert pd.read_pickle(os.path.join(str(tmp_path), "data.pkl")).equals(one.data)
    assert pd.read_pickle(os.path.join(str(tmp_path), "psd.pkl")).equals(one.psd)
    raw = np.load(os.path.join(str(tmp_path), "raw.npz"))
    for name in ("psd_counts", "po_counts", "po_access", "cover", "field", "labels"):
        mine = getattr(one, name)
        assert raw[name].dtype == mine.dtype and np.array_equal(raw[name], mine), name
    assert one.cover.shape == (4, 7, 6, 5) and one.psd_counts.shape == (4, 14) and one.psd_counts.dtype == np.uint64
    assert one.po_counts.shape == one.po_access.shape == (4, 2)
    # the new columns are the helper's on the restated integers, behind the columns of accessibility alone
    plain = P.Pore.from_trajectory(packed, delta_Step=10, distributed=False, **dict(CLASS_KW, psd=False))
    base = list(plain.data.columns)
    assert one.data[base].equals(plain.data) and not hasattr(plain, "psd") and not hasattr(plain, "cover")
    mass = float(np.asarray(packed.masses, dtype=np.float64).sum())
    cols, dist = P.psd_columns(one.psd_counts, one.po_counts, one.po_access, plain.data["Unitcell_volume"].to_numpy(), mass, [0.0, 1.2],
                               (7, 6, 5), 0.25)
    assert list(one.data.columns) == base + list(cols) and dist.equals(one.psd)
    for name, col in cols.items():
        assert np.array_equal(one.data[name].to_numpy(), col), name
    assert (one.po_counts >= one.probe_counts).all() and (one.po_access <= one.po_counts).all() and (one.psd_counts.sum(axis=1) == 210).all()
    assert ((one.cover >= one.field) | (one.field < 0)).all()
    # without accessibility: the POV columns alone, the field tier's call
    bare = P.Pore.from_trajectory(packed, delta_Step=10, distributed=False, **dict(CLASS_KW, accessibility=False, per_point=False))
    first = list(P.Pore.from_trajectory(packed, delta_Step=10, distributed=False, probe_radius=(0.0, 1.2), grid=(7, 6, 5), dr=0.25,
                                        dmax=3.0).data.columns)
    assert list(bare.data.columns) == first + ["POV_" + y + "-" + rp for rp in ("0", "1.2") for y in ("Volume_fraction", "A^3", "cm^3/g")]
    assert np.array_equal(bare.po_counts, one.po_counts) and not hasattr(bare, "po_access") and not hasattr(bare, "cover")
    for ctx in lanes.values():
        ctx.close_lane()


def test_class_walks_a_stream_batch_by_batch(tmp_path, monkeypatch):
    from amof_amd import trajectory as T
    from amof_amd.stream import XyzStream
    from tests import pore_cases
    lanes = _install(monkeypatch)
    packed = pore_cases.case("sheared").packed
    path = str(tmp_path / "s.xyz")
    T.write_xyz(path, packed, comment_lattice=False, fmt="%.17g")
    kw = dict(CLASS_KW, distributed=False)
    whole = P.Pore.from_trajectory(packed, **kw)
    walked = P.Pore.from_trajectory(XyzStream(path, cell=packed.cell[0], batch_frames=2, pinned=False), **kw)
    assert walked.data.equals(whole.data) and walked.psd.equals(whole.psd)
    for name in ("psd_counts", "po_counts", "po_access", "cover", "field", "labels"):
        assert np.array_equal(getattr(walked, name), getattr(whole, name)), name
    assert lanes[1].calls == ["psd"] * 3
    for ctx in lanes.values():
        ctx.close_lane()
