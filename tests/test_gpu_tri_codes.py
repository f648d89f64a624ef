"""Every variant of the general-cell tile kernel ("rdf_tile_tri": near modes 0 .. 4, the x wrap with the y term, the
exact-half forms; each with and without slab culling) on pairs planted on the image decisions it makes
(tests/tri_plant.py): bit-exact against the C oracle.

A wrong near threshold, x wrap or twin choice loses or doubles a periodic image of exactly the pairs that sit on that
decision; random walks hold a handful of them, the guard-band cells of test_gpu_guard_band.py all run code 0.  Here
every reachable (code, culling) has a cell (pinned to the selection on the CPU by tests/test_tri_select_cpu.py), most
atoms are pairs within 1e-3 of the cell of a decision -- on it, a few grid units either side -- with a distance at a bin
edge or the cutoff, and the code that ran is read back from the library's debug line: a silent fall to another variant
fails the test.  The debug line does not say whether the culled or the unculled instantiation ran: that a cell takes
culling by itself rests on the CPU table's restatement of the host's rule (2 * 1.05 * rmax < the slab axis's smallest
height); both forms run here for every cell and both must equal the oracle."""

import functools
import os
import re

import numpy as np
import pytest

from amof_amd.frames import PackedTrajectory
from oracle import clib
from tests import edge_plant as E
from tests import tri_plant as T

pytestmark = pytest.mark.gpu

TILE = {"AMOF_RDF_NOCELL": "1", "AMOF_RDF_NORANGE": "1", "AMOF_RDF_DEBUG": "1"}
LINE = re.compile(r"rdf_tile_tri: code (\d+) \(near mode (\d), x wrap (\d)\) axes \((\d), (\d) \| (\d)\)")


class _env(object):
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _case(name, nbins):
    """the planted trajectory and the oracle's histogram, once per (case, nbins)"""
    pl = T.plant_tri(name, nbins, seed=nbins)
    packed = pl.packed
    kinds, sp = E._species(packed.numbers)
    ref, _ = clib.rdf_hist(packed.pos, packed.cell, sp, len(kinds), T.case_rmax(name), nbins, cell_list=True)
    ref.setflags(write=False)
    assert ref.sum() > 0
    return packed, ref


def _same(got, ref, what):
    bad = np.argwhere(got != ref)
    if len(bad):
        s, t, b = (int(x) for x in bad[0])
        total = int(np.abs(got.astype(np.int64) - ref.astype(np.int64)).sum())
        print("%s: sum |diff| = %d over %d entries; first (pair, bin) = ((%d, %d), %d): got %d, oracle %d"
              % (what, total, len(bad), s, t, b, int(got[s, t, b]), int(ref[s, t, b])))
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist())


PARAMS = [(name, nb) for name in T.CASES for nb in T.NBINS] + sorted(T.NBINS_BIG.items())


def test_parametrisation_covers_every_reachable_variant():
    have = {(T.CASES[n]["expect"][0], T.CASES[n]["expect"][4]) for n, _ in PARAMS}
    assert have == {(code, cull) for code in (0, 1, 2, 4, 5, 6, 7, 9, 10, 11) for cull in (0, 1)} | {(3, 0), (8, 0)}
    assert sum(nb == 31744 for _, nb in PARAMS) == 2 and len(T.DEVICE_INPUT) == 3


@pytest.mark.parametrize("name,nbins", PARAMS)
def test_rdf_tri_variant_on_planted_image_decisions(hip_ctx, capfd, name, nbins):
    case = T.CASES[name]
    code, ax0, ax1, axis, _cull = case["expect"]
    rmax = T.case_rmax(name)
    packed, ref = _case(name, nbins)
    inputs = [("host", packed)]
    if name in T.DEVICE_INPUT:
        import torch
        inputs.append(("device", PackedTrajectory(torch.as_tensor(packed.pos).cuda(), packed.cell, packed.numbers)))
    env = dict(TILE, AMOF_RDF_NOHALF="1") if case.get("nohalf") else TILE
    for label, inp in inputs:
        for extra in ({}, {"AMOF_RDF_NOCULL": "1"}):
            with _env(**dict(env, **extra)):
                capfd.readouterr()
                got, _, _ = hip_ctx.rdf_accumulate(inp, rmax, nbins)
                ran = hip_ctx.last_path()
                err = capfd.readouterr().err
            assert ran == "rdf_tile_tri", (name, nbins, extra, ran)
            m = LINE.search(err)
            assert m, err
            assert int(m.group(1)) == code, (name, nbins, extra, m.group(0))
            assert (int(m.group(4)), int(m.group(5)), int(m.group(6))) == (ax0, ax1, axis), (name, m.group(0))
            assert int(m.group(2)) == (4 if code >= 10 else code % 5) and int(m.group(3)) == (2 if code >= 10 else code // 5)
            _same(got, ref, "%s nbins %d %s %s code %d" % (name, nbins, label, "NOCULL" if extra else "as selected", code))
    # whatever kernel answers without the variant gives the same integers
    with _env(**dict(env, AMOF_RDF_NOTRI="1")):
        old, _, _ = hip_ctx.rdf_accumulate(packed, rmax, nbins)
        ran = hip_ctx.last_path()
    assert ran != "rdf_tile_tri", ran
    _same(old, ref, "%s nbins %d AMOF_RDF_NOTRI (%s)" % (name, nbins, ran))
