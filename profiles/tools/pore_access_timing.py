"""Timings of amof_pore_access on the headline shape (profiles/pore/pore_access_timing.md).

    python profiles/tools/pore_access_timing.py [--frames 50] [--free-frames 4] [--out profiles/pore]     # GPU: json + md
    python profiles/tools/pore_access_timing.py --report                                                   # md from the json

The first ``frames`` frames of the bench's random walk (9792 atoms, 3 x 3 x 4 ZIF-4 cells) resident in HBM, the grid of
spacing 0.2 A (232 x 232 x 369), table radii, dr = 0.05, the default dmax, probes 0 and 1.2 A -- the shape of
profiles/tools/pore_timing.py.  Median of five warm calls after one cold call, the library's own HIP events
(amof_last_kernel_seconds): 0 = the whole call of amof_pore_field (the field alone), 4 = the labelling stage of
amof_pore_access.  The labelling stage's events enclose its kernels, its device-to-host copies of the wrap links and the
component list, and the host's winding resolver between them: it is the time a frame's labelling adds to the call, not kernel
time alone.  Two thresholds per frame: "one labelling" is that stage over 2 x frames.  The LDS path ("pore_label_tile") and
AMOF_PORE_LABEL_GLOBAL=1 ("pore_label_global") alternate in one process and their results are compared bit for bit.  The
free-sphere search runs on the first ``free-frames`` frames: its time is the labelling stage with the search minus without,
its labellings are amof_last_kernel_launches minus the two of the thresholds.

A labelling pass reads the field (8 G bytes) and writes the parents (4 G bytes): 12 G bytes over the time of one labelling,
against 8 TB/s (MI355X_MICROARCH.md), is the share of the HBM peak the table gives -- a lower bound on the traffic (merge,
flatten and counting passes read and write the parents again).  Wrap links and components are counted from the results of
frame 0 (numpy, from the field and the access rows)."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
GLOBAL = {"AMOF_PORE_LABEL_GLOBAL": "1"}


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v), "all": v}


class Env(object):
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


def timed(ctx, fn, env, which):
    with Env(**env):
        t0 = time.perf_counter()
        res = fn()
        wall = time.perf_counter() - t0
        with ctx._lock:
            secs = [ctx._lib.amof_last_kernel_seconds(ctx._h, w) for w in which]
            launches = int(ctx._lib.amof_last_kernel_launches(ctx._h))
        path = ctx.last_path()
    return res, [wall] + secs, launches, path


def wrap_links(void, pbc):
    """pairs of void points through the periodic faces of one frame's mask"""
    n = 0
    for ax in range(3):
        if pbc[ax]:
            lo = np.take(void, 0, axis=ax)
            hi = np.take(void, void.shape[ax] - 1, axis=ax)
            n += int((lo & hi).sum())
    return n


def render(d):
    sh = d["shape"]
    G = sh["points"]
    L = ["# amof_pore_access on the headline shape\n"]
    L.append("Written by `profiles/tools/pore_access_timing.py` (its docstring says what is timed and how) from "
             "`pore_access_timing.json` beside this file; one MI355X, trajectory resident in HBM.  Shape: the first %d frames of the "
             "bench's random walk, %d atoms, grid %d x %d x %d = %s points, probes 0 and 1.2 A, dmax = %g A.  Median of five warm "
             "calls; per frame.\n" % (sh["frames"], sh["atoms"], sh["grid"][0], sh["grid"][1], sh["grid"][2], format(G, ","), sh["dmax"]))
    L.append("| what | per frame | min .. max of the five calls, per frame |")
    L.append("|---|---|---|")
    f = d["field"]
    L.append("| the field alone (`amof_pore_field`, whole call) | %.2f ms | %.2f .. %.2f ms |" % (f["median"] * 1e3, f["min"] * 1e3, f["max"] * 1e3))
    for key, name in (("tile", "one labelling, `pore_label_tile` (LDS tiles of 8 x 8 x 32)"),
                      ("global", "one labelling, `pore_label_global` (`AMOF_PORE_LABEL_GLOBAL=1`)")):
        r = d[key]
        L.append("| %s | %.2f ms | %.2f .. %.2f ms |" % (name, r["median"] * 1e3, r["min"] * 1e3, r["max"] * 1e3))
    fs = d["free_sphere"]
    L.append("| the free-sphere search (`%s`, %d frames) | %.1f ms | %.1f .. %.1f ms |\n"
             % (fs["path"], fs["frames"], fs["median"] * 1e3, fs["min"] * 1e3, fs["max"] * 1e3))
    L.append("The free-sphere search took %.1f labellings per frame (bisection over the sorted field, then one full labelling at t*; "
             "log2 G = %.1f).  Frame 0: t* = %.4f A, Dif / 2 = %.4f A.\n" % (fs["labellings_per_frame"], np.log2(G), fs["tstar_frame0"], fs["dif_half_frame0"]))
    L.append("One labelling must move 12 G = %.0f MB (8 G read, 4 G written): at the times above that is %.1f %% (`pore_label_tile`) and "
             "%.1f %% (`pore_label_global`) of the 8 TB/s HBM peak -- the stage also waits for its own copies to the host and for the "
             "host's resolver, which the events enclose.\n" % (12.0 * G / 1e6, d["tile"]["hbm_share"] * 100, d["global"]["hbm_share"] * 100))
    L.append("The two paths' results (access rows of all frames): identical = %s.  `pore_label_tile` %s `pore_label_global` in this table "
             "(ratio %.2f).\n" % (d["identical"], "is not slower than" if d["tile"]["median"] <= d["global"]["median"] else "IS SLOWER THAN",
                                  d["tile"]["median"] / d["global"]["median"]))
    c = d["counts"]
    L.append("Frame 0, per probe radius (0, 1.2 A): wrap links %s; components %s (channels %s, pockets %s); accessible points %s of %s in "
             "the void; largest channel dimension %s.\n" % (c["wrap_links"], c["components"], c["channels"], c["pockets"], c["accessible"],
                                                            c["void"], c["dimension"]))
    return "\n".join(L)


def write(out_dir, d):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "pore_access_timing.json"), "w") as fh:
        json.dump(d, fh, indent=1, sort_keys=True)
        fh.write("\n")
    with open(os.path.join(out_dir, "pore_access_timing.md"), "w") as fh:
        fh.write(render(d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--free-frames", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pore"))
    ap.add_argument("--report", action="store_true", help="no GPU: render the markdown from the JSON")
    a = ap.parse_args()
    if a.report:
        with open(os.path.join(a.out, "pore_access_timing.json")) as fh:
            write(a.out, json.load(fh))
        return

    import torch
    from amof_amd import _hip
    from amof_amd import pore as P
    from tests import helpers as H

    traj = H.device_walk(torch.device("cuda", 0), (3, 3, 4), a.frames, 0.05, 20261003)
    torch.cuda.synchronize()
    ctx = _hip.get_context(0)
    kinds, _ = _hip.packed_species(traj)
    radii = P.species_radii(kinds)
    grid = P.default_grid(traj.cell[0], 0.2)
    dr = 0.05
    dmax = P.default_dmax(traj.cell, traj.pbc, float(radii.max()), dr)
    probes = (0.0, 1.2)
    args = (radii, grid, dr, dmax, probes)
    G = grid[0] * grid[1] * grid[2]
    F, FF = a.frames, min(a.free_frames, a.frames)
    out = {"shape": {"atoms": int(traj.n_atoms), "frames": F, "grid": list(grid), "points": G, "dmax": dmax, "probes": list(probes)}}

    def field():
        return ctx.pore_field(traj, *args, frame_range=(0, F))

    def access(frames=F, free=False):
        return ctx.pore_access(traj, *args, frame_range=(0, frames), free_sphere=free)

    timed(ctx, field, {}, (0,))
    timed(ctx, access, {}, (4,))
    timed(ctx, access, GLOBAL, (4,))
    timed(ctx, lambda: access(FF, True), {}, (4,))
    rows = {"field": [], "tile": [], "global": [], "free": [], "free_base": []}
    res_t = res_g = res_f = None
    launches_f = 0
    for _ in range(5):
        _, r, _, _ = timed(ctx, field, {}, (0,))
        rows["field"].append(r[1] / F)
        res_t, r, _, path_t = timed(ctx, access, {}, (4,))
        rows["tile"].append(r[1] / (F * len(probes)))
        res_g, r, _, path_g = timed(ctx, access, GLOBAL, (4,))
        rows["global"].append(r[1] / (F * len(probes)))
        res_f, r, launches_f, path_f = timed(ctx, lambda: access(FF, True), {}, (4,))
        _, rb, _, _ = timed(ctx, lambda: access(FF, False), {}, (4,))
        rows["free"].append((r[1] - rb[1]) / FF)
    assert (path_t, path_g) == ("pore_label_tile", "pore_label_global"), (path_t, path_g)
    out["field"] = stats(rows["field"])
    for key in ("tile", "global"):
        out[key] = stats(rows[key])
        out[key]["hbm_share"] = 12.0 * G / out[key]["median"] / HBM_PEAK
    out["free_sphere"] = dict(stats(rows["free"]), frames=FF, path=path_f, labellings_per_frame=launches_f / FF - len(probes),
                              tstar_frame0=float(res_f[5][0, 0]), dif_half_frame0=float(res_f[5][0, 1]))
    out["identical"] = bool(all(np.array_equal(x, y) for x, y in zip(res_t, res_g)))
    # frame 0: wrap links from the field, components from the access rows
    one = ctx.pore_access(traj, *args, frame_range=(0, 1), per_point=True)
    fld, acc, cnt = one[5][0], one[4][0], one[1][0]
    out["counts"] = {"wrap_links": [wrap_links(fld >= t, traj.pbc) for t in probes], "components": [int(x[1] + x[2]) for x in acc],
                     "channels": [int(x[1]) for x in acc], "pockets": [int(x[2]) for x in acc], "accessible": [int(x[0]) for x in acc],
                     "void": [int(x) for x in cnt], "dimension": [int(x[3]) for x in acc]}
    write(a.out, out)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
