"""Timings of the surface stage of amof_pore_surface on the headline shape (profiles/pore/pore_surface_timing.md).

    python profiles/tools/pore_surface_timing.py [--frames 50] [--exact-frames 5] [--exact-calls 3] [--out profiles/pore]    # GPU: json + md
    python profiles/tools/pore_surface_timing.py --report                                                  # md from the json

The first ``frames`` frames of the bench's random walk (9792 atoms, 3 x 3 x 4 ZIF-4 cells) resident in HBM, the grid of
spacing 0.2 A, table radii, dr = 0.05, the default dmax, probes 0 and 1.2 A -- the shape of profiles/tools/pore_timing.py --
and 256 directions per atom (``sphere_points``).  One GPU process; median of five warm calls after one cold call, the library's
own HIP events (amof_last_kernel_seconds): 3 = the field kernels, 6 = the surface stage.  The surface stage's events enclose its
cell sort (one per frame), its kernel (one launch per frame and probe), the copy of the launch's counters to the host and the
host's share between them: it is the time the stage adds to a frame, not kernel time alone.

  surface, "pore_surface_list"    stage 6 without accessibility, per frame (both probes)
  surface, "pore_surface_exact"   AMOF_PORE_SURFACE_EXACT=1 on the first ``exact-frames`` frames only (a lane per sample walks every
                                  atom of the frame up to the one that buries it), the median of ``exact-calls`` warm calls, not
                                  five; the list path on the same frames beside it, every integer and byte compared
  surface, records unsorted       AMOF_PORE_SURFACE_UNSORTED=1: the neighbour records in the order of the gather instead of those that
                                  bury a quarter of the sphere or more first; the same 50 frames, and once more with 4096 directions,
                                  where the sweep outweighs the launches
  records, re-decisions, exits    amof_pore_surface_stats over a call on the list path"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

EXACT = {"AMOF_PORE_SURFACE_EXACT": "1"}
UNSORTED = {"AMOF_PORE_SURFACE_UNSORTED": "1"}
POINTS = 256


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


def timed(ctx, fn, env):
    with Env(**env):
        t0 = time.perf_counter()
        res = fn()
        wall = time.perf_counter() - t0
        with ctx._lock:
            secs = [ctx._lib.amof_last_kernel_seconds(ctx._h, w) for w in (3, 6)]
        return res, [wall] + secs, ctx.last_path(), ctx.pore_surface_stats()


def render(d):
    sh = d["shape"]
    L = ["# The surface stage of amof_pore_surface on the headline shape\n"]
    L.append("Written by `profiles/tools/pore_surface_timing.py` (its docstring says what is timed and how) from "
             "`pore_surface_timing.json` beside this file; one MI355X, trajectory resident in HBM.  Shape: the first %d frames of the "
             "bench's random walk, %d atoms, %d directions per atom (%s samples per frame and probe), probes 0 and 1.2 A; the field's "
             "grid %d x %d x %d.  Median of the warm calls; per frame, both probes together.\n"
             % (sh["frames"], sh["atoms"], sh["points"], format(sh["atoms"] * sh["points"], ","), sh["grid"][0], sh["grid"][1], sh["grid"][2]))
    L.append("| what | per frame | min .. max of the calls, per frame |")
    L.append("|---|---|---|")
    for key, name in (("field", "the field kernels (stage 3 of the same calls)"),
                      ("list", "surface stage, `pore_surface_list` (%d frames, 5 calls)" % sh["frames"]),
                      ("unsorted", "surface stage, `pore_surface_list`, records unsorted (%d frames, 5 calls)" % sh["frames"]),
                      ("list_4096", "surface stage, `pore_surface_list`, 4096 directions (%d frames, 5 calls)" % sh["frames"]),
                      ("unsorted_4096", "surface stage, `pore_surface_list`, 4096 directions, records unsorted"),
                      ("list_few", "surface stage, `pore_surface_list` (the first %d frames)" % d["exact_frames"]),
                      ("exact", "surface stage, `pore_surface_exact` (the first %d frames, %d calls)" % (d["exact_frames"], d["exact_calls"]))):
        r = d[key]
        L.append("| %s | %.3f ms | %.3f .. %.3f ms |" % (name, r["median"] * 1e3, r["min"] * 1e3, r["max"] * 1e3))
    L.append("")
    L.append("On the list path (means over the %d frames and both probes): %.1f neighbour records per atom, %.2e float64 re-decisions "
             "per sample, %.1f %% of the samples ended by the early exit (buried before the end of their list); %.2f launches per frame "
             "and probe.  With the records unsorted %.1f %% end early and the stage takes %.3f times as long (%.3f with 4096 "
             "directions); the exposed counts are the same.\n"
             % (sh["frames"], d["records_per_atom"], d["redecisions_per_sample"], 100.0 * d["early_exit_share"], d["launches_per_row"],
                100.0 * d["early_exit_share_unsorted"], d["unsorted"]["median"] / d["list"]["median"],
                d["unsorted_4096"]["median"] / d["list_4096"]["median"]))
    ratio = d["exact"]["median"] / d["list_few"]["median"]
    L.append("The two paths' results on the first %d frames (exposed counts per species, the per-sample bytes): identical = %s.  "
             "`pore_surface_list` %s `pore_surface_exact` in the same binary (exact / list = %.1f).\n"
             % (d["exact_frames"], d["identical"], "is faster than" if ratio > 1.0 else "IS NOT FASTER THAN", ratio))
    L.append("Frame 0: exposed samples per species %s at probe 0, %s at probe 1.2 A, of %s per species; SA = %.1f and %.1f A^2.\n"
             % (d["exposed_frame0"][0], d["exposed_frame0"][1], d["samples_per_species"], d["area_frame0"][0], d["area_frame0"][1]))
    return "\n".join(L)


def write(out_dir, d):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "pore_surface_timing.json"), "w") as fh:
        json.dump(d, fh, indent=1, sort_keys=True)
        fh.write("\n")
    with open(os.path.join(out_dir, "pore_surface_timing.md"), "w") as fh:
        fh.write(render(d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--exact-frames", type=int, default=5)
    ap.add_argument("--exact-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pore"))
    ap.add_argument("--report", action="store_true", help="no GPU: render the markdown from the JSON")
    a = ap.parse_args()
    if a.report:
        with open(os.path.join(a.out, "pore_surface_timing.json")) as fh:
            write(a.out, json.load(fh))
        return

    import torch
    from amof_amd import _hip
    from amof_amd import pore as P
    from tests import helpers as H

    traj = H.device_walk(torch.device("cuda", 0), (3, 3, 4), a.frames, 0.05, 20261003)
    torch.cuda.synchronize()
    ctx = _hip.get_context(0)
    kinds, species = _hip.packed_species(traj)
    radii = P.species_radii(kinds)
    grid = P.default_grid(traj.cell[0], 0.2)
    dr = 0.05
    dmax = P.default_dmax(traj.cell, traj.pbc, float(radii.max()), dr)
    probes = (0.0, 1.2)
    dirs = P.sphere_points(POINTS)
    args = (radii, grid, dr, dmax, probes)
    F, EF = a.frames, min(a.exact_frames, a.frames)
    out = {"shape": {"atoms": int(traj.n_atoms), "frames": F, "grid": list(grid), "points": POINTS, "dmax": dmax, "probes": list(probes)},
           "exact_frames": EF, "exact_calls": a.exact_calls}

    def surface(frames=F, per_point=False, table=dirs):
        return ctx.pore_surface(traj, *args, dirs=table, frame_range=(0, frames), per_point=per_point)

    timed(ctx, surface, {})
    rows = {"field": [], "list": [], "unsorted": [], "list_4096": [], "unsorted_4096": [], "list_few": [], "exact": []}
    st = None
    many = P.sphere_points(4096)
    timed(ctx, lambda: surface(table=many), {})
    for _ in range(5):
        res_u, ru, _, st_u = timed(ctx, surface, UNSORTED)
        rows["unsorted"].append(ru[2] / F)
        rows["list_4096"].append(timed(ctx, lambda: surface(table=many), {})[1][2] / F)
        rows["unsorted_4096"].append(timed(ctx, lambda: surface(table=many), UNSORTED)[1][2] / F)
        res_s, r, path, st = timed(ctx, surface, {})
        assert np.array_equal(res_s[-1], res_u[-1])
        out["early_exit_share_unsorted"] = st_u["early_exits"] / max(1.0, st_u["samples"])
        assert path == "pore_surface_list", path
        launches = ctx._lib.amof_last_kernel_launches(ctx._h)
        rows["field"].append(r[1] / F)
        rows["list"].append(r[2] / F)
        _, rf, _, _ = timed(ctx, lambda: surface(EF), {})
        rows["list_few"].append(rf[2] / EF)
    out["records_per_atom"] = st["records"] / max(1.0, st["atoms"])
    out["redecisions_per_sample"] = st["redecisions"] / max(1.0, st["samples"])
    out["early_exit_share"] = st["early_exits"] / max(1.0, st["samples"])
    out["launches_per_row"] = launches / float(F * len(probes))
    few_l, _, path_l, _ = timed(ctx, lambda: surface(EF, True), {})
    few_e, _, path_e, _ = timed(ctx, lambda: surface(EF, True), EXACT)         # (the cold call: compared, not timed)
    assert (path_l, path_e) == ("pore_surface_list", "pore_surface_exact"), (path_l, path_e)
    for _ in range(a.exact_calls):
        _, rn, _, _ = timed(ctx, lambda: surface(EF), EXACT)
        rows["exact"].append(rn[2] / EF)
        print("exact call done: %.4f s per frame" % rows["exact"][-1], flush=True)
    for key in rows:
        out[key] = stats(rows[key])
    out["identical"] = bool(all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(few_l, few_e)))
    assert out["identical"], "pore_surface_list and pore_surface_exact disagree"
    exposed = few_l[-2]
    out["exposed_frame0"] = [[int(x) for x in exposed[0, k]] for k in range(len(probes))]
    out["samples_per_species"] = [int((np.asarray(species) == s).sum()) * POINTS for s in range(len(kinds))]
    out["area_frame0"] = [float(P.surface_area(exposed[0, k], radii, rp, POINTS)) for k, rp in enumerate(probes)]
    write(a.out, out)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
