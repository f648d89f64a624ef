"""Timings of amof_pore_psd on the headline shape (profiles/pore/pore_psd_timing.md).

    python profiles/tools/pore_psd_timing.py [--frames 50] [--exact-frames 2] [--exact-calls 3] [--out profiles/pore]     # GPU: json + md
    python profiles/tools/pore_psd_timing.py --report                                                    # md from the json

The first ``frames`` frames of the bench's random walk (9792 atoms, 3 x 3 x 4 ZIF-4 cells) resident in HBM, the grid of
spacing 0.2 A (232 x 232 x 369), table radii, dr = 0.05, the default dmax, probes 0 and 1.2 A -- the shape of
profiles/tools/pore_timing.py and pore_access_timing.py.  One GPU process; median of five warm calls after one cold call, the
library's own HIP events (amof_last_kernel_seconds): 3 = the field kernels, 5 = the covering stage.  The covering stage's
events enclose its kernels (brick maxima, the covering pass, the histogram of w), the copy of the brick maxima and of the
frame's counters to the host and the host's share between them: it is the time the stage adds to a frame, not kernel time alone.

  covering, "pore_cover_brick"   stage 5 of amof_pore_psd without accessibility, per frame
  accessible pass                stage 5 with accessibility minus without, per frame and threshold that has a channel
  covering, "pore_cover_exact"   AMOF_PORE_COVER_EXACT=1 on the first ``exact-frames`` frames only (a lane per point walks
                                 thousands of offsets there: 7941 in frame 0), the median of ``exact-calls`` (three) warm calls,
                                 not five; the brick path on the same frames beside it, w and every integer compared bit for bit
  list records, source bricks    amof_pore_cover_stats: per destination brick, means over the full passes of a call"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

EXACT = {"AMOF_PORE_COVER_EXACT": "1"}


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
        path = ctx.last_path()
        cover = ctx.pore_cover_stats()
    return res, [wall] + secs, path, cover


def render(d):
    sh = d["shape"]
    G = sh["points"]
    L = ["# amof_pore_psd on the headline shape\n"]
    L.append("Written by `profiles/tools/pore_psd_timing.py` (its docstring says what is timed and how) from `pore_psd_timing.json` "
             "beside this file; one MI355X, trajectory resident in HBM.  Shape: the first %d frames of the bench's random walk, %d atoms, "
             "grid %d x %d x %d = %s points, probes 0 and 1.2 A, dmax = %g A.  Median of the warm calls; per frame.\n"
             % (sh["frames"], sh["atoms"], sh["grid"][0], sh["grid"][1], sh["grid"][2], format(G, ","), sh["dmax"]))
    L.append("| what | per frame | min .. max of the calls, per frame |")
    L.append("|---|---|---|")
    for key, name in (("field", "the field kernels (stage 3 of the same calls)"),
                      ("brick", "covering stage, `pore_cover_brick` (%d frames, 5 calls)" % sh["frames"]),
                      ("access_pass", "one accessible pass, `pore_cover_brick` (per threshold with a channel)"),
                      ("brick_few", "covering stage, `pore_cover_brick` (the first %d frames)" % d["exact_frames"]),
                      ("exact", "covering stage, `pore_cover_exact` (the first %d frames, %d calls)" % (d["exact_frames"], d["exact_calls"]))):
        r = d[key]
        L.append("| %s | %.2f ms | %.2f .. %.2f ms |" % (name, r["median"] * 1e3, r["min"] * 1e3, r["max"] * 1e3))
    L.append("")
    L.append("Per destination brick of 8 x 8 x 8 points (means over the %d frames): %.1f source bricks kept of the reach box, %.1f centre "
             "records swept.  The largest field value of frame 0 is %.3f A: the exact path's table holds %s offsets per point.\n"
             % (sh["frames"], d["source_bricks_per_brick"], d["records_per_brick"], d["vmax_frame0"], format(d["offsets_frame0"], ",")))
    ratio = d["exact"]["median"] / d["brick_few"]["median"]
    L.append("The two paths' results on the first %d frames (w of every point, histogram, occupiable counts, counts covered from "
             "channels): identical = %s.  `pore_cover_brick` %s `pore_cover_exact` in the same binary (exact / brick = %.1f).\n"
             % (d["exact_frames"], d["identical"], "is faster than" if ratio > 1.0 else "IS NOT FASTER THAN", ratio))
    c = d["counts"]
    L.append("Frame 0, per probe radius (0, 1.2 A): probe-centre points %s, probe-occupiable points %s, of those covered from a channel "
             "%s; points covered by no sphere %d of %s.\n" % (c["centre"], c["occupiable"], c["accessible"], c["uncovered"], format(G, ",")))
    return "\n".join(L)


def write(out_dir, d):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "pore_psd_timing.json"), "w") as fh:
        json.dump(d, fh, indent=1, sort_keys=True)
        fh.write("\n")
    with open(os.path.join(out_dir, "pore_psd_timing.md"), "w") as fh:
        fh.write(render(d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--exact-frames", type=int, default=2)
    ap.add_argument("--exact-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pore"))
    ap.add_argument("--report", action="store_true", help="no GPU: render the markdown from the JSON")
    a = ap.parse_args()
    if a.report:
        with open(os.path.join(a.out, "pore_psd_timing.json")) as fh:
            write(a.out, json.load(fh))
        return

    import torch
    from amof_amd import _hip
    from amof_amd import pore as P
    from tests import helpers as H
    from tests import pore_cover_ref

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
    F, EF = a.frames, min(a.exact_frames, a.frames)
    out = {"shape": {"atoms": int(traj.n_atoms), "frames": F, "grid": list(grid), "points": G, "dmax": dmax, "probes": list(probes)},
           "exact_frames": EF, "exact_calls": a.exact_calls}

    def psd(frames=F, access=False, per_point=False):
        return ctx.pore_psd(traj, *args, frame_range=(0, frames), accessibility=access, per_point=per_point)

    timed(ctx, psd, {}, (3, 5))
    timed(ctx, lambda: psd(F, True), {}, (3, 5))
    rows = {"field": [], "brick": [], "access_pass": [], "brick_few": [], "exact": []}
    cover = None
    with_channel = 1
    for _ in range(5):
        res, r, path, cover = timed(ctx, psd, {}, (3, 5))
        assert path == "pore_cover_brick", path
        rows["field"].append(r[1] / F)
        rows["brick"].append(r[2] / F)
        res_a, ra, path, _ = timed(ctx, lambda: psd(F, True), {}, (3, 5))
        assert path == "pore_cover_brick", path
        with_channel = max(1, int((res_a[4][:, :, 1] > 0).sum()))
        rows["access_pass"].append((ra[2] - r[2]) / with_channel)
        _, rf, _, _ = timed(ctx, lambda: psd(EF), {}, (3, 5))
        rows["brick_few"].append(rf[2] / EF)
    out["passes_with_channel"] = with_channel
    out["source_bricks_per_brick"] = cover["source_bricks"] / max(1.0, cover["bricks"])
    out["records_per_brick"] = cover["records"] / max(1.0, cover["bricks"])
    few_b, _, path_b, _ = timed(ctx, lambda: psd(EF, True, True), {}, (5,))
    few_e, _, path_e, _ = timed(ctx, lambda: psd(EF, True, True), EXACT, (5,))         # (the cold call: compared, not timed)
    for _ in range(a.exact_calls):
        _, rn, _, _ = timed(ctx, lambda: psd(EF), EXACT, (5,))
        rows["exact"].append(rn[1] / EF)
        print("exact call done: %.3f s per frame" % rows["exact"][-1], flush=True)
    assert (path_b, path_e) == ("pore_cover_brick", "pore_cover_exact"), (path_b, path_e)
    for key in rows:
        out[key] = stats(rows[key])
    out["identical"] = bool(all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(few_b, few_e)))
    assert out["identical"], "pore_cover_brick and pore_cover_exact disagree"
    hist, counts, vmax = few_b[0], few_b[1], few_b[2]
    A = pore_cover_ref.step_vectors(traj.cell[0], grid)
    R = pore_cover_ref.reach(A, float(vmax[0]))
    i, j, k = np.meshgrid(*[np.arange(-r, r + 1, dtype=np.float64) for r in R], indexing="ij")
    s = [(i * A[0][c] + j * A[1][c]) + k * A[2][c] for c in range(3)]
    out["vmax_frame0"] = float(vmax[0])
    out["offsets_frame0"] = int((((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]) <= float(vmax[0]) ** 2).sum())
    out["counts"] = {"centre": [int(x) for x in counts[0]], "occupiable": [int(x) for x in few_b[7][0]],
                     "accessible": [int(x) for x in few_b[8][0]], "uncovered": int(few_b[6][0, 0])}
    write(a.out, out)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
