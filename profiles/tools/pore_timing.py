"""Timings of amof_pore_field on the headline shape (profiles/pore/pore_timing.md).

    python profiles/tools/pore_timing.py [--frames 50] [--out profiles/pore]      # writes pore_timing.json and pore_timing.md
    rocprofv3 --kernel-trace --stats --output-format csv -d pore_trace -- python3 profiles/tools/pore_timing.py --trace-run
    python profiles/tools/pore_timing.py --report --kernel-stats pore_trace/.../*_kernel_stats.csv \
        --bench "run A:parent:a/parent_1.json" --bench "run A:this commit:a/new_1.json" ...

The first form measures (GPU).  ``--report`` (no GPU) merges the kernel rows of a rocprofv3 stats file and the result lines of
bench.py runs -- ``series:label:file`` in the order they ran -- into pore_timing.json and renders pore_timing.md from that
file alone, so the document is reproduced by this tool from the numbers it keeps.

The first ``frames`` frames of the bench's random walk (9792 atoms, 3 x 3 x 4 ZIF-4 cells) resident in HBM, the grid of
spacing 0.2 A, table radii, dr = 0.05, the default dmax, probes 0 and 1.2 A.  "pore_brick" against AMOF_PORE_EXACT=1 in the
same process, alternating, five warm calls each after one cold call: the library's own HIP events (amof_last_kernel_seconds:
0 = the whole call, 2 = the cell sort, 3 = the field kernels) and the wall time of the call.  "pore_exact" visits every atom
for every grid point; where five calls of it on all frames would take longer than ``--exact-budget`` seconds, it is timed on
the first frames that fit (at least 2) and the file says on how many.  The two paths' results are compared bit for bit on
the frames both computed.

Counted on the host, from the shapes: for a sample of bricks of frame 0 the images a brick keeps (the gather rule of
pore_brick_kernel restated in numpy), hence candidate evaluations per grid point (two sweeps over the list), and the atoms
per point whose float64 value lies within 2 eps_c of the point's minimum, an estimate of the refined atoms.  VALU
operations are ESTIMATED from the source, not counted in the ISA: 9 per point and atom in the first sweep (3 subtractions, a
product and 2 fma for d2, the sum and the square of the threshold, the compare), 10 in the second; over the field kernels'
time, against 78.6e12 lane operations per second (1024 SIMDs x 32 lanes per cycle x 2.4 GHz: MI355X_MICROARCH gives a wave64
v_fma_f32 two cycles on a SIMD; that is half its 157.3 TFLOPS vector peak, which counts an fma as two).  The share of peak
is therefore an estimate over an issue rate, good to the accuracy of the instruction count."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

VALU_PEAK = 78.6e12
OPS_SWEEP1, OPS_SWEEP2 = 9, 10
BRICK = 8


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


def one_call(ctx, traj, args, env, frames):
    with Env(**env):
        t0 = time.perf_counter()
        res = ctx.pore_field(traj, *args, frame_range=(0, frames))
        wall = time.perf_counter() - t0
        lib = ctx._lib
        with ctx._lock:
            row = [wall] + [lib.amof_last_kernel_seconds(ctx._h, w) for w in (0, 2, 3)]
        path = ctx.last_path()
    return res, row, path


def brick_sample(pos0, cell, numbers, radii_of, grid, dmax, eps_c, n_bricks, seed):
    """images kept per brick and near-minimal atoms per point, for ``n_bricks`` random bricks of one frame (host, numpy; any
    cell: the 27 images around the rounded fractional difference to the brick centre)"""
    import itertools
    from amof_amd import pore as P
    rng = np.random.default_rng(seed)
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    inv = np.linalg.inv(cell)
    R = np.array([radii_of[int(z)] for z in numbers])
    nb = [(n + BRICK - 1) // BRICK for n in grid]
    half = 0.5 * (BRICK - 1) / np.array(grid, dtype=np.float64)
    hd = max(float(np.linalg.norm((half * np.array(sg)) @ cell)) for sg in itertools.product((1, -1), repeat=3))
    pts = P.grid_points(cell, grid)
    shifts = np.array(list(itertools.product((-1, 0, 1), repeat=3)), dtype=np.float64) @ cell
    kept, near, pts_total = [], 0, 0
    for _ in range(n_bricks):
        b = [int(rng.integers(0, n)) for n in nb]
        centre = ((np.array(b) * BRICK + 0.5 * BRICK) / np.array(grid)) @ cell
        d = pos0 - centre
        d = d - np.rint(d @ inv) @ cell
        img = (d[None, :, :] + shifts[:, None, :]).reshape(-1, 3)
        Rimg = np.tile(R, len(shifts))
        keep = np.sqrt((img ** 2).sum(axis=1)) - Rimg < dmax + hd
        kept.append(int(keep.sum()))
        sl = tuple(slice(b[k] * BRICK, min(grid[k], b[k] * BRICK + BRICK)) for k in range(3))
        Pts = pts[sl].reshape(-1, 3)
        v = np.sqrt((((img[keep] + centre)[None] - Pts[:, None]) ** 2).sum(axis=2)) - Rimg[keep][None]
        vmin = v.min(axis=1)
        sel = (v <= vmin[:, None] + 2.0 * eps_c) & (vmin[:, None] < dmax + 2.0 * eps_c)
        near += int(sel.sum())
        pts_total += len(Pts)
    return {"bricks_sampled": n_bricks, "images_per_brick": stats(kept), "half_diagonal": float(hd),
            "near_minimal_atoms_per_point": near / pts_total}


def kernel_rows(path):
    """the library's kernels from a rocprofv3 ``*_kernel_stats.csv``"""
    import csv
    rows = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            if "amof::" in r["Name"]:
                name = r["Name"].replace("void ", "").split("(")[0].replace("amof::", "")
                rows.append({"name": name, "calls": int(r["Calls"]), "average_ns": float(r["AverageNs"]), "min_ns": float(r["MinNs"]),
                             "max_ns": float(r["MaxNs"]), "percentage": float(r["Percentage"])})
    return rows


def bench_rows(items):
    out = []
    for item in items:
        series, label, path = item.split(":", 2)
        with open(path) as fh:
            d = json.loads(fh.read().strip().splitlines()[-1])
        out.append({"series": series, "label": label, "steps": d["steps"], "warmup": d["warmup"], "ms_per_step": d["ms_per_step"],
                    "rdf_tile_s": d["kernel_seconds_per_step"]["rdf_tile"],
                    "host_s": d["host_seconds_per_step"]["rdf_wall_minus_kernels"]})
    return out


def render(d):
    """pore_timing.md from pore_timing.json"""
    sh, b, e, c = d["shape"], d["pore_brick"], d["pore_exact"], d["counts"]
    L = []
    L.append("# amof_pore_field on the headline shape\n")
    L.append("Written by `profiles/tools/pore_timing.py` (its docstring says what is timed and how) from `pore_timing.json` beside this "
             "file; one MI355X, trajectory resident in HBM.  Shape: the first %d frames of the bench's random walk, %d atoms (3 x 3 x 4 "
             "ZIF-4 cells), grid %d x %d x %d = %s points (spacing %g A), table radii, dr = %g A, dmax = %g A (the default rule), probes "
             "0 and 1.2 A.  Nothing earlier exists to compare with.\n"
             % (sh["frames"], sh["atoms"], sh["grid"][0], sh["grid"][1], sh["grid"][2], format(sh["points"], ","), sh["spacing"], sh["dr"],
                sh["dmax"]))
    L.append("## Call times (the library's HIP events, median of five warm calls, the two paths alternating in one process)\n")
    L.append("| path | frames | whole call | per frame | cell sort per frame | field kernels per frame | min .. max of the five calls |")
    L.append("|---|---|---|---|---|---|---|")
    L.append("| `pore_brick` | %d | %.1f ms | **%.2f ms** | %.2f us | %.2f ms | %.1f .. %.1f ms |"
             % (b["frames"], b["all_s"]["median"] * 1e3, b["all_s_per_frame"] * 1e3, b["cell_sort_s_per_frame"] * 1e6,
                b["field_s_per_frame"] * 1e3, b["all_s"]["min"] * 1e3, b["all_s"]["max"] * 1e3))
    L.append("| `pore_exact` (`AMOF_PORE_EXACT=1`) | %d | %.2f s | **%.0f ms** | - | %.0f ms | %.2f .. %.2f s |\n"
             % (e["frames"], e["all_s"]["median"], e["all_s_per_frame"] * 1e3, e["field_s_per_frame"] * 1e3, e["all_s"]["min"],
                e["all_s"]["max"]))
    L.append("`pore_exact` ran on %d of the %d frames.  Ratio per frame: %.1f x.  The two paths' rows, probe counts, largest values and "
             "indices on those frames: identical = %s.  Cold first call of `pore_brick`: %.1f ms.  Wall time of a warm call: %.1f ms "
             "(host work outside the kernels: %.2f ms).  Frame 0: %.1f %% of the points inside a van der Waals sphere, Di = %.2f A, "
             "%d overflow points in all frames.\n"
             % (d["exact_frames"], sh["frames"], d["speedup_per_frame_all_s"], d["identical_on_exact_frames"], b["cold"]["all_s"] * 1e3,
                b["wall_s"]["median"] * 1e3, (b["wall_s"]["median"] - b["all_s"]["median"]) * 1e3,
                d["result"]["inside_fraction_frame0"] * 100, d["result"]["Di_frame0"], d["result"]["overflow_points"]))
    if d.get("kernel_trace"):
        L.append("## Kernel time (a separate `rocprofv3 --kernel-trace --stats` run of `--trace-run`: one cold and two warm `pore_brick` calls)\n")
        L.append("| kernel | calls | average | min .. max | share of the run's kernel time |")
        L.append("|---|---|---|---|---|")
        for r in d["kernel_trace"]:
            L.append("| `%s` | %d | %.4g ms | %.4g .. %.4g ms | %.3g %% |" % (r["name"], r["calls"], r["average_ns"] * 1e-6, r["min_ns"] * 1e-6,
                                                                        r["max_ns"] * 1e-6, r["percentage"]))
        L.append("")
    else:
        L.append("## Kernel time\n\nnot measured (no rocprofv3 stats file given to `--report`)\n")
    L.append("## Counted on the host, from the shapes\n")
    L.append("%d random bricks of frame 0, the gather rule restated in numpy: a brick keeps %.0f atom images (median; %.0f .. %.0f; capacity "
             "2048), half-diagonal %.2f A.  Candidate evaluations per grid point: %.0f (two sweeps over the list).  Atoms per point within "
             "2 eps_c (eps_c = %.3g A) of the point's float64 minimum, i.e. re-evaluated in float64: %.4f.\n"
             % (c["bricks_sampled"], c["images_per_brick"]["median"], c["images_per_brick"]["min"], c["images_per_brick"]["max"],
                c["half_diagonal"], c["candidate_evaluations_per_point"], c["eps_c"], c["near_minimal_atoms_per_point"]))
    L.append("VALU lane operations per frame, ESTIMATED from the source (%d per point and atom in sweep 1, %d in sweep 2; not counted in "
             "the ISA): %.3g.  Over the field kernels' time that is %.0f %% of 78.6e12 lane operations per second (1024 SIMDs x 32 lanes "
             "per cycle x 2.4 GHz, from MI355X_MICROARCH's two cycles per wave64 v_fma_f32; half its 157.3 TFLOPS, which counts an fma as "
             "two).  An estimate of issue occupancy, as good as the instruction count.  A frame reads %d atom records and writes three "
             "partial words per brick: not HBM-bound.  Untried levers: four points per lane (half the LDS reads per evaluation), a "
             "list sorted by distance from the centre so that sweep 1 stops early, a dmax below the 8 A cap where the largest cavity is "
             "known to be smaller.\n"
             % (OPS_SWEEP1, OPS_SWEEP2, c["valu_lane_ops_per_frame"], c["valu_share_of_peak"] * 100, sh["atoms"]))
    L.append("## bench.py, this commit against its parent\n")
    if d.get("bench"):
        series = []
        for r in d["bench"]:
            if r["series"] not in series:
                series.append(r["series"])
        for sname in series:
            rows = [r for r in d["bench"] if r["series"] == sname]
            L.append("%s: `python bench.py --gpus 1 --steps %d --warmup %d`, the runs in the order of the table, one after the other on "
                     "the same GPU.\n" % (sname, rows[0]["steps"], rows[0]["warmup"]))
            L.append("| run | ms per step | rdf_tile kernel per step | host time per step outside the kernels |")
            L.append("|---|---|---|---|")
            for r in rows:
                L.append("| %s | %.2f | %.1f ms | %.1f ms |" % (r["label"], r["ms_per_step"], r["rdf_tile_s"] * 1e3, r["host_s"] * 1e3))
            by = {}
            for r in rows:
                by.setdefault(r["label"].split(",")[0], []).append(r["ms_per_step"])
            L.append("")
            L.append("Means: " + "; ".join("%s %.2f ms (spread %.2f over %d repeats)" % (k, float(np.mean(v)), max(v) - min(v), len(v))
                                           for k, v in by.items()) + ".\n")
        L.append("The dominant kernel's code object is the parent's (one code object per translation unit) and nothing of the new "
                 "translation unit runs during the benchmark; the runs differ in host time outside the kernels and in the kernel's own "
                 "repeat spread.\n")
    else:
        L.append("not measured\n")
    return "\n".join(L)


def write(out_dir, d):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "pore_timing.json"), "w") as fh:
        json.dump(d, fh, indent=1, sort_keys=True)
        fh.write("\n")
    with open(os.path.join(out_dir, "pore_timing.md"), "w") as fh:
        fh.write(render(d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pore"))
    ap.add_argument("--exact-budget", type=float, default=100.0)
    ap.add_argument("--trace-run", action="store_true", help="one cold and two warm pore_brick calls, nothing written")
    ap.add_argument("--report", action="store_true", help="no GPU: merge --kernel-stats / --bench into the JSON, write the markdown")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *_kernel_stats.csv of a --trace-run")
    ap.add_argument("--bench", action="append", default=[], help="series:label:file of a bench.py result line; in the order run")
    a = ap.parse_args()
    if a.report:
        with open(os.path.join(a.out, "pore_timing.json")) as fh:
            d = json.load(fh)
        if a.kernel_stats:
            d["kernel_trace"] = kernel_rows(a.kernel_stats)
        if a.bench:
            d["bench"] = bench_rows(a.bench)
        write(a.out, d)
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
    args = (radii, grid, dr, dmax, (0.0, 1.2))
    G = grid[0] * grid[1] * grid[2]
    if a.trace_run:
        for _ in range(3):
            one_call(ctx, traj, args, {}, a.frames)
        return

    out = {"shape": {"atoms": int(traj.n_atoms), "frames": a.frames, "grid": list(grid), "points": G, "spacing": 0.2, "dr": dr,
                     "dmax": dmax, "radii": {str(k): float(r) for k, r in zip(kinds, radii)}, "probes": [0.0, 1.2]}}
    # cold calls; pore_exact on two frames first: what five calls of it on all frames would take
    res_b, cold_b, path_b = one_call(ctx, traj, args, {}, a.frames)
    _, cold_e2, path_e = one_call(ctx, traj, args, {"AMOF_PORE_EXACT": "1"}, 2)
    _, warm_e2, _ = one_call(ctx, traj, args, {"AMOF_PORE_EXACT": "1"}, 2)
    per_frame_exact = warm_e2[0] / 2.0
    fe = int(max(2, min(a.frames, a.exact_budget / (6.0 * per_frame_exact))))
    out["paths"] = {"fast": path_b, "exact": path_e}
    out["exact_frames"] = fe
    rows_b, rows_e, rows_bs = [], [], []
    res_e = None
    for rep in range(5):
        res_b, rb, _ = one_call(ctx, traj, args, {}, a.frames)
        res_e, re_, _ = one_call(ctx, traj, args, {"AMOF_PORE_EXACT": "1"}, fe)
        res_bs, rbs, _ = one_call(ctx, traj, args, {}, fe)          # the fast path on the frames pore_exact was given
        rows_b.append(rb)
        rows_e.append(re_)
        rows_bs.append(rbs)
    names = ("wall_s", "all_s", "cell_sort_s", "field_s")
    for key, rows, nf, cold in (("pore_brick", rows_b, a.frames, cold_b), ("pore_exact", rows_e, fe, None),
                                ("pore_brick_on_exact_frames", rows_bs, fe, None)):
        rows = np.array(rows)
        rec = {"frames": nf}
        if cold is not None:
            rec["cold"] = dict(zip(names, [float(x) for x in cold]))
        for k, name in enumerate(names):
            rec[name] = stats(rows[:, k])
            rec[name + "_per_frame"] = rec[name]["median"] / nf
        out[key] = rec
    out["identical_on_exact_frames"] = bool(all(np.array_equal(x[:fe], y) for x, y in zip(res_b, res_e)))
    out["speedup_per_frame_all_s"] = out["pore_exact"]["all_s_per_frame"] / out["pore_brick_on_exact_frames"]["all_s_per_frame"]
    hist = res_b[0]
    out["result"] = {"inside_fraction_frame0": float(hist[0, 0]) / G, "overflow_points": int(hist[:, -1].sum()),
                     "Di_frame0": 2.0 * float(res_b[2][0])}

    # host counts from the shapes
    eps_c = _hip.pore_candidate_bound(traj.cell[0], dmax + float(radii.max()))
    pos0 = traj.pos[0].cpu().numpy()
    sample = brick_sample(pos0, traj.cell[0], traj.numbers, dict(zip(kinds, radii)), grid, dmax, eps_c, 48, 5)
    sample["eps_c"] = eps_c
    n_list = sample["images_per_brick"]["median"]
    sample["candidate_evaluations_per_point"] = 2.0 * n_list
    ops = float(G) * n_list * (OPS_SWEEP1 + OPS_SWEEP2)
    field_s = out["pore_brick"]["field_s_per_frame"]
    sample["valu_lane_ops_per_frame"] = ops
    sample["valu_share_of_peak"] = ops / field_s / VALU_PEAK
    out["counts"] = sample
    write(a.out, out)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
