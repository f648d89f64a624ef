"""Stage timings of amof_lindemann on the headline shape: writes lindemann_timing.md and lindemann_timing.json.

    python profiles/tools/lindemann_timing.py [output directory, default profiles/lindemann]

9792 atoms x 5000 frames resident in HBM (the bench's random walk).  Configurations: {'Zn-N': 2.5} with B = 5000 (one block);
{'Zn-N': 2.5} with B = S = 500 (ten blocks); the four-cutoff dictionary of the quick start with B = S = 500.  Per stage from
amof_last_kernel_seconds (2 = pair lists, 3 = moments, 4 = reduction) and the whole call (device events); the first call of
a configuration is reported apart, then the median of five warm calls with min and max.  "lindemann_chunk" against
"lindemann_simple" (AMOF_LINDEMANN_SIMPLE=1) in the same binary, with the results compared bit for bit.  The ten-block Zn-N
configuration once more with per_atom=True (the int64 global atomics, the memset per set, the read-back and the host copy),
with the host's wall time of the call beside the device time.  The rate of the moments stage on algorithmic bytes, 24 B x atoms
x frames read, against 8 TB/s: the atoms are ALL atoms of the sets' species, an upper bound on the distinct atoms of the pair
table, so the rate and its share of the peak are upper bounds too and are written "<=".  The yardstick:
amof_bond_reorientation's third stage (vector table + sums) on {'Zn-N': 2.5} in the same session."""

import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
NAMES = ("list_s", "moments_s", "reduce_s", "all_s", "wall_s")
TITLES = ("pair lists", "moments", "reduction", "whole call (device)", "whole call (host wall)")


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)}


def measure(ctx, call):
    rows = []
    for rep in range(6):
        t0 = time.perf_counter()
        res = call()
        wall = time.perf_counter() - t0
        st = ctx.last_stage_seconds()
        rows.append((st["rho"], st["corr"], st["self"], ctx.last_kernel_seconds(dominant=False), wall))
    rec = {"first": dict(zip(NAMES, [float(x) for x in rows[0]])), "path": ctx.last_path()}
    warm = np.array(rows[1:])
    for k, name in enumerate(NAMES):
        rec[name] = stats(warm[:, k])
    return rec, res


def cell(rec, name):
    s = rec[name]
    return "%.3f ms (%.3f .. %.3f)" % (s["median"] * 1e3, s["min"] * 1e3, s["max"] * 1e3)


def main():
    import torch
    from amof_amd import _hip
    from amof_amd import atom as amatom
    from amof_amd.lags import window_setup
    from tests import helpers as H

    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lindemann")
    os.makedirs(out_dir, exist_ok=True)
    frames = int(os.environ.get("LINDEMANN_TIMING_FRAMES", "5000"))
    traj = H.device_walk(torch.device("cuda", 0), (3, 3, 4), frames, 0.05, 20261003)
    torch.cuda.synchronize()
    ctx = _hip.get_context(0)
    kinds, _ = _hip.packed_species(traj)
    numbers = np.asarray(traj.numbers)
    four = {'Zn-N': 2.5, 'C-N': 1.6, 'C-C': 1.6, 'C-H': 1.2}
    z = {'Zn': 30, 'N': 7, 'C': 6, 'H': 1}
    configs = [("Zn-N, B = %d" % frames, {'Zn-N': 2.5}, frames, frames), ("Zn-N, B = S = %d" % (frames // 10), {'Zn-N': 2.5}, frames // 10, frames // 10),
               ("four cutoffs, B = S = %d" % (frames // 10), four, frames // 10, frames // 10)]
    out = {"shape": {"atoms": int(traj.n_atoms), "frames": frames}, "configs": []}
    for label, cut, B, S in configs:
        rcm = amatom.cutoff_matrix(amatom.format_cutoff(cut), kinds)
        sets = [(kinds.index(z[k.split('-')[0]]), kinds.index(z[k.split('-')[1]])) for k in cut]
        rec = {"label": label, "B": B, "S": S, "sets": list(cut)}
        rec["chunk"], res = measure(ctx, lambda: ctx.lindemann(traj, rcm, sets, B, S, 100, 0.005))
        os.environ["AMOF_LINDEMANN_SIMPLE"] = "1"
        try:
            rec["simple"], res_s = measure(ctx, lambda: ctx.lindemann(traj, rcm, sets, B, S, 100, 0.005))
        finally:
            del os.environ["AMOF_LINDEMANN_SIMPLE"]
        assert rec["chunk"]["path"] == "lindemann_chunk" and rec["simple"]["path"] == "lindemann_simple"
        assert all(np.array_equal(a, b) for a, b in zip(res, res_s)), "the two kernels differ"
        sums, hist, scale = res
        nb = sums.shape[0]
        rec["pairs"] = [int(x) for x in sums[:, :, 0].sum(axis=0)]
        rec["index"] = [[float(x) for x in sums[:, s, 1] * 2.0 ** -int(scale[s]) / np.maximum(sums[:, s, 0], 1)] for s in range(len(sets))]
        # algorithmic bytes of the moments stage: every atom of a set's two species that has a pair, once per frame of a block
        # (an upper bound on the distinct atoms: all atoms of the two species)
        atoms = sum(int((numbers == z[k.split('-')[0]]).sum()) + (0 if k.split('-')[0] == k.split('-')[1] else int((numbers == z[k.split('-')[1]]).sum()))
                    for k in cut)
        rec["atoms_read"] = atoms
        rec["algorithmic_bytes"] = 24 * atoms * B * nb
        rec["moments_bytes_per_s"] = rec["algorithmic_bytes"] / rec["chunk"]["moments_s"]["median"]
        rec["pair_frames"] = int(sums[:, :, 0].sum()) * B
        rec["ns_per_pair_frame"] = rec["chunk"]["moments_s"]["median"] * 1e9 / max(rec["pair_frames"], 1)
        out["configs"].append(rec)
    # per_atom rows: the ten-block Zn-N configuration with and without them, device and host time
    label, cut, B, S = configs[1]
    rcm = amatom.cutoff_matrix(amatom.format_cutoff(cut), kinds)
    sets = [(kinds.index(30), kinds.index(7))]
    out["per_atom"] = {"label": label}
    out["per_atom"]["off"], res = measure(ctx, lambda: ctx.lindemann(traj, rcm, sets, B, S, 100, 0.005))
    out["per_atom"]["on"], res_pa = measure(ctx, lambda: ctx.lindemann(traj, rcm, sets, B, S, 100, 0.005, per_atom=True))
    assert all(np.array_equal(a, b) for a, b in zip(res, res_pa[:3])) and np.array_equal(res_pa[3].sum(axis=2), res[0])
    out["per_atom"]["bytes_read_back"] = int(res_pa[3].nbytes)
    # the yardstick: bond reorientation's third stage (vector table + sums) on the same input
    rcm = amatom.cutoff_matrix(amatom.format_cutoff({'Zn-N': 2.5}), kinds)
    sets = [(kinds.index(30), kinds.index(7))]
    window, _ = window_setup(frames, 100, "half", 1)
    out["reorientation"] = {}
    for stride in (1, 25):
        rec, _ = measure(ctx, lambda: ctx.bond_reorientation(traj, rcm, sets, window, origin_stride=stride))
        out["reorientation"]["stride%d" % stride] = rec
    with open(os.path.join(out_dir, "lindemann_timing.json"), "w") as f:
        json.dump(out, f, indent=1)
    lines = ["# amof_lindemann: stage timings on the headline shape", "",
             "Written by `profiles/tools/lindemann_timing.py`.  %d atoms x %d frames resident in HBM, nbins 100, ddelta 0.005;" % (traj.n_atoms, frames),
             "device events, the first call apart, then the median of five warm calls (min .. max).", ""]
    for rec in out["configs"]:
        lines += ["## %s (%d blocks, pairs per set: %s)" % (rec["label"], len(rec["index"][0]), rec["pairs"]), "",
                  "| stage | lindemann_chunk | first call | lindemann_simple | first call |", "|---|---|---|---|---|"]
        for name, title in zip(NAMES, TITLES):
            lines.append("| %s | %s | %.3f | %s | %.3f |" % (title, cell(rec["chunk"], name), rec["chunk"]["first"][name] * 1e3,
                                                            cell(rec["simple"], name), rec["simple"]["first"][name] * 1e3))
        lines += ["", "Moments stage: <= %.3g algorithmic bytes (24 B x %d atoms x frames read; all atoms of the sets' species, an upper bound on "
                  "the distinct atoms of the pair table), <= %.3g B/s = <= %.1f %% of the 8 TB/s peak; %.3g ns per bonded pair and frame." % (rec["algorithmic_bytes"], rec["atoms_read"], rec["moments_bytes_per_s"],
                                                   100.0 * rec["moments_bytes_per_s"] / HBM_PEAK, rec["ns_per_pair_frame"]), ""]
    pa = out["per_atom"]
    lines += ["## per_atom rows: %s, lindemann_chunk (%d bytes read back per call)" % (pa["label"], pa["bytes_read_back"]), "",
              "| stage | per_atom=False | per_atom=True |", "|---|---|---|"]
    for name, title in zip(NAMES, TITLES):
        lines.append("| %s | %s | %s |" % (title, cell(pa["off"], name), cell(pa["on"], name)))
    lines += [""]
    lines += ["## The yardstick: amof_bond_reorientation, {'Zn-N': 2.5}, same session", "",
              "| origin_stride | bond lists | bit series | vector table + sums | whole call |", "|---|---|---|---|---|"]
    for stride in (1, 25):
        rec = out["reorientation"]["stride%d" % stride]
        lines.append("| %d | %s | %s | %s | %s |" % (stride, cell(rec, "list_s"), cell(rec, "moments_s"), cell(rec, "reduce_s"), cell(rec, "all_s")))
    with open(os.path.join(out_dir, "lindemann_timing.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"configs": [(r["label"], r["chunk"]["all_s"]["median"], r["simple"]["all_s"]["median"]) for r in out["configs"]]}))


if __name__ == "__main__":
    main()
