"""Timings of amof_dihedral_hist and of the code it shares with Bad and BondOrder (profiles/dihedral/dihedral_timing.md).

    python profiles/tools/dihedral_timing.py --shared-only > parent.json     # at the parent commit: Bad and BondOrder alone
    python profiles/tools/dihedral_timing.py --parent parent.json            # at this commit: everything, and the report

Dihedral: the first 50 frames of the headline trajectory (9792 atoms, the bench's random walk, resident in HBM), the four
quick-start cutoffs, the default patterns, dphi = 1, on "dihedral_frame" and on "dihedral_exact": the whole call, the list stage
(the adjacency rows on the exact path) and the dihedral kernel, from the library's device events (amof_last_kernel_seconds 0, 2,
3).  Shared code: Bad ({'Zn-N': 2.5}, dtheta = 0.5) and BondOrder (l = 4, 6) on the whole headline trajectory, kernel seconds of
the whole call.  Every figure: the first call on its own, then the median, minimum and maximum of five warm calls."""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ZIF_CUT = {'Zn-N': 2.5, 'C-N': 1.6, 'C-C': 1.6, 'C-H': 1.2}
# hipcc -Rpass-analysis=kernel-resource-usage, gfx950 (VGPRs, SGPRs, scratch bytes per lane, waves per SIMD; LDS is dynamic:
# 96 T bytes of wave sums and 4 T nb of histogram)
RESOURCES = [("dihedral_rows_kernel", 93, 106, 0, 5), ("dihedral_exact_kernel<true>", 93, 106, 0, 5),
             ("dihedral_exact_kernel<false>", 117, 106, 0, 4), ("dihedral_totals_kernel", 14, 20, 0, 8)]


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v), "spread": max(v) - min(v), "first": None, "all": v}


def measure(call, read, names):
    rows = []
    for _ in range(6):
        res = call()
        rows.append(read())
    warm = np.array(rows[1:], dtype=np.float64)
    rec = {}
    for k, name in enumerate(names):
        rec[name] = stats(warm[:, k])
        rec[name]["first"] = float(rows[0][k])
    return rec, res


def shared(ctx, traj):
    from amof_amd import _hip
    from amof_amd import atom as amatom
    kinds, _ = _hip.packed_species(traj)
    rcm = amatom.cutoff_matrix(amatom.format_cutoff({'Zn-N': 2.5}), kinds)
    zn, n = kinds.index(30), kinds.index(7)
    edges = np.arange(int(180 // 0.5) + 2) * 0.5
    out = {}
    out["bad"], _ = measure(lambda: ctx.bad_hist(traj, rcm, [(zn, n), (n, zn), (zn, -1)], edges),
                            lambda: (ctx.last_kernel_seconds(dominant=False),), ("all_s",))
    out["bad"]["path"] = ctx.last_path()
    out["bond_order"], _ = measure(lambda: ctx.bond_order(traj, rcm, [(zn, n)], (4, 6), 100, 400),
                                   lambda: (ctx.last_kernel_seconds(dominant=False),), ("all_s",))
    out["bond_order"]["path"] = ctx.last_path()
    return out


def dihedral(ctx, traj, frames):
    from amof_amd import _hip
    from amof_amd import atom as amatom
    from amof_amd import dihedral as amdihedral
    kinds, _ = _hip.packed_species(traj)
    cut = amatom.format_cutoff(ZIF_CUT, sort_pair=True)
    rcm = amatom.cutoff_matrix(cut, kinds)
    chains = amdihedral.default_chains(cut, kinds)
    idx = [[kinds.index(z) for z in c] for c in chains]
    edges, _ = amdihedral.bins(1.0)
    out = {"frames": frames, "patterns": [amdihedral.chain_name(c) for c in chains]}

    def read():
        st = ctx.last_stage_seconds()
        return ctx.last_kernel_seconds(dominant=False), st["rho"], st["corr"]
    first = None
    for label, env in (("dihedral_frame", None), ("dihedral_exact", "1")):
        if env:
            os.environ["AMOF_DIHEDRAL_EXACT"] = env
        try:
            rec, res = measure(lambda: ctx.dihedral_hist(traj, rcm, idx, edges, frame_range=(0, frames)), read, ("all_s", "list_s", "kernel_s"))
            rec["path"] = ctx.last_path()
        finally:
            os.environ.pop("AMOF_DIHEDRAL_EXACT", None)
        assert rec["path"] == label, rec["path"]
        first = res if first is None else first
        assert all(np.array_equal(x, y) for x, y in zip(res, first)), "the paths differ"
        out[label] = rec
    hist, n_def, n_undef, _ = first
    out["chains_per_frame"] = float(int(n_def.sum()) + int(n_undef.sum())) / frames
    out["undefined_share"] = float(int(n_undef.sum())) / max(1, int(n_def.sum()) + int(n_undef.sum()))
    return out


def line(name, rec, key):
    s = rec[key]
    return "| %s | %.3f | %.3f | %.3f | %.3f |" % (name, 1e3 * s["first"], 1e3 * s["median"], 1e3 * s["min"], 1e3 * s["max"])


def report(out, parent):
    d = out["dihedral"]
    head = "| | first call (ms) | median of 5 warm (ms) | min | max |\n|---|---|---|---|---|"
    text = ["# amof_dihedral_hist on MI355X", "",
            "%d atoms, the first %d frames of the headline trajectory, cutoffs %s, %d default patterns, dphi = 1; kernel time from"
            " the library's device events." % (out["atoms"], d["frames"], ZIF_CUT, len(d["patterns"])), "",
            "%.0f chains per frame, %.2e of them undefined." % (d["chains_per_frame"], d["undefined_share"]), ""]
    for path, stage in (("dihedral_frame", "list stage"), ("dihedral_exact", "adjacency rows")):
        text += ["## %s" % path, "", head, line("whole call", d[path], "all_s"), line(stage, d[path], "list_s"),
                 line("dihedral kernel", d[path], "kernel_s"), ""]
    text += ["## Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)", "",
             "| kernel | VGPRs | SGPRs | scratch (B/lane) | waves/SIMD |", "|---|---|---|---|---|"]
    text += ["| %s | %d | %d | %d | %d |" % r for r in RESOURCES]
    text += ["", "Dynamic LDS of both dihedral kernels: 96 T bytes of per-wave frame sums and 4 T nb bytes of histogram (T patterns, nb"
             " bins; %.1f KB here)." % ((96 * len(d["patterns"]) + 4 * len(d["patterns"]) * 181) / 1e3), "",
             "Lane mapping: a lane owns a (frame, atom b) and walks b's central bonds.  The lane per central bond (b, slot) that the"
             " design also allows was not built and not measured.", "",
             "## Shared code: Bad and BondOrder on the whole headline trajectory (%d frames)" % out["shared_frames"], "",
             "The list kernel writes the partner's index only in the instantiations the dihedral tier launches (a template flag):"
             " the instantiations Bad and BondOrder launch report the same registers, scratch and LDS as the parent's.", "", head]
    for name, key in (("Bad {'Zn-N': 2.5}", "bad"), ("BondOrder l = 4, 6", "bond_order")):
        if parent:
            text.append(line(name + ", parent commit", parent["shared"][key], "all_s"))
        text.append(line(name + ", this commit", out["shared"][key], "all_s"))
    if parent:
        text.append("")
        for name, key in (("Bad", "bad"), ("BondOrder", "bond_order")):
            p, n = parent["shared"][key]["all_s"], out["shared"][key]["all_s"]
            text.append("%s: median %.3f ms against the parent's %.3f ms; the parent's own spread (max - min) is %.3f ms: %s." % (
                name, 1e3 * n["median"], 1e3 * p["median"], 1e3 * p["spread"],
                "within it" if n["median"] - p["median"] <= p["spread"] else "BEYOND it"))
    return "\n".join(text) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shared-only", action="store_true")
    ap.add_argument("--parent", default=None, help="JSON of a --shared-only run at the parent commit")
    ap.add_argument("--frames", type=int, default=int(os.environ.get("DIHEDRAL_TIMING_FRAMES", "5000")))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dihedral", "dihedral_timing.md"))
    args = ap.parse_args()
    import torch
    from amof_amd import _hip
    from tests import helpers as H
    traj = H.device_walk(torch.device("cuda", 0), (3, 3, 4), args.frames, 0.05, 20261003)
    torch.cuda.synchronize()
    ctx = _hip.get_context(0)
    out = {"atoms": int(traj.n_atoms), "shared_frames": args.frames, "shared": shared(ctx, traj)}
    if not args.shared_only:
        out["dihedral"] = dihedral(ctx, traj, min(50, args.frames))
        parent = json.load(open(args.parent)) if args.parent else None
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report(out, parent))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
