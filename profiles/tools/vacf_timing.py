"""Timings of amof_vacf_window and of the column code it shares with WindowMsd and WindowVanHove
(profiles/vacf/vacf_timing.md).

    python profiles/tools/vacf_timing.py --shared-only > parent1.json    # at the parent commit: msd_window, vanhove_window alone
    python profiles/tools/vacf_timing.py > this.json                     # at this commit: everything
    python profiles/tools/vacf_timing.py --shared-only > parent2.json    # the parent once more, another process
    python profiles/tools/vacf_timing.py --report-from this.json --parent parent1.json parent2.json     # the report (no GPU)

VACF: the headline trajectory (9792 atoms x 5000 frames, the bench's random walk, resident in HBM), every lag 0 .. 2499.  The
column stage and the correlation stage from the library's device events (amof_last_kernel_seconds 2, 3); "vacf_lds" and
"vacf_general" (AMOF_VACF_GENERAL=1) on the same first 256 atoms; "vacf_lds" with two column buffers where the rule takes one
(AMOF_VACF_DB=1); the fma rate of the correlation stage against the float64
vector peak it assumes.  Shared code: msd_window and vanhove_window at the headline's 25 windows, kernel seconds of the whole
call.  Every figure: the first call on its own, then the median, minimum and maximum of five warm calls."""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# "MI355X's FP64 vector rate is high (~78 TFLOP/s, half its FP32 rate)" -- 256 CUs x 64 fma lanes x 2.4 GHz
PEAK_F64_FMA_PER_S = 78.0e12 / 2
# hipcc -Rpass-analysis=kernel-resource-usage, gfx950 (VGPRs, scratch bytes per lane, waves per SIMD by registers)
RESOURCES = [("vacf_lds_kernel<true>", 98, 0, 4), ("vacf_lds_kernel<false>", 76, 0, 6), ("vacf_general_kernel", 15, 0, 8),
             ("vacf_reduce_kernel", 13, 0, 8), ("velocity_transpose_kernel", 12, 0, 6)]
SUB_ATOMS = 256


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
    F = traj.n_frames
    window = np.arange(0, F // 2, 100, dtype=np.int32)
    nbins = int(float(np.min(traj.cell_lengths()) / 2) // 0.01)
    out = {}
    out["msd"], _ = measure(lambda: ctx.msd_window(traj, window), lambda: (ctx.last_kernel_seconds(dominant=False),), ("all_s",))
    out["msd"]["path"] = ctx.last_path()
    out["vanhove"], _ = measure(lambda: ctx.vanhove_window(traj, window, 0.01, nbins),
                                lambda: (ctx.last_kernel_seconds(dominant=False),), ("all_s",))
    out["vanhove"]["path"] = ctx.last_path()
    return out


def vacf(ctx, traj):
    F, N = traj.n_frames, traj.n_atoms
    window = np.arange(F // 2, dtype=np.int32)
    out = {"lags": len(window)}

    def read():
        st = ctx.last_stage_seconds()
        return ctx.last_kernel_seconds(dominant=False), st["rho"], st["corr"], ctx.last_kernel_seconds(dominant=True)
    names = ("all_s", "columns_s", "corr_s", "kernel_s")
    out["whole"], whole = measure(lambda: ctx.vacf_window(traj, window), read, names)
    out["whole"]["path"] = ctx.last_path()
    os.environ["AMOF_VACF_DB"] = "1"
    try:
        out["whole_db"], whole_db = measure(lambda: ctx.vacf_window(traj, window), read, names)
    finally:
        os.environ.pop("AMOF_VACF_DB", None)
    assert ctx.last_path() == "vacf_lds" and np.array_equal(whole[0].view(np.uint64), whole_db[0].view(np.uint64))
    sub = (0, min(SUB_ATOMS, N))
    out["sub_lds"], fast = measure(lambda: ctx.vacf_window(traj, window, atom_range=sub), read, names)
    out["sub_lds"]["path"] = ctx.last_path()
    os.environ["AMOF_VACF_GENERAL"] = "1"
    try:
        out["sub_general"], general = measure(lambda: ctx.vacf_window(traj, window, atom_range=sub), read, names)
        out["sub_general"]["path"] = ctx.last_path()
    finally:
        os.environ.pop("AMOF_VACF_GENERAL", None)
    assert (out["whole"]["path"], out["sub_lds"]["path"], out["sub_general"]["path"]) == ("vacf_lds", "vacf_lds", "vacf_general")
    assert np.array_equal(fast[0].view(np.uint64), general[0].view(np.uint64)), "the kernels differ"
    out["sub_atoms"] = sub[1]
    # products the definition asks for: 3 N n(m) per lag
    out["fma"] = float(3 * N * sum(max(F - int(m) - 1, 0) for m in window))
    out["c0"] = [float(x) for x in whole[0][:, 0]]
    return out


def line(name, rec, key):
    s = rec[key]
    return "| %s | %.3f | %.3f | %.3f | %.3f |" % (name, 1e3 * s["first"], 1e3 * s["median"], 1e3 * s["min"], 1e3 * s["max"])


def report(out, parent):
    v = out["vacf"]
    head = "| | first call (ms) | median of 5 warm (ms) | min | max |\n|---|---|---|---|---|"
    rate = v["fma"] / v["whole"]["kernel_s"]["median"]
    ratio = v["sub_general"]["kernel_s"]["median"] / v["sub_lds"]["kernel_s"]["median"]
    text = ["# amof_vacf_window on MI355X", "",
            "%d atoms x %d frames (the headline trajectory, resident in HBM), every lag 0 .. %d, origin stride 1, positions mode;"
            " kernel time from the library's device events." % (out["atoms"], out["frames"], v["lags"] - 1), "",
            "## The whole system on \"%s\"" % v["whole"]["path"], "", head, line("whole call", v["whole"], "all_s"),
            line("column stage (build_step_columns)", v["whole"], "columns_s"),
            line("correlation stage (kernel + reduction)", v["whole"], "corr_s"), line("vacf_lds_kernel alone", v["whole"], "kernel_s"), "",
            "The definition asks for %.3e products (3 N n(m) summed over the lags).  Over the kernel's median that is %.2f T fma/s,"
            " %.0f %% of the %.0f T fma/s of the float64 vector peak assumed here (SURVEY.md section 7: about 78 TFLOP/s, i.e. 256 CUs x 64"
            " lanes x 2.4 GHz; not measured in this project).  The kernel also multiplies the zero tail of the lanes that share a wave"
            " with shorter lags and the padding lanes of the last wave: those products are not counted." % (
                v["fma"], rate / 1e12, 100.0 * rate / PEAK_F64_FMA_PER_S, PEAK_F64_FMA_PER_S / 1e12), "",
            "## One column buffer or two", "",
            "At this shape a column and its zero tail are 5000 + 2828 doubles, 62 624 bytes: with one buffer two workgroups share"
            " a CU, with two (the next column loaded behind the arithmetic; AMOF_VACF_DB=1) one workgroup owns it.  vacf_select takes"
            " the second buffer only where two workgroups with two buffers each fit the 160 KiB of a CU.  Same bits either way"
            " (checked in this run).", "", head,
            line("vacf_lds_kernel, one buffer (the rule)", v["whole"], "kernel_s"),
            line("vacf_lds_kernel, two buffers", v["whole_db"], "kernel_s"), "",
            "## Both kernels on the same first %d atoms" % v["sub_atoms"], "", head,
            line("vacf_lds, kernel", v["sub_lds"], "kernel_s"), line("vacf_general, kernel", v["sub_general"], "kernel_s"),
            line("vacf_lds, whole call", v["sub_lds"], "all_s"), line("vacf_general, whole call", v["sub_general"], "all_s"), "",
            "vacf_general / vacf_lds (kernel medians): %.2f.  The two results are the same bits (checked in this run).  %s" % (
                ratio, "vacf_lds beats vacf_general: it ships." if ratio > 1.0 else "vacf_lds does NOT beat vacf_general."), "",
            "## Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)", "",
            "| kernel | VGPRs | scratch (B/lane) | waves/SIMD by registers |", "|---|---|---|---|"]
    text += ["| %s | %d | %d | %d |" % r for r in RESOURCES]
    text += ["", "vacf_lds at this shape: one lag tile of 256 lanes (11 lags each).", "",
             "## Shared code: WindowMsd's and WindowVanHove's entry points at the headline's 25 windows", "",
             "msd_columns.h is unchanged and every translation unit compiles its own copy of its kernels.", "", head]
    for name, key in (("msd_window", "msd"), ("vanhove_window", "vanhove")):
        for i, p in enumerate(parent):
            text.append(line("%s (%s), parent commit, process %d" % (name, p["shared"][key]["path"], i + 1), p["shared"][key], "all_s"))
        text.append(line("%s (%s), this commit" % (name, out["shared"][key]["path"]), out["shared"][key], "all_s"))
    if parent:
        text += ["", "The session's spread: the largest max - min of a process's five warm calls, or the distance between the parent's"
                 " processes where that is larger (every process generates the trajectory anew)."]
        for name, key in (("msd_window", "msd"), ("vanhove_window", "vanhove")):
            ps, n = [p["shared"][key]["all_s"] for p in parent], out["shared"][key]["all_s"]
            meds = [p["median"] for p in ps]
            spread = max([p["spread"] for p in ps] + [n["spread"], max(meds) - min(meds)])
            dist = min(abs(n["median"] - m) for m in meds)
            text.append("%s: median %.3f ms against the parent's %s ms; the session's spread is %.3f ms: %s." % (
                name, 1e3 * n["median"], " / ".join("%.3f" % (1e3 * m) for m in meds), 1e3 * spread,
                "within it" if dist <= spread else "BEYOND it"))
    return "\n".join(text) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shared-only", action="store_true")
    ap.add_argument("--parent", default=[], nargs="*", help="JSON of --shared-only runs at the parent commit")
    ap.add_argument("--report-from", default=None, help="JSON of a full run at this commit: write the report from it")
    ap.add_argument("--frames", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vacf", "vacf_timing.md"))
    args = ap.parse_args()
    parent = [json.load(open(p)) for p in args.parent]
    if args.report_from:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report(json.load(open(args.report_from)), parent))
        return
    import torch
    from amof_amd import _hip
    from tests import helpers as H
    traj = H.device_walk(torch.device("cuda", 0), (3, 3, 4), args.frames, 0.05, 20261003)
    torch.cuda.synchronize()
    ctx = _hip.get_context(0)
    out = {"atoms": int(traj.n_atoms), "frames": args.frames, "shared": shared(ctx, traj)}
    if not args.shared_only:
        out["vacf"] = vacf(ctx, traj)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report(out, parent))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
