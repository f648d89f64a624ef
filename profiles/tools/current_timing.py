"""Stage timings of CurrentCorrelation's kernels on the first frames of the headline trajectory (9792 atoms, 4 species,
device resident, qmax 2.0, dq 0.02): records, table and correlation for IntermediateScattering's default sparse lags and for
every lag up to F // 2; IntermediateScattering (coherent only) on the same vectors in the same session; and
IntermediateScattering, StructureFactor and VelocityAutocorrelation in this tree against another tree (the parent commit,
built), alternating, with the other tree's own run-to-run spread as the noise.  Device events, medians of warm calls.
Writes a markdown report and prints one JSON line.

    python profiles/tools/current_timing.py [--frames 200] [--calls 5] [--parent-tree DIR] [--out profiles/current/current_timing.md]
    python profiles/tools/current_timing.py --parent-tree DIR --stage-report profiles/current/lag_scaffold_timing.md [--rounds 4]
"""

import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
med = statistics.median


def _timed(fn, read, calls):
    fn()                    # warm: code objects, scratch growth
    rows = []
    for _ in range(calls):
        fn()
        rows.append(read())
    return rows


def _setup(frames):
    import numpy as np
    import torch
    from amof_amd import _hip
    from amof_amd import structure_factor as sf
    from tests import helpers as H
    packed = H.device_walk(torch.device("cuda", 0), (3, 3, 4), frames, 0.05, 20261003)
    torch.cuda.synchronize()
    dq, qmax = 0.02, 2.0
    return packed, _hip.get_context(0), sf.enumerate_hkl(packed.cell, qmax, dq=dq), dq, sf.n_bins(qmax, dq), np


def baseline(frames, calls):
    """kernel seconds of the three existing analyses (medians): what must not move"""
    packed, ctx, hkl, dq, nbins, np = _setup(frames)
    dense = np.arange(frames // 2, dtype=np.int32)
    total = lambda: ctx.job_stats()["kernel_s_all"]
    return {"isf": med(_timed(lambda: ctx.isf_accumulate(packed, hkl, dense[::10], dq, nbins, self_part=False), total, calls)),
            "sq": med(_timed(lambda: ctx.sq_accumulate(packed, hkl, dq, nbins, frame_range=(1, frames)), total, calls)),
            "vacf": med(_timed(lambda: ctx.vacf_window(packed, dense), total, calls))}


def current(frames, calls):
    packed, ctx, hkl, dq, nbins, np = _setup(frames)
    from amof_amd import _hip
    from amof_amd.lags import n_origins, window_setup
    sparse, _ = window_setup(frames)
    dense = np.arange(frames // 2, dtype=np.int32)
    S = len(_hip.packed_species(packed)[0])
    out = {"shape": {"atoms": int(packed.n_atoms), "frames": frames, "species": S, "vectors": int(len(hkl)), "nbins": nbins}}
    for name, windows in (("sparse", np.asarray(sparse, dtype=np.int32)), ("dense", dense)):
        cur = _timed(lambda: ctx.current_accumulate(packed, hkl, windows, dq, nbins),
                     lambda: dict(ctx.last_current_stage_seconds(), all=ctx.job_stats()["kernel_s_all"], path=ctx.last_path()), calls)
        isf = _timed(lambda: ctx.isf_accumulate(packed, hkl, windows, dq, nbins, self_part=False),
                     lambda: dict(ctx.last_stage_seconds(), all=ctx.job_stats()["kernel_s_all"]), calls)
        row = {k: med(r[k] for r in cur) for k in ("records", "table", "corr", "all")}
        row.update(path=cur[0]["path"], lags=int(len(windows)), entries=int(n_origins(frames, windows, 1).sum()),
                   isf_rho=med(r["rho"] for r in isf), isf_corr=med(r["corr"] for r in isf), isf_all=med(r["all"] for r in isf))
        row["table_vs_isf_rho"] = row["table"] / row["isf_rho"]
        row["corr_share"] = row["corr"] / row["all"]
        # the table is streamed once per lag: rows of both ends of every (lag, origin) entry
        row["corr_rows_bytes_per_s"] = 2.0 * row["entries"] * len(hkl) * S * 48 / row["corr"]
        out[name] = row
    return out


def _child(tree, frames, calls, mode="--baseline-only"):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, "--tree", tree, "--frames", str(frames),
                        "--calls", str(calls)], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("%s run in %s failed: %s" % (mode, tree, r.stderr[-1500:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


STAGES = (("C(q, t) records", "records"), ("C(q, t) table", "table"), ("C(q, t) correlation", "corr"), ("C(q, t) all kernels", "all"),
          ("F(q, t) table", "isf_rho"), ("F(q, t) correlation", "isf_corr"), ("F(q, t) all kernels", "isf_all"))


def stage_report(parent, this, calls, path):
    """the stages of both lag analyses, dense lags, this tree against the parent: inside the parent's own spread or not"""
    sh = this[0]["shape"]
    ms = lambda x: "%.3f" % (1e3 * x)
    lines = ["# F(q, t) and C(q, t): stage timings, this tree against the parent commit", "",
             "%d atoms, %d species, %d frames (device resident), %d vectors, every lag up to %d; alternating runs in fresh processes, "
             "device events, kernel milliseconds (medians of %d warm calls each); `profiles/tools/current_timing.py --stage-report`.  "
             "Spread = min .. max of the parent's own repeated runs." % (sh["atoms"], sh["species"], sh["frames"], sh["vectors"],
                                                                         this[0]["dense"]["lags"], calls), "",
             "| stage | parent runs ms | this tree runs ms | parent spread | difference of medians | inside the spread |",
             "|---|---|---|---|---|---|"]
    verdict = {}
    for label, k in STAGES:
        p, t = [r["dense"][k] for r in parent], [r["dense"][k] for r in this]
        verdict[k] = min(p) <= med(t) <= max(p)
        lines.append("| %s | %s | %s | %.1f %% | %+.1f %% | %s |" % (label, ", ".join(ms(x) for x in p), ", ".join(ms(x) for x in t),
                                                                    100 * (max(p) - min(p)) / med(p), 100 * (med(t) - med(p)) / med(p),
                                                                    "yes" if verdict[k] else "no"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return verdict


def report(out, path):
    ms = lambda x: "%.3f" % (1e3 * x)
    sh = out["shape"]
    lines = ["# CurrentCorrelation: stage timings", "",
             "%d atoms, %d species, %d frames (device resident), %d vectors (qmax 2.0, dq 0.02, %d bins); device events, medians of "
             "%d warm calls; `profiles/tools/current_timing.py`.  R = %d vectors per thread of `current_rho_kernel`, %d VGPRs, no "
             "scratch (compiler resource report)." % (sh["atoms"], sh["species"], sh["frames"], sh["vectors"], sh["nbins"],
                                                      out["calls"], out["R"], out["vgprs"]), "",
             "| lags | entries | path | records ms | table ms | correlation ms | all kernels ms | F(q, t) table ms | F(q, t) correlation ms "
             "| table / F(q, t) table | correlation share |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in ("sparse", "dense"):
        r = out[name]
        lines.append("| %s (%d) | %d | %s | %s | %s | %s | %s | %s | %s | %.2f | %.0f %% |" % (
            name, r["lags"], r["entries"], r["path"], ms(r["records"]), ms(r["table"]), ms(r["corr"]), ms(r["all"]), ms(r["isf_rho"]),
            ms(r["isf_corr"]), r["table_vs_isf_rho"], 100 * r["corr_share"]))
    lines += ["", "The correlation stage reads both rows of every (lag, origin) entry once per lag: %.0f GB/s of table rows in the "
              "dense setting." % (out["dense"]["corr_rows_bytes_per_s"] / 1e9)]
    if "parent" in out:
        lines += ["", "## Existing analyses, this tree against the parent commit", "",
                  "Alternating runs in fresh processes, kernel milliseconds (medians of %d warm calls each); noise = the spread of the "
                  "parent's own repeated runs." % out["calls"], "",
                  "| analysis | parent runs ms | this tree runs ms | parent spread | difference of medians |", "|---|---|---|---|---|"]
        for k, label in (("isf", "IntermediateScattering (coherent, %d lags)" % len(range(0, sh["frames"] // 2, 10))),
                         ("sq", "StructureFactor"), ("vacf", "VelocityAutocorrelation (every lag)")):
            p, t = [r[k] for r in out["parent"]], [r[k] for r in out["this"]]
            lines.append("| %s | %s | %s | %.1f %% | %+.1f %% |" % (label, ", ".join(ms(x) for x in p), ", ".join(ms(x) for x in t),
                                                                   100 * (max(p) - min(p)) / med(p), 100 * (med(t) - med(p)) / med(p)))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--tree", default=HERE, help="the source tree whose package is timed")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--stages-only", action="store_true", help="print the stage timings of --tree as one JSON line")
    ap.add_argument("--stage-report", default=None, metavar="FILE", help="with --parent-tree: the stages of F(q, t) and C(q, t) in "
                    "both trees, alternating, as a markdown table")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: the existing analyses are timed in both")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--vgprs", type=int, default=88, help="VGPRs of current_rho_kernel from the compiler's resource report")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "current", "current_timing.md"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if args.baseline_only:
        print(json.dumps(baseline(args.frames, args.calls)))
        return
    if args.stages_only:
        print(json.dumps(current(args.frames, args.calls)))
        return
    if args.stage_report:
        parent, this = [], []
        for _ in range(args.rounds):
            parent.append(_child(args.parent_tree, args.frames, args.calls, "--stages-only"))
            this.append(_child(HERE, args.frames, args.calls, "--stages-only"))
        print(json.dumps({"inside_parent_spread": stage_report(parent, this, args.calls, args.stage_report), "parent": parent, "this": this}))
        return
    out = current(args.frames, args.calls)
    import re
    with open(os.path.join(HERE, "amof_amd", "csrc", "current_plan.h")) as fh:
        run = int(re.search(r"constexpr\s+int\s+CUR_RUN\s*=\s*(\d+)\s*;", fh.read()).group(1))
    out.update(calls=args.calls, R=run, vgprs=args.vgprs)
    if args.parent_tree:
        out["parent"], out["this"] = [], []
        for _ in range(args.rounds):
            out["parent"].append(_child(args.parent_tree, args.frames, args.calls))
            out["this"].append(_child(HERE, args.frames, args.calls))
    report(out, args.out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
