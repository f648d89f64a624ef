"""Stage timings of amof_bond_survival on the headline shape (profiles/bond/bond_timing.md).

    python profiles/tools/bond_timing.py            # prints one JSON line

9792 atoms x 5000 frames resident in HBM (the bench's random walk), {'Zn-N': 2.5}, default windows, origin_stride 1 and 25.
Per stage from amof_last_kernel_seconds (2 = bond lists, 3 = bit series, 4 = correlations), one warm-up call, then 5 calls:
median and all values.  Beside them: amof_cn_count over the same 5000 frames (all kernels), the series kernel in the other
layout (AMOF_BOND_LAYOUT=frames) and the number of pairs followed (AMOF_BOND_REPORT=1, read back from stderr of a child)."""

import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v), "all": v}


def main():
    import torch
    from amof_amd import _hip
    from amof_amd import atom as amatom
    from amof_amd.lags import window_setup
    from tests import helpers as H

    frames = int(os.environ.get("BOND_TIMING_FRAMES", "5000"))
    traj = H.device_walk(torch.device("cuda", 0), (3, 3, 4), frames, 0.05, 20261003)
    torch.cuda.synchronize()
    ctx = _hip.get_context(0)
    kinds, _ = _hip.packed_species(traj)
    rcm = amatom.cutoff_matrix(amatom.format_cutoff({'Zn-N': 2.5}), kinds)
    sets = [(kinds.index(30), kinds.index(7))]
    window, _ = window_setup(frames, 100, "half", 1)

    if len(sys.argv) > 1 and sys.argv[1] == "report":       # child: one call with the pair report on stderr
        os.environ["AMOF_BOND_REPORT"] = "1"
        ctx.bond_survival(traj, rcm, sets, window, origin_stride=int(sys.argv[2]))
        return

    out = {"shape": {"atoms": int(traj.n_atoms), "frames": frames, "lags": int(len(window)), "set": "Zn-N", "rc": 2.5}}
    cn = []
    for rep in range(6):
        ctx.cn_count(traj, rcm, sets)
        cn.append(ctx.last_kernel_seconds(dominant=False))
    out["cn_count_s"] = stats(cn[1:])
    out["cn_path"] = ctx.last_path()
    for stride in (1, 25):
        rec = {}
        for layout in ("by_pair", "by_frame"):
            if layout == "by_frame":
                os.environ["AMOF_BOND_LAYOUT"] = "frames"
            else:
                os.environ.pop("AMOF_BOND_LAYOUT", None)
            rows = []
            for rep in range(6):
                counts = ctx.bond_survival(traj, rcm, sets, window, origin_stride=stride)
                st = ctx.last_stage_seconds()       # (slots 2 .. 4 of amof_last_kernel_seconds: lists, series, correlations)
                rows.append((st["rho"], st["corr"], st["self"], ctx.last_kernel_seconds(dominant=False)))
            rows = np.array(rows[1:])
            rec[layout] = {"list_s": stats(rows[:, 0]), "series_s": stats(rows[:, 1]), "corr_s": stats(rows[:, 2]),
                           "all_s": stats(rows[:, 3]), "path": ctx.last_path()}
        os.environ.pop("AMOF_BOND_LAYOUT", None)
        rec["counts_lag0"] = [int(x) for x in counts[0, 0]]
        rec["counts_last_lag"] = [int(x) for x in counts[0, -1]]
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "report", str(stride)], stderr=subprocess.PIPE,
                               stdout=subprocess.DEVNULL, timeout=600)
        if child.returncode != 0:       # a fault in the child: start nothing more on the GPU
            sys.stderr.write(child.stderr.decode()[-2000:])
            sys.exit("bond_timing: the report child ended with status %d" % child.returncode)
        pairs = sum(int(x) for x in re.findall(r"(\d+) pairs", child.stderr.decode()))
        rec["pairs"] = pairs
        model = pairs * frames * 2 * 24
        rec["series_model_bytes"] = model
        rec["series_fraction_of_8TBs"] = model / rec["by_pair"]["series_s"]["median"] / 8e12
        out["stride%d" % stride] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
