"""Stage timings of amof_bond_reorientation on the headline shape (profiles/reorientation/reorient_timing.md).

    python profiles/tools/reorient_timing.py            # prints one JSON line

9792 atoms x 5000 frames resident in HBM (the bench's random walk), {'Zn-N': 2.5}, default windows, origin_stride 1 and 25.
Per stage from amof_last_kernel_seconds (2 = bond lists, 3 = bit series, 4 = vector table + reorientation sums), and the
whole call; the first call of each entry point is reported on its own ("cold": for the reorientation it follows the
survival calls in the same process), then the median of 5 warm calls with all values.  Beside them
amof_bond_survival on the same input in the same process (4 = its correlations), whose kernels and launches this analysis
leaves as they were: the difference of the third stage and of the whole call is the cost of the new work."""

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v), "all": v}


def measure(ctx, call):
    rows = []
    for rep in range(6):
        res = call()
        st = ctx.last_stage_seconds()
        rows.append((st["rho"], st["corr"], st["self"], ctx.last_kernel_seconds(dominant=False)))
    cold, warm = rows[0], np.array(rows[1:])
    rec = {"cold": dict(zip(("list_s", "series_s", "third_s", "all_s"), [float(x) for x in cold]))}
    for k, name in enumerate(("list_s", "series_s", "third_s", "all_s")):
        rec[name] = stats(warm[:, k])
    rec["path"] = ctx.last_path()
    return rec, res


def main():
    import torch
    from amof_amd import _hip
    from amof_amd import atom as amatom
    from amof_amd.lags import window_setup
    from tests import helpers as H

    frames = int(os.environ.get("REORIENT_TIMING_FRAMES", "5000"))
    traj = H.device_walk(torch.device("cuda", 0), (3, 3, 4), frames, 0.05, 20261003)
    torch.cuda.synchronize()
    ctx = _hip.get_context(0)
    kinds, _ = _hip.packed_species(traj)
    rcm = amatom.cutoff_matrix(amatom.format_cutoff({'Zn-N': 2.5}), kinds)
    sets = [(kinds.index(30), kinds.index(7))]
    window, _ = window_setup(frames, 100, "half", 1)

    out = {"shape": {"atoms": int(traj.n_atoms), "frames": frames, "lags": int(len(window)), "set": "Zn-N", "rc": 2.5}}
    for stride in (1, 25):
        rec = {}
        rec["bond_survival"], counts = measure(ctx, lambda: ctx.bond_survival(traj, rcm, sets, window, origin_stride=stride))
        rec["bond_reorientation"], (sums, scale) = measure(
            ctx, lambda: ctx.bond_reorientation(traj, rcm, sets, window, origin_stride=stride))
        assert np.array_equal(sums[:, :, 0].view(np.uint64), counts[:, :, 1])
        rec["scale_log2"] = int(scale[0])
        rec["terms"] = int(sums[0, :, 0].sum())
        q = 2.0 ** -int(scale[0])
        with np.errstate(divide="ignore", invalid="ignore"):
            rec["c1"] = [float(x) for x in sums[0, :, 1] * q / sums[0, :, 0]]
            rec["c2"] = [float(x) for x in sums[0, :, 2] * q / sums[0, :, 0]]
        out["stride%d" % stride] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
