"""Stage timings of amof_bond_order on the headline shape (profiles/bond_order/bond_order_timing.md).

    python profiles/tools/bond_order_timing.py              # prints one JSON line
    python profiles/tools/bond_order_timing.py --bad-only   # Bad's call alone (runs on a commit without amof_bond_order)

9792 atoms x 5000 frames resident in HBM (the bench's random walk), {'Zn-N': 2.5}, l = (4, 6), 100 / 400 bins.  Per stage from
amof_last_kernel_seconds (2 = the list stage, 3 = the order kernel) and the whole call (0), for the two forms of the
per-frame sums: reduced inside the wave where its lanes share a frame (the default) and per-lane atomics
(AMOF_ORDER_SUMS=lane).  Beside them amof_bad_hist for the triple N-Zn-N on the same input in the same process: it runs the
same list stage and then bad_rows_kernel over the same rows; its dominant span (1) covers both, so Bad's dominant span minus
the list stage measured here is what bad_rows_kernel takes.  The first call of each is reported on its own, then the median
of 5 warm calls with all values."""

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v), "all": v}


def measure(ctx, call, names, read):
    rows = []
    for rep in range(6):
        res = call()
        rows.append(read())
    cold, warm = rows[0], np.array(rows[1:])
    rec = {"cold": dict(zip(names, [float(x) for x in cold]))}
    for k, name in enumerate(names):
        rec[name] = stats(warm[:, k])
    rec["path"] = ctx.last_path()
    return rec, res


def main():
    import torch
    from amof_amd import _hip
    from amof_amd import atom as amatom
    from tests import helpers as H

    frames = int(os.environ.get("ORDER_TIMING_FRAMES", "5000"))
    traj = H.device_walk(torch.device("cuda", 0), (3, 3, 4), frames, 0.05, 20261003)
    torch.cuda.synchronize()
    ctx = _hip.get_context(0)
    kinds, _ = _hip.packed_species(traj)
    rcm = amatom.cutoff_matrix(amatom.format_cutoff({'Zn-N': 2.5}), kinds)
    zn, n = kinds.index(30), kinds.index(7)
    edges = np.arange(int(180 // 0.5) + 2) * 0.5

    out = {"shape": {"atoms": int(traj.n_atoms), "frames": frames, "set": "Zn-N", "rc": 2.5, "l": [4, 6], "nbins": 100,
                     "nbins_tet": 400}}
    out["bad_N-Zn-N"], (hist, nang) = measure(
        ctx, lambda: ctx.bad_hist(traj, rcm, [(zn, n)], edges), ("dominant_s", "all_s"),
        lambda: (ctx.last_kernel_seconds(dominant=True), ctx.last_kernel_seconds(dominant=False)))
    out["angles"] = int(nang[0])
    if "--bad-only" not in sys.argv:
        def read():
            st = ctx.last_stage_seconds()
            return st["rho"], st["corr"], ctx.last_kernel_seconds(dominant=False)
        first = None
        for label, value in (("wave_sums", None), ("lane_sums", "lane")):
            if value is None:
                os.environ.pop("AMOF_ORDER_SUMS", None)
            else:
                os.environ["AMOF_ORDER_SUMS"] = value
            rec, res = measure(ctx, lambda: ctx.bond_order(traj, rcm, [(zn, n)], (4, 6), 100, 400), ("list_s", "order_s", "all_s"), read)
            os.environ.pop("AMOF_ORDER_SUMS", None)
            first = res if first is None else first
            assert all(np.array_equal(x, y) for x, y in zip(res, first))
            out["bond_order_" + label] = rec
        hist_q, hist_tet, sums = first
        assert int(sums[:, 0, 3].sum()) == int(nang[0])
        centres = float(sums[:, 0, 1].sum())
        out["mean_q4"] = float(sums[:, 0, 4].sum() * 2.0 ** -30 / centres)
        out["mean_q6"] = float(sums[:, 0, 5].sum() * 2.0 ** -30 / centres)
        out["mean_qtet"] = float(sums[:, 0, 6].sum() * 2.0 ** -30 / max(1.0, float(sums[:, 0, 2].sum())))
        out["f4"] = float(sums[:, 0, 2].sum() / (frames * float((np.asarray(traj.numbers) == 30).sum())))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
