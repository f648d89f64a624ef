"""Distinct Van Hove function at the headline shape (profiles/vanhove_distinct/headline.txt): 9792 atoms (ZIF-4 3x3x4,
tests.helpers.device_walk) x F frames, delta_time 100 (lags 0, 100, ...), origin_stride 25, dr 0.01 (half-cell rmax).
Library event times per path (the exact kernel on the first `exact_items` entries of the work list only), the time per
(origin, lag) pair, the class call, and the determinism of repeated calls.

    python3 profiles/tools/time_vanhove_distinct.py [frames] [calls] [exact_items] [output directory for the JSON record]
    rocprofv3 --kernel-trace --stats -d vhd_trace -- python3 profiles/tools/time_vanhove_distinct.py 5000 2 100
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
os.environ.setdefault("AMOF_ASYNC", "0")
import torch                                                # noqa: E402
from amof_amd import _hip                                   # noqa: E402
from amof_amd import vanhove_distinct as vd                 # noqa: E402
from amof_amd.lags import n_origins, window_setup           # noqa: E402
from tests import helpers as H                              # noqa: E402

F = int(sys.argv[1]) if len(sys.argv) > 1 else 5000
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 2
exact_items = int(sys.argv[3]) if len(sys.argv) > 3 else 100
stride = 25
ctx = _hip.get_context(0)
packed = H.device_walk(torch.device("cuda", 0), (3, 3, 4), F, 0.05, 99)
torch.cuda.synchronize()
rmax = float(np.min(packed.cell_lengths()) / 2)
nbins = int(rmax // 0.01)
windows, _ = window_setup(F, 100)
windows = windows.astype(np.int32)
items = int(n_origins(F, windows, stride).sum())
rec = {"atoms": packed.n_atoms, "frames": F, "lags": len(windows), "origin_stride": stride, "nbins": nbins, "pairs": items,
       "calls": []}


def run(env, work_range, tag):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        t0 = time.perf_counter()
        h, _ = ctx.vanhove_distinct(packed, windows, rmax, nbins, origin_stride=stride, work_range=work_range)
        wall = time.perf_counter() - t0
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    st = ctx.job_stats()
    n = work_range[1] - work_range[0]
    rec["calls"].append({"tag": tag, "pairs": n, "wall_s": wall, "kernel_total_s": st["kernel_s_all"],
                         "kernel_dominant_s": st["kernel_s_dominant"], "launches": st["kernel_launches"], "path": st["path"],
                         "us_per_pair_dominant": 1e6 * st["kernel_s_dominant"] / max(n, 1)})
    return h


first = None
for c in range(calls):
    h = run({}, (0, items), "tile")
    if first is None:
        first = h
    else:
        rec["bit_identical"] = bool(np.array_equal(first, h))
m = min(exact_items, items)
h_exact = run({"AMOF_VANHOVE_DISTINCT_EXACT": "1"}, (0, m), "exact")
h_tile = run({}, (0, m), "tile_subset")
rec["exact_equals_tile_on_subset"] = bool(np.array_equal(h_exact, h_tile))
t0 = time.perf_counter()
g = vd.DistinctVanHove.from_trajectory(packed, delta_time=100, timestep=1, dr=0.01, origin_stride=stride, device=0)
_ = g.data
rec["class_wall_s"] = time.perf_counter() - t0
zn_n = g.data["Zn-N"].values.reshape(len(windows), nbins)
rec["Zn-N_peak_by_lag"] = [[float(windows[w]), float(np.argmax(zn_n[w]) * rmax / nbins), float(zn_n[w].max())]
                           for w in range(0, len(windows), 6)]
print(json.dumps(rec, indent=1))
if len(sys.argv) > 4:
    os.makedirs(sys.argv[4], exist_ok=True)
    with open(os.path.join(sys.argv[4], "vhd_headline_%d_%d.json" % (F, calls)), "w") as fh:
        json.dump(rec, fh, indent=1)
