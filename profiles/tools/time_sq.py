"""S(q) at the headline shape (profiles/sq/headline.txt): 9792 atoms (ZIF-4 3x3x4, tests.helpers.device_walk) x F frames,
qmax = 5 / A, dq = 0.02.  Library event times of a few calls, the class call, and the determinism of repeated calls.

    python3 profiles/tools/time_sq.py [frames] [calls] [output directory for the JSON record]
    rocprofv3 --kernel-trace --stats -d sq_trace -- python3 profiles/tools/time_sq.py 500 2
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
from amof_amd import structure_factor as sf                 # noqa: E402
from tests import helpers as H                              # noqa: E402

F = int(sys.argv[1]) if len(sys.argv) > 1 else 500
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda", 0)
ctx = _hip.get_context(0)
packed = H.device_walk(dev, (3, 3, 4), F, 0.05, 99)
torch.cuda.synchronize()
qmax, dq = 5.0, 0.02
hkl = sf.enumerate_hkl(packed.cell, qmax)
nbins = sf.n_bins(qmax, dq)
rec = {"atoms": packed.n_atoms, "frames": F, "K": len(hkl), "nbins": nbins,
       "atom_modes_per_frame": packed.n_atoms * len(hkl), "calls": []}
first = None
for c in range(calls):
    t0 = time.perf_counter()
    res = ctx.sq_accumulate(packed, hkl, dq, nbins)
    wall = time.perf_counter() - t0
    st = ctx.job_stats()
    rec["calls"].append({"wall_s": wall, "kernel_total_s": st["kernel_s_all"], "kernel_dominant_s": st["kernel_s_dominant"],
                         "launches": st["kernel_launches"], "path": st["path"]})
    if first is None:
        first = res
    else:
        rec["bit_identical"] = bool(np.array_equal(first[0], res[0]) and np.array_equal(first[1].view(np.uint64), res[1].view(np.uint64)))
t0 = time.perf_counter()
s = sf.StructureFactor.from_trajectory(packed, dq=dq, qmax=qmax, device=0)
_ = s.data
rec["class_wall_s"] = time.perf_counter() - t0
best = min(c["kernel_total_s"] for c in rec["calls"])
rec["ms_per_frame"] = 1e3 * best / F
rec["X-X_peak"] = [float(s.data["q"].values[np.nanargmax(s.data["X-X"].values)]), float(np.nanmax(s.data["X-X"].values))]
print(json.dumps(rec, indent=1))
if len(sys.argv) > 3:
    os.makedirs(sys.argv[3], exist_ok=True)
    with open(os.path.join(sys.argv[3], "sq_headline_%d_%d.json" % (F, calls)), "w") as fh:
        json.dump(rec, fh, indent=1)
