"""Stage timings of IntermediateScattering's kernels on the headline shape (9792 atoms x 5000 frames, device resident,
default windows, qmax 2.0, dq 0.02): the rho table against S(q) on the same frames and vectors, the correlation kernel
against its byte model, the self part against its share of the rho table.  Prints one JSON line.

    python profiles/tools/isf_timing.py [--frames 5000] [--calls 5]
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--self-stride", type=int, default=25)
    args = ap.parse_args()
    import numpy as np
    import torch
    from amof_amd import _hip
    from amof_amd import structure_factor as sf
    from amof_amd.lags import n_origins, window_setup
    from tests import helpers as H

    F = args.frames
    packed = H.device_walk(torch.device("cuda", 0), (3, 3, 4), F, 0.05, 20261003)
    torch.cuda.synchronize()
    ctx = _hip.get_context(0)
    windows, _ = window_setup(F)
    dq, qmax = 0.02, 2.0
    nbins = sf.n_bins(qmax, dq)
    hkl = sf.enumerate_hkl(packed.cell, qmax, dq=dq)
    S = len(_hip.packed_species(packed)[0])
    K, W = len(hkl), len(windows)
    med = statistics.median

    def timed(fn, read):
        fn()                    # warm: code objects, scratch growth
        rows = []
        for _ in range(args.calls):
            fn()
            rows.append(read())
        return rows

    sq = timed(lambda: ctx.sq_accumulate(packed, hkl, dq, nbins, frame_range=(1, F)), lambda: ctx.job_stats()["kernel_s_all"])
    coh = timed(lambda: ctx.isf_accumulate(packed, hkl, windows, dq, nbins, self_part=False),
                lambda: dict(ctx.last_stage_seconds(), all=ctx.job_stats()["kernel_s_all"], path=ctx.last_path()))
    s = args.self_stride
    slf = timed(lambda: ctx.isf_accumulate(packed, hkl, windows, dq, nbins, origin_stride=s),
                lambda: dict(ctx.last_stage_seconds(), all=ctx.job_stats()["kernel_s_all"]))
    n1, ns = n_origins(F, windows, 1), n_origins(F, windows, s)
    touched = len(set(int(1 + s * o + m) for m, n in zip(windows, ns) for o in range(int(n))) |
                  set(int(1 + s * o) for o in range(int(ns[0]))))
    corr = med(r["corr"] for r in coh)
    model_bytes = float(n1[0]) * K * (1 + W) * S * 16
    exact_bytes = (float(n1[0]) + float(n1.sum())) * K * S * 16
    rho = med(r["rho"] for r in coh)
    out = {
        "shape": {"atoms": int(packed.n_atoms), "frames": F, "species": S, "vectors": K, "lags": W, "nbins": nbins,
                  "entries_stride1": int(n1.sum()), "entries_self": int(ns.sum()), "self_stride": s},
        "path": coh[0]["path"],
        "sq_kernel_s": {"median": med(sq), "all": sq},
        "isf_rho_s": {"median": rho, "all": [r["rho"] for r in coh], "vs_sq": rho / med(sq)},
        "isf_corr_s": {"median": corr, "all": [r["corr"] for r in coh], "model_bytes": model_bytes,
                       "model_bytes_per_s": model_bytes / corr, "rows_read_bytes": exact_bytes,
                       "rows_read_bytes_per_s": exact_bytes / corr},
        "isf_coherent_all_s": med(r["all"] for r in coh),
        "isf_self_s": {"median": med(r["self"] for r in slf), "all": [r["self"] for r in slf],
                       "rho_of_that_call_s": med(r["rho"] for r in slf), "frames_touched_by_that_call": touched,
                       "model_s": float(ns.sum()) / F * rho},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
