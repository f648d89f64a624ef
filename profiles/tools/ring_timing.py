"""Stage timings of amof_ring_stats on the headline shape; writes profiles/ring/ring_timing.md (and prints one JSON line).

    python profiles/tools/ring_timing.py [--out FILE] [--frames 10] [--depth 32]

The first frames of the bench's random walk (9792 atoms, resident in HBM) with {'Zn-N': 2.5, 'C-N': 1.6, 'C-C': 1.6, 'C-H': 1.2}.
Per stage from amof_last_kernel_seconds (device events on the context's stream: 2 = adjacency, 3 = breadth-first searches with
the candidate passes, 4 = ring search) and the whole call (0), for "ring_wave" and, in the same process, for "ring_simple"
(AMOF_RING_SIMPLE=1: a thread per source, no candidate buffer, so its BFS span has one pass where the wave path has two).
One cold call each, then the median of five warm calls.  Candidates per source and the share that close a ring come from
amof_ring_search_stats.  Fetched bytes of the D lookups need a counter run of their own and are not collected here."""

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CUT = {'Zn-N': 2.5, 'C-N': 1.6, 'C-C': 1.6, 'C-H': 1.2}
NAMES = ("adjacency_s", "bfs_s", "search_s", "all_s")


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def measure(ctx, call):
    rows = []
    for rep in range(6):
        res = call()
        st = ctx.last_stage_seconds()
        rows.append((st["rho"], st["corr"], st["self"], ctx.last_kernel_seconds(dominant=False)))
    warm = np.array(rows[1:])
    rec = {"path": ctx.last_path(), "cold": dict(zip(NAMES, [float(x) for x in rows[0]]))}
    for k, name in enumerate(NAMES):
        rec[name] = {"median": float(np.median(warm[:, k])), "min": float(warm[:, k].min()), "max": float(warm[:, k].max())}
    rec["stats"] = ctx.ring_search_stats()
    return rec, res


def main():
    import torch
    from amof_amd import _hip
    from amof_amd import atom as amatom
    from tests import helpers as H

    frames, depth = arg("--frames", 10), arg("--depth", 32)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ring", "ring_timing.md")
    traj = H.device_walk(torch.device("cuda", 0), (3, 3, 4), frames, 0.05, 20261003)
    torch.cuda.synchronize()
    ctx = _hip.get_context(0)
    kinds, _ = _hip.packed_species(traj)
    rcm = amatom.cutoff_matrix(amatom.format_cutoff(CUT, sort_pair=True), kinds)
    out = {"shape": {"atoms": int(traj.n_atoms), "frames": frames, "max_size": depth, "cutoffs": CUT}}
    first = None
    for label, env in (("ring_wave", None), ("ring_simple", "1")):
        os.environ.pop("AMOF_RING_SIMPLE", None)
        if env:
            os.environ["AMOF_RING_SIMPLE"] = env
        rec, res = measure(ctx, lambda: ctx.ring_stats(traj, rcm, depth, per_atom=True))
        os.environ.pop("AMOF_RING_SIMPLE", None)
        assert rec["path"] == label
        first = res if first is None else first
        assert all(np.array_equal(x, y) for x, y in zip(res, first)), "the two paths differ"
        out[label] = rec
    counts, truncated, _ = first
    sizes = np.arange(counts.shape[2])
    rings = {int(n): (counts[:, 0, n] // n).tolist() for n in sizes[3:] if counts[:, 0, n].any()}
    assert not (counts[:, 0, 3:] % sizes[None, 3:]).any()
    out["rings_per_frame"] = rings
    out["truncated_sources"] = truncated.tolist()
    print(json.dumps(out))

    w, s = out["ring_wave"], out["ring_simple"]
    per = 1e3 / frames
    lines = ["# amof_ring_stats on the headline shape", "",
             "%d atoms x %d frames resident in HBM, cutoffs %s, max_size = %d.  Device-event spans" % (traj.n_atoms, frames, CUT, depth),
             "(amof_last_kernel_seconds), median of five warm calls [min .. max], in ms PER FRAME.  Written by",
             "profiles/tools/ring_timing.py; both paths ran in one process and returned identical integers.", "",
             "| stage | ring_wave | ring_simple |", "|---|---|---|"]
    for name, title in zip(NAMES, ("adjacency", "BFS + candidates", "ring search", "whole call")):
        lines.append("| %s | %s | %s |" % (title, *("%.3f [%.3f .. %.3f]" % (r[name]["median"] * per, r[name]["min"] * per, r[name]["max"] * per)
                                                    for r in (w, s))))
    lines += ["| first (cold) call, whole | %.3f | %.3f |" % (w["cold"]["all_s"] * per, s["cold"]["all_s"] * per), "",
              "ring_wave writes and reads a candidate buffer (two BFS passes: count, then write); ring_simple finds its candidates",
              "itself inside the search span (one BFS pass), so the spans to compare are the search span and the whole call.", ""]
    for label, r in (("ring_wave", w), ("ring_simple", s)):
        st = r["stats"]
        lines.append("- %s: %.1f candidates per source, %.1f %% of them close at least one ring (%d sources)"
                     % (label, st["candidates"] / max(st["sources"], 1.0), 100.0 * st["closed"] / max(st["candidates"], 1.0), int(st["sources"])))
    ratio = s["search_s"]["median"] / w["search_s"]["median"] if w["search_s"]["median"] > 0 else float("nan")
    lines += ["- search span, ring_simple / ring_wave: %.2f; whole call: %.2f" % (ratio, s["all_s"]["median"] / w["all_s"]["median"]),
              "- rings per frame by size: %s" % json.dumps(rings), "- truncated sources per frame: %s" % truncated.tolist(),
              "- fetched bytes of the D lookups: not collected (a counter run of its own)", ""]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
