"""Stage timings and round counts of amof_fragment_stats on the headline shape; writes profiles/fragment/fragment_timing.md (and
prints one JSON line).

    python profiles/tools/fragment_timing.py [--out FILE] [--frames 50]

The first frames of the bench's random walk (9792 atoms, resident in HBM), built as profiles/tools/ring_timing.py builds it, with
two dictionaries: the ligand dictionary {'C-N': 1.6, 'C-C': 1.6, 'C-H': 1.2} with the link {'Zn-N': 2.5} (thousands of small
fragments, a handful of rounds) and the quick start's full four-cutoff dictionary (one percolating fragment: the worst case for
rounds).  Frame 0 is the reference frame; labels, kinds and centres of mass are asked for, as the class does.  Per stage from
amof_last_kernel_seconds (device events on the context's stream: 2 = adjacency, link rows included, 3 = labelling, 4 = reduction
with the census) and the whole call (0), for "fragment_frame" and, in the same process, for "fragment_global"
(AMOF_FRAGMENT_GLOBAL=1).  One cold call each, then the median of five warm calls.  Rounds per frame from
amof_fragment_round_stats.  There is no parent-commit time: the analysis is new."""

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

LIGAND = {'C-N': 1.6, 'C-C': 1.6, 'C-H': 1.2}
LINK = {'Zn-N': 2.5}
FULL = {'Zn-N': 2.5, 'C-N': 1.6, 'C-C': 1.6, 'C-H': 1.2}
NAMES = ("adjacency_s", "labelling_s", "reduction_s", "all_s")


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
    rec["rounds"] = ctx.fragment_round_stats()
    return rec, res


def main():
    import torch
    from amof_amd import _hip
    from amof_amd import atom as amatom
    from amof_amd import fragment as amfrag
    from tests import helpers as H

    frames = arg("--frames", 50)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "fragment", "fragment_timing.md")
    traj = H.device_walk(torch.device("cuda", 0), (3, 3, 4), frames, 0.05, 20261003)
    torch.cuda.synchronize()
    ctx = _hip.get_context(0)
    kinds, species = _hip.packed_species(traj)
    matrix = lambda d: amatom.cutoff_matrix(amatom.format_cutoff(d, sort_pair=True), kinds)     # noqa: E731
    out = {"shape": {"atoms": int(traj.n_atoms), "frames": frames}}
    for title, cut, link in (("ligand", LIGAND, LINK), ("full", FULL, None)):
        rcm, lm = matrix(cut), matrix(link) if link else None
        label = ctx.fragment_stats(traj, rcm, frame_range=(0, 1), per_atom=True)[3][0]
        table, formulas, _ = amfrag.kinds_of(label, species, kinds)
        first = None
        out[title] = {"cutoffs": cut, "links": link, "kinds": formulas}
        for path, env in (("fragment_frame", None), ("fragment_global", "1")):
            os.environ.pop("AMOF_FRAGMENT_GLOBAL", None)
            if env:
                os.environ["AMOF_FRAGMENT_GLOBAL"] = env
            rec, res = measure(ctx, lambda: ctx.fragment_stats(traj, rcm, link=lm, ref_label=label, kinds=table, per_atom=True, com=True))
            os.environ.pop("AMOF_FRAGMENT_GLOBAL", None)
            assert rec["path"] == path
            first = res if first is None else first
            assert all(np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(res, first)), "the two kernels differ"
            out[title][path] = rec
        summary = first[0]
        out[title]["fragments_per_frame"] = [int(summary[:, 0].min()), int(summary[:, 0].max())]
        out[title]["frames_in_reduced_trajectory"] = int(((summary[:, 3] == 0) & (summary[:, 2] == 0)).sum())
    print(json.dumps(out))

    per = 1e3 / frames
    lines = ["# amof_fragment_stats on the headline shape", "",
             "Measured on an MI355X.  %d atoms x %d frames resident in HBM; frame 0 is the reference frame; labels, shifts and" % (traj.n_atoms, frames),
             "centres of mass asked for.  Device-event spans (amof_last_kernel_seconds), median of five warm calls [min .. max], in ms",
             "PER FRAME.  Written by profiles/tools/fragment_timing.py; both kernels ran in one process and returned identical bits.",
             "There is no parent-commit time: the analysis is new.", ""]
    for title in ("ligand", "full"):
        r = out[title]
        lines += ["## %s dictionary: %s%s" % (title, r["cutoffs"], ", links %s" % r["links"] if r["links"] else ""), "",
                  "| stage | fragment_frame | fragment_global |", "|---|---|---|"]
        for name, what in zip(NAMES, ("adjacency%s" % (" (two passes)" if r["links"] else ""), "labelling (bond images, rounds)", "reduction + census", "whole call")):
            lines.append("| %s | %s | %s |" % (what, *("%.3f [%.3f .. %.3f]" % (r[p][name]["median"] * per, r[p][name]["min"] * per, r[p][name]["max"] * per)
                                                       for p in ("fragment_frame", "fragment_global"))))
        lines.append("| first (cold) call, whole | %.3f | %.3f |" % tuple(r[p]["cold"]["all_s"] * per for p in ("fragment_frame", "fragment_global")))
        rd = r["fragment_frame"]["rounds"]
        assert rd == r["fragment_global"]["rounds"]
        lines += ["", "- rounds per frame: mean %.1f, maximum %d (the same on both kernels)" % (rd["rounds"] / max(rd["frames"], 1.0), int(rd["max_rounds"])),
                  "- fragments per frame: %d .. %d; kinds of the reference frame: %d; frames whose partition equals frame 0's: %d of %d"
                  % (r["fragments_per_frame"][0], r["fragments_per_frame"][1], len(r["kinds"]), r["frames_in_reduced_trajectory"], frames),
                  "- labelling / adjacency (one pass): fragment_frame %.2f, fragment_global %.2f"
                  % tuple(r[p]["labelling_s"]["median"] / (r[p]["adjacency_s"]["median"] / (2 if r["links"] else 1)) for p in ("fragment_frame", "fragment_global")), ""]
    lines += ["The adjacency stage is ring.hip's all-pairs kernel (profiles/ring/ring_timing.md: 0.30 ms per frame and pass at 9792", "atoms); replacing it with a cell list is out of scope here.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
