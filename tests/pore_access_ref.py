"""Pure-numpy / pure-Python restatement of the accessibility definitions of include/amof_hip.h (amof_pore_access), written
from the definitions; it never calls the product, and it is another algorithm than the library's.

The library labels without the links through the cell's faces, merges those links afterwards and resolves the windings on
the host from the links alone.  Here one breadth-first search per component walks the PERIODIC graph directly and carries
an integer image offset per point: reaching an already visited point with another offset than it has is a closed path
with that difference as its winding vector.  The dimension is ``numpy.linalg.matrix_rank`` of the vectors collected.
t* comes from a sequential offset-carrying union-find that adds the points in descending field order until the first
winding appears."""

import numpy as np


def _steps(n, pbc):
    for k in range(3):
        assert not pbc[k] or n[k] >= 3, "a periodic axis needs 3 grid points"
    return (n[1] * n[2], n[2], 1)


def components(mask, pbc=(True, True, True)):
    """``(labels int32 [nx][ny][nz], [(label, size, dimension)])`` of a boolean mask: label = the smallest linear index
    ``(i ny + j) nz + k`` of the component, -1 outside the mask; components in ascending label order"""
    mask = np.asarray(mask, dtype=bool)
    n = mask.shape
    stride = _steps(n, pbc)
    G = mask.size
    inside = mask.reshape(-1).tolist()
    label = [-1] * G
    off = [None] * G
    comps = []
    for seed in range(G):
        if not inside[seed] or label[seed] >= 0:
            continue
        label[seed] = seed
        off[seed] = (0, 0, 0)
        todo = [seed]
        size = 0
        windings = set()
        while todo:
            p = todo.pop()
            size += 1
            idx = (p // stride[0], (p // stride[1]) % n[1], p % n[2])
            here = off[p]
            for ax in range(3):
                for d in (1, -1):
                    c, shift = idx[ax] + d, 0
                    if c == n[ax]:
                        c, shift = 0, 1
                    elif c < 0:
                        c, shift = n[ax] - 1, -1
                    if shift and not pbc[ax]:
                        continue
                    q = p + (c - idx[ax]) * stride[ax]
                    if not inside[q]:
                        continue
                    o = tuple(here[k] + (shift if k == ax else 0) for k in range(3))
                    if label[q] < 0:
                        label[q] = seed
                        off[q] = o
                        todo.append(q)
                    elif o != off[q]:
                        windings.add(tuple(o[k] - off[q][k] for k in range(3)))
        dim = int(np.linalg.matrix_rank(np.array(sorted(windings), dtype=np.float64))) if windings else 0
        comps.append((seed, size, dim))
    return np.array(label, dtype=np.int32).reshape(n), comps


def access_row(comps):
    """``[accessible points, channels, pockets, largest channel dimension]`` of ``components``' list"""
    ch = [c for c in comps if c[2] > 0]
    return [sum(c[1] for c in ch), len(ch), len(comps) - len(ch), max([c[2] for c in ch] + [0])]


def access(field, thresholds, pbc=(True, True, True)):
    """``(access int64 [n_t][4], labels int32 [n_t][nx][ny][nz])`` of one frame's field: V(t) = {field >= t}, float64 compare"""
    field = np.asarray(field, dtype=np.float64)
    rows, labels = [], []
    for t in thresholds:
        lab, comps = components(field >= np.float64(t), pbc)
        rows.append(access_row(comps))
        labels.append(lab)
    return np.array(rows, dtype=np.int64).reshape(len(thresholds), 4), np.array(labels, dtype=np.int32).reshape((len(thresholds),) + field.shape)


def first_winding(field, pbc=(True, True, True), floor=None):
    """the field value at which the first winding appears when the points are added in descending order (None: never, or
    not before the values fall below ``floor``): the largest t for which {field >= t} has a channel"""
    field = np.asarray(field, dtype=np.float64)
    n = field.shape
    stride = _steps(n, pbc)
    flat = field.reshape(-1)
    order = np.argsort(-flat, kind="stable").tolist()
    vals = flat.tolist()
    G = flat.size
    parent = [-1] * G           # -1: not added yet
    off = [(0, 0, 0)] * G       # image of the point relative to its parent

    def find(x):
        path = []
        while parent[x] != x:
            path.append(x)
            x = parent[x]
        acc = (0, 0, 0)
        for y in reversed(path):
            acc = (acc[0] + off[y][0], acc[1] + off[y][1], acc[2] + off[y][2])
            off[y] = acc
            parent[y] = x
        return x, acc

    for p in order:
        if floor is not None and vals[p] < floor:
            return None
        parent[p] = p
        idx = (p // stride[0], (p // stride[1]) % n[1], p % n[2])
        for ax in range(3):
            for d in (1, -1):
                c, shift = idx[ax] + d, 0
                if c == n[ax]:
                    c, shift = 0, 1
                elif c < 0:
                    c, shift = n[ax] - 1, -1
                if shift and not pbc[ax]:
                    continue
                q = p + (c - idx[ax]) * stride[ax]
                if parent[q] < 0:
                    continue
                rp, op = find(p)
                rq, oq = find(q)
                w = tuple(op[k] + (shift if k == ax else 0) - oq[k] for k in range(3))     # image(rq) - image(rp)
                if rp == rq:
                    if w != (0, 0, 0):
                        return vals[p]
                else:
                    parent[rq] = rp
                    off[rq] = w
    return None


def free_sphere(field, pbc=(True, True, True), dmax=None):
    """``(t*, Dif / 2)`` of one frame.  ``dmax=None``: the rule of amof_pore_access_field (any sign; (-inf, -inf) without a
    channel).  With ``dmax``: amof_pore_access' rule -- t* >= 0 only, (0, 0) if V(0) has no channel, +inf where V(dmax) has a
    channel, Dif / 2 = +inf where the largest value over the channels is the cap"""
    field = np.asarray(field, dtype=np.float64)
    t = first_winding(field, pbc, floor=None if dmax is None else 0.0)
    if t is None:
        return (-np.inf, -np.inf) if dmax is None else (0.0, 0.0)
    if dmax is not None and t >= dmax:
        return np.inf, np.inf
    lab, comps = components(field >= np.float64(t), pbc)
    channels = [c[0] for c in comps if c[2] > 0]
    assert channels
    big = float(field[np.isin(lab, channels)].max())
    return float(t), (np.inf if dmax is not None and big >= dmax else big)
