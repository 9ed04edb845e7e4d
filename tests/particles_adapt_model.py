"""Particles following the mesh through stop_refining, in plain Python over
the oracle (a helper, not a test).

After the caller changed ``model.o`` (refine_completely / unrefine_completely
and stop_refining on the oracle grid), ``remesh(model)`` re-reads the leaves
and redistributes ``model.cells`` as ``Dccrg.particles_follow_mesh`` specifies:

- a cell that stays keeps its records;
- a refined parent's records go to the leaf of the new mesh that the model's
  own ``locate`` names for the stored position (not rewritten), each child's
  in the parent's order; a record whose leaf is not one of the parent's eight
  children is lost;
- the new parent of a merged family receives the removed children's records,
  ascending child id, each child's in their own order.

It works for ``ParticleModel`` and ``StretchedParticleModel`` alike: only
``locate`` differs between them.
"""
import numpy as np


def remesh(m):
    """Returns dict(to_children, to_parents, lost)."""
    old = m.cells
    m.leaves = np.sort(m.o.cells()[0])
    m._nof = {}
    now = set(int(c) for c in m.leaves)
    new = {c: [] for c in now}
    stats = dict(to_children=0, to_parents=0, lost=0)
    gone = np.array(sorted(c for c in old if c not in now), np.uint64)
    for c in old:
        if c in now:
            new[c].append(old[c])
    if gone.size:
        b = m.o.mapping.batch(gone)
        first = b["child"]
        kids = m.o.mapping.batch(first)["siblings"]
        for i, c in enumerate(int(x) for x in gone):
            rec = old[c]
            if int(first[i]) != c and int(first[i]) in now:
                # refined: the children, ascending id
                ch = [int(k) for k in kids[i]]
                assert all(k in now for k in ch), (c, ch)
                if rec.shape[0] == 0:
                    continue
                dst = m.locate(rec[:, 0:3])
                placed = np.zeros(rec.shape[0], bool)
                for k in ch:
                    sel = dst == np.uint64(k)
                    new[k].append(rec[sel])
                    placed |= sel
                stats["to_children"] += int(placed.sum())
                stats["lost"] += int((~placed).sum())
            else:
                p = int(b["parent"][i])
                assert p != c and p in now, (c, p)
                new[p].append(rec)  # gone is ascending: ascending child id
                stats["to_parents"] += rec.shape[0]
    m.cells = {c: (np.concatenate(v) if v else np.zeros((0, m.K))) for c, v in new.items()}
    return stats
