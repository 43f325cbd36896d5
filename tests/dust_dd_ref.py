"""The order in which the reference's multi-rank dust_drag applies the grains to a gas particle, on top of
the serial restatement of tests/dust_ref.py.  Nothing here imports the product.

With one export round (dust.c:560-746) a task first applies its own grains in the order of its active
list (dust_evaluate_select, mode 0), then the imported ones: the export table is sorted by task and,
within a task, by the sender's local particle index (DataIndexTable[].Index, dust.c:617-621), and the
received records are evaluated in that order (Recv_offset, rank by rank)."""
import numpy as np

import dust_ref as R


def rank_orders(lists, local):
    """lists[s]: the grains of rank s as positions in a global grain table, in rank s's list order;
    local[s]: their local particle indices on rank s.  Returns per rank s the grain positions in the order
    a gas particle of rank s receives them: its own list, then the other ranks in ascending order, each by
    local particle index."""
    P = len(lists)
    out = []
    for s in range(P):
        parts = [np.asarray(lists[s], np.int64)]
        for r in range(P):
            if r != s:
                li = np.asarray(lists[r], np.int64)
                parts.append(li[np.argsort(np.asarray(local[r]), kind="stable")])
        out.append(np.concatenate(parts) if parts else np.zeros(0, np.int64))
    return out


def shard_scatter(par, gpos, ghsml, grho, dmom, de, pos, mass, ptype, ngas, dt_gas, vel, entropy, heat, orders,
                  gas_of_rank):
    """dust_ref.gas_scatter on each rank's gas (global gas indices gas_of_rank[s]) with the grains (rows of
    gpos ... in a global grain table) in that rank's order.  vel [ngas][3], entropy, heat [ngas] are
    global arrays, updated in place.  Returns the per-rank counts of gas_scatter."""
    counts = []
    for o, g in zip(orders, gas_of_rank):
        g = np.asarray(g, np.int64)
        v, e, h = vel[g].copy(), entropy[g].copy(), heat[g].copy()
        o = np.asarray(o, np.int64)
        c = R.gas_scatter(par, gpos[o], ghsml[o], grho[o], dmom[o], de[o], pos, mass, ptype, ngas, dt_gas, v,
                          e, h, gas_idx=g)
        vel[g], entropy[g], heat[g] = v, e, h
        counts.append(c)
    return counts
