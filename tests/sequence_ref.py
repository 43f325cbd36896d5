"""rearrange_particle_sequence() (sfr_eff.c:1018-1129, -DSFR -DBLACK_HOLES -DDUST) and peano_hilbert_order()
(peano.c:25-185) restated twice, on arrays of records:

* LITERALLY and serially, swaps, `i--` and the cycle-following reorder included.  A record is named by the index
  it had before the call: `P[i]` is the name of the particle_data in slot i, `SphP[i]` the name of the record whose
  sph_particle_data sits in slot i (the reference never moves SphP[] of a converted particle, so the two differ
  behind the gas block, where nothing reads SphP).
* as the SPECIFICATION of ghip_rearrange / ghip_peano_order: a stable compaction and a stable sort per block.

The reference's swap-from-the-end leaves another order than the compaction; its merge sort (mysort_peano,
peano.c:530-566, takes the left run while b1->key <= b2->key) is stable, so after the sort the two sequences can
differ only inside runs of equal keys.  TimeBinCount[] / NumForceUpdate of sfr_eff.c:1065-1072 are bookkeeping of
the host's lists, rebuilt by reconstruct_timebins(), and are not restated."""
import numpy as np


# ---- literal ----
def literal_rearrange(ptype, mass, n_gas, sfr=True, black_holes=True):
    """-> dict(P, SphP, N_gas, NumPart, count_elim, count_gaselim, count_dustelim, flag)"""
    ptype, mass = np.asarray(ptype), np.asarray(mass)
    NumPart, N_gas = len(ptype), int(n_gas)
    P = list(range(NumPart))
    SphP = list(range(N_gas))
    flag = 0
    # what cooling_and_starformation counted (sfr_eff.c:459-476): the records of the gas block that are not gas
    Stars_converted = int((ptype[:N_gas] != 0).sum())
    if sfr and Stars_converted:                                   # :1031
        N_gas -= Stars_converted                                  # :1033
        Stars_converted = 0
        for i in range(N_gas):                                    # :1036
            if ptype[P[i]] != 0:                                  # :1037
                j = N_gas
                while j < NumPart:                                # :1039
                    if ptype[P[j]] == 0:
                        break
                    j += 1
                if j >= NumPart:                                  # :1043
                    raise RuntimeError("endrun(181170)")
                psave = P[i]                                      # :1046
                P[i] = P[j]
                SphP[i] = SphP[j]
                P[j] = psave
        flag = 1
    count_elim = count_gaselim = count_dustelim = 0
    if black_holes:
        i = 0
        while i < NumPart:                                        # :1062
            if mass[P[i]] == 0:                                   # :1063
                if ptype[P[i]] == 0:                              # :1070
                    P[i] = P[N_gas - 1]                           # :1074
                    SphP[i] = SphP[N_gas - 1]
                    P[N_gas - 1] = P[NumPart - 1]                 # :1077
                    N_gas -= 1
                    count_gaselim += 1
                else:                                             # :1084, -DDUST
                    if ptype[P[i]] == 2:
                        count_dustelim += 1
                    P[i] = P[NumPart - 1]
                NumPart -= 1                                      # :1091
                i -= 1
                count_elim += 1
            i += 1
        if count_elim:
            flag = 1
    return dict(P=P[:NumPart], SphP=SphP[:N_gas], N_gas=N_gas, NumPart=NumPart, count_elim=count_elim,
                count_gaselim=count_gaselim, count_dustelim=count_dustelim, flag=flag)


def _reorder(P, SphP, Id, lo, hi):
    """reorder_gas (peano.c:106-145; SphP given) / reorder_particles (:148-185): slot i goes to slot Id[i]"""
    for i in range(lo, hi):
        if Id[i] != i:
            Psource = P[i]
            Ssource = SphP[i] if SphP is not None else None
            idsource = Id[i]
            dest = Id[i]
            while True:
                Psave = P[dest]
                Ssave = SphP[dest] if SphP is not None else None
                idsave = Id[dest]
                P[dest] = Psource
                if SphP is not None:
                    SphP[dest] = Ssource
                Id[dest] = idsource
                if dest == i:
                    break
                Psource, Ssource, idsource = Psave, Ssave, idsave
                dest = idsource


def literal_peano_order(P, SphP, key_of_slot, N_gas):
    """peano_hilbert_order on the slots (key_of_slot[i] = Key[i]); returns (P, SphP) reordered"""
    P, SphP = list(P), list(SphP)
    NumPart = len(P)
    key = [int(k) for k in key_of_slot]
    for lo, hi, S in ((0, N_gas, SphP), (N_gas, NumPart, None)):
        if hi - lo <= 0:                                          # :32, :59
            continue
        mp = sorted(range(lo, hi), key=lambda i: key[i])          # a stable sort, as mysort_peano is
        Id = {}
        for rank, i in enumerate(mp):                             # :49, :79
            Id[i] = lo + rank
        _reorder(P, S, Id, lo, hi)
    return P, SphP


def literal_sequence(ptype, mass, n_gas, key):
    """domain_Decomposition's pair of calls: rearrange, then order by the keys of the records -> the dict of
    literal_rearrange with P and SphP in their final order"""
    r = literal_rearrange(ptype, mass, n_gas)
    key = np.asarray(key)
    r["P"], r["SphP"] = literal_peano_order(r["P"], r["SphP"], [key[p] for p in r["P"]], r["N_gas"])
    return r


# ---- specification ----
def spec_rearrange(ptype, mass, n_gas, fix_converted=True, eliminate_massless=True):
    """-> dict(old_of_new, new_of_old, numpart, ngas, converted, count_elim, count_gaselim, count_dustelim, changed)"""
    ptype, mass = np.asarray(ptype), np.asarray(mass)
    n = len(ptype)
    idx = np.arange(n)
    elim = (mass == 0) if eliminate_massless else np.zeros(n, bool)
    conv = ~elim & (idx < n_gas) & (ptype != 0) if fix_converted else np.zeros(n, bool)
    gas = ~elim & (idx < n_gas) & ~conv
    other = ~elim & (idx >= n_gas)
    old_of_new = np.concatenate([idx[gas], idx[conv], idx[other]]).astype(np.int32)
    new_of_old = np.full(n, -1, np.int32)
    new_of_old[old_of_new] = np.arange(len(old_of_new), dtype=np.int32)
    return dict(old_of_new=old_of_new, new_of_old=new_of_old, numpart=len(old_of_new), ngas=int(gas.sum()),
                converted=int(conv.sum()), count_elim=int(elim.sum()), count_gaselim=int((elim & (ptype == 0)).sum()),
                count_dustelim=int((elim & (ptype == 2)).sum()),
                changed=int(elim.any() or conv.any()))


def spec_peano_order(key, n_gas):
    """-> old_of_new: each block sorted stably by key"""
    key = np.asarray(key, np.uint64)
    a = np.argsort(key[:n_gas], kind="stable")
    b = np.argsort(key[n_gas:], kind="stable") + n_gas
    return np.concatenate([a, b]).astype(np.int32)


def spec_sequence(ptype, mass, n_gas, key):
    """rearrange then order -> (dict of spec_rearrange, old_of_new of the whole: final slot -> first index)"""
    r = spec_rearrange(ptype, mass, n_gas)
    o = spec_peano_order(np.asarray(key, np.uint64)[r["old_of_new"]], r["ngas"])
    return r, r["old_of_new"][o]
