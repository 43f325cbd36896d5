"""find_next_sync_point_and_drift() without the drift, restated in NumPy from run.c:199-320 (the reference
for ghip_find_next_sync_point and the sync-point form of GHIP_DD_DECOMPOSE).  Integers only.

  run.c:199-219  the next kick of every populated bin, the least of them (over all ranks: MPI_Allreduce MIN)
  run.c:222      an output is due when that is not before All.Ti_nextoutput >= 0
  run.c:278-289  bin 0 is always active, bin n > 0 when 2^n divides the next sync point
  run.c:291-296  NumForceUpdate, its sum over the ranks, Flag_FullStep
  run.c:300-320  the active particles (chained bin-major there; here, as on the device, in ascending index)
"""
import numpy as np

TIMEBINS = 29
TIMEBASE = 1 << 29


def bin_counts(timebin, ptype):
    """TimeBinCount[32], TimeBinCountSph[32] (allvars.h:337-338) of one rank's particles"""
    tb = np.asarray(timebin, np.int64)
    cnt = np.bincount(tb, minlength=32).astype(np.int64)
    sph = np.bincount(tb[np.asarray(ptype) == 0], minlength=32).astype(np.int64)
    return cnt, sph


def next_sync_point(ti_current, ti_nextoutput, timebin, ptype, others=()):
    """The sync point of a rank that holds `timebin` / `ptype`; `others`: the time bins of the other ranks'
    particles (arrays).  Returns a dict with the members of ghip_sync_point and `active`, the rank's own active
    particle indices in ascending order (None when an output is due: the list stays as it was)."""
    cnt, sph = bin_counts(timebin, ptype)
    glob = cnt.copy()
    for t in others:
        glob += np.bincount(np.asarray(t, np.int64), minlength=32)
    ti_next = TIMEBASE
    for n in range(TIMEBINS):                                   # run.c:199-217
        if glob[n]:
            if n > 0:
                dt_bin = 1 << n
                ti_bin = (ti_current // dt_bin) * dt_bin + dt_bin
            else:
                ti_bin = ti_current
            ti_next = min(ti_next, ti_bin)
    out = dict(TimeBinCount=cnt, TimeBinCountSph=sph)
    if ti_next >= ti_nextoutput >= 0:                           # run.c:222
        out.update(Ti_next=int(ti_nextoutput), output_due=1, TimeBinActive=0, NumForceUpdate=0,
                   GlobNumForceUpdate=0, Flag_FullStep=0, active=None)
        return out
    mask, nforce, nglob = 1, int(cnt[0]), int(glob[0])          # run.c:278-289
    for n in range(1, TIMEBINS):
        if ti_next % (1 << n) == 0:
            mask |= 1 << n
            nforce += int(cnt[n])
            nglob += int(glob[n])
    tb = np.asarray(timebin, np.int64)
    active = np.nonzero((mask >> tb) & 1)[0].astype(np.int32)   # run.c:300-320, ascending
    assert len(active) == nforce                                # run.c:332 "terrible"
    out.update(Ti_next=int(ti_next), output_due=0, TimeBinActive=mask, NumForceUpdate=nforce,
               GlobNumForceUpdate=nglob, Flag_FullStep=int(nglob == int(glob[:TIMEBINS].sum())), active=active)
    return out


def same_sync_point(got, want):
    """every member of a SyncPoint (bindings) against next_sync_point's dict: the names that differ"""
    bad = [k for k in ("Ti_next", "output_due", "TimeBinActive", "NumForceUpdate", "GlobNumForceUpdate",
                       "Flag_FullStep") if int(getattr(got, k)) != int(want[k])]
    for k in ("TimeBinCount", "TimeBinCountSph"):
        if not np.array_equal(np.array(getattr(got, k)[:], np.int64), want[k]):
            bad.append(k)
    return bad
