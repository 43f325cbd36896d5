"""Inputs that send advance_and_find_timesteps (timestep.c:142-260 with get_timestep and do_the_kick) and
drift_particle / do_box_wrapping (predict.c:129-310) down the branches the stock inputs leave out, shared by
tests/test_kick_edges_cpu.py (kick_ref against the oracle, the labels counted) and tests/test_gpu_kick_edges.py
(the device against kick_ref).  Plain numpy; the judge is tests/kick_ref.py.

kick_edge_case(comoving): about 800 particles of types 0...5 (300 gas) at four times of the integer timeline --
    t0     Ti_Current = 0: every old bin 0, every bin active (all raised; the kick intervals start in the first
           two cells of the kick tables)
    mid    Ti_Current = 2^27: old bins 1...27, ti_begstep + 2^binold == Ti_Current for the active ones (those whose
           bin is in TimeBinActive), the others in mid-step; the mask allows some raises and blocks others
    late   Ti_Current = TIMEBASE - 2^20: nothing above bin 20 is active, every raise beyond it is blocked
    end    Ti_Current = TIMEBASE: everyone ends in bin 0 with step 0 (tend = TIMEBASE: the end clamp of the tables)
`mid` runs four times: MaxSizeTimestep below dt_displacement ("max" wins), above it ("disp" wins), with
AdaptiveGravsoftForGasHsml, and with the shipped bundle's switches (grains, virtual particles, sinks, DUST_TIMESTEP).

drift_edge_case(comoving, box, when): about 600 particles; a third already at time1; MinGasHsml the median of the
drifted h; a set of particles whose drifted coordinates sit on the edges of do_box_wrapping."""
import math

import numpy as np

import kick_ref as R

TIMEBASE = R.TIMEBASE
SOFT = [0.01, 0.02, 0.005, 0.01, 0.03, 0.01]
MASK_MID = sum(1 << b for b in list(range(1, 18)) + [19, 21, 22, 24, 26])
MASK_LATE = sum(1 << b for b in list(range(1, 19)) + [20])
ALL_BINS = (1 << 29) - 1


def _tables():
    t = np.linspace(0.01, 1.0, 1000)
    return [np.cumsum(t ** 1.5) * 1e-3, np.cumsum(t ** 0.5) * 1e-3, np.cumsum(t ** 0.2) * 1e-3]


def _params(comoving, **over):
    p = dict(Ti_Current=0, Timebase_interval=1.0 / (1 << 29), ComovingIntegrationOn=0, Time=1.0, hubble_a=1.0,
             ErrTolIntAccuracy=0.025, CourantFac=0.15, MaxSizeTimestep=0.2, MinSizeTimestep=1e-12,
             dt_displacement=0.06, SofteningTable=list(SOFT), MinEgySpec=0.0, TimeBinActive=ALL_BINS,
             logTimeBegin=0.0, logTimeMax=0.0, AdaptiveGravsoftForGasHsml=0, pmgrid=0, dt_gravkickB=0.0)
    if comoving:
        p.update(ComovingIntegrationOn=1, Time=0.37, hubble_a=1.9, MinEgySpec=0.02, logTimeBegin=math.log(0.02),
                 logTimeMax=math.log(1.0))
        p["Timebase_interval"] = (p["logTimeMax"] - p["logTimeBegin"]) / (1 << 29)
    p.update(over)
    return p


def _state(seed, ngas=300, nother=500):
    rng = np.random.default_rng(seed)
    n = ngas + nother
    ptype = np.zeros(n, np.int32)
    ptype[ngas:] = 1 + np.arange(nother) % 5
    mass = np.full(n, 1e-3)
    sinks = np.where(ptype == 5)[0]
    mass[sinks] = np.where(np.arange(len(sinks)) % 2 == 0, 0.8, 0.05)
    mass[rng.choice(ngas, 3, replace=False)] = 0.0
    entropy = 0.05 * (1 + rng.random(ngas))
    entropy[rng.choice(ngas, 40, replace=False)] = 1e-3 * (1 + rng.random(40))      # under the MinEgySpec floor
    return R.state(
        type=ptype, mass=mass, vel=rng.standard_normal((n, 3)),
        grav=rng.standard_normal((n, 3)) * 10 ** rng.uniform(-3.5, 4.5, (n, 1)),
        hyd=rng.standard_normal((ngas, 3)) * 3.0, velpred=rng.standard_normal((ngas, 3)), entropy=entropy,
        dtentropy=np.where(rng.random(ngas) < 0.3, -50.0, 0.3) * rng.random(ngas),
        density=1.0 + rng.random(ngas), hsml=0.02 * (0.5 + rng.random(n)),
        vsig=(0.5 + 2 * rng.random(ngas)) * 10 ** rng.uniform(-1.5, 1.5, ngas),
        timebin=np.zeros(n, np.int32), ti_begstep=np.zeros(n, np.int32),
        drag=rng.standard_normal((ngas, 3)) * 2.0, ddm=rng.standard_normal((ngas, 3)) * 1e-4)


def _bins(s, rng, ti, mask, lo, hi):
    """old bins lo...hi; a particle whose bin is in `mask` is active and ends its step at `ti`, the others are
    half-way through theirs.  Returns the active list."""
    n = len(s["type"])
    b = rng.integers(lo, hi + 1, n).astype(np.int32)
    on = ((mask >> b) & 1).astype(bool)
    s["timebin"][:] = b
    s["ti_begstep"][:] = np.where(on, ti - (1 << b.astype(np.int64)), ti - (1 << b.astype(np.int64)) // 2)
    assert s["ti_begstep"].min() >= 0
    return np.where(on)[0].astype(np.int32)


def kick_edge_case(comoving, seed=41):
    """-> the runs, each dict(name, p, f, s, active, tables): p the kick parameters, f kick_ref's flags, s the
    state before the kick (R.state; nobody changes it: copy it), active None or the list, tables the three tables
    (drift, gravkick, hydrokick) or None.  flagfree: f is the minimal flag set (the oracle restates it)."""
    tabs = _tables() if comoving else None
    runs = []

    def add(name, ti, mask, lo, hi, f=None, sd=0, **over):
        s = _state(seed + sd)
        rng = np.random.default_rng(seed + 100 + sd)
        active = None
        if lo == hi == 0:
            pass
        else:
            active = _bins(s, rng, ti, mask, lo, hi)
            if len(active) == len(s["type"]):
                active = None
        runs.append(dict(name=name, p=_params(comoving, Ti_Current=ti, TimeBinActive=mask, **over),
                         f=R.flags() if f is None else f, flagfree=f is None, s=s, active=active, tables=tabs))

    bundle = R.bundle(OuterBoundary=300.0, FeedBackVelocity=10.0)
    add("t0", 0, ALL_BINS, 0, 0)
    add("mid-max", 1 << 27, MASK_MID, 1, 27, sd=1, MaxSizeTimestep=0.05, dt_displacement=0.1)
    add("mid-disp", 1 << 27, MASK_MID, 1, 27, sd=2)
    add("mid-adaptive", 1 << 27, MASK_MID, 1, 27, sd=3, AdaptiveGravsoftForGasHsml=1)
    add("mid-bundle", 1 << 27, MASK_MID, 1, 27, f=bundle, sd=4)
    add("late", TIMEBASE - (1 << 20), MASK_LATE, 1, 22, sd=5)
    add("end", TIMEBASE, ALL_BINS, 1, 28, sd=6)
    return runs


def copy_state(s):
    return {k: v.copy() for k, v in s.items()}


def run_reference(run):
    """kick_ref on a copy of the run's state -> (state after, result of advance_timesteps, trace)"""
    s = copy_state(run["s"])
    trace = {}
    out = R.advance_timesteps(run["p"], run["f"], s, active=run["active"],
                              tables=None if run["tables"] is None else run["tables"][1:], trace=trace)
    return s, out, trace


def table_cells(run, s_before, s_after):
    """which cells of the kick tables the run's kick intervals end in: the set of "first" (i <= 1), "interior",
    "clamp" (i >= DRIFT_TABLE_LENGTH) over tstart, tcurrent and tend of every kicked particle"""
    p = run["p"]
    idx = np.arange(len(s_before["type"])) if run["active"] is None else run["active"]
    cells = set()
    for i in idx:
        bo, bn = int(s_before["timebin"][i]), int(s_after["timebin"][i])
        so, sn = (1 << bo) if bo else 0, (1 << bn) if bn else 0
        tb0 = int(s_before["ti_begstep"][i])
        for t in (tb0 + so // 2, tb0 + so, tb0 + so + sn // 2):
            u = (t * p["Timebase_interval"]) / (p["logTimeMax"] - p["logTimeBegin"]) * R.TABLE
            cells.add("first" if int(u) <= 1 else "clamp" if int(u) >= R.TABLE else "interior")
    return cells


# ------------------------------------------------------------------------------------------------
# endrun codes: one offending particle among valid ones
# ------------------------------------------------------------------------------------------------
def endrun_cases():
    """-> [(name, code, p, s, i)]: the non-comoving `late` state (Ti_Current = TIMEBASE - 2^20) with everyone in
    bin 18 and accelerations that keep every new step within bins 16 ... 20, and one particle, i, that fails one
    check.  Without particle i's change every case passes (asserted on the CPU)."""
    out = []
    base = [r for r in kick_edge_case(False) if r["name"] == "late"][0]

    def case(name, code, accel=None, allow=None, **over):
        s = copy_state(base["s"])
        n = len(s["type"])
        i = 400
        rng = np.random.default_rng(61)
        g = rng.standard_normal((n, 3))           # |GravAccel| in 10^2.5 ... 10^4: steps of bins 16 ... 20
        s["grav"] = g / np.linalg.norm(g, axis=1)[:, None] * 10 ** rng.uniform(2.5, 4.0, (n, 1))
        s["timebin"][:] = 18
        s["ti_begstep"][:] = base["p"]["Ti_Current"] - (1 << 18)
        p = dict(base["p"], TimeBinActive=MASK_LATE, MinSizeTimestep=0.0)
        p.update(over)
        soft = p["SofteningTable"][int(s["type"][i])]
        if accel is not None:                     # dt = accel x Timebase_interval for particle i alone
            dt = accel * p["Timebase_interval"]
            s["grav"][i] = [2 * p["ErrTolIntAccuracy"] * soft / (dt * dt), 0.0, 0.0]
        if allow is not None:                     # particle i: tiny acceleration, old bin 20, bin 21 active
            s["grav"][i] = [1e-6, 0.0, 0.0]
            s["timebin"][i] = 20
            s["ti_begstep"][i] = p["Ti_Current"] - (1 << 20)
            p["TimeBinActive"] = MASK_LATE | (1 << allow)
            p["MaxSizeTimestep"] = p["dt_displacement"] = (1 << allow) * p["Timebase_interval"] * 1.5
        out.append((name, code, p, s, i))
    # dt of particle i below MinSizeTimestep, everyone else above it
    case("888-min", 888, accel=1000.0, MinSizeTimestep=1e-5)
    case("818", 818, accel=0.5)                   # dt / Timebase_interval truncates to 0
    case("112313", 112313, accel=1.5)             # ti_step == 1: get_timestep_bin's endrun
    case("888-end", 888, allow=21)                # TIMEBASE - Ti_Current = 2^20 < ti_step = 2^21
    return out


# ------------------------------------------------------------------------------------------------
# drift
# ------------------------------------------------------------------------------------------------
DRIFT_WHEN = ("first", "interior", "end")
WRAP_ROWS = 8


def drift_edge_case(comoving, box, when, seed=51):
    """-> dict(p, s, time1, tables, noop, wrapset, box): s is kick_ref's state with pos, ti_current, divvel and
    pressure; p the drift parameters with box_wrap and BoxSize.  when: where [time0, time1] lies on the tables --
    "first" (both in the first two cells, where the factor is u * table[0]), "interior", "end" (time1 = TIMEBASE: the end clamp; time0 from the first
    cell to the interior).  noop: the third of the particles with ti_current == time1.  wrapset: particles with
    velocity 0 whose coordinates are, row by row and in all three axes, -1e-17, BoxSize, -2.25 and -2.5 boxes
    (the far edge of the span), 2.25 and 2 boxes, -1 box and the largest number below BoxSize; not comoving, where
    dt is a power of two and Vel * dt therefore exact, a second set reaches the same coordinates by drifting from
    0.25 boxes (from 0.0 for the first row)."""
    rng = np.random.default_rng(seed)
    ngas, nother = 240, 360
    n = ngas + nother
    s = _state(seed, ngas, nother)
    s["grav"] = rng.standard_normal((n, 3))
    s["timebin"][:] = rng.integers(1, 4, n)
    time1 = {"first": 1 << 20, "interior": 3 << 27, "end": TIMEBASE}[when]
    span = {"first": 1 << 18, "interior": 1 << 27, "end": 1 << 28}[when]
    # time0: time1 (no-op), time1 - span, or time1 - 2 span.  "first": a table cell is 2^29 / 1000 = 2^19.03 ticks,
    # so time1 = 2^20 and time0 = 3 x 2^18 lie in cell 1, time0 = 2^19 in cell 0: both sides of `i <= 1` with i = 1
    # on either end of the interval.  "end": time0 = 2^28 (interior) and 0.
    k = rng.integers(0, 3, n)
    k[:WRAP_ROWS] = np.arange(WRAP_ROWS) % 3            # the wrap set has all three kinds as well
    time0 = (time1 - k.astype(np.int64) * span).astype(np.int32)
    p = _params(comoving)
    dp = dict(Timebase_interval=p["Timebase_interval"], ComovingIntegrationOn=p["ComovingIntegrationOn"],
              logTimeBegin=p["logTimeBegin"], logTimeMax=p["logTimeMax"], MinGasHsml=0.0, box_wrap=1,
              BoxSize=float(box))
    speed = 0.2 * box / (2 * span * p["Timebase_interval"]) if not comoving else 0.2 * box
    s["vel"] = speed * rng.standard_normal((n, 3)) / 3.0
    s["pos"] = box * rng.random((n, 3))
    s["ti_current"] = time0
    s["divvel"] = rng.standard_normal(ngas) / (2 * span * p["Timebase_interval"]) * (0.2 if not comoving else 1e-3)
    s["pressure"] = rng.random(ngas)
    s["hsml"][:ngas] = 0.03 * box * (0.5 + rng.random(ngas))
    below = float(np.nextafter(box, 0.0))
    rows = np.array([-1e-17, box, -2.25 * box, -2.5 * box, 2.25 * box, 2.0 * box, -box, below])
    wrapset = np.arange(WRAP_ROWS)
    s["vel"][wrapset] = 0.0
    s["pos"][wrapset] = rows[:, None]
    if not comoving:
        drifted = np.arange(n - WRAP_ROWS, n)
        s["ti_current"][drifted] = time1 - span
        dt = span * p["Timebase_interval"]                 # a power of two
        start = np.full(WRAP_ROWS, 0.25 * box)
        start[0] = 0.0
        s["pos"][drifted] = start[:, None]
        s["vel"][drifted] = ((rows - start) / dt)[:, None]
        want = start + ((rows - start) / dt) * dt
        keep = want == rows                                # rows a quarter box cannot reach exactly stay out
        keep[7] = False
        drifted = drifted[keep]
        wrapset = np.concatenate([wrapset, drifted])
    noop = np.where(s["ti_current"] == time1)[0]
    return dict(p=dp, s=s, time1=time1, tables=_tables() if comoving else None, noop=noop, wrapset=wrapset,
                box=float(box), rows=rows)


def drift_reference(case):
    """kick_ref.drift on a copy; MinGasHsml = the median (times 1 + 1e-6) of the h a clamp-free drift gives the moved
    gas, so that it sits above some and below others.  -> (state after, p with MinGasHsml, (clamped, free) counts)"""
    s = copy_state(case["s"])
    assert R.drift(case["p"], R.flags(), s, case["time1"], tables=case["tables"]) == 0
    ngas = len(s["entropy"])
    moved = np.where(case["s"]["ti_current"][:ngas] != case["time1"])[0]
    minh = float(np.median(s["hsml"][moved])) * (1 + 1e-6)      # off the median itself: no h within rounding of it
    assert np.abs(s["hsml"][moved] / minh - 1).min() > 1e-10
    p = dict(case["p"], MinGasHsml=minh)
    s = copy_state(case["s"])
    assert R.drift(p, R.flags(), s, case["time1"], tables=case["tables"]) == 0
    clamped = int((s["hsml"][moved] == minh).sum())
    return s, p, (clamped, len(moved) - clamped)
