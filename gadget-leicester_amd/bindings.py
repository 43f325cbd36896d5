"""ctypes bindings of libghip.so (include/ghip.h).  Thin: every method is one C call.

No CPU fallback: constructing ForcePath without the library or without a GPU raises.
"""
import ctypes as C
import importlib
import os

import numpy as np

_pkg = importlib.import_module(__package__)

# enum ghip_field
(F_POS, F_VEL, F_MASS, F_TYPE, F_OLDACC, F_HSML, F_TIMEBIN, F_TI_BEGSTEP, F_VELPRED, F_ENTROPY,
 F_DTENTROPY, F_GRAVACCEL, F_GRAVCOST, F_NUMNGB, F_DENSITY, F_DHSMLFAC, F_DIVVEL, F_CURLVEL,
 F_PRESSURE, F_HYDROACCEL, F_MAXSIGNALVEL, F_TI_CURRENT, F_GRAVPM, F_ID, F_COUNT) = range(25)

_FIELD_INFO = {  # gas-sized?, ncomp, is int
    F_POS: (0, 3, 0), F_VEL: (0, 3, 0), F_MASS: (0, 1, 0), F_TYPE: (0, 1, 1), F_OLDACC: (0, 1, 0),
    F_HSML: (0, 1, 0), F_TIMEBIN: (0, 1, 1), F_TI_BEGSTEP: (0, 1, 1), F_VELPRED: (1, 3, 0),
    F_ENTROPY: (1, 1, 0), F_DTENTROPY: (1, 1, 0), F_GRAVACCEL: (0, 3, 0), F_GRAVCOST: (0, 1, 1),
    F_NUMNGB: (1, 1, 0), F_DENSITY: (1, 1, 0), F_DHSMLFAC: (1, 1, 0), F_DIVVEL: (1, 1, 0),
    F_CURLVEL: (1, 1, 0), F_PRESSURE: (1, 1, 0), F_HYDROACCEL: (1, 3, 0), F_MAXSIGNALVEL: (1, 1, 0),
    F_TI_CURRENT: (0, 1, 1), F_GRAVPM: (0, 3, 0), F_ID: (0, 1, 1)}

WALK_NEWTON, WALK_SHORTRANGE, WALK_EWALD, WALK_NEWTON_EWALD = 0, 1, 2, 3
PRIM_SCAN, PRIM_WSCAN, PRIM_SELECT, PRIM_WSELECT, PRIM_SORT_U32 = 0, 1, 2, 3, 4   # ghip_debug_prim
EN = 64

GHIP_ERRORS = {-90001: "GHIP_EHIP", -90002: "GHIP_EINVAL", -90003: "GHIP_ENOMEM",
               -90004: "GHIP_ENOCONV", -90005: "GHIP_ENODEVICE", -90006: "GHIP_ETIMESTEP",
               -90008: "GHIP_EDEVICE", -90009: "GHIP_ECOMM", -90010: "GHIP_EREGION"}
GHIP_ENOCONV = -90004


class Layout(C.Structure):
    _fields_ = [(k, C.c_int) for k in (
        "p_stride", "p_pos", "p_vel", "p_mass", "p_gravaccel", "p_oldacc", "p_gravcost",
        "p_ti_begstep", "p_type", "p_timebin", "p_hsml", "p_numngb",
        "s_stride", "s_entropy", "s_pressure", "s_velpred", "s_maxsignalvel", "s_density",
        "s_dtentropy", "s_hydroaccel", "s_dhsmlfac", "s_divvel", "s_curlvel", "s_hsml",
        "s_numngb", "p_ti_current", "p_gravpm")]


class GravParams(C.Structure):
    _fields_ = [("ErrTolTheta", C.c_double), ("ErrTolForceAcc", C.c_double),
                ("ForceSoftening", C.c_double * 6), ("BoxSize", C.c_double),
                ("periodic", C.c_int), ("unequal_softenings", C.c_int),
                ("Rcut", C.c_double), ("Asmth", C.c_double)]


class DensParams(C.Structure):
    _fields_ = [("DesNumNgb", C.c_double), ("MaxNumNgbDeviation", C.c_double),
                ("MinGasHsml", C.c_double), ("BoxSize", C.c_double), ("periodic", C.c_int),
                ("Ti_Current", C.c_int), ("Timebase_interval", C.c_double), ("MaxIter", C.c_int)]


class HydroParams(C.Structure):
    _fields_ = [("ArtBulkViscConst", C.c_double), ("BoxSize", C.c_double), ("periodic", C.c_int),
                ("ComovingIntegrationOn", C.c_int), ("hubble_a2", C.c_double),
                ("fac_mu", C.c_double), ("fac_vsic_fix", C.c_double),
                ("Timebase_interval", C.c_double), ("raw_dtentropy", C.c_int)]


class DriftParams(C.Structure):
    _fields_ = [("time1", C.c_int), ("Timebase_interval", C.c_double),
                ("ComovingIntegrationOn", C.c_int), ("logTimeBegin", C.c_double),
                ("logTimeMax", C.c_double), ("DriftTable", C.c_void_p),
                ("GravKickTable", C.c_void_p), ("HydroKickTable", C.c_void_p),
                ("MinGasHsml", C.c_double), ("box_wrap", C.c_int), ("BoxSize", C.c_double),
                ("pmgrid", C.c_int)]


class KickParams(C.Structure):
    _fields_ = [("Ti_Current", C.c_int), ("Timebase_interval", C.c_double),
                ("ComovingIntegrationOn", C.c_int), ("Time", C.c_double), ("hubble_a", C.c_double),
                ("ErrTolIntAccuracy", C.c_double), ("CourantFac", C.c_double),
                ("MaxSizeTimestep", C.c_double), ("MinSizeTimestep", C.c_double),
                ("dt_displacement", C.c_double), ("SofteningTable", C.c_double * 6),
                ("MinEgySpec", C.c_double), ("TimeBinActive", C.c_uint),
                ("logTimeBegin", C.c_double), ("logTimeMax", C.c_double),
                ("GravKickTable", C.c_void_p), ("HydroKickTable", C.c_void_p),
                ("AdaptiveGravsoftForGasHsml", C.c_int), ("pmgrid", C.c_int),
                ("dt_gravkickB", C.c_double)]


class PmKickParams(C.Structure):
    """ghip_pmkick_params (the long-range kick ending a PM step, timestep.c:269-345)"""
    _fields_ = [("Ti_Current", C.c_int), ("Timebase_interval", C.c_double),
                ("ComovingIntegrationOn", C.c_int), ("logTimeBegin", C.c_double),
                ("logTimeMax", C.c_double), ("GravKickTable", C.c_void_p),
                ("HydroKickTable", C.c_void_p), ("dt_gravkick", C.c_double),
                ("dt_gravkickB", C.c_double)]


class BhParams(C.Structure):
    """ghip_bh_params: the sink passes of the shipped flag bundle (include/ghip.h, row N4)"""
    _fields_ = [("BoxSize", C.c_double), ("periodic", C.c_int), ("ascale", C.c_double),
                ("dt_fac", C.c_double), ("SMBHmass", C.c_double), ("InnerBoundary", C.c_double),
                ("SinkBoundary", C.c_double), ("SofteningBndry", C.c_double),
                ("CritDensity", C.c_double), ("FeedbackCoeff", C.c_double),
                ("UnitMass_in_g", C.c_double), ("dust", C.c_int),
                ("accretion_of_dust_only", C.c_int), ("accretion_density", C.c_int)]


# columns of the resident sink table (GHIP_SK_*, include/ghip.h)
(SK_BH_MASS, SK_ACCDISC_MASS, SK_BH_MDOT, SK_DUST_MASS, SK_TOTAL_MASS, SK_BH_DENSITY, SK_BH_ENTROPY,
 SK_GASVEL) = range(8)
SK_NUMNGB = SK_GASVEL + 3
SK_ACC_MASS, SK_ACC_BHMASS, SK_ACC_DUSTMASS, SK_ACC_MOMENTUM = range(SK_NUMNGB + 1, SK_NUMNGB + 5)
SK_COUNT = SK_ACC_MOMENTUM + 3


class BhAccretionParams(C.Structure):
    """ghip_bh_accretion_params: the Mdot step and the finish of blackhole_accretion() (include/ghip.h)"""
    _fields_ = [("limited_accretion", C.c_int), ("accretion_at_eddington_rate", C.c_int),
                ("enforce_eddington_limit", C.c_int), ("bh_mass_real", C.c_int), ("medd_fac", C.c_double),
                ("tvisc", C.c_double), ("EddingtonFactor", C.c_double)]


class BhAccretionReport(C.Structure):
    """ghip_bh_accretion_report"""
    _fields_ = [("TimeBin_BH_mass", C.c_double * 32), ("TimeBin_BH_dynamicalmass", C.c_double * 32),
                ("TimeBin_BH_Mdot", C.c_double * 32), ("swallowed", C.c_longlong * 3),
                ("nactive_sinks", C.c_int), ("missing", C.c_int), ("missing_id", C.c_uint), ("pad", C.c_int)]


class SfrFormReport(C.Structure):
    """ghip_sfr_form_report"""
    _fields_ = [("stars_converted", C.c_int), ("pad", C.c_int), ("sum_mass_stars", C.c_double),
                ("converted_in_bin", C.c_int * 32)]


class DustParams(C.Structure):
    """ghip_dust_params: the dust-gas drag passes of the shipped flag bundle (include/ghip.h)"""
    _fields_ = [("periodic", C.c_int), ("BoxSize", C.c_double), ("dt_fac", C.c_double),
                ("dt_fac_gas", C.c_double), ("MinEgySpec", C.c_double), ("MeanWeight", C.c_double),
                ("UnitLength_in_cm", C.c_double), ("UnitMass_in_g", C.c_double),
                ("UnitDensity_in_cgs", C.c_double), ("UnitVelocity_in_cm_per_s", C.c_double)]


class DustModel(C.Structure):
    """ghip_dust_model: the physics switches of the dust passes (ghip_set_dust_model, include/ghip.h)"""
    _fields_ = [(k, C.c_int) for k in ("growth", "real_pebble_collisions", "vaporize", "fe_and_ice_grains",
                                        "epstein", "no_friction_heating")] + \
        [(k, C.c_double) for k in ("Time", "VirtualTime", "FragmentationVelocity", "InitialDustRadius",
                                   "UnitEnergy_in_cgs")]


class DustGrains(C.Structure):
    """ghip_dust_grains: the arrays of a grain list (include/ghip.h)"""
    _fields_ = [("ndust", C.c_int), ("dust_idx", C.c_void_p), ("particle_density", C.c_void_p),
                ("dust_density", C.c_void_p), ("dust_entropy", C.c_void_p), ("dust_gasvel", C.c_void_p),
                ("dust_radius", C.c_void_p), ("particle_velocity", C.c_void_p), ("delta_momentum", C.c_void_p),
                ("delta_energy", C.c_void_p), ("vcoll", C.c_void_p), ("log_radius_by_dt", C.c_void_p),
                ("counts", C.c_void_p)]


def dust_grains(dust, particle_density=None, dust_density=None, dust_entropy=None, dust_gasvel=None,
                dust_radius=None, particle_velocity=None, vcoll=None, log_radius_by_dt=None, logr=True):
    """(DustGrains, arrays): the struct and the dict of numpy arrays it points into -- inputs copied, outputs
    allocated; logr = False leaves log_radius_by_dt NULL.  Keep `arrays` alive while the struct is used."""
    nd = len(dust)
    f64 = lambda v, shape: np.zeros(shape) if v is None else \
        np.ascontiguousarray(v, np.float64).reshape(shape).copy()
    a = dict(dust_idx=np.ascontiguousarray(dust, np.int32), particle_density=f64(particle_density, nd),
             dust_density=f64(dust_density, nd), dust_entropy=f64(dust_entropy, nd),
             dust_gasvel=f64(dust_gasvel, (nd, 3)), dust_radius=f64(dust_radius, nd),
             particle_velocity=f64(particle_velocity, (nd, 3)), delta_momentum=np.zeros((nd, 3)),
             delta_energy=np.zeros(nd), vcoll=f64(vcoll, nd), counts=np.zeros(4, np.int64))
    if logr:
        a["log_radius_by_dt"] = f64(log_radius_by_dt, nd)
    g = DustGrains()
    g.ndust = nd
    for k, v in a.items():
        setattr(g, k, v.ctypes.data)
    return g, a


class WindParams(C.Structure):
    """ghip_wind_params: the wind particles of the shipped flag bundle (FB_MOMENTUM, include/ghip.h)"""
    _fields_ = [("periodic", C.c_int)] + \
        [(k, C.c_double) for k in ("BoxSize", "Time", "dt_fac", "dt_fac_gas", "FeedBackVelocity",
                                   "UnitVelocity_in_cm_per_s", "UnitDensity_in_cgs", "UnitLength_in_cm",
                                   "VirtualCrosSection", "VirtualMass", "VirtualTime", "OuterBoundary",
                                   "DesNumNgb", "OriginalGasMass", "SofteningGas", "SofteningGasMaxPhys",
                                   "SofteningBulgeMaxPhys", "PhotonSearchRadius", "dt_total_floor")] + \
        [(k, C.c_int) for k in ("fly_through_empty_space", "variable_search_radius", "rad_accel", "max_iter")]


class WindState(C.Structure):
    """ghip_wind_state: the per-particle arrays of ghip_wind_feedback, in list order (include/ghip.h)"""
    _fields_ = [(k, C.c_void_p) for k in ("stellar_age", "birth_energy", "old_momentum", "new_density", "drmin",
                                           "dt1", "dt2", "dt_jump", "delta_momentum", "deleted")]


class WindResult(C.Structure):
    """ghip_wind_result (include/ghip.h)"""
    _fields_ = [("iterations", C.c_int), ("bits", C.c_longlong), ("ndeleted", C.c_int),
                ("deleted_momentum", C.c_double)]


# columns of the resident wind table (GHIP_WK_*, include/ghip.h)
(WK_STELLAR_AGE, WK_BIRTH_ENERGY, WK_OLD_MOMENTUM, WK_NEW_DENSITY, WK_DRMIN, WK_DT1, WK_DT2, WK_DT_JUMP,
 WK_DELTA_MOMENTUM, WK_DELETED, WK_COUNT) = range(11)


class WindSpawnParams(C.Structure):
    """ghip_wind_spawn_params: the creation of wind particles by the massive sinks (momentum_feedback.c:70-246)"""
    _fields_ = [(k, C.c_double) for k in ("Time", "dt_fac", "SMBHmass", "VirtualStart", "VirtualFeedBack",
                                           "VirtualMomentum", "VirtualMass", "FeedBackVelocity",
                                           "UnitVelocity_in_cm_per_s", "UnitTime_in_s", "SofteningBndryMaxPhys",
                                           "InnerBoundary")] + \
        [(k, C.c_int) for k in ("NumCurrentTiStep", "MaxPart", "fraction_of_ledd_feedback",
                                "accretion_at_eddington_rate", "startup_luminosity", "isotropic",
                                "accretion_radius", "fly_through_empty_space")] + \
        [("rnd_table", C.c_void_p), ("nrnd", C.c_int), ("pad", C.c_int)]


class WindSpawnReport(C.Structure):
    """ghip_wind_spawn_report (include/ghip.h)"""
    _fields_ = [("spawned", C.c_int), ("nsinks_emitting", C.c_int), ("first_index", C.c_int), ("pad", C.c_int),
                ("new_wind_exact_sum", C.c_double), ("gsl_draws", C.c_longlong)]


class DdWindArgs(C.Structure):
    """ghip_dd_wind_args (include/ghip.h): the wind particles resident on one multi-GPU shard, GHIP_DD_WIND"""
    _fields_ = [("p", C.POINTER(WindParams)), ("nwind", C.c_int), ("wind_idx", C.c_void_p),
                ("state", C.POINTER(WindState)), ("dt_jump", C.c_void_p), ("new_density", C.c_void_p),
                ("drmin", C.c_void_p), ("delta_momentum", C.c_void_p), ("result", C.POINTER(WindResult)),
                ("counts", C.c_void_p)]


class DdWindsArgs(C.Structure):
    """ghip_dd_winds_args (include/ghip.h): GHIP_DD_WIND with walk = WINDS_RESIDENT_FORM, the loop from the
    shard's wind table (p, result, counts), or WINDS_SPAWN_FORM, the creation of wind particles (spawn, report,
    tot_spawned)"""
    _fields_ = [("p", C.POINTER(WindParams)), ("result", C.POINTER(WindResult)), ("counts", C.c_void_p),
                ("spawn", C.POINTER(WindSpawnParams)), ("report", C.POINTER(WindSpawnReport)),
                ("tot_spawned", C.POINTER(C.c_longlong))]


class IntegrationFlags(C.Structure):
    """ghip_integration_flags: the shipped bundle's rules of get_timestep / do_the_kick /
    drift_particle (include/ghip.h)"""
    _fields_ = [(k, C.c_int) for k in ("dust", "dust_timestep", "black_holes", "accretion_radius",
                                        "virtual_particles")] + \
        [(k, C.c_double) for k in ("OuterBoundary", "AccDtBlackHole", "SMBHmass", "InnerBoundary",
                                   "SinkBoundary", "FeedBackVelocity", "UnitVelocity_in_cm_per_s")]


class ViscParams(C.Structure):
    """ghip_visc_params: TIME_DEP_ART_VISC and the uniform switches of the SPH pair loop (include/ghip.h)"""
    _fields_ = [(k, C.c_int) for k in ("time_dependent", "conventional", "no_limiter",
                                        "no_shear_limiter")] + \
        [(k, C.c_double) for k in ("ArtBulkViscConst", "AlphaMin", "ViscSource", "DecayTime",
                                   "dtalpha_comoving_div")]


# DoCooling variants of ghip_sfr_cooling (include/ghip.h)
COOL_NONE, COOL_ISOTHERM, COOL_EVAPORATION, COOL_EVAPORATION_RADIAL, COOL_BETA = 0, 1, 2, 3, 4


class SfrParams(C.Structure):
    """ghip_sfr_params: cooling_and_starformation with DoCooling and the drag heating (include/ghip.h)"""
    _fields_ = [("cooling", C.c_int), ("beta_tapper_off", C.c_int), ("dust", C.c_int),
                ("comoving", C.c_int)] + [(k, C.c_double) for k in (
                    "Timebase_interval", "Time", "hubble_a", "CritPhysDensity_code", "MinEgySpec",
                    "OriginalGasMass", "MeanWeight", "UnitEnergy_in_cgs", "UnitMass_in_g",
                    "UnitDensity_in_cgs", "EqTemp", "BetaCool", "Cool_ind", "rho_cool_ind",
                    "Evap_dens")] + [("smbh_pos", C.c_double * 3)]


class PmParams(C.Structure):
    _fields_ = [("pmgrid", C.c_int), ("BoxSize", C.c_double), ("G", C.c_double),
                ("Asmth", C.c_double)]


class PmRegion(C.Structure):
    """ghip_pm_region: the allowed region of the non-periodic mesh (pm_init_regionsize, pm_nonperiodic.c:91-212)"""
    _fields_ = [("pmgrid", C.c_int), ("Xmintot", C.c_double * 3), ("Xmaxtot", C.c_double * 3),
                ("TotalMeshSize", C.c_double), ("Corner", C.c_double * 3), ("UpperCorner", C.c_double * 3),
                ("Asmth", C.c_double), ("Rcut", C.c_double)]

    def asdict(self):
        return {k: (np.array(getattr(self, k)) if k in ("Xmintot", "Xmaxtot", "Corner", "UpperCorner")
                    else getattr(self, k)) for k, _ in self._fields_}


class PmnpParams(C.Structure):
    """ghip_pmnp_params (ghip_pm_nonperiodic / GHIP_DD_PM_NONPERIODIC)"""
    _fields_ = [("pmgrid", C.c_int), ("G", C.c_double), ("comoving", C.c_int), ("Omega0", C.c_double),
                ("OmegaLambda", C.c_double), ("Hubble", C.c_double)]


class PotParams(C.Structure):
    """ghip_pot_params (compute_potential, potential.c:22-325)"""
    _fields_ = [("grav", GravParams), ("pm", PmParams), ("G", C.c_double),
                ("SofteningTable", C.c_double * 6), ("comoving", C.c_int), ("Omega0", C.c_double),
                ("OmegaLambda", C.c_double), ("Hubble", C.c_double)]


class DecompParams(C.Structure):
    """ghip_dd_decomp_params (GHIP_DD_DECOMPOSE): level 0 = automatic, else 1..7; use_work: weigh by
    domain_particle_costfactor; find_extent: domain_findExtent over all ranks first"""
    _fields_ = [("level", C.c_int), ("use_work", C.c_int), ("find_extent", C.c_int), ("reserved", C.c_int)]


class SyncParams(C.Structure):
    """ghip_sync_params (ghip_find_next_sync_point / GHIP_DD_DECOMPOSE with walk = SYNC_POINT_FORM)"""
    _fields_ = [("Ti_Current", C.c_int), ("Ti_nextoutput", C.c_int)]


class SyncPoint(C.Structure):
    """ghip_sync_point: what find_next_sync_point_and_drift (run.c:190-340) decides before it drifts"""
    _fields_ = [("Ti_next", C.c_int), ("output_due", C.c_int), ("TimeBinActive", C.c_uint),
                ("NumForceUpdate", C.c_longlong), ("GlobNumForceUpdate", C.c_longlong),
                ("Flag_FullStep", C.c_int), ("TimeBinCount", C.c_longlong * 32),
                ("TimeBinCountSph", C.c_longlong * 32)]

    def asdict(self):
        return {k: (np.array(getattr(self, k)[:], dtype=np.int64) if k.startswith("TimeBinCount")
                    else int(getattr(self, k))) for k, _ in self._fields_}


class RearrangeParams(C.Structure):
    """ghip_rearrange_params: the -DSFR part (converted gas leaves the gas block) and the -DBLACK_HOLES part with
    -DDUST (Mass == 0 is eliminated, whatever the type) of rearrange_particle_sequence, sfr_eff.c:1018-1129"""
    _fields_ = [("fix_converted", C.c_int), ("eliminate_massless", C.c_int)]


class RearrangeResult(C.Structure):
    """ghip_rearrange_result: the counts after the call and what this context eliminated"""
    _fields_ = [("numpart", C.c_int), ("ngas", C.c_int), ("converted", C.c_int), ("count_elim", C.c_int),
                ("count_gaselim", C.c_int), ("count_dustelim", C.c_int), ("changed", C.c_int)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class FofParams(C.Structure):
    """ghip_fof_params (fof_fof, fof.c:94-333): LinkL <= 0 asks for the LINKLENGTH rule on the device"""
    _fields_ = [("LinkL", C.c_double), ("linklength", C.c_double), ("rhodm", C.c_double),
                ("primary_types", C.c_int), ("secondary_types", C.c_int), ("group_min_len", C.c_int),
                ("BoxSize", C.c_double), ("periodic", C.c_int), ("MaxIter", C.c_int)]


class FofResult(C.Structure):
    """ghip_fof_result"""
    _fields_ = [("Ngroups", C.c_int), ("Nids", C.c_longlong), ("largest", C.c_int), ("LinkL", C.c_double),
                ("nearest_iterations", C.c_int)]


class FofGroup(C.Structure):
    """ghip_fof_group: the members of struct group_properties (fof.h:26-60) the resident state can fill"""
    _fields_ = [("Len", C.c_int), ("Offset", C.c_int), ("MinID", C.c_int), ("GrNr", C.c_int),
                ("LenType", C.c_int * 6), ("MassType", C.c_double * 6), ("Mass", C.c_double),
                ("CM", C.c_double * 3), ("Vel", C.c_double * 3), ("MaxDens", C.c_double),
                ("index_maxdens", C.c_int)]


# numpy view of FofGroup[] (same offsets, trailing padding included)
FOF_GROUP_DTYPE = np.dtype({"names": ["Len", "Offset", "MinID", "GrNr", "LenType", "MassType", "Mass", "CM", "Vel",
                                      "MaxDens", "index_maxdens"],
                            "formats": ["<i4", "<i4", "<i4", "<i4", ("<i4", 6), ("<f8", 6), "<f8", ("<f8", 3),
                                        ("<f8", 3), "<f8", "<i4"],
                            "offsets": [FofGroup.Len.offset, FofGroup.Offset.offset, FofGroup.MinID.offset,
                                        FofGroup.GrNr.offset, FofGroup.LenType.offset, FofGroup.MassType.offset,
                                        FofGroup.Mass.offset, FofGroup.CM.offset, FofGroup.Vel.offset,
                                        FofGroup.MaxDens.offset, FofGroup.index_maxdens.offset],
                            "itemsize": C.sizeof(FofGroup)})


class GlobalParams(C.Structure):
    """ghip_global_params (compute_global_quantities_of_system, global.c:18-238)"""
    _fields_ = [("Ti_Current", C.c_int), ("Timebase_interval", C.c_double),
                ("ComovingIntegrationOn", C.c_int), ("Time", C.c_double),
                ("logTimeBegin", C.c_double), ("logTimeMax", C.c_double),
                ("GravKickTable", C.c_void_p), ("HydroKickTable", C.c_void_p), ("pmgrid", C.c_int),
                ("dt_gravkick_pm", C.c_double), ("OldPhotonMomentum", C.c_void_p),
                ("rad_fac", C.c_double), ("Potential", C.c_void_p)]


class GlobalSums(C.Structure):
    """ghip_global_sums: the per-type members of struct state_of_system (allvars.h:1646-1667)"""
    _fields_ = [("MassComp", C.c_double * 6), ("EnergyKinComp", C.c_double * 6),
                ("EnergyPotComp", C.c_double * 6), ("EnergyIntComp", C.c_double * 6),
                ("MomentumComp", (C.c_double * 4) * 6), ("AngMomentumComp", (C.c_double * 4) * 6),
                ("CenterOfMassComp", (C.c_double * 4) * 6), ("EnergyRadComp", C.c_double)]

    def asdict(self):
        out = {}
        for k, _ in self._fields_:
            v = getattr(self, k)
            out[k] = float(v) if isinstance(v, float) else np.ctypeslib.as_array(v).copy()
        return out


class NodeLayout(C.Structure):
    """ghip_node_layout: byte offsets of struct NODE / struct extNODE (allvars.h:1847-1916)"""
    _fields_ = [(k, C.c_int) for k in
                ("node_stride", "n_len", "n_center", "n_s", "n_mass", "n_bitflags", "n_sibling",
                 "n_nextnode", "n_father", "n_ti_current", "ext_stride", "e_dp", "e_vs", "e_vmax",
                 "e_divvmax", "e_hmax", "e_ti_lastkicked", "e_flag", "n_maxsoft")]


# struct NODE / struct extNODE of the minimal periodic flag set (88 / 80 bytes)
NODE_DTYPE = np.dtype({"names": ["len", "center", "s", "mass", "bitflags", "sibling", "nextnode",
                                 "father", "Ti_current"],
                       "formats": ["f8", ("f8", 3), ("f8", 3), "f8", "u4", "i4", "i4", "i4", "i4"],
                       "offsets": [0, 8, 32, 56, 64, 68, 72, 76, 80], "itemsize": 88})
# struct NODE with ADAPTIVE_GRAVSOFT_FORGAS: maxsoft sits before the union (allvars.h:1857-1860), 96 bytes
NODE_ADAPTIVE_DTYPE = np.dtype({"names": ["len", "center", "maxsoft", "s", "mass", "bitflags",
                                          "sibling", "nextnode", "father", "Ti_current"],
                                "formats": ["f8", ("f8", 3), "f8", ("f8", 3), "f8", "u4", "i4", "i4",
                                            "i4", "i4"],
                                "offsets": [0, 8, 32, 40, 64, 72, 76, 80, 84, 88], "itemsize": 96})
EXTNODE_DTYPE = np.dtype({"names": ["dp", "vs", "vmax", "divVmax", "hmax", "Ti_lastkicked", "Flag"],
                          "formats": [("f8", 3), ("f8", 3), "f8", "f8", "f8", "i4", "i4"],
                          "offsets": [0, 24, 48, 56, 64, 72, 76], "itemsize": 80})


class Stats(C.Structure):
    _fields_ = [("grav_interactions", C.c_longlong), ("grav_targets", C.c_longlong),
                ("ewald_interactions", C.c_longlong), ("dens_neighbours", C.c_longlong),
                ("dens_target_evals", C.c_longlong), ("dens_iterations", C.c_int),
                ("hydro_pairs", C.c_longlong), ("hydro_targets", C.c_longlong),
                ("tree_nodes", C.c_int), ("gastree_nodes", C.c_int),
                ("ms_tree", C.c_float), ("ms_grav", C.c_float), ("ms_ewald", C.c_float),
                ("ms_dens", C.c_float), ("ms_hmax", C.c_float), ("ms_hydro", C.c_float),
                ("grav_wave_steps", C.c_longlong), ("ewald_wave_steps", C.c_longlong),
                ("ms_kick", C.c_float), ("ms_pm", C.c_float)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RunStats(C.Structure):
    """ghip_run_stats: a run of steps without a host synchronisation per step"""
    _fields_ = ([(k, C.c_longlong) for k in (
        "steps", "steps_timed", "launches", "blocking_syncs", "grav_interactions",
        "ewald_interactions", "dens_neighbours", "hydro_pairs", "grav_wave_steps",
        "ewald_wave_steps", "dens_extra_iterations")] +
        [(k, C.c_double) for k in (
            "ms_tree", "ms_grav", "ms_ewald", "ms_dens", "ms_hmax", "ms_hydro", "ms_kick",
            "ms_steps_device", "ms_between_steps", "ms_first_to_last")])

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class GhipError(RuntimeError):
    def __init__(self, code, msg):
        self.code = code
        RuntimeError.__init__(self, "%s (%d): %s" % (GHIP_ERRORS.get(code, "GHIP_E?"), code, msg))


_LIB = None

# int allgather(void *user, const void *send, size_t bytes, void *recv)
ALLGATHER_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)

EXPORTS = [
    "ghip_create", "ghip_destroy", "ghip_last_error", "ghip_version", "ghip_device_bytes_in_use",
    "ghip_set_counts",
    "ghip_set_field", "ghip_get_field", "ghip_upload_aos", "ghip_download_aos", "ghip_set_active",
    "ghip_set_shard", "ghip_tree_build", "ghip_ewald_init", "ghip_ewald_get_table", "ghip_gravity",
    "ghip_gravity_ext", "ghip_gravity_finish", "ghip_gravity_finish_ex", "ghip_gravity_direct",
    "ghip_density",
    "ghip_update_hmax", "ghip_hydro", "ghip_density_evaluate", "ghip_ngb_treefind",
    "ghip_peano_hilbert_keys", "ghip_morton_keys", "ghip_get_stats", "ghip_tree_dump",
    "ghip_stream", "ghip_sync", "ghip_shard_pack", "ghip_shard_unpack", "ghip_shard_count",
    "ghip_drift", "ghip_gravity_finish_all", "ghip_advance_timesteps",
    "ghip_timestep_endrun_code", "ghip_velocity_moments", "ghip_download_aos_kick",
    "ghip_tree_export", "ghip_pm_periodic", "ghip_set_adaptive_gravsoft", "ghip_gravity_ext_soft",
    "ghip_gravity_vacuum_energy", "ghip_pm_kick",
    "ghip_dd_init", "ghip_dd_set_domain", "ghip_dd_set_splits", "ghip_dd_set_segments", "ghip_dd_keys", "ghip_dd_find_split",
    "ghip_set_dynamic_tree", "ghip_tree_substep", "ghip_tree_kick_nodes", "ghip_tree_kick_nodes_vmax",
    "ghip_tree_dump_dynamic",
    "ghip_gas_block_mixed", "ghip_set_massless_gas_rule", "ghip_set_hydro_release", "ghip_download_aos_async",
    "ghip_gravity_to_records", "ghip_pin_host", "ghip_unpin_host", "ghip_dd_set_ghost_margin", "ghip_dd_rccl_unique_id", "ghip_dd_rccl_connect",
    "ghip_dd_rccl_library", "ghip_dd_begin", "ghip_dd_step", "ghip_dd_exchange",
    "ghip_dd_exchange_local", "ghip_dd_exchange_host", "ghip_dd_run", "ghip_dd_get_info",
    "ghip_sink_density", "ghip_sink_reset", "ghip_blackhole_evaluate", "ghip_blackhole_swallow",
    "ghip_sink_get_marks", "ghip_sink_set_marks", "ghip_cooling_and_starformation",
    "ghip_set_async", "ghip_timebin_counts", "ghip_run_begin", "ghip_step_begin", "ghip_step_end",
    "ghip_run_end", "ghip_dust_density", "ghip_dust_drag", "ghip_dust_get_drag_heating",
    "ghip_dust_set_drag_heating", "ghip_sfr_cooling", "ghip_find_smbh", "ghip_set_integration_flags",
    "ghip_kick_set_fields", "ghip_kick_get_drag_accel", "ghip_potential", "ghip_get_potential",
    "ghip_potential_interactions", "ghip_get_potential_interactions", "ghip_global_quantities",
    "ghip_dd_bytes_sent", "ghip_dd_get_splits", "ghip_dd_get_domain",
    "ghip_pm_find_region", "ghip_pm_set_region", "ghip_pm_get_region", "ghip_pm_nonperiodic",
    "ghip_set_dust_model", "ghip_dust_model_size", "ghip_dust_grains_size", "ghip_dust_density_grains",
    "ghip_dust_drag_grains",
    "ghip_set_viscosity", "ghip_visc_set_alpha", "ghip_visc_get", "ghip_visc_derive", "ghip_visc_params_size",
    "ghip_set_rnd_table", "ghip_tree_max_level", "ghip_dd_set_guests", "ghip_dd_guest_counts",
    "ghip_debug_prim",
    "ghip_find_next_sync_point", "ghip_get_active", "ghip_find_extent", "ghip_dd_get_sync_point",
    "ghip_fof", "ghip_fof_get_groups", "ghip_fof_get_ids", "ghip_fof_get_labels", "ghip_fof_params_size",
    "ghip_fof_group_size", "ghip_fof_get_timing", "ghip_fof_get_maxdens_task", "ghip_dd_fof_args_size",
    "ghip_wind_params_size", "ghip_wind_density", "ghip_wind_spread", "ghip_wind_feedback",
    "ghip_wind_get_injected", "ghip_wind_set_injected", "ghip_wind_get_rad_accel", "ghip_wind_set_rad_accel",
    "ghip_set_rad_accel", "ghip_wind_get_timing", "ghip_dd_wind_args_size",
    "ghip_dd_winds_args_size", "ghip_dd_winds_set_table", "ghip_dd_winds_get_table", "ghip_dd_winds_clear",
    "ghip_kick_get_fields", "ghip_rearrange", "ghip_peano_order", "ghip_sequence_get_map", "ghip_sequence_get_info",
    "ghip_sinks_set_table", "ghip_sinks_get_table", "ghip_sinks_clear", "ghip_sinks_density",
    "ghip_blackhole_accretion", "ghip_sfr_form_sinks", "ghip_dd_sinks_args_size"]


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(_pkg.lib_path())
        vp = C.c_void_p
        L.ghip_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.ghip_destroy.argtypes = [vp]
        L.ghip_destroy.restype = None
        L.ghip_last_error.argtypes = [vp]
        L.ghip_last_error.restype = C.c_char_p
        L.ghip_version.restype = C.c_char_p
        L.ghip_device_bytes_in_use.argtypes = []
        L.ghip_device_bytes_in_use.restype = C.c_longlong
        L.ghip_set_counts.argtypes = [vp, C.c_int, C.c_int]
        L.ghip_set_field.argtypes = [vp, C.c_int, vp]
        L.ghip_get_field.argtypes = [vp, C.c_int, vp]
        L.ghip_upload_aos.argtypes = [vp, vp, vp, C.POINTER(Layout), C.c_int, C.c_int]
        L.ghip_download_aos.argtypes = [vp, vp, vp, C.POINTER(Layout), C.c_int, C.c_int, C.c_int]
        L.ghip_set_active.argtypes = [vp, vp, C.c_int]
        L.ghip_set_shard.argtypes = [vp, C.c_int, C.c_int]
        L.ghip_tree_build.argtypes = [vp, vp, vp, C.c_double, vp]
        L.ghip_ewald_init.argtypes = [vp, C.c_double]
        L.ghip_ewald_get_table.argtypes = [vp, vp]
        L.ghip_gravity.argtypes = [vp, C.POINTER(GravParams), C.c_int]
        L.ghip_gravity_ext.argtypes = [vp, C.POINTER(GravParams), C.c_int, C.c_int, vp, vp, vp,
                                       vp, vp]
        L.ghip_gravity_ext_soft.argtypes = [vp, C.POINTER(GravParams), C.c_int, C.c_int, vp, vp, vp,
                                            vp, vp, vp]
        L.ghip_set_adaptive_gravsoft.argtypes = [vp, C.c_int]
        L.ghip_gravity_vacuum_energy.argtypes = [vp, C.c_double]
        L.ghip_pm_kick.argtypes = [vp, C.POINTER(PmKickParams)]
        L.ghip_gravity_finish.argtypes = [vp, C.c_double]
        L.ghip_gravity_finish_all.argtypes = [vp, C.c_double]
        L.ghip_gravity_finish_ex.argtypes = [vp, C.c_double, C.c_int, C.c_double, C.c_int]
        L.ghip_gravity_direct.argtypes = [vp, C.POINTER(GravParams)]
        L.ghip_density.argtypes = [vp, C.POINTER(DensParams)]
        L.ghip_update_hmax.argtypes = [vp]
        L.ghip_hydro.argtypes = [vp, C.POINTER(HydroParams)]
        L.ghip_density_evaluate.argtypes = [vp, C.POINTER(DensParams), C.c_int, C.c_double, vp]
        L.ghip_ngb_treefind.argtypes = [vp, vp, C.c_double, C.c_int, C.c_int, C.c_double, vp,
                                        C.c_int, C.POINTER(C.c_int)]
        L.ghip_debug_prim.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.POINTER(C.c_int)]
        L.ghip_peano_hilbert_keys.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp]
        L.ghip_morton_keys.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp]
        L.ghip_get_stats.argtypes = [vp, C.POINTER(Stats)]
        L.ghip_tree_dump.argtypes = [vp, C.c_int, C.POINTER(C.c_int), vp, vp, vp, vp, vp]
        L.ghip_set_dynamic_tree.argtypes = [vp, C.c_int]
        L.ghip_tree_substep.argtypes = [vp, C.c_double]
        L.ghip_tree_kick_nodes.argtypes = [vp, C.c_int, vp, vp]
        L.ghip_tree_dump_dynamic.argtypes = [vp, C.POINTER(C.c_int), vp, vp, vp, vp]
        L.ghip_stream.argtypes = [vp]
        L.ghip_stream.restype = vp
        L.ghip_sync.argtypes = [vp]
        L.ghip_drift.argtypes = [vp, C.POINTER(DriftParams)]
        L.ghip_advance_timesteps.argtypes = [vp, C.POINTER(KickParams), vp, vp]
        L.ghip_timestep_endrun_code.argtypes = [vp]
        L.ghip_velocity_moments.argtypes = [vp, vp, vp, vp]
        L.ghip_download_aos_kick.argtypes = [vp, vp, vp, C.POINTER(Layout)]
        L.ghip_pm_periodic.argtypes = [vp, C.POINTER(PmParams)]
        L.ghip_pm_find_region.argtypes = [vp, C.c_int, C.POINTER(PmRegion)]
        L.ghip_pm_set_region.argtypes = [vp, C.POINTER(PmRegion)]
        L.ghip_pm_get_region.argtypes = [vp, C.POINTER(PmRegion)]
        L.ghip_pm_nonperiodic.argtypes = [vp, C.POINTER(PmnpParams)]
        L.ghip_tree_export.argtypes = [vp, C.POINTER(NodeLayout), C.c_int, C.c_int, C.c_int, vp, vp,
                                       vp, vp, C.c_int, C.POINTER(C.c_int)]
        L.ghip_shard_count.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.ghip_shard_pack.argtypes = [vp, C.c_int, vp]
        L.ghip_shard_unpack.argtypes = [vp, C.c_int, vp, C.c_int]
        L.ghip_dd_init.argtypes = [vp, C.c_int, C.c_int]
        L.ghip_dd_set_domain.argtypes = [vp, vp, vp, C.c_double, vp]
        L.ghip_dd_set_splits.argtypes = [vp, vp]
        L.ghip_dd_set_segments.argtypes = [vp, C.c_int, vp, vp]
        L.ghip_dd_keys.argtypes = [vp, vp]
        L.ghip_dd_find_split.argtypes = [C.c_int, C.c_int, vp, vp, vp]
        L.ghip_dd_set_ghost_margin.argtypes = [vp, C.c_double]
        L.ghip_dd_rccl_unique_id.argtypes = [vp]
        L.ghip_dd_rccl_connect.argtypes = [vp, vp]
        L.ghip_dd_rccl_library.restype = C.c_char_p
        L.ghip_dd_begin.argtypes = [vp, C.c_int, vp, C.c_int]
        L.ghip_dd_step.argtypes = [vp]
        L.ghip_dd_exchange.argtypes = [vp]
        L.ghip_dd_exchange_local.argtypes = [vp, C.c_int]
        L.ghip_dd_run.argtypes = [vp, C.c_int, vp, C.c_int]
        L.ghip_dd_exchange_host.argtypes = [vp, ALLGATHER_CB, vp]
        L.ghip_dd_get_info.argtypes = [vp, vp]
        L.ghip_dd_set_guests.argtypes = [vp, C.c_int]
        L.ghip_dd_guest_counts.argtypes = [vp, vp]
        L.ghip_sink_density.argtypes = [vp, C.POINTER(DensParams), C.c_double, C.c_int, vp, vp, vp,
                                        vp, vp, vp, C.POINTER(C.c_int)]
        L.ghip_sink_reset.argtypes = [vp]
        L.ghip_blackhole_evaluate.argtypes = [vp, C.POINTER(BhParams), C.c_int, vp, vp, vp, vp]
        L.ghip_blackhole_swallow.argtypes = [vp, C.POINTER(BhParams), C.c_int, vp, vp, vp, vp, vp,
                                             vp, vp, vp]
        L.ghip_sinks_set_table.argtypes = [vp, C.c_int, vp, vp]
        L.ghip_sinks_get_table.argtypes = [vp, C.POINTER(C.c_int), vp, vp]
        L.ghip_sinks_clear.argtypes = [vp]
        L.ghip_sinks_density.argtypes = [vp, C.POINTER(DensParams), C.c_double, C.POINTER(C.c_int)]
        L.ghip_blackhole_accretion.argtypes = [vp, C.POINTER(BhParams), C.POINTER(BhAccretionParams),
                                               C.POINTER(BhAccretionReport)]
        L.ghip_sfr_form_sinks.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(SfrFormReport)]
        L.ghip_set_async.argtypes = [vp, C.c_int]
        L.ghip_timebin_counts.argtypes = [vp, vp, vp]
        L.ghip_run_begin.argtypes = [vp, C.c_int]
        L.ghip_step_begin.argtypes = [vp]
        L.ghip_step_end.argtypes = [vp]
        L.ghip_run_end.argtypes = [vp, C.POINTER(RunStats)]
        L.ghip_sink_get_marks.argtypes = [vp, vp, vp]
        L.ghip_sink_set_marks.argtypes = [vp, vp, vp]
        L.ghip_cooling_and_starformation.argtypes = [vp, C.c_double, C.c_double, C.c_double,
                                                     C.c_double, vp]
        L.ghip_dust_density.argtypes = [vp, C.POINTER(DustParams), C.c_int, vp, vp]
        L.ghip_dust_drag.argtypes = [vp, C.POINTER(DustParams), C.c_int] + [vp] * 10
        L.ghip_dust_get_drag_heating.argtypes = [vp, vp]
        L.ghip_set_dust_model.argtypes = [vp, C.POINTER(DustModel)]
        L.ghip_dust_density_grains.argtypes = [vp, C.POINTER(DustParams), C.POINTER(DustGrains)]
        L.ghip_dust_drag_grains.argtypes = [vp, C.POINTER(DustParams), C.POINTER(DustGrains)]
        for fn, cls in ((L.ghip_dust_model_size, DustModel), (L.ghip_dust_grains_size, DustGrains)):
            fn.argtypes = []
            fn.restype = C.c_size_t
            if fn() != C.sizeof(cls):
                raise RuntimeError("%s: %d bytes here, %d in libghip.so" % (cls.__name__, C.sizeof(cls), fn()))
        L.ghip_dust_set_drag_heating.argtypes = [vp, vp]
        L.ghip_wind_params_size.argtypes = []
        L.ghip_wind_params_size.restype = C.c_size_t
        if L.ghip_wind_params_size() != C.sizeof(WindParams):
            raise RuntimeError("WindParams: %d bytes here, %d in libghip.so"
                               % (C.sizeof(WindParams), L.ghip_wind_params_size()))
        L.ghip_dd_wind_args_size.argtypes = []
        L.ghip_dd_wind_args_size.restype = C.c_size_t
        if L.ghip_dd_wind_args_size() != C.sizeof(DdWindArgs):
            raise RuntimeError("DdWindArgs: %d bytes here, %d in libghip.so"
                               % (C.sizeof(DdWindArgs), L.ghip_dd_wind_args_size()))
        L.ghip_dd_winds_args_size.argtypes = []
        L.ghip_dd_winds_args_size.restype = C.c_size_t
        if L.ghip_dd_winds_args_size() != C.sizeof(DdWindsArgs):
            raise RuntimeError("DdWindsArgs: %d bytes here, %d in libghip.so"
                               % (C.sizeof(DdWindsArgs), L.ghip_dd_winds_args_size()))
        L.ghip_dd_sinks_args_size.argtypes = []
        L.ghip_dd_sinks_args_size.restype = C.c_size_t
        if L.ghip_dd_sinks_args_size() != C.sizeof(DdSinksArgs):
            raise RuntimeError("DdSinksArgs: %d bytes here, %d in libghip.so"
                               % (C.sizeof(DdSinksArgs), L.ghip_dd_sinks_args_size()))
        L.ghip_wind_density.argtypes = [vp, C.POINTER(WindParams), C.c_int, vp, vp, vp, vp]
        L.ghip_wind_spread.argtypes = [vp, C.POINTER(WindParams), C.c_int, vp, vp, vp, vp]
        L.ghip_wind_feedback.argtypes = [vp, C.POINTER(WindParams), C.c_int, vp, C.POINTER(WindState),
                                         C.POINTER(WindResult)]
        for fn in (L.ghip_wind_get_injected, L.ghip_wind_set_injected, L.ghip_wind_get_rad_accel,
                   L.ghip_wind_set_rad_accel, L.ghip_wind_get_timing):
            fn.argtypes = [vp, vp]
        L.ghip_set_rad_accel.argtypes = [vp, C.c_int]
        for fn, cls in ((L.ghip_wind_spawn_params_size, WindSpawnParams),
                        (L.ghip_wind_spawn_report_size, WindSpawnReport)):
            fn.argtypes = []
            fn.restype = C.c_size_t
            if fn() != C.sizeof(cls):
                raise RuntimeError("%s: %d bytes here, %d in libghip.so" % (cls.__name__, C.sizeof(cls), fn()))
        L.ghip_winds_set_table.argtypes = [vp, C.c_int, vp, vp]
        L.ghip_winds_get_table.argtypes = [vp, C.POINTER(C.c_int), vp, vp]
        L.ghip_winds_clear.argtypes = [vp]
        L.ghip_dd_winds_set_table.argtypes = [vp, C.c_int, vp, vp]
        L.ghip_dd_winds_get_table.argtypes = [vp, C.POINTER(C.c_int), vp, vp]
        L.ghip_dd_winds_clear.argtypes = [vp]
        L.ghip_winds_feedback.argtypes = [vp, C.POINTER(WindParams), C.POINTER(WindResult)]
        L.ghip_wind_spawn.argtypes = [vp, C.POINTER(WindSpawnParams), C.POINTER(WindSpawnReport)]
        L.ghip_sfr_cooling.argtypes = [vp, C.POINTER(SfrParams), C.POINTER(C.c_int), vp]
        L.ghip_find_smbh.argtypes = [vp, C.c_double, vp, C.POINTER(C.c_int)]
        L.ghip_set_integration_flags.argtypes = [vp, C.POINTER(IntegrationFlags)]
        L.ghip_kick_set_fields.argtypes = [vp, vp, vp, vp]
        L.ghip_kick_get_drag_accel.argtypes = [vp, vp]
        L.ghip_potential.argtypes = [vp, C.POINTER(PotParams)]
        L.ghip_get_potential.argtypes = [vp, vp]
        L.ghip_potential_interactions.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        L.ghip_get_potential_interactions.argtypes = [vp, vp]
        L.ghip_dd_bytes_sent.argtypes = [vp, C.c_int, C.POINTER(C.c_longlong)]
        L.ghip_dd_get_splits.argtypes = [vp, vp]
        L.ghip_dd_get_domain.argtypes = [vp, vp, vp, C.POINTER(C.c_double)]
        L.ghip_ewald_get_pot_table.argtypes = [vp, C.c_double, vp]
        L.ghip_global_quantities.argtypes = [vp, C.POINTER(GlobalParams), C.POINTER(GlobalSums)]
        L.ghip_set_viscosity.argtypes = [vp, C.POINTER(ViscParams)]
        L.ghip_visc_set_alpha.argtypes = [vp, vp, vp]
        L.ghip_visc_get.argtypes = [vp, vp, vp]
        L.ghip_visc_derive.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.ghip_visc_derive.restype = None
        L.ghip_visc_params_size.argtypes = []
        L.ghip_visc_params_size.restype = C.c_size_t
        L.ghip_set_rnd_table.argtypes = [vp, vp, C.c_int]
        L.ghip_tree_max_level.argtypes = []
        L.ghip_find_next_sync_point.argtypes = [vp, C.POINTER(SyncParams), C.POINTER(SyncPoint)]
        L.ghip_kick_get_fields.argtypes = [vp, vp, vp, vp, vp]
        L.ghip_rearrange.argtypes = [vp, C.POINTER(RearrangeParams), C.POINTER(RearrangeResult)]
        L.ghip_peano_order.argtypes = [vp, vp, C.c_double, C.POINTER(C.c_int)]
        L.ghip_sequence_get_map.argtypes = [vp, vp, vp]
        L.ghip_sequence_get_info.argtypes = [vp, vp]
        L.ghip_get_active.argtypes = [vp, vp, C.POINTER(C.c_int)]
        L.ghip_find_extent.argtypes = [vp, vp, vp, C.POINTER(C.c_double)]
        L.ghip_dd_get_sync_point.argtypes = [vp, C.POINTER(SyncPoint)]
        L.ghip_fof.argtypes = [vp, C.POINTER(FofParams), C.POINTER(FofResult)]
        L.ghip_fof_get_groups.argtypes = [vp, vp]
        L.ghip_fof_get_ids.argtypes = [vp, vp]
        L.ghip_fof_get_labels.argtypes = [vp, vp, vp]
        L.ghip_fof_get_timing.argtypes = [vp, vp]
        L.ghip_fof_get_maxdens_task.argtypes = [vp, vp]
        L.ghip_dd_fof_args_size.restype = C.c_size_t
        L.ghip_dd_fof_args_size.argtypes = []
        for fn, cls in ((L.ghip_fof_params_size, FofParams), (L.ghip_fof_group_size, FofGroup)):
            fn.argtypes = []
            fn.restype = C.c_size_t
            if fn() != C.sizeof(cls):
                raise RuntimeError("%s: %d bytes here, %d in libghip.so" % (cls.__name__, C.sizeof(cls), fn()))
        if L.ghip_dd_fof_args_size() != C.sizeof(DdFofArgs):
            raise RuntimeError("DdFofArgs: %d bytes here, %d in libghip.so"
                               % (C.sizeof(DdFofArgs), L.ghip_dd_fof_args_size()))
        _LIB = L
    return _LIB


def visc_derive(visc_source0, decay_length):
    """(All.ViscSource, All.DecayTime) of begrun.c:132-133 from the parameter file's ViscSource0, DecayLength"""
    a, b = C.c_double(), C.c_double()
    lib().ghip_visc_derive(float(visc_source0), float(decay_length), C.byref(a), C.byref(b))
    return a.value, b.value


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class ForcePath:
    """One device context (one per process / GPU)."""

    def __init__(self, device=0):
        self.L = lib()
        h = C.c_void_p()
        rc = self.L.ghip_create(int(device), C.byref(h))
        if rc != 0:
            raise GhipError(rc, "ghip_create(device=%d) failed: no usable GPU; this package has "
                                "no CPU path" % device)
        self.h = h
        self.n = 0
        self.ngas = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.ghip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # walk constant of the overlapped Newton+Ewald pair (sharded.py uses it when present)
    WALK_PAIR = (WALK_NEWTON, WALK_EWALD, WALK_NEWTON_EWALD)

    def _chk(self, rc):
        if rc != 0:
            e = GhipError(rc, self.L.ghip_last_error(self.h).decode())
            if GHIP_ERRORS.get(rc) == "GHIP_ETIMESTEP":   # (also when a deferred kick reports late)
                e.endrun = self.L.ghip_timestep_endrun_code(self.h)
            raise e

    # ---- data ----
    def set_counts(self, n, ngas):
        self._chk(self.L.ghip_set_counts(self.h, int(n), int(ngas)))
        self.n, self.ngas = int(n), int(ngas)

    def _shape(self, field):
        gas, ncomp, isint = _FIELD_INFO[field]
        cnt = self.ngas if gas else self.n
        return ((cnt, 3) if ncomp == 3 else (cnt,)), (np.int32 if isint else np.float64)

    def set_field(self, field, arr):
        shape, dt = self._shape(field)
        a = np.ascontiguousarray(arr, dtype=dt)
        if a.shape != shape:
            raise ValueError("field %d: expected shape %s, got %s" % (field, shape, a.shape))
        self._chk(self.L.ghip_set_field(self.h, field, _ptr(a)))

    def get_field(self, field):
        shape, dt = self._shape(field)
        a = np.zeros(shape, dtype=dt)
        self._chk(self.L.ghip_get_field(self.h, field, _ptr(a)))
        return a

    def upload_aos(self, P, SphP, layout):
        n, ng = len(P), (0 if SphP is None else len(SphP))
        self._chk(self.L.ghip_upload_aos(self.h, _ptr(P), _ptr(SphP) if ng else None,
                                         C.byref(layout), n, ng))
        self.n, self.ngas = n, ng

    def download_aos(self, P, SphP, layout, gravity=True, density=True, hydro=True):
        self._chk(self.L.ghip_download_aos(self.h, _ptr(P), _ptr(SphP) if self.ngas else None,
                                           C.byref(layout), int(gravity), int(density),
                                           int(hydro)))

    def set_active(self, idx=None):
        if idx is None:
            self._chk(self.L.ghip_set_active(self.h, None, 0))
            self._active_n = None
        else:
            a = np.ascontiguousarray(idx, dtype=np.int32)
            self._active_keep = a
            self._chk(self.L.ghip_set_active(self.h, _ptr(a), len(a)))
            self._active_n = len(a)

    def find_next_sync_point(self, ti_current, ti_nextoutput=-1):
        """ghip_find_next_sync_point: the next sync point and the active list from the resident TIMEBIN
        (find_next_sync_point_and_drift, run.c:190-340, without the drift) -> SyncPoint.  With output_due the
        list stays as it was; drift to .Ti_next yourself (drift())."""
        p, out = SyncParams(int(ti_current), int(ti_nextoutput)), SyncPoint()
        self._chk(self.L.ghip_find_next_sync_point(self.h, C.byref(p), C.byref(out)))
        return out

    def rearrange(self, fix_converted=True, eliminate_massless=True):
        """ghip_rearrange: rearrange_particle_sequence (sfr_eff.c:1018-1129) as an order-preserving compaction of
        the resident state -> RearrangeResult; .n and .ngas follow.  Converted records of the gas block go behind
        it, Mass == 0 records are eliminated; every field and every optional array held for the current counts
        travels.  After a call that changed something: tree_build, and find_next_sync_point for the active list."""
        p = RearrangeParams(int(bool(fix_converted)), int(bool(eliminate_massless)))
        out = RearrangeResult()
        self._chk(self.L.ghip_rearrange(self.h, C.byref(p), C.byref(out)))
        self.n, self.ngas = out.numpart, out.ngas
        if out.changed:
            self._active_n = None
        return out

    def peano_order(self, corner=None, dlen=0.0):
        """ghip_peano_order: peano_hilbert_order (peano.c:25-185), the gas block and the block behind it each
        sorted stably by the key of dd_keys() in the cube (corner, dlen) -> True when a record moved.  corner
        None: the domain of a dd_init context.  GhipError (GHIP_EINVAL), nothing moved, for a position outside
        the cube."""
        c0 = None if corner is None else np.ascontiguousarray(corner, np.float64)
        ch = C.c_int(0)
        self._chk(self.L.ghip_peano_order(self.h, _ptr(c0), float(dlen), C.byref(ch)))
        if ch.value:
            self._active_n = None
        return bool(ch.value)

    def sequence_info(self):
        """ghip_sequence_get_info of the last rearrange() / peano_order(): dict(n_before, n_after, bytes_moved,
        planes)"""
        out = np.zeros(4, np.int64)
        self._chk(self.L.ghip_sequence_get_info(self.h, _ptr(out)))
        return dict(n_before=int(out[0]), n_after=int(out[1]), bytes_moved=int(out[2]), planes=int(out[3]))

    def sequence_map(self):
        """ghip_sequence_get_map of the last rearrange() / peano_order() -> (new_of_old int32[n before], -1 for
        an eliminated record; old_of_new int32[n after])"""
        info = self.sequence_info()
        new_of_old = np.zeros(max(info["n_before"], 0), np.int32)
        old_of_new = np.zeros(max(info["n_after"], 0), np.int32)
        self._chk(self.L.ghip_sequence_get_map(self.h, _ptr(new_of_old), _ptr(old_of_new)))
        return new_of_old, old_of_new

    def fof(self, link_length=0.0, primary_types=2, secondary_types=0, group_min_len=32, boxsize=0.0,
            periodic=False, max_iter=150, linklength=0.2, rhodm=0.0):
        """ghip_fof: friends-of-friends groups of the resident state on the gravity tree in place (fof_fof,
        fof.c:94-333) -> FofResult.  link_length <= 0: the LINKLENGTH rule, linklength * (mass / number of the
        primaries / rhodm)^(1/3), on the device.  The catalogue: fof_groups(), fof_ids(), fof_labels()."""
        p = FofParams(float(link_length), float(linklength), float(rhodm), int(primary_types), int(secondary_types),
                      int(group_min_len), float(boxsize), int(bool(periodic)), int(max_iter))
        out = FofResult()
        self._chk(self.L.ghip_fof(self.h, C.byref(p), C.byref(out)))
        self._fof = (out.Ngroups, out.Nids)
        return out

    def fof_groups(self):
        """ghip_fof_get_groups -> structured array (FOF_GROUP_DTYPE) in GrNr order"""
        g = np.zeros(self._fof[0], FOF_GROUP_DTYPE)
        self._chk(self.L.ghip_fof_get_groups(self.h, _ptr(g) if len(g) else None))
        return g

    def fof_ids(self):
        """ghip_fof_get_ids -> int32[Nids], sorted by (GrNr, ID)"""
        ids = np.zeros(self._fof[1], np.int32)
        self._chk(self.L.ghip_fof_get_ids(self.h, _ptr(ids) if len(ids) else None))
        return ids

    def fof_labels(self):
        """ghip_fof_get_labels -> (MinID of each particle's group, its GrNr or -1), int32[n] each"""
        minid, grnr = np.zeros(self.n, np.int32), np.zeros(self.n, np.int32)
        self._chk(self.L.ghip_fof_get_labels(self.h, _ptr(minid), _ptr(grnr)))
        return minid, grnr

    def fof_timing(self):
        """device milliseconds of the last fof(): linking, flattening and labels, secondary rounds, catalogue"""
        ms = np.zeros(4)
        self._chk(self.L.ghip_fof_get_timing(self.h, _ptr(ms)))
        return ms

    def fof_maxdens_task(self):
        """ghip_fof_get_maxdens_task -> int32[Ngroups]: the shard whose local index index_maxdens is (-1: no gas
        member; 0 on a context without a decomposition)"""
        task = np.zeros(self._fof[0], np.int32)
        self._chk(self.L.ghip_fof_get_maxdens_task(self.h, _ptr(task) if len(task) else None))
        return task

    def fof_adopt(self, keep):
        """after a completed DD_GLOBAL_QUANTITIES with walk = FOF_FORM (dd_fof_args -> keep): the sizes the
        catalogue getters read -- Ngroups of the whole system, this shard's own members of kept groups"""
        self._fof = (keep["out"].Ngroups, int(keep["counts"][0]))
        return keep["out"]

    def get_active(self):
        """ghip_get_active: the particle indices of the list in force (int32; 0 .. n-1 when all are active)"""
        n = C.c_int(0)
        self._chk(self.L.ghip_get_active(self.h, None, C.byref(n)))
        idx = np.zeros(n.value, np.int32)
        if n.value:
            self._chk(self.L.ghip_get_active(self.h, _ptr(idx), C.byref(n)))
        return idx

    def find_extent(self):
        """ghip_find_extent: (corner[3], center[3], len) of domain_findExtent over the resident positions --
        what tree_build takes"""
        corner, center, ln = np.zeros(3), np.zeros(3), C.c_double(0)
        self._chk(self.L.ghip_find_extent(self.h, _ptr(corner), _ptr(center), C.byref(ln)))
        return corner, center, ln.value

    def dd_get_sync_point(self):
        """the result of this shard's last completed sync point (DD_DECOMPOSE, walk = SYNC_POINT_FORM) -> SyncPoint"""
        out = SyncPoint()
        self._chk(self.L.ghip_dd_get_sync_point(self.h, C.byref(out)))
        return out

    def set_shard(self, rank, nranks):
        self._chk(self.L.ghip_set_shard(self.h, int(rank), int(nranks)))

    # ---- the path ----
    def tree_build(self, corner, center, dlen, force_softening):
        c0 = np.ascontiguousarray(corner, dtype=np.float64)
        c1 = np.ascontiguousarray(center, dtype=np.float64)
        sf = np.ascontiguousarray(force_softening, dtype=np.float64)
        self._chk(self.L.ghip_tree_build(self.h, _ptr(c0), _ptr(c1), float(dlen), _ptr(sf)))

    def ewald_init(self, boxsize):
        self._chk(self.L.ghip_ewald_init(self.h, float(boxsize)))

    def ewald_table(self):
        t = np.zeros((3, EN + 1, EN + 1, EN + 1))
        self._chk(self.L.ghip_ewald_get_table(self.h, _ptr(t)))
        return t

    def gravity(self, params, walk=WALK_NEWTON):
        self._chk(self.L.ghip_gravity(self.h, C.byref(params), int(walk)))

    def gravity_ext(self, params, pos, ptype, oldacc, walk=WALK_NEWTON, soft=None):
        """soft: gravdata_in.Soft (Hsml of gas targets), used under set_adaptive_gravsoft."""
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        ptype = np.ascontiguousarray(ptype, dtype=np.int32)
        oldacc = np.ascontiguousarray(oldacc, dtype=np.float64)
        soft = None if soft is None else np.ascontiguousarray(soft, dtype=np.float64)
        nt = len(pos)
        acc = np.zeros((nt, 3))
        nint = np.zeros(nt, np.int32)
        self._chk(self.L.ghip_gravity_ext_soft(self.h, C.byref(params), int(walk), nt, _ptr(pos),
                                               _ptr(ptype), None if soft is None else _ptr(soft),
                                               _ptr(oldacc), _ptr(acc), _ptr(nint)))
        return acc, nint

    def set_adaptive_gravsoft(self, on=True):
        """ADAPTIVE_GRAVSOFT_FORGAS: gas softening = Hsml; call before tree_build."""
        self._chk(self.L.ghip_set_adaptive_gravsoft(self.h, int(bool(on))))

    def gravity_finish(self, G):
        self._chk(self.L.ghip_gravity_finish(self.h, float(G)))

    def gravity_finish_ex(self, G, pmgrid=False, comoving_fac=0.0, all_shards=False):
        self._chk(self.L.ghip_gravity_finish_ex(self.h, float(G), int(bool(pmgrid)),
                                                float(comoving_fac), int(bool(all_shards))))

    def gravity_finish_all(self, G):
        self._chk(self.L.ghip_gravity_finish_all(self.h, float(G)))

    def gravity_vacuum_energy(self, fac):
        """GravAccel += fac * Pos (gravtree.c:470-483), fac = OmegaLambda * Hubble^2."""
        self._chk(self.L.ghip_gravity_vacuum_energy(self.h, float(fac)))

    def gravity_direct(self, params):
        self._chk(self.L.ghip_gravity_direct(self.h, C.byref(params)))

    def drift(self, time1, timebase, min_gas_hsml=0.0, box_wrap=False, boxsize=1.0, tables=None,
              log_time_begin=0.0, log_time_max=0.0, pmgrid=False):
        p = DriftParams()
        p.pmgrid = int(bool(pmgrid))
        p.time1, p.Timebase_interval = int(time1), float(timebase)
        p.MinGasHsml, p.box_wrap, p.BoxSize = float(min_gas_hsml), int(box_wrap), float(boxsize)
        if tables is not None:
            self._tabs = [np.ascontiguousarray(t, dtype=np.float64) for t in tables]
            p.ComovingIntegrationOn = 1
            p.logTimeBegin, p.logTimeMax = float(log_time_begin), float(log_time_max)
            p.DriftTable, p.GravKickTable, p.HydroKickTable = [t.ctypes.data for t in self._tabs]
        self._chk(self.L.ghip_drift(self.h, C.byref(p)))

    def pm_kick(self, ti_current, timebase, dt_gravkick, dt_gravkickB, kick_tables=None,
                log_time_begin=0.0, log_time_max=0.0):
        """ghip_pm_kick: Vel += GravPM * dt_gravkick for every particle, VelPred of gas rebuilt."""
        p = PmKickParams()
        p.Ti_Current, p.Timebase_interval = int(ti_current), float(timebase)
        p.dt_gravkick, p.dt_gravkickB = float(dt_gravkick), float(dt_gravkickB)
        if kick_tables is not None:
            self._pktabs = [np.ascontiguousarray(t, dtype=np.float64) for t in kick_tables]
            p.ComovingIntegrationOn = 1
            p.logTimeBegin, p.logTimeMax = float(log_time_begin), float(log_time_max)
            p.GravKickTable, p.HydroKickTable = [t.ctypes.data for t in self._pktabs]
        self._chk(self.L.ghip_pm_kick(self.h, C.byref(p)))

    def set_async(self, on=True):
        """ghip_set_async: drift / kick stop waiting for the device (errors surface at the next sync)"""
        self._chk(self.L.ghip_set_async(self.h, int(bool(on))))

    def run_begin(self, max_steps):
        self._chk(self.L.ghip_run_begin(self.h, int(max_steps)))

    def step_begin(self):
        self._chk(self.L.ghip_step_begin(self.h))

    def step_end(self):
        self._chk(self.L.ghip_step_end(self.h))

    def run_end(self):
        s = RunStats()
        self._chk(self.L.ghip_run_end(self.h, C.byref(s)))
        return s.asdict()

    def timebin_counts(self):
        cnt = (C.c_longlong * 32)()
        sph = (C.c_longlong * 32)()
        self._chk(self.L.ghip_timebin_counts(self.h, cnt, sph))
        return np.array(cnt[:], dtype=np.int64), np.array(sph[:], dtype=np.int64)

    def advance_timesteps(self, params, kick_tables=None, counts=True):
        """ghip_advance_timesteps; returns (TimeBinCount[32], TimeBinCountSph[32]) -- or None with
        counts=False (no recount; under set_async the call then does not wait).  A timestep failure
        raises GhipError with .endrun = the reference's endrun code."""
        if kick_tables is not None:
            self._ktabs = [np.ascontiguousarray(t, dtype=np.float64) for t in kick_tables]
            params.GravKickTable, params.HydroKickTable = [t.ctypes.data for t in self._ktabs]
        if not counts:
            self._chk(self.L.ghip_advance_timesteps(self.h, C.byref(params), None, None))
            return None
        cnt = (C.c_longlong * 32)()
        sph = (C.c_longlong * 32)()
        rc = self.L.ghip_advance_timesteps(self.h, C.byref(params), cnt, sph)
        if rc != 0:
            try:
                self._chk(rc)
            except GhipError as e:
                e.endrun = self.L.ghip_timestep_endrun_code(self.h)
                raise
        return np.array(cnt[:], dtype=np.int64), np.array(sph[:], dtype=np.int64)

    def tree_export(self, maxpart=None, ti_current=0, unequal=0, max_nodes=None, adaptive=False):
        """ghip_tree_export into numpy records of the minimal-flag-set NODE / extNODE layout
        (adaptive: the 96-byte NODE of an ADAPTIVE_GRAVSOFT_FORGAS build, with maxsoft);
        returns (Nodes, Extnodes, Nextnode, Father) with Nodes[k] = node maxpart + k."""
        maxpart = self.n if maxpart is None else int(maxpart)
        max_nodes = int(2.0 * maxpart + 16) if max_nodes is None else int(max_nodes)
        lay = NodeLayout()
        ndt = NODE_ADAPTIVE_DTYPE if adaptive else NODE_DTYPE
        lay.node_stride = ndt.itemsize
        lay.n_maxsoft = ndt.fields["maxsoft"][1] if adaptive else -1
        for name, key in (("len", "n_len"), ("center", "n_center"), ("s", "n_s"), ("mass", "n_mass"),
                          ("bitflags", "n_bitflags"), ("sibling", "n_sibling"),
                          ("nextnode", "n_nextnode"), ("father", "n_father"),
                          ("Ti_current", "n_ti_current")):
            setattr(lay, key, ndt.fields[name][1])
        lay.ext_stride = EXTNODE_DTYPE.itemsize
        for name, key in (("dp", "e_dp"), ("vs", "e_vs"), ("vmax", "e_vmax"),
                          ("divVmax", "e_divvmax"), ("hmax", "e_hmax"),
                          ("Ti_lastkicked", "e_ti_lastkicked"), ("Flag", "e_flag")):
            setattr(lay, key, EXTNODE_DTYPE.fields[name][1])
        nodes = np.zeros(max_nodes, ndt)
        ext = np.zeros(max_nodes, EXTNODE_DTYPE)
        nxt = np.full(maxpart, -1, np.int32)
        fat = np.full(maxpart, -1, np.int32)
        nn = C.c_int(0)
        self._chk(self.L.ghip_tree_export(self.h, C.byref(lay), maxpart, int(ti_current),
                                          int(unequal), _ptr(nodes), _ptr(ext), _ptr(nxt), _ptr(fat),
                                          max_nodes, C.byref(nn)))
        return nodes[:nn.value], ext[:nn.value], nxt, fat

    def potential(self, params):
        """ghip_potential(PotParams): compute_potential() of every particle (see get_potential)."""
        self._chk(self.L.ghip_potential(self.h, C.byref(params)))

    def get_potential(self):
        a = np.zeros(self.n)
        self._chk(self.L.ghip_get_potential(self.h, _ptr(a)))
        return a

    def potential_interactions(self):
        """(sum over targets, largest per target) of the last potential walk's interactions"""
        s, m = C.c_longlong(0), C.c_longlong(0)
        self._chk(self.L.ghip_potential_interactions(self.h, C.byref(s), C.byref(m)))
        return s.value, m.value

    def get_potential_interactions(self):
        """interactions of the last potential walk per target, host order (ghip_get_potential_interactions)"""
        a = np.zeros(self.n, np.int64)
        self._chk(self.L.ghip_get_potential_interactions(self.h, _ptr(a)))
        return a

    def ewald_pot_table(self, boxsize):
        """potcorr[EN+1][EN+1][EN+1] / BoxSize of ewald_init (forcetree.c:4466-4525)"""
        t = np.zeros((EN + 1, EN + 1, EN + 1))
        self._chk(self.L.ghip_ewald_get_pot_table(self.h, float(boxsize), _ptr(t)))
        return t

    def global_quantities(self, params, grav_kick_table=None, hydro_kick_table=None,
                          old_photon_momentum=None, potential=None):
        """ghip_global_quantities(GlobalParams) -> dict of the per-type sums (GlobalSums.asdict).
        The host arrays go into a copy of params (the caller's object keeps no pointers to them) and
        stay alive for the call; potential: P[].p.Potential, None = the last potential() of this state."""
        p = GlobalParams.from_buffer_copy(params)
        keep = []
        for name, arr in (("GravKickTable", grav_kick_table), ("HydroKickTable", hydro_kick_table),
                          ("OldPhotonMomentum", old_photon_momentum), ("Potential", potential)):
            a = None if arr is None else np.ascontiguousarray(arr, dtype=np.float64)
            if a is not None and name in ("OldPhotonMomentum", "Potential") and len(a) != self.n:
                raise ValueError("%s: expected %d values, got %d" % (name, self.n, len(a)))
            keep.append(a)
            setattr(p, name, None if a is None else a.ctypes.data)
        out = GlobalSums()
        self._chk(self.L.ghip_global_quantities(self.h, C.byref(p), C.byref(out)))
        return out.asdict()

    def pm_periodic(self, pmgrid, boxsize, G, asmth=None):
        """ghip_pm_periodic: fills F_GRAVPM; asmth defaults to ASMTH * BoxSize / PMGRID."""
        p = PmParams(int(pmgrid), float(boxsize), float(G),
                     float(1.25 * boxsize / pmgrid if asmth is None else asmth))
        self._chk(self.L.ghip_pm_periodic(self.h, C.byref(p)))


    def pm_find_region(self, pmgrid):
        """ghip_pm_find_region: the region of the non-periodic mesh from the resident positions, stored in
        the context; returns it (PmRegion)"""
        r = PmRegion()
        self._chk(self.L.ghip_pm_find_region(self.h, int(pmgrid), C.byref(r)))
        return r

    def pm_set_region(self, region):
        """ghip_pm_set_region(PmRegion): a region the host kept (restart)"""
        self._chk(self.L.ghip_pm_set_region(self.h, C.byref(region)))

    def pm_get_region(self):
        """ghip_pm_get_region: the region in force (GHIP_EINVAL: none)"""
        r = PmRegion()
        rc = self.L.ghip_pm_get_region(self.h, C.byref(r))
        if rc != 0:
            raise GhipError(rc, "ghip_pm_get_region: no region is set")
        return r

    def pm_nonperiodic(self, pmgrid, G, comoving=0, omega0=0.0, omega_lambda=0.0, hubble=0.0):
        """ghip_pm_nonperiodic: fills F_GRAVPM (mesh force and the tail of long_range_force); GhipError with
        GHIP_EREGION when a particle left the region: pm_find_region(), then call again"""
        p = PmnpParams(int(pmgrid), float(G), int(comoving), float(omega0), float(omega_lambda), float(hubble))
        self._chk(self.L.ghip_pm_nonperiodic(self.h, C.byref(p)))

    def velocity_moments(self):
        v2 = (C.c_double * 6)()
        mm = (C.c_double * 6)()
        cnt = (C.c_longlong * 6)()
        self._chk(self.L.ghip_velocity_moments(self.h, v2, mm, cnt))
        return np.array(v2[:]), np.array(mm[:]), np.array(cnt[:], dtype=np.int64)

    def density(self, params):
        self._chk(self.L.ghip_density(self.h, C.byref(params)))

    def update_hmax(self):
        self._chk(self.L.ghip_update_hmax(self.h))

    def hydro(self, params):
        self._chk(self.L.ghip_hydro(self.h, C.byref(params)))

    def density_evaluate(self, params, target, h):
        out = np.zeros(7)
        self._chk(self.L.ghip_density_evaluate(self.h, C.byref(params), int(target), float(h),
                                               _ptr(out)))
        return out

    def ngb_treefind(self, center, hsml, pairs, periodic, boxsize, cap=None):
        c = np.ascontiguousarray(center, dtype=np.float64)
        cap = self.ngas if cap is None else cap
        buf = np.zeros(max(cap, 1), np.int32)
        nf = C.c_int(0)
        self._chk(self.L.ghip_ngb_treefind(self.h, _ptr(c), float(hsml), int(pairs),
                                           int(periodic), float(boxsize), _ptr(buf), int(cap),
                                           C.byref(nf)))
        return buf[:min(nf.value, cap)].copy(), nf.value

    def debug_prim(self, prim, values=None, flags=None, end_bit=0):
        """one device primitive on host ints (PRIM_*): the scan, (the selected values, their count), the sort's permutation"""
        a, f = [None if v is None else np.ascontiguousarray(v, dtype=np.int32) for v in (values, flags)]
        out, cnt = np.zeros(len(f if a is None else a), np.int32), C.c_int(-1)
        self._chk(self.L.ghip_debug_prim(self.h, int(prim), len(out), int(end_bit), _ptr(a), _ptr(f), _ptr(out), C.byref(cnt)))
        return (out[:cnt.value].copy(), cnt.value) if prim in (PRIM_SELECT, PRIM_WSELECT) else out

    def peano_hilbert_keys(self, x, y, z, bits=21):
        x, y, z = [np.ascontiguousarray(a, dtype=np.int32) for a in (x, y, z)]
        k = np.zeros(len(x), np.uint64)
        self._chk(self.L.ghip_peano_hilbert_keys(self.h, len(x), _ptr(x), _ptr(y), _ptr(z),
                                                 int(bits), _ptr(k)))
        return k

    def morton_keys(self, x, y, z, bits=21):
        x, y, z = [np.ascontiguousarray(a, dtype=np.int32) for a in (x, y, z)]
        k = np.zeros(len(x), np.uint64)
        self._chk(self.L.ghip_morton_keys(self.h, len(x), _ptr(x), _ptr(y), _ptr(z), int(bits),
                                          _ptr(k)))
        return k

    def stats(self):
        s = Stats()
        self._chk(self.L.ghip_get_stats(self.h, C.byref(s)))
        return s.asdict()

    def tree_dump(self, which=0):
        ne = C.c_int(0)
        self._chk(self.L.ghip_tree_dump(self.h, which, C.byref(ne), None, None, None, None, None))
        ne = ne.value
        npart = self.ngas if which else self.n
        out = dict(xm=np.zeros((ne, 4)), cl=np.zeros((ne, 4)), lk=np.zeros((ne, 4), np.int32),
                   aux=np.zeros(ne), perm=np.zeros(npart, np.int32))
        n2 = C.c_int(0)
        self._chk(self.L.ghip_tree_dump(self.h, which, C.byref(n2), _ptr(out["xm"]),
                                        _ptr(out["cl"]), _ptr(out["lk"]), _ptr(out["aux"]),
                                        _ptr(out["perm"])))
        return out

    # ---- sub-steps on the tree of the last full build (forcetree.c:1356-1651) ----
    def set_massless_gas_rule(self, rule=3):
        self._chk(self.L.ghip_set_massless_gas_rule(self.h, int(rule)))

    def set_dynamic_tree(self, on=True):
        self._chk(self.L.ghip_set_dynamic_tree(self.h, int(bool(on))))

    def tree_substep(self, dt_drift):
        self._chk(self.L.ghip_tree_substep(self.h, float(dt_drift)))

    def tree_kick_nodes(self, idx, dv):
        idx = np.ascontiguousarray(idx, np.int32)
        dv = np.ascontiguousarray(dv, np.float64)
        assert dv.shape == (len(idx), 3)
        self._chk(self.L.ghip_tree_kick_nodes(self.h, len(idx), _ptr(idx), _ptr(dv)))

    def tree_dump_dynamic(self):
        ne = C.c_int(0)
        self._chk(self.L.ghip_tree_dump_dynamic(self.h, C.byref(ne), None, None, None, None))
        ne = ne.value
        out = dict(xm=np.zeros((ne, 4)), cl=np.zeros((ne, 4)), ev=np.zeros((ne, 4)),
                   lk=np.zeros((ne, 4), np.int32))
        n2 = C.c_int(0)
        self._chk(self.L.ghip_tree_dump_dynamic(self.h, C.byref(n2), _ptr(out["xm"]), _ptr(out["cl"]),
                                                _ptr(out["ev"]), _ptr(out["lk"])))
        return out

    def sync(self):
        self._chk(self.L.ghip_sync(self.h))

    @property
    def stream(self):
        return self.L.ghip_stream(self.h)

    # ---- "next" row N4: sinks ----
    def sink_density(self, params, ngb_factor, sinks, hsml):
        sinks = np.ascontiguousarray(sinks, np.int32)
        ns = len(sinks)
        out = dict(hsml=np.ascontiguousarray(hsml, np.float64).copy(), numngb=np.zeros(ns),
                   density=np.zeros(ns), entropy=np.zeros(ns), gasvel=np.zeros((ns, 3)))
        it = C.c_int(0)
        self._chk(self.L.ghip_sink_density(self.h, C.byref(params), float(ngb_factor), ns, _ptr(sinks),
                                           _ptr(out["hsml"]), _ptr(out["numngb"]),
                                           _ptr(out["density"]), _ptr(out["entropy"]),
                                           _ptr(out["gasvel"]), C.byref(it)))
        out["iterations"] = it.value
        return out

    # ---- the sinks on the resident state: the table keyed by ID, blackhole_accretion(), BH_FORM ----
    def sinks_set_table(self, ids, rows):
        """ghip_sinks_set_table: ids [nsink] (P[].ID), rows [nsink][SK_COUNT], in any order"""
        ids = np.ascontiguousarray(ids, np.uint32)
        rows = np.ascontiguousarray(rows, np.float64).reshape(len(ids), SK_COUNT)
        self._chk(self.L.ghip_sinks_set_table(self.h, len(ids), _ptr(ids), _ptr(rows)))

    def sinks_table(self):
        """ghip_sinks_get_table -> (ids uint32 [nsink] ascending, rows [nsink][SK_COUNT])"""
        ns = C.c_int(0)
        self._chk(self.L.ghip_sinks_get_table(self.h, C.byref(ns), None, None))
        ids, rows = np.zeros(ns.value, np.uint32), np.zeros((ns.value, SK_COUNT))
        self._chk(self.L.ghip_sinks_get_table(self.h, C.byref(ns), _ptr(ids), _ptr(rows)))
        return ids, rows

    def sinks_clear(self):
        self._chk(self.L.ghip_sinks_clear(self.h))

    def sinks_density(self, params, ngb_factor):
        """ghip_sinks_density for the active Type-5 particles -> the iteration count; Hsml goes to F_HSML, the
        other results into the table's rows"""
        it = C.c_int(0)
        self._chk(self.L.ghip_sinks_density(self.h, C.byref(params), float(ngb_factor), C.byref(it)))
        return it.value

    def blackhole_accretion(self, bh_params, acc_params):
        """ghip_blackhole_accretion -> dict(bin_mass, bin_dynmass, bin_mdot [32], counts [3] = gas / sinks /
        dust swallowed, nactive)"""
        rep = BhAccretionReport()
        self._chk(self.L.ghip_blackhole_accretion(self.h, C.byref(bh_params), C.byref(acc_params), C.byref(rep)))
        return dict(bin_mass=np.array(rep.TimeBin_BH_mass), bin_dynmass=np.array(rep.TimeBin_BH_dynamicalmass),
                    bin_mdot=np.array(rep.TimeBin_BH_Mdot), counts=np.array(rep.swallowed, np.int64),
                    nactive=rep.nactive_sinks)

    def sfr_form_sinks(self, ncand, u01, limited_accretion=True):
        """ghip_sfr_form_sinks for the candidates of the last sfr_cooling() -> dict(stars_converted,
        sum_mass_stars, converted_in_bin [32])"""
        u = np.ascontiguousarray(u01, np.float64)
        if len(u) < ncand:
            raise ValueError("u01 holds %d draws for %d candidates" % (len(u), ncand))
        rep = SfrFormReport()
        self._chk(self.L.ghip_sfr_form_sinks(self.h, int(ncand), _ptr(u), int(bool(limited_accretion)),
                                             C.byref(rep)))
        return dict(stars_converted=rep.stars_converted, sum_mass_stars=rep.sum_mass_stars,
                    converted_in_bin=np.array(rep.converted_in_bin, np.int64))

    def sink_reset(self):
        self._chk(self.L.ghip_sink_reset(self.h))

    def blackhole_evaluate(self, params, sinks, sink_ids, mdot, bh_density):
        sinks = np.ascontiguousarray(sinks, np.int32)
        ids = np.ascontiguousarray(sink_ids, np.uint32)
        md = np.ascontiguousarray(mdot, np.float64)
        rho = np.ascontiguousarray(bh_density, np.float64)
        self._chk(self.L.ghip_blackhole_evaluate(self.h, C.byref(params), len(sinks), _ptr(sinks),
                                                 _ptr(ids), _ptr(md), _ptr(rho)))

    def blackhole_swallow(self, params, sinks, sink_ids, sink_bh_mass):
        sinks = np.ascontiguousarray(sinks, np.int32)
        ids = np.ascontiguousarray(sink_ids, np.uint32)
        ns = len(sinks)
        out = dict(bh_mass=np.ascontiguousarray(sink_bh_mass, np.float64).copy(),
                   acc_mass=np.zeros(ns), acc_bhmass=np.zeros(ns), acc_dustmass=np.zeros(ns),
                   acc_momentum=np.zeros((ns, 3)), counts=np.zeros(3, np.int64))
        self._chk(self.L.ghip_blackhole_swallow(self.h, C.byref(params), ns, _ptr(sinks), _ptr(ids),
                                                _ptr(out["bh_mass"]), _ptr(out["acc_mass"]),
                                                _ptr(out["acc_bhmass"]), _ptr(out["acc_dustmass"]),
                                                _ptr(out["acc_momentum"]), _ptr(out["counts"])))
        return out

    def sink_marks(self):
        sw = np.zeros(self.n, np.uint32)
        inj = np.zeros(self.ngas)
        self._chk(self.L.ghip_sink_get_marks(self.h, _ptr(sw), _ptr(inj)))
        return sw, inj

    def set_sink_marks(self, swallow_id=None, injected=None):
        sw = None if swallow_id is None else np.ascontiguousarray(swallow_id, np.uint32)
        inj = None if injected is None else np.ascontiguousarray(injected, np.float64)
        self._chk(self.L.ghip_sink_set_marks(self.h, _ptr(sw), _ptr(inj)))

    def cooling_and_starformation(self, timebase, crit_density, min_egy, u_to_temp_fac):
        flag = np.zeros(self.ngas, np.int32)
        self._chk(self.L.ghip_cooling_and_starformation(self.h, float(timebase), float(crit_density),
                                                        float(min_egy), float(u_to_temp_fac),
                                                        _ptr(flag)))
        return flag

    def sfr_cooling(self, params, count_only=False):
        """ghip_sfr_cooling -> the sink candidates' particle indices in active-list order (int32);
        with count_only, their number"""
        nc = C.c_int(0)
        if count_only:
            self._chk(self.L.ghip_sfr_cooling(self.h, C.byref(params), C.byref(nc), None))
            return nc.value
        cap = max(self.counts()[0], getattr(self, "_active_n", None) or 0, 1)   # >= the active count
        cand = np.zeros(cap, np.int32)
        self._chk(self.L.ghip_sfr_cooling(self.h, C.byref(params), C.byref(nc), _ptr(cand)))
        return cand[:nc.value].copy()

    def find_smbh(self, smbh_mass):
        """ghip_find_smbh -> (pos [3], count) of FindQuasars over the active particles"""
        pos = np.zeros(3)
        cnt = C.c_int(0)
        self._chk(self.L.ghip_find_smbh(self.h, float(smbh_mass), _ptr(pos), C.byref(cnt)))
        return pos, cnt.value

    # ---- dust-gas drag (dust.c): grains in list order ----
    def dust_density(self, params, dust):
        dust = np.ascontiguousarray(dust, np.int32)
        out = np.zeros(len(dust))
        self._chk(self.L.ghip_dust_density(self.h, C.byref(params), len(dust), _ptr(dust), _ptr(out)))
        return out

    def dust_drag(self, params, dust, dust_density, dust_entropy, dust_gasvel, dust_radius,
                  particle_density, particle_velocity, vcoll):
        """-> dict(particle_velocity, delta_momentum, delta_energy, vcoll); the in/out arrays are copies"""
        dust = np.ascontiguousarray(dust, np.int32)
        nd = len(dust)
        f = [np.ascontiguousarray(a, np.float64) for a in
             (dust_density, dust_entropy, dust_gasvel, dust_radius, particle_density)]
        assert f[2].shape == (nd, 3)
        out = dict(particle_velocity=np.ascontiguousarray(particle_velocity, np.float64).reshape(nd, 3).copy(),
                   delta_momentum=np.zeros((nd, 3)), delta_energy=np.zeros(nd),
                   vcoll=np.ascontiguousarray(vcoll, np.float64).copy())
        self._chk(self.L.ghip_dust_drag(self.h, C.byref(params), nd, _ptr(dust), *[_ptr(a) for a in f],
                                        _ptr(out["particle_velocity"]), _ptr(out["delta_momentum"]),
                                        _ptr(out["delta_energy"]), _ptr(out["vcoll"])))
        return out

    def set_dust_model(self, model=None):
        """DustModel or None (the shipped bundle: no switch); governs both dust passes, on one rank and on
        shards"""
        self._chk(self.L.ghip_set_dust_model(self.h, None if model is None else C.byref(model)))

    def dust_density_grains(self, params, dust):
        """-> dict(particle_density, particle_velocity): d7 and, with real_pebble_collisions, the raw d9 sums
        (left at zero otherwise)"""
        g, a = dust_grains(dust)
        self._chk(self.L.ghip_dust_density_grains(self.h, C.byref(params), C.byref(g)))
        return dict(particle_density=a["particle_density"], particle_velocity=a["particle_velocity"])

    def dust_drag_grains(self, params, dust, dust_density, dust_entropy, dust_gasvel, dust_radius,
                         particle_density, particle_velocity, vcoll, log_radius_by_dt=None, logr=True):
        """-> dict(particle_velocity, delta_momentum, delta_energy, vcoll, dust_radius, log_radius_by_dt); the
        in/out arrays are copies.  logr = False passes log_radius_by_dt = NULL."""
        g, a = dust_grains(dust, particle_density, dust_density, dust_entropy, dust_gasvel, dust_radius,
                           particle_velocity, vcoll, log_radius_by_dt, logr)
        assert a["dust_gasvel"].shape == (len(a["dust_idx"]), 3)
        self._chk(self.L.ghip_dust_drag_grains(self.h, C.byref(params), C.byref(g)))
        return {k: a[k] for k in ("particle_velocity", "delta_momentum", "delta_energy", "vcoll", "dust_radius",
                                  "log_radius_by_dt") if k in a}

    def dust_drag_heating(self):
        dh = np.zeros(self.ngas)
        self._chk(self.L.ghip_dust_get_drag_heating(self.h, _ptr(dh)))
        return dh

    def set_dust_drag_heating(self, dh):
        dh = np.ascontiguousarray(dh, np.float64)
        assert dh.shape == (self.ngas,)
        self._chk(self.L.ghip_dust_set_drag_heating(self.h, _ptr(dh)))

    # ---- wind particles (momentum_feedback.c): Type-3 particles in list order ----
    def wind_density(self, params, wind, dt_jump):
        """one virtual_density(): -> (new_density, drmin)"""
        wind = np.ascontiguousarray(wind, np.int32)
        dtj = np.ascontiguousarray(dt_jump, np.float64)
        assert dtj.shape == wind.shape
        rho, drmin = np.zeros(len(wind)), np.zeros(len(wind))
        self._chk(self.L.ghip_wind_density(self.h, C.byref(params), len(wind), _ptr(wind), _ptr(dtj), _ptr(rho),
                                           _ptr(drmin)))
        return rho, drmin

    def wind_spread(self, params, wind, dt_jump, new_density, delta_momentum):
        """one virtual_spread_momentum() into the resident Injected_BH_Momentum"""
        wind = np.ascontiguousarray(wind, np.int32)
        a = [np.ascontiguousarray(v, np.float64) for v in (dt_jump, new_density, delta_momentum)]
        assert all(v.shape == wind.shape for v in a)
        self._chk(self.L.ghip_wind_spread(self.h, C.byref(params), len(wind), _ptr(wind), *[_ptr(v) for v in a]))

    def wind_feedback(self, params, wind, stellar_age, birth_energy, old_momentum, new_density, drmin,
                      check=True):
        """the propagation loop -> dict(rc, old_momentum, new_density, drmin, dt1, dt2, dt_jump, delta_momentum,
        deleted, iterations, bits, ndeleted, deleted_momentum); check = False returns GHIP_ENOCONV as rc"""
        wind = np.ascontiguousarray(wind, np.int32)
        nw = len(wind)
        f64 = lambda v: np.ascontiguousarray(v, np.float64).reshape(nw).copy()
        a = dict(stellar_age=f64(stellar_age), birth_energy=f64(birth_energy), old_momentum=f64(old_momentum),
                 new_density=f64(new_density), drmin=f64(drmin), dt1=np.zeros(nw), dt2=np.zeros(nw),
                 dt_jump=np.zeros(nw), delta_momentum=np.zeros(nw), deleted=np.zeros(nw, np.int32))
        st = WindState()
        for k, v in a.items():
            setattr(st, k, v.ctypes.data)
        res = WindResult()
        rc = self.L.ghip_wind_feedback(self.h, C.byref(params), nw, _ptr(wind), C.byref(st), C.byref(res))
        if check or rc != GHIP_ENOCONV:
            self._chk(rc)
        a.update(rc=rc, iterations=res.iterations, bits=res.bits, ndeleted=res.ndeleted,
                 deleted_momentum=res.deleted_momentum)
        return a

    # ---- the wind particles on the resident state: the table keyed by particle index, the loop, the spawn ----
    def winds_set_table(self, idx, rows):
        """ghip_winds_set_table: idx [nwind] (particle indices of Type-3 particles), rows [nwind][WK_COUNT], in
        any order"""
        idx = np.ascontiguousarray(idx, np.int32)
        rows = np.ascontiguousarray(rows, np.float64).reshape(len(idx), WK_COUNT)
        self._chk(self.L.ghip_winds_set_table(self.h, len(idx), _ptr(idx), _ptr(rows)))

    def winds_table(self):
        """ghip_winds_get_table -> (idx int32 [nwind] ascending, rows [nwind][WK_COUNT])"""
        nw = C.c_int(0)
        self._chk(self.L.ghip_winds_get_table(self.h, C.byref(nw), None, None))
        idx, rows = np.zeros(nw.value, np.int32), np.zeros((nw.value, WK_COUNT))
        self._chk(self.L.ghip_winds_get_table(self.h, C.byref(nw), _ptr(idx), _ptr(rows)))
        return idx, rows

    def winds_clear(self):
        self._chk(self.L.ghip_winds_clear(self.h))

    def dd_winds_set_table(self, idx, rows):
        """ghip_dd_winds_set_table: the wind table of this shard (a dd_init context of any rank count); idx are
        LOCAL particle indices"""
        idx = np.ascontiguousarray(idx, np.int32)
        rows = np.ascontiguousarray(rows, np.float64).reshape(len(idx), WK_COUNT)
        self._chk(self.L.ghip_dd_winds_set_table(self.h, len(idx), _ptr(idx), _ptr(rows)))

    def dd_winds_table(self):
        """ghip_dd_winds_get_table -> (local idx int32 [nwind] ascending, rows [nwind][WK_COUNT])"""
        nw = C.c_int(0)
        self._chk(self.L.ghip_dd_winds_get_table(self.h, C.byref(nw), None, None))
        idx, rows = np.zeros(nw.value, np.int32), np.zeros((nw.value, WK_COUNT))
        self._chk(self.L.ghip_dd_winds_get_table(self.h, C.byref(nw), _ptr(idx), _ptr(rows)))
        return idx, rows

    def dd_winds_clear(self):
        self._chk(self.L.ghip_dd_winds_clear(self.h))

    def winds_feedback(self, params, check=True):
        """ghip_winds_feedback: the propagation loop for the active Type-3 particles with a row and StellarAge <
        Time -> dict(rc, iterations, bits, ndeleted, deleted_momentum); the state is in winds_table().  check =
        False returns GHIP_ENOCONV as rc"""
        res = WindResult()
        rc = self.L.ghip_winds_feedback(self.h, C.byref(params), C.byref(res))
        if check or rc != GHIP_ENOCONV:
            self._chk(rc)
        return dict(rc=rc, iterations=res.iterations, bits=res.bits, ndeleted=res.ndeleted,
                    deleted_momentum=res.deleted_momentum)

    def wind_spawn(self, params, rnd_table=None):
        """ghip_wind_spawn: the massive active sinks create wind particles -> dict(spawned, nsinks_emitting,
        first_index, new_wind_exact_sum, gsl_draws); .n follows.  rnd_table None: the table of set_rnd_table.
        After a call that spawned: tree_build."""
        t = None if rnd_table is None else np.ascontiguousarray(rnd_table, np.float64)
        params.rnd_table = None if t is None else t.ctypes.data
        params.nrnd = 0 if t is None else len(t)
        rep = WindSpawnReport()
        self._chk(self.L.ghip_wind_spawn(self.h, C.byref(params), C.byref(rep)))
        self.n += rep.spawned
        if rep.spawned and getattr(self, "_active_n", None) is not None:
            self._active_n += rep.spawned
        return dict(spawned=rep.spawned, nsinks_emitting=rep.nsinks_emitting, first_index=rep.first_index,
                    new_wind_exact_sum=rep.new_wind_exact_sum, gsl_draws=rep.gsl_draws)

    def wind_injected(self):
        out = np.zeros((self.ngas, 3))
        self._chk(self.L.ghip_wind_get_injected(self.h, _ptr(out)))
        return out

    def set_wind_injected(self, v):
        v = np.ascontiguousarray(v, np.float64)
        assert v.shape == (self.ngas, 3)
        self._chk(self.L.ghip_wind_set_injected(self.h, _ptr(v)))

    def wind_rad_accel(self):
        out = np.zeros((self.ngas, 3))
        self._chk(self.L.ghip_wind_get_rad_accel(self.h, _ptr(out)))
        return out

    def set_wind_rad_accel(self, v):
        v = np.ascontiguousarray(v, np.float64)
        assert v.shape == (self.ngas, 3)
        self._chk(self.L.ghip_wind_set_rad_accel(self.h, _ptr(v)))

    def set_rad_accel(self, on):
        """RAD_ACCEL in advance_timesteps, pm_kick and drift"""
        self._chk(self.L.ghip_set_rad_accel(self.h, int(bool(on))))

    def wind_timing(self):
        """ms of the last wind_feedback: move, density, spread, list, whole call"""
        ms = np.zeros(5)
        self._chk(self.L.ghip_wind_get_timing(self.h, _ptr(ms)))
        return ms

    # ---- the shipped bundle's integrator rules (ghip_set_integration_flags) ----
    def set_integration_flags(self, flags=None):
        """IntegrationFlags or None (the minimal flag set); governs advance_timesteps and drift"""
        self._chk(self.L.ghip_set_integration_flags(self.h, None if flags is None else C.byref(flags)))

    # ---- the viscosity of the SPH pair loop (ghip_set_viscosity) ----
    def set_viscosity(self, params=None):
        """ViscParams or None (the constant viscosity of HydroParams); governs hydro, DD_HYDRO and
        advance_timesteps"""
        self._chk(self.L.ghip_set_viscosity(self.h, None if params is None else C.byref(params)))

    # ---- randomised subnodes for coincident particles (ghip_set_rnd_table) ----
    def set_rnd_table(self, table=None):
        """the host's RndTable (any length; entries in [0, 1)) or None: unbind.  Copied by the call; governs
        every tree_build after it.  IDs are the F_ID field."""
        if table is None:
            self._chk(self.L.ghip_set_rnd_table(self.h, None, 0))
            return
        t = np.ascontiguousarray(table, np.float64)
        self._chk(self.L.ghip_set_rnd_table(self.h, _ptr(t), len(t)))

    def tree_max_level(self):
        """GHIP_TREE_MAXLEVEL: digits of a particle's path while a table is bound"""
        return int(self.L.ghip_tree_max_level())

    def visc_set_alpha(self, alpha, dtalpha=None):
        """SphP[].alpha and SphP[].Dtalpha (None: zeros) of the resident gas, [ngas]"""
        a = np.ascontiguousarray(alpha, np.float64)
        d = None if dtalpha is None else np.ascontiguousarray(dtalpha, np.float64)
        assert a.shape == (self.ngas,) and (d is None or d.shape == (self.ngas,))
        self._chk(self.L.ghip_visc_set_alpha(self.h, _ptr(a), _ptr(d)))

    def visc_get(self):
        """(alpha, Dtalpha) of the resident gas"""
        a, d = np.zeros(self.ngas), np.zeros(self.ngas)
        self._chk(self.L.ghip_visc_get(self.h, _ptr(a), _ptr(d)))
        return a, d

    visc_derive = staticmethod(visc_derive)

    def kick_set_fields(self, drag_accel=None, gas_dust_momentum=None, new_density=None):
        """gas DragAccel [ngas][3], gas DeltaDustMomentum [ngas][3], NewDensity [n]; None = zero"""
        a = [None if v is None else np.ascontiguousarray(v, np.float64) for v in
             (drag_accel, gas_dust_momentum, new_density)]
        for v, shape in zip(a, ((self.ngas, 3), (self.ngas, 3), (self.n,))):
            assert v is None or v.shape == shape
        self._chk(self.L.ghip_kick_set_fields(self.h, *[None if v is None else _ptr(v) for v in a]))

    def kick_fields(self):
        """ghip_kick_get_fields -> (DragAccel [ngas][3], DeltaDustMomentum [ngas][3], NewDensity [n]); None for an
        array the context does not hold for its current counts"""
        a = [np.zeros((self.ngas, 3)), np.zeros((self.ngas, 3)), np.zeros(self.n)]
        held = np.zeros(3, np.int32)
        self._chk(self.L.ghip_kick_get_fields(self.h, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(held)))
        return tuple(v if h else None for v, h in zip(a, held))

    def kick_drag_accel(self):
        out = np.zeros((self.ngas, 3))
        self._chk(self.L.ghip_kick_get_drag_accel(self.h, _ptr(out)))
        return out

    # ---- multi-GPU: domain decomposition with tree-node / ghost exchange (include/ghip.h) ----
    def dd_init(self, rank, nranks):
        self._chk(self.L.ghip_dd_init(self.h, int(rank), int(nranks)))

    def dd_set_domain(self, corner, center, dlen, force_softening):
        c0 = np.ascontiguousarray(corner, np.float64)
        c1 = np.ascontiguousarray(center, np.float64)
        so = np.ascontiguousarray(force_softening, np.float64)
        self._chk(self.L.ghip_dd_set_domain(self.h, _ptr(c0), _ptr(c1), float(dlen), _ptr(so)))

    def dd_set_splits(self, splits):
        sp = np.ascontiguousarray(splits, np.uint64)
        self._chk(self.L.ghip_dd_set_splits(self.h, _ptr(sp)))

    def dd_get_splits(self):
        """the key ranges in force (nranks + 1 uint64): what dd_set_splits or DD_DECOMPOSE stored last"""
        out = np.zeros(self.dd_info()["nranks"] + 1, np.uint64)
        self._chk(self.L.ghip_dd_get_splits(self.h, _ptr(out)))
        return out

    def dd_get_domain(self):
        """(corner[3], center[3], len) of the domain cube in force"""
        corner, center, ln = np.zeros(3), np.zeros(3), C.c_double(0)
        self._chk(self.L.ghip_dd_get_domain(self.h, _ptr(corner), _ptr(center), C.byref(ln)))
        return corner, center, ln.value

    def dd_keys(self):
        out = np.zeros(self.n, np.uint64)
        self._chk(self.L.ghip_dd_keys(self.h, _ptr(out)))
        return out

    def dd_set_ghost_margin(self, margin):
        self._chk(self.L.ghip_dd_set_ghost_margin(self.h, float(margin)))

    def dd_set_guests(self, on=True):
        """ghip_dd_set_guests: accept resident particles whose keys left this shard's pieces of the curve
        (the same value on every shard)"""
        self._chk(self.L.ghip_dd_set_guests(self.h, int(bool(on))))

    def dd_begin(self, op, params, walk=0):
        self._dd_params = params          # keep the struct alive
        ptr = None if params is None else C.cast(C.byref(params), C.c_void_p)
        self._chk(self.L.ghip_dd_begin(self.h, int(op), ptr, int(walk)))

    def counts(self):
        """(numpart, ngas) of the context -- they change when particles migrate"""
        out = np.zeros(16, np.int64)
        self._chk(self.L.ghip_dd_get_info(self.h, _ptr(out)))
        self.n, self.ngas = int(out[11]), int(out[12])
        return self.n, self.ngas

    def dd_step(self):
        rc = self.L.ghip_dd_step(self.h)
        if rc < 0:
            self._chk(rc)
        return rc

    def dd_exchange(self):
        self._chk(self.L.ghip_dd_exchange(self.h))

    @staticmethod
    def allgather_callback(allgather):
        """`allgather(send: bytes) -> bytes of all ranks, rank-major` as the C callback of
        ghip_dd_exchange_host (keep the returned object alive while it is in use)."""
        def cb(_user, send, nbytes, recv):
            try:
                data = C.string_at(send, nbytes)
                out = allgather(data)
                C.memmove(recv, out, len(out))
                return 0
            except Exception:   # noqa: BLE001 -- reported through the C return code
                import traceback
                traceback.print_exc()
                return 1
        return ALLGATHER_CB(cb)

    def dd_exchange_host(self, fn):
        self._chk(self.L.ghip_dd_exchange_host(self.h, fn, None))

    def dd_set_segments(self, keys, owner):
        keys = np.ascontiguousarray(keys, np.uint64)
        owner = np.ascontiguousarray(owner, np.int32)
        assert len(keys) == len(owner) + 1
        self._chk(self.L.ghip_dd_set_segments(self.h, len(owner), _ptr(keys), _ptr(owner)))

    def dd_run_host(self, op, params, allgather, walk=0):
        """The operation with every exchange staged through the host and `allgather(send: bytes)
        -> bytes of all ranks, rank-major` (ghip_dd_exchange_host)."""
        fn = self.allgather_callback(allgather)
        self.dd_begin(op, params, walk)
        while True:
            rc = self.dd_step()
            if rc == 0:
                break
            self._chk(self.L.ghip_dd_exchange_host(self.h, fn, None))
        if op == DD_MIGRATE:
            self.counts()

    def dd_run(self, op, params, walk=0):
        ptr = None if params is None else C.cast(C.byref(params), C.c_void_p)
        self._chk(self.L.ghip_dd_run(self.h, int(op), ptr, int(walk)))
        if op == DD_MIGRATE:
            self.counts()

    def dd_rccl_connect(self, id128):
        buf = (C.c_char * 128).from_buffer_copy(bytes(id128))
        self._chk(self.L.ghip_dd_rccl_connect(self.h, C.cast(buf, C.c_void_p)))

    def dd_info(self):
        out = np.zeros(16, np.int64)
        self._chk(self.L.ghip_dd_get_info(self.h, _ptr(out)))
        keys = ("rank", "nranks", "let_imported", "let_sent", "ghosts_imported", "ghosts_sent",
                "bytes_gravity", "bytes_density", "hsml_growth_e6", "grav_elements", "gas_elements",
                "numpart", "ngas", "migrated_out", "migrated_in", "bytes_migrate")
        info = dict(zip(keys, (int(v) for v in out)))
        guests = np.zeros(2, np.int64)
        self._chk(self.L.ghip_dd_guest_counts(self.h, _ptr(guests)))
        info["guests_held"], info["guests_hosted"] = int(guests[0]), int(guests[1])
        return info

    def dd_bytes_sent(self, op):
        """bytes this shard sent over links in its last operation `op` (DD_*)"""
        b = C.c_longlong(0)
        self._chk(self.L.ghip_dd_bytes_sent(self.h, int(op), C.byref(b)))
        return b.value

    # ---- multi-GPU shard exchange helpers (device pointers, e.g. torch tensors' data_ptr()) ----
    def shard_count(self, gas):
        per = C.c_int(0)
        mine = C.c_int(0)
        self._chk(self.L.ghip_shard_count(self.h, int(gas), C.byref(per), C.byref(mine)))
        return per.value, mine.value

    def shard_pack(self, group, dev_ptr):
        self._chk(self.L.ghip_shard_pack(self.h, int(group), C.c_void_p(dev_ptr)))

    def shard_unpack(self, group, dev_ptr, nranks):
        self._chk(self.L.ghip_shard_unpack(self.h, int(group), C.c_void_p(dev_ptr), int(nranks)))


# ---- multi-GPU module-level helpers ----
DD_MIGRATE, DD_GRAVITY, DD_DENSITY, DD_HYDRO = 1, 2, 3, 4
DD_SINK_DENSITY, DD_BH_EVALUATE, DD_BH_SWALLOW, DD_PM = 5, 6, 7, 8
DD_DUST_DENSITY, DD_DUST_DRAG = 9, 10
DD_POTENTIAL, DD_GLOBAL_QUANTITIES = 11, 12
DD_DECOMPOSE = 13
DD_PM_REGION, DD_PM_NONPERIODIC = 14, 15
WIND_OP = DD_DUST_DRAG   # GHIP_DD_WIND: the wind particles on shards share the dust drag's operation code ...
WIND_FORM, WIND_DENSITY_FORM, WIND_SPREAD_FORM = 16, 17, 18   # ... and are its forms: `walk` of dd_begin / dd_run
WINDS_RESIDENT_FORM = 32   # GHIP_DD_WIND from the shard's wind table (DdWindsArgs): ghip_winds_feedback as a collective
WINDS_SPAWN_FORM = 33      # ... ghip_wind_spawn as a collective (the spawn members of DdWindsArgs)
WIND_COUNTS = ("records_sent", "records_received", "imported_pairs", "exchanges", "bytes_sent", "iterations")
FOF_FORM = 1             # `walk` of dd_begin / dd_run for DD_GLOBAL_QUANTITIES with DdFofArgs: the FOF groups of all shards
SYNC_POINT_FORM = 1      # `walk` of dd_begin / dd_run for DD_DECOMPOSE with SyncParams: the sync point of all shards
DUST_GRAINS_FORM = 1     # `walk` of dd_begin / dd_run for DD_DUST_DENSITY / DD_DUST_DRAG with DdDustGrainsArgs


class DdSinkArgs(C.Structure):
    """ghip_dd_sink_args (include/ghip.h): the sink passes on a multi-GPU shard"""
    _fields_ = [("dens", C.POINTER(DensParams)), ("ngb_factor", C.c_double),
                ("bh", C.POINTER(BhParams)), ("nsink", C.c_int), ("sink_idx", C.c_void_p),
                ("sink_id", C.c_void_p), ("hsml", C.c_void_p), ("numngb", C.c_void_p),
                ("bh_density", C.c_void_p), ("bh_entropy", C.c_void_p), ("bh_gasvel", C.c_void_p),
                ("bh_mdot", C.c_void_p), ("bh_density_in", C.c_void_p),
                ("sink_bh_mass", C.c_void_p), ("acc_mass", C.c_void_p), ("acc_bhmass", C.c_void_p),
                ("acc_dustmass", C.c_void_p), ("acc_momentum", C.c_void_p), ("counts", C.c_void_p)]


def dd_sink_args(sinks, sink_ids=None, dens=None, ngb_factor=1.0, bh=None, hsml=None, mdot=None,
                 bh_density=None, sink_bh_mass=None):
    """(args, arrays): a filled DdSinkArgs and the dict of numpy arrays it points into -- inputs
    copied, outputs allocated; keep `arrays` alive until the operation has finished."""
    ns = len(sinks)
    f64 = lambda v: None if v is None else np.ascontiguousarray(v, np.float64).copy()
    a = dict(sink_idx=np.ascontiguousarray(sinks, np.int32),
             sink_id=None if sink_ids is None else np.ascontiguousarray(sink_ids, np.uint32),
             hsml=f64(hsml), numngb=np.zeros(ns), density=np.zeros(ns), entropy=np.zeros(ns),
             gasvel=np.zeros((ns, 3)), mdot=f64(mdot), bh_density_in=f64(bh_density),
             bh_mass=f64(sink_bh_mass), acc_mass=np.zeros(ns), acc_bhmass=np.zeros(ns),
             acc_dustmass=np.zeros(ns), acc_momentum=np.zeros((ns, 3)), counts=np.zeros(3, np.int64),
             _dens=dens, _bh=bh)
    A = DdSinkArgs()
    A.dens = C.pointer(dens) if dens is not None else None
    A.ngb_factor = float(ngb_factor)
    A.bh = C.pointer(bh) if bh is not None else None
    A.nsink = ns
    vp = lambda v: None if v is None else v.ctypes.data
    A.sink_idx, A.sink_id, A.hsml = vp(a["sink_idx"]), vp(a["sink_id"]), vp(a["hsml"])
    A.numngb, A.bh_density, A.bh_entropy = vp(a["numngb"]), vp(a["density"]), vp(a["entropy"])
    A.bh_gasvel, A.bh_mdot, A.bh_density_in = vp(a["gasvel"]), vp(a["mdot"]), vp(a["bh_density_in"])
    A.sink_bh_mass, A.acc_mass, A.acc_bhmass = vp(a["bh_mass"]), vp(a["acc_mass"]), vp(a["acc_bhmass"])
    A.acc_dustmass, A.acc_momentum, A.counts = vp(a["acc_dustmass"]), vp(a["acc_momentum"]), vp(a["counts"])
    return A, a


SINKS_RESIDENT_FORM = 1   # `walk` of dd_begin / dd_run for DD_SINK_DENSITY / DD_BH_SWALLOW with DdSinksArgs


class DdSinksArgs(C.Structure):
    """ghip_dd_sinks_args (include/ghip.h): the resident form of the sink operations on a multi-GPU shard"""
    _fields_ = [("dens", C.POINTER(DensParams)), ("ngb_factor", C.c_double), ("iterations", C.POINTER(C.c_int)),
                ("bh", C.POINTER(BhParams)), ("acc", C.POINTER(BhAccretionParams)),
                ("report", C.POINTER(BhAccretionReport))]


def dd_sinks_args(dens=None, ngb_factor=1.0, bh=None, acc=None):
    """(args, keep) for DD_SINK_DENSITY (dens, ngb_factor) or DD_BH_SWALLOW (bh, acc) begun with walk =
    SINKS_RESIDENT_FORM on one shard: a filled DdSinksArgs and the dict of what it points to -- keep it alive until
    the operation has finished; then keep["iterations"].value and dd_sinks_report(keep) hold the results."""
    keep = dict(iterations=C.c_int(0), report=BhAccretionReport(), _dens=dens, _bh=bh, _acc=acc)
    A = DdSinksArgs()
    A.dens = C.pointer(dens) if dens is not None else None
    A.ngb_factor = float(ngb_factor)
    A.iterations = C.pointer(keep["iterations"])
    A.bh = C.pointer(bh) if bh is not None else None
    A.acc = C.pointer(acc) if acc is not None else None
    A.report = C.pointer(keep["report"])
    return A, keep


def dd_sinks_report(keep):
    """what a finished DD_BH_SWALLOW (walk = SINKS_RESIDENT_FORM) left in `keep` of dd_sinks_args, as
    ForcePath.blackhole_accretion returns it: the sums over THIS shard's sinks, counts = the particles of this
    shard that were swallowed"""
    rep = keep["report"]
    return dict(bin_mass=np.array(rep.TimeBin_BH_mass), bin_dynmass=np.array(rep.TimeBin_BH_dynamicalmass),
                bin_mdot=np.array(rep.TimeBin_BH_Mdot), counts=np.array(rep.swallowed, np.int64),
                nactive=rep.nactive_sinks)


class DdDustArgs(C.Structure):
    """ghip_dd_dust_args (include/ghip.h): the dust passes on a multi-GPU shard"""
    _fields_ = [("p", C.POINTER(DustParams)), ("ndust", C.c_int), ("dust_idx", C.c_void_p),
                ("particle_density", C.c_void_p), ("dust_density", C.c_void_p), ("dust_entropy", C.c_void_p),
                ("dust_gasvel", C.c_void_p), ("dust_radius", C.c_void_p), ("particle_velocity", C.c_void_p),
                ("delta_momentum", C.c_void_p), ("delta_energy", C.c_void_p), ("vcoll", C.c_void_p),
                ("counts", C.c_void_p)]


def dd_dust_args(params, dust, particle_density=None, dust_density=None, dust_entropy=None, dust_gasvel=None,
                 dust_radius=None, particle_velocity=None, vcoll=None):
    """(args, arrays) for GHIP_DD_DUST_DENSITY (params, dust) or GHIP_DD_DUST_DRAG (all inputs): a filled
    DdDustArgs and the dict of numpy arrays it points into -- inputs copied, outputs allocated
    (particle_density, particle_velocity, delta_momentum, delta_energy, vcoll, counts [4]); keep `arrays`
    alive until the operation has finished."""
    g, a = dust_grains(dust, particle_density, dust_density, dust_entropy, dust_gasvel, dust_radius,
                       particle_velocity, vcoll, logr=False)
    A = DdDustArgs()
    A.p = C.pointer(params)
    for k, _ in DdDustArgs._fields_[1:]:
        setattr(A, k, getattr(g, k))
    a["_params"] = params
    return A, a


def dd_wind_args(params, wind, state=None, dt_jump=None, new_density=None, delta_momentum=None):
    """(args, arrays) for GHIP_DD_WIND on one shard: `wind` are its local indices in list order.  WIND_FORM:
    state = dict(stellar_age, birth_energy, old_momentum, new_density, drmin) as ForcePath.wind_feedback takes
    them; WIND_DENSITY_FORM: dt_jump; WIND_SPREAD_FORM: dt_jump, new_density, delta_momentum.  A filled DdWindArgs
    and the dict of numpy arrays it points into -- inputs copied, outputs allocated (the state arrays, new_density,
    drmin, result: WindResult, counts: int64[6], WIND_COUNTS); keep `arrays` alive until the operation has
    finished."""
    wind = np.ascontiguousarray(wind, np.int32)
    nw = len(wind)
    f64 = lambda v: np.zeros(nw) if v is None else np.ascontiguousarray(v, np.float64).reshape(nw).copy()
    a = dict(wind_idx=wind, dt_jump_in=f64(dt_jump), new_density=f64(new_density), drmin=np.zeros(nw),
             delta_momentum_in=f64(delta_momentum), counts=np.zeros(6, np.int64), result=WindResult(),
             _params=params)
    A = DdWindArgs()
    A.p = C.pointer(params)
    A.nwind = nw
    A.wind_idx = wind.ctypes.data
    if state is not None:
        st = dict(stellar_age=f64(state["stellar_age"]), birth_energy=f64(state["birth_energy"]),
                  old_momentum=f64(state["old_momentum"]), new_density=f64(state["new_density"]),
                  drmin=f64(state["drmin"]), dt1=np.zeros(nw), dt2=np.zeros(nw), dt_jump=np.zeros(nw),
                  delta_momentum=np.zeros(nw), deleted=np.zeros(nw, np.int32))
        S = WindState()
        for k, v in st.items():
            setattr(S, k, v.ctypes.data)
        a.update(state=st, _state=S)
        A.state = C.pointer(S)
    A.dt_jump = a["dt_jump_in"].ctypes.data
    A.new_density = a["new_density"].ctypes.data
    A.drmin = a["drmin"].ctypes.data
    A.delta_momentum = a["delta_momentum_in"].ctypes.data
    A.result = C.pointer(a["result"])
    A.counts = a["counts"].ctypes.data
    return A, a


def dd_winds_args(params=None, spawn=None, rnd_table=None):
    """(args, arrays) for GHIP_DD_WIND on one shard, a filled DdWindsArgs and what it points into.  walk =
    WINDS_RESIDENT_FORM: params (WindParams) -> result: WindResult, counts: int64[6] (WIND_COUNTS); the list and
    the state are the shard's wind table and active list; dd_wind_result(arrays) reads it when the operation has
    finished.  walk = WINDS_SPAWN_FORM: spawn (WindSpawnParams) and rnd_table, which must be given (a copy of the
    params points to a copy of it) -> report: WindSpawnReport, tot_spawned: c_longlong; dd_winds_spawn_report(arrays)."""
    a = dict(counts=np.zeros(6, np.int64), result=WindResult(), report=WindSpawnReport(),
             tot_spawned=C.c_longlong(0), _params=params)
    A = DdWindsArgs()
    if params is not None:
        A.p = C.pointer(params)
    A.result = C.pointer(a["result"])
    A.counts = a["counts"].ctypes.data
    if spawn is not None:
        sp = WindSpawnParams()
        C.memmove(C.byref(sp), C.byref(spawn), C.sizeof(sp))
        t = None if rnd_table is None else np.ascontiguousarray(rnd_table, np.float64).copy()
        sp.rnd_table = None if t is None else t.ctypes.data
        sp.nrnd = 0 if t is None else len(t)
        a.update(_spawn=sp, _rnd=t)
        A.spawn = C.pointer(sp)
        A.report = C.pointer(a["report"])
        A.tot_spawned = C.pointer(a["tot_spawned"])
    return A, a


def dd_winds_spawn_report(arrays):
    """what a finished GHIP_DD_WIND (walk = WINDS_SPAWN_FORM) left in `arrays` of dd_winds_args, as ForcePath.wind_spawn
    returns it, and tot_spawned, the sum over all shards"""
    rep = arrays["report"]
    return dict(spawned=rep.spawned, nsinks_emitting=rep.nsinks_emitting, first_index=rep.first_index,
                new_wind_exact_sum=rep.new_wind_exact_sum, gsl_draws=rep.gsl_draws,
                tot_spawned=int(arrays["tot_spawned"].value))


def dd_wind_result(arrays):
    """what a finished GHIP_DD_WIND (walk = WIND_FORM) left in `arrays` of dd_wind_args, as ForcePath.wind_feedback returns
    it: the state arrays, iterations (global), and this shard's bits, ndeleted, deleted_momentum; counts"""
    res = arrays["result"]
    out = dict(arrays["state"]) if "state" in arrays else {}
    out.update(iterations=res.iterations, bits=res.bits, ndeleted=res.ndeleted,
               deleted_momentum=res.deleted_momentum, counts=arrays["counts"].copy())
    return out


class DdDustGrainsArgs(C.Structure):
    """ghip_dd_dust_grains_args (include/ghip.h): the dust passes on a shard with the arrays of DustGrains"""
    _fields_ = [("p", C.POINTER(DustParams)), ("g", DustGrains)]


def dd_dust_grains_args(params, dust, **arrays):
    """(args, arrays) for GHIP_DD_DUST_DENSITY / GHIP_DD_DUST_DRAG begun with walk = DUST_GRAINS_FORM:
    dust_grains() with the params; keep `arrays` alive until the operation has finished."""
    g, a = dust_grains(dust, **arrays)
    a["_params"] = params
    A = DdDustGrainsArgs()
    A.p = C.pointer(params)
    A.g = g
    return A, a


class DdGlobalArgs(C.Structure):
    """ghip_dd_global_args (include/ghip.h): compute_global_quantities_of_system() on a multi-GPU shard"""
    _fields_ = [("p", C.POINTER(GlobalParams)), ("out", C.POINTER(GlobalSums))]


def dd_global_args(params, n, grav_kick_table=None, hydro_kick_table=None, old_photon_momentum=None,
                   potential=None):
    """(args, keep) for GHIP_DD_GLOBAL_QUANTITIES on a shard of n particles: a filled DdGlobalArgs and the
    dict it points into -- a copy of params with the host arrays set (as ForcePath.global_quantities takes
    them; potential None = the shard's last GHIP_DD_POTENTIAL) and the GlobalSums `out` the operation fills.
    Keep `keep` alive until the operation has finished."""
    p = GlobalParams.from_buffer_copy(params)
    keep = dict(params=p, out=GlobalSums())
    for name, arr in (("GravKickTable", grav_kick_table), ("HydroKickTable", hydro_kick_table),
                      ("OldPhotonMomentum", old_photon_momentum), ("Potential", potential)):
        a = None if arr is None else np.ascontiguousarray(arr, dtype=np.float64)
        if a is not None and name in ("OldPhotonMomentum", "Potential") and len(a) != n:
            raise ValueError("%s: expected %d values, got %d" % (name, n, len(a)))
        keep[name] = a
        setattr(p, name, None if a is None else a.ctypes.data)
    A = DdGlobalArgs()
    A.p = C.pointer(p)
    A.out = C.pointer(keep["out"])
    return A, keep


class DdFofArgs(C.Structure):
    """ghip_dd_fof_args (include/ghip.h): the friends-of-friends groups of all shards, DD_GLOBAL_QUANTITIES begun
    with walk = FOF_FORM"""
    _fields_ = [("p", C.POINTER(FofParams)), ("out", C.POINTER(FofResult)), ("counts", C.POINTER(C.c_longlong))]


FOF_COUNTS = ("members", "primaries_sent", "primaries_received", "label_rounds", "queries_sent", "partials_sent",
              "bytes_sent", "groups_owned")


def dd_fof_args(link_length=0.0, primary_types=2, secondary_types=0, group_min_len=32, boxsize=0.0,
                periodic=False, max_iter=150, linklength=0.2, rhodm=0.0):
    """(args, keep) for DD_GLOBAL_QUANTITIES with walk = FOF_FORM: a filled DdFofArgs and the dict it points into
    (params: FofParams as ForcePath.fof takes them, the same on every shard; out: FofResult; counts: int64[8],
    FOF_COUNTS).  Keep `keep` alive until the operation has finished; then ForcePath.fof_adopt(keep)."""
    p = FofParams(float(link_length), float(linklength), float(rhodm), int(primary_types), int(secondary_types),
                  int(group_min_len), float(boxsize), int(bool(periodic)), int(max_iter))
    keep = dict(params=p, out=FofResult(), counts=np.zeros(8, np.int64))
    A = DdFofArgs()
    A.p = C.pointer(p)
    A.out = C.pointer(keep["out"])
    A.counts = C.cast(keep["counts"].ctypes.data, C.POINTER(C.c_longlong))
    return A, keep


def dd_rccl_unique_id():
    """128 bytes of ncclGetUniqueId (rank 0 calls it, the host broadcasts them)."""
    buf = (C.c_char * 128)()
    rc = lib().ghip_dd_rccl_unique_id(C.cast(buf, C.c_void_p))
    if rc != 0:
        raise GhipError(rc, "ghip_dd_rccl_unique_id failed (no librccl next to the HIP runtime?)")
    return bytes(buf)


def dd_rccl_library():
    return lib().ghip_dd_rccl_library().decode()


def dd_exchange_local(paths):
    """Run the pending exchange of several shards living in this process (ghip_dd_exchange_local)."""
    arr = (C.c_void_p * len(paths))(*[p.h for p in paths])
    rc = lib().ghip_dd_exchange_local(C.cast(arr, C.c_void_p), len(paths))
    if rc != 0:
        raise GhipError(rc, lib().ghip_last_error(paths[0].h).decode())


def dd_run_local(paths, op, params, walk=0):
    """One operation on all shards of this process: compute phases shard after shard, exchanges in
    between (what ghip_dd_run does over RCCL with one shard per process)."""
    for p, prm in zip(paths, params):
        p.dd_begin(op, prm, walk)
    while True:
        rcs = [p.dd_step() for p in paths]
        if any(r != rcs[0] for r in rcs):
            raise RuntimeError("shards out of step: %r" % (rcs,))
        if rcs[0] == 0:
            if op == DD_MIGRATE:
                for p in paths:
                    p.counts()
            return
        dd_exchange_local(paths)


def dd_find_split(ncpu, work):
    """domain_findSplit_work_balanced (domain.c:1075-1113) through the library's host function."""
    w = np.ascontiguousarray(work, np.float64)
    start = np.zeros(ncpu, np.int32)
    end = np.zeros(ncpu, np.int32)
    rc = lib().ghip_dd_find_split(int(ncpu), len(w), _ptr(w), _ptr(start), _ptr(end))
    if rc != 0:
        raise GhipError(rc, "ghip_dd_find_split: bad arguments")
    return start, end
