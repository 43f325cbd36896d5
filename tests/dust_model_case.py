"""The test case of the dust model tests (CPU and GPU): DustCase of test_gpu_dust.py with grain groups that
reach every branch of dust.c:449-609 -- hot gas around some grains (rock and ice vapour), radii next to
both clamps, radii below the lower clamp on grains with dt == 0.  The reference results are computed once
per (periodic) and shared."""
import functools

import numpy as np

import dust_model_ref as MR
from test_gpu_dust import DustCase


class DustModelCase(DustCase):
    def __init__(self, periodic, ndust=600, ng=10, seed=7):
        super().__init__(periodic, ndust=ndust, ng=ng, seed=seed)
        nd = len(self.dust)
        rng = np.random.default_rng(seed + 100)
        a = np.arange(nd)
        sub = (a // 6) % 10                      # rows of six grains (one per stopping-time group)
        self.sub = sub
        # cold gas (T ~ 130 K: no vapour, rock or ice) but around the rows sub = 1 (T ~ 1900 K: rock starts to
        # vaporise) and sub = 2, 3 (T ~ 2500 K: rock shrinks by centimetres per step); ice is hot in all three
        self.ent = self.ent * np.choose(np.minimum(sub, 4), [0.4, 6.0, 8.0, 8.0, 0.4])
        self.radius = self.radius.copy()
        self.radius[sub == 3] = 0.1000001        # next to the lower clamp, in hot gas
        self.radius[sub == 4] = 99999.999        # next to the upper clamp; a slow grain (its DustVcoll follows
        self.grav[self.dust[sub == 4]] *= 1.e-6  # |GravAccel| ts, and ts its radius), so that it grows
        self.radius[(sub == 3) & (a % 6 == 5)] = 0.05   # dt == 0 and below the clamp: clamped without moving
        self.ids = self.sp.ids[self.dust]
        self.logr0 = 1.0 + rng.random(nd)        # the caller's LogDustRadius_by_dt
        self._ref = {}

    def dt(self, sel=None):
        i = self.dust if sel is None else self.dust[sel]
        return np.where(self.timebin[i] > 0, (1 << self.timebin[i]).astype(np.float64), 0.0) * self.par["dt_fac"]

    def ref_density9(self, m, dust=None):
        """(d7, raw d9 or None) by brute force"""
        pr = self.pr
        dust = self.dust if dust is None else dust
        return MR.dust_density(pr.ic["pos"], pr.ic["vel"], self.mass, pr.ic["type"], self.hsml, dust, pr.box,
                               pr.periodic, m)

    def base(self):
        """d7 and the raw d9 sums of the whole list, once"""
        if "base" not in self._ref:
            self._ref["base"] = self.ref_density9(MR.model("real_pebble_collisions"))
        return self._ref["base"]

    def vfrag(self):
        """All.FragmentationVelocity of the case: the median DustVcoll the flags-off update leaves"""
        if "vfrag" not in self._ref:
            d7, _ = self.base()
            self._ref["vfrag"] = float(np.median(self.ref_grains(np.arange(len(self.dust)), d7)["vcoll"]))
        return self._ref["vfrag"]

    def model(self, *on, **over):
        over.setdefault("FragmentationVelocity", self.vfrag())
        # (with the latent heat of a grain born at 1 cm the centimetres these grains lose in a step would take
        # ten thousand times the thermal energy of the gas around them: the entropy update of the scatter would
        # cross zero, and a test of its rounding errors would test cancellation)
        over.setdefault("InitialDustRadius", 1.e5)
        return MR.model(*on, **over)

    def d9_in(self, m):
        """what the drag pass gets as d9: the density pass's raw sums with real_pebble_collisions, the
        caller's invention without"""
        return self.base()[1] if m["real_pebble_collisions"] else self.d9

    def ref_model(self, m, sel=None, d7=None):
        """the reference's grain update of the list positions `sel` under the model m"""
        sel = np.arange(len(self.dust)) if sel is None else sel
        d7 = self.base()[0][sel] if d7 is None else d7
        i = self.dust[sel]
        return MR.grain_update(self.par, m, self.pr.ic["vel"][i], self.mass[i], self.grav[i], self.dt(sel),
                               self.rho[sel], self.ent[sel], self.gasvel[sel], self.radius[sel], d7,
                               self.d9_in(m)[sel], self.vcoll[sel], ids=self.ids[sel], logr=self.logr0[sel])

    def gmodel(self, m):
        from common import bindings
        g = bindings().DustModel()
        for k, v in m.items():
            setattr(g, k, v)
        return g


@functools.lru_cache(maxsize=None)
def case(periodic):
    return DustModelCase(periodic)


ALL_SIX = MR.SWITCHES
