// ghip_walkrec.h -- the 64-byte element records of the gravity walks (layout: ghip_walk.h), shared
// with the potential walk (ghip_potential.hip), which must not include the force walk's kernels.
#pragma once

struct __attribute__((aligned(64))) WalkHot
{
  double x, y, z, m;
  double mlen2, len2;
  int skip, pidx;
  double aux;
};
struct __attribute__((aligned(64))) WalkCold
{
  double cx, cy, cz, len;
  double len06;
  double spare[3];
};
