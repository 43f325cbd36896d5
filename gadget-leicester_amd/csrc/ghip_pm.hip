// ghip_pm.hip -- "next" row N3: the periodic particle-mesh long-range force of the
// TreePM configurations on the device.
//
// Replaces pmforce_periodic() (pm_periodic.c:199-800): CIC mass assignment onto a PMGRID^3 mesh
// (:226-330), forward FFT, multiplication with the Green's function -exp(-k^2 asmth^2)/k^2 and the
// CIC deconvolution sinc^-4 (:430-486), inverse FFT, 4-point finite differences of the potential
// in each dimension (:489-560) and CIC interpolation of the mesh force to the particles (:640-690)
// into P[].GravPM.  The reference distributes the mesh in slabs over MPI ranks and sorts the
// particles' mesh points to exchange them; on one GPU the whole 128^3 (16 MB) mesh is resident
// and none of that exists.  FFTs: hipFFT (rocFFT), unnormalised in both directions like FFTW --
// the reference's prefactor G/(pi L) * PMGRID/(2L) already assumes that.
//
// Deliberate difference: pm_periodic.c:263-264 clamps `slab_y` where `slab_z` is meant (a typo that
// only matters for a coordinate exactly equal to BoxSize); the clamp is applied to slab_z here.
// The mass assignment uses fp64 atomic adds: the summation order on a mesh point is not fixed,
// so the long-range force is reproducible to rounding (1e-16 relative per mesh point), not bitwise.
//
// Second half of the file: the non-periodic mesh of TreePM with open boundaries (pm_nonperiodic.c), see there.
#include <hipfft/hipfft.h>

#include <cfloat>

#include "ghip_internal.h"

#define FFTCHK(call)                                                                          \
  do                                                                                          \
    {                                                                                         \
      hipfftResult r_ = (call);                                                               \
      if(r_ != HIPFFT_SUCCESS)                                                                \
        return ghip_fail(ctx, GHIP_EHIP, "%s failed with hipfftResult %d", #call, (int) r_);  \
    }                                                                                         \
  while(0)

// One cloud-in-cell cell: the mesh cell below a particle and the particle's offset inside it, in cells.  Both
// meshes fill it (d_pm_cell, d_pmnp_cell); the weights come from d_cic_weight alone.
struct CicCell
{
  int s[3];
  double d[3];
};

// a times the weight of corner (xx, yy, zz), as ((a wx) wy) wz.  a = 1.0 gives the bare weight wx wy wz, exactly.
__device__ __forceinline__ double d_cic_weight(double a, const CicCell &c, int xx, int yy, int zz)
{
  return a * (xx ? c.d[0] : 1.0 - c.d[0]) * (yy ? c.d[1] : 1.0 - c.d[1]) * (zz ? c.d[2] : 1.0 - c.d[2]);
}

// (f_x f_y f_z)^-4 with f = sin(pi k / N) / (pi k / N): the CIC deconvolution, for assignment and read-out
// (pm_periodic.c:455-476, pm_nonperiodic.c:520-545); kx, ky, kz are whole wave numbers of a mesh of side N
__device__ __forceinline__ double d_cic_deconv(double kx, double ky, double kz, int N)
{
  double fx = 1, fy = 1, fz = 1;
  if(kx != 0)
    {
      fx = (M_PI * kx) / N;
      fx = sin(fx) / fx;
    }
  if(ky != 0)
    {
      fy = (M_PI * ky) / N;
      fy = sin(fy) / fy;
    }
  if(kz != 0)
    {
      fz = (M_PI * kz) / N;
      fz = sin(fz) / fz;
    }
  const double ff = 1 / (fx * fy * fz);
  return ff * ff * ff * ff;
}

// the periodic cell rule of pm_periodic.c:318-325: scale, truncate, the offset BEFORE the clamp, clamp the
// upper side (a coordinate equal to BoxSize lands in the last cell with offset 1)
__device__ __forceinline__ CicCell d_pm_cell(int N, double to_slab_fac, int n, int i, const double *__restrict__ pos)
{
  CicCell c;
  for(int j = 0; j < 3; j++)
    {
      const double p = to_slab_fac * pos[(size_t) j * n + i];
      c.s[j] = (int) p;
      c.d[j] = p - c.s[j];
      if(c.s[j] >= N)
        c.s[j] = N - 1;
    }
  return c;
}

// mesh point of corner (xx, yy, zz) of a periodic cell: the +1 corner of the last cell wraps
__device__ __forceinline__ size_t d_pm_corner(int N, const CicCell &c, int xx, int yy, int zz)
{
  int gx = c.s[0] + xx, gy = c.s[1] + yy, gz = c.s[2] + zz;
  if(gx >= N)
    gx -= N;
  if(gy >= N)
    gy -= N;
  if(gz >= N)
    gz -= N;
  return ((size_t) gx * N + gy) * N + gz;
}

// pm_periodic.c:226-330: cloud-in-cell assignment of the particle masses
__global__ void k_pm_deposit(int n, int N, double to_slab_fac, const double *__restrict__ pos,
                             const double *__restrict__ mass, double *__restrict__ rho)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  const CicCell c = d_pm_cell(N, to_slab_fac, n, i, pos);
  const double m = mass[i];
  for(int xx = 0; xx < 2; xx++)
    for(int yy = 0; yy < 2; yy++)
      for(int zz = 0; zz < 2; zz++)
        atomicAdd(&rho[d_pm_corner(N, c, xx, yy, zz)], d_cic_weight(m, c, xx, yy, zz));
}

// pm_periodic.c:430-486 on hipFFT's layout [x][y][z = 0..N/2]
__global__ void k_pm_green(int N, double asmth2, double2 *__restrict__ fk)
{
  const int nz = N / 2 + 1;
  size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
  if(idx >= (size_t) N * N * nz)
    return;
  int z = (int) (idx % nz), y = (int) ((idx / nz) % N), x = (int) (idx / ((size_t) nz * N));
  double kx = x > N / 2 ? x - N : x, ky = y > N / 2 ? y - N : y, kz = z > N / 2 ? z - N : z;
  double k2 = kx * kx + ky * ky + kz * kz;
  double2 v = fk[idx];
  if(k2 > 0)
    {
      double smth = -exp(-k2 * asmth2) / k2;
      smth *= d_cic_deconv(kx, ky, kz, N);
      v.x *= smth;
      v.y *= smth;
    }
  else
    v.x = v.y = 0;   // :485
  fk[idx] = v;
}

// pm_periodic.c:489-560: force_dim = fac * (4/3 (phi[-1] - phi[+1]) - 1/6 (phi[-2] - phi[+2]))
// along dimension dim; the three components as planes of `force`
__global__ void k_pm_gradient(int N, double fac, const double *__restrict__ phi,
                              double *__restrict__ force)
{
  size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n3 = (size_t) N * N * N;
  if(idx >= n3)
    return;
  int z = (int) (idx % N), y = (int) ((idx / N) % N), x = (int) (idx / ((size_t) N * N));
  for(int dim = 0; dim < 3; dim++)
    {
      int c = dim == 0 ? x : dim == 1 ? y : z;
      int l = c - 1, r = c + 1, ll = c - 2, rr = c + 2;
      if(r >= N)
        r -= N;
      if(rr >= N)
        rr -= N;
      if(l < 0)
        l += N;
      if(ll < 0)
        ll += N;
      size_t stride = dim == 0 ? (size_t) N * N : dim == 1 ? (size_t) N : 1;
      size_t base = idx - (size_t) c * stride;
      force[(size_t) dim * n3 + idx] =
        fac * ((4.0 / 3) * (phi[base + l * stride] - phi[base + r * stride]) -
               (1.0 / 6) * (phi[base + ll * stride] - phi[base + rr * stride]));
    }
}

// pm_periodic.c:640-690: CIC interpolation of the mesh force, GravPM[dim] += acc_dim
__global__ void k_pm_interpolate(int n, int N, double to_slab_fac, const double *__restrict__ pos,
                                 const double *__restrict__ force, double *__restrict__ gravpm)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  const size_t n3 = (size_t) N * N * N;
  const CicCell c = d_pm_cell(N, to_slab_fac, n, i, pos);
  double acc[3] = {0, 0, 0};
  for(int xx = 0; xx < 2; xx++)
    for(int yy = 0; yy < 2; yy++)
      for(int zz = 0; zz < 2; zz++)
        {
          const double w = d_cic_weight(1.0, c, xx, yy, zz);
          const size_t g = d_pm_corner(N, c, xx, yy, zz);
          for(int dim = 0; dim < 3; dim++)
            acc[dim] += force[(size_t) dim * n3 + g] * w;   // same corner order as the reference
        }
  for(int dim = 0; dim < 3; dim++)
    gravpm[(size_t) dim * n + i] += acc[dim];
}

// pmpotential_periodic (pm_periodic.c:808-1195): the same deposit and Green's function as the force
// (:1040-1097), the inverse transform is the potential mesh, read out with the CIC weights of :1172-1189
// and multiplied by fac = G / (pi BoxSize) (:837).  (The fork computes fac and never applies it; without
// it the mesh potential is not in the units of the tree potential, so it is applied here.)
__global__ void k_pm_pot_readout(int n, int N, double to_slab_fac, double fac,
                                 const double *__restrict__ pos, const double *__restrict__ phi,
                                 double *__restrict__ pot)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  const CicCell c = d_pm_cell(N, to_slab_fac, n, i, pos);
  double v = 0;
  for(int xx = 0; xx < 2; xx++)
    for(int yy = 0; yy < 2; yy++)
      for(int zz = 0; zz < 2; zz++)
        v += phi[d_pm_corner(N, c, xx, yy, zz)] * d_cic_weight(1.0, c, xx, yy, zz);
  pot[i] += fac * v;
}

// rank-ordered sum of the all-gathered meshes (identical on every shard, whatever the transport); rank r's
// mesh begins at all[r * stride]
__global__ void k_pm_sum_meshes(size_t n3, size_t stride, int nranks, const double *__restrict__ all,
                                double *__restrict__ rho)
{
  size_t g = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
  if(g >= n3)
    return;
  double s = 0;
  for(int r = 0; r < nranks; r++)
    s += all[(size_t) r * stride + g];
  rho[g] = s;
}

static int pm_check(ghip_ctx *ctx, const ghip_pm_params *p)
{
  const int N = p->pmgrid;
  if(N < 4 || N > 2048 || (N & 1) || !(p->BoxSize > 0) || !(p->Asmth > 0))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_pm_periodic: need an even PMGRID >= 4, BoxSize > 0, Asmth > 0");
  return GHIP_OK;
}

// Plans for a real transform of side G on the context's stream, the mesh and its transform: the one place where
// plans are made, for both meshes.  Another side renews the object (plans and both buffers) and nothing else.
static int pm_fft_prepare(ghip_ctx *ctx, PmFft &t, int G)
{
  if(t.n != G)
    {
      // (the object owns each plan from the moment it exists: a failure below leaves nothing behind)
      ghip_renew(t);
      hipfftHandle f, b;
      FFTCHK(hipfftPlan3d(&f, G, G, G, HIPFFT_D2Z));
      t.fwd = (void *) f;
      FFTCHK(hipfftPlan3d(&b, G, G, G, HIPFFT_Z2D));
      t.inv = (void *) b;
      FFTCHK(hipfftSetStream(f, ctx->stream));
      FFTCHK(hipfftSetStream(b, ctx->stream));
      t.n = G;
    }
  GCHK(ghip_ensure(ctx, t.rho, (size_t) G * G * G * sizeof(double)));
  GCHK(ghip_ensure(ctx, t.k, (size_t) G * G * (G / 2 + 1) * sizeof(double2)));
  return GHIP_OK;
}

PmFft::~PmFft()
{
  if(fwd)
    (void) hipfftDestroy((hipfftHandle) fwd);
  if(inv)
    (void) hipfftDestroy((hipfftHandle) inv);
}

// plans and mesh buffers for PMGRID = N
static int pm_prepare(ghip_ctx *ctx, int N)
{
  GCHK(pm_fft_prepare(ctx, ctx->pm.fft, N));
  return ghip_ensure(ctx, ctx->pm.force, 3 * (size_t) N * N * N * sizeof(double));
}

static double pm_to_slab_fac(const ghip_pm_params *p) { return p->pmgrid / p->BoxSize; }   // pm_periodic.c:102

// mass of this context's particles onto the (zeroed) mesh; zero_gravpm: GRAVPM zeroed as long_range_force() does
static int pm_deposit(ghip_ctx *ctx, const ghip_pm_params *p, bool zero_gravpm)
{
  hipStream_t st = ctx->stream;
  const int N = p->pmgrid, n = ctx->n;
  double *rho = P<double>(ctx->pm.fft.rho);
  HIPCHK(hipMemsetAsync(rho, 0, (size_t) N * N * N * sizeof(double), st));
  if(n > 0)
    {
      if(zero_gravpm)
        HIPCHK(hipMemsetAsync(ctx->f[GHIP_F_GRAVPM].p, 0, (size_t) n * 3 * sizeof(double), st));
      k_pm_deposit<<<cdiv(n, 256), 256, 0, st>>>(n, N, pm_to_slab_fac(p), P<double>(ctx->f[GHIP_F_POS]),
                                                 P<double>(ctx->f[GHIP_F_MASS]), rho);
      HIPCHK(hipGetLastError());
    }
  return GHIP_OK;
}

// (all != nullptr: the mesh is the sum of the nranks all-gathered ones, in rank order) mesh density -> the
// potential mesh, in place
static int pm_potential_mesh(ghip_ctx *ctx, const ghip_pm_params *p, int nranks, const double *all)
{
  hipStream_t st = ctx->stream;
  const int N = p->pmgrid;
  const size_t n3 = (size_t) N * N * N, nk = (size_t) N * N * (N / 2 + 1);
  PmFft &t = ctx->pm.fft;
  double *rho = P<double>(t.rho);
  double2 *fk = P<double2>(t.k);
  if(all)
    {
      k_pm_sum_meshes<<<cdiv((long long) n3, 256), 256, 0, st>>>(n3, n3, nranks, all, rho);
      HIPCHK(hipGetLastError());
    }
  double asmth2 = (2 * M_PI) * p->Asmth / p->BoxSize;          // :221-222, :834-835
  asmth2 *= asmth2;
  FFTCHK(hipfftExecD2Z((hipfftHandle) t.fwd, rho, reinterpret_cast<hipfftDoubleComplex *>(fk)));
  k_pm_green<<<cdiv((long long) nk, 256), 256, 0, st>>>(N, asmth2, fk);
  HIPCHK(hipGetLastError());
  FFTCHK(hipfftExecZ2D((hipfftHandle) t.inv, reinterpret_cast<hipfftDoubleComplex *>(fk), rho));
  return GHIP_OK;
}

// the force: potential mesh -> force field -> GRAVPM of this context's particles
static int pm_force(ghip_ctx *ctx, const ghip_pm_params *p, int nranks, const double *all)
{
  hipStream_t st = ctx->stream;
  const int N = p->pmgrid, n = ctx->n;
  const size_t n3 = (size_t) N * N * N;
  double *force = P<double>(ctx->pm.force);
  GCHK(pm_potential_mesh(ctx, p, nranks, all));
  double fac = p->G / (M_PI * p->BoxSize);                     // :224-225
  fac *= 1 / (2 * p->BoxSize / N);
  k_pm_gradient<<<cdiv((long long) n3, 256), 256, 0, st>>>(N, fac, P<double>(ctx->pm.fft.rho), force);
  if(n > 0)
    k_pm_interpolate<<<cdiv(n, 256), 256, 0, st>>>(n, N, pm_to_slab_fac(p), P<double>(ctx->f[GHIP_F_POS]),
                                                   force, P<double>(ctx->f[GHIP_F_GRAVPM]));
  HIPCHK(hipGetLastError());
  return GHIP_OK;
}

// the potential: potential mesh -> pot[i] += its value at particle i
static int pm_potential(ghip_ctx *ctx, const ghip_pm_params *p, int nranks, const double *all, double *pot)
{
  const int N = p->pmgrid, n = ctx->n;
  GCHK(pm_potential_mesh(ctx, p, nranks, all));
  const double fac = p->G / (M_PI * p->BoxSize);               // :837 (pm.G = All.G)
  if(n > 0)
    k_pm_pot_readout<<<cdiv(n, 256), 256, 0, ctx->stream>>>(n, N, pm_to_slab_fac(p), fac,
                                                            P<double>(ctx->f[GHIP_F_POS]),
                                                            P<double>(ctx->pm.fft.rho), pot);
  HIPCHK(hipGetLastError());
  return GHIP_OK;
}

extern "C" int ghip_pm_periodic(ghip_ctx *ctx, const ghip_pm_params *p)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !p)
    return GHIP_EINVAL;
  GCHK(pm_check(ctx, p));
  if(ctx->dd.on)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_pm_periodic: on a multi-GPU shard use GHIP_DD_PM");
  if(ctx->n == 0)
    return GHIP_OK;
  hipStream_t st = ctx->stream;
  GCHK(pm_prepare(ctx, p->pmgrid));
  HIPCHK(hipEventRecord(ctx->evp[14], st));
  GCHK(pm_deposit(ctx, p, true));
  GCHK(pm_force(ctx, p, 1, nullptr));
  HIPCHK(hipEventRecord(ctx->evp[15], st));
  return GHIP_OK;
}

// GHIP_DD_PM (ghip_dd_begin / ghip_dd_step): phase 0 deposits and posts the all-gather of the meshes,
// phase 1 adds them and solves
int ghip_dd_pm_begin(ghip_ctx *ctx, int, const void *params, int)
{
  GHIP_JOIN(ctx);
  ctx->dd.pm = *reinterpret_cast<const ghip_pm_params *>(params);
  return pm_check(ctx, &ctx->dd.pm);
}

int ghip_dd_pm_step(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  const ghip_pm_params *p = &D.pm;
  hipStream_t st = ctx->stream;
  const size_t n3 = (size_t) p->pmgrid * p->pmgrid * p->pmgrid;
  enum { DEPOSIT, SOLVE };
  if(D.phase == DEPOSIT)
    {
      GCHK(pm_prepare(ctx, p->pmgrid));
      HIPCHK(hipEventRecord(ctx->evp[14], st));
      GCHK(pm_deposit(ctx, p, true));
      ghip_dd_set_allgather(D, ctx->pm.fft.rho.p, n3 * sizeof(double), &D.pm_all);
      D.phase = SOLVE;
      return 1;
    }
  if(D.phase == SOLVE)
    {
      GCHK(pm_force(ctx, p, D.nranks, P<double>(D.pm_all)));
      HIPCHK(hipEventRecord(ctx->evp[15], st));
      return 0;
    }
  return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: the mesh force has no phase %d", D.phase);
}

// =============================================================================================
// The non-periodic mesh: PMGRID without PERIODIC, the TreePM scheme for open boundaries (pm_nonperiodic.c,
// mesh 0 only: no PLACEHIGHRESREGION, SCALARFIELD, ENLARGEREGION; GRIDBOOST 2, GRID = 2 PMGRID).
//
//   region   pm_init_regionsize (:91-212): extremes by k_decomp_extent (ghip_decomp.hip), :123-159 on the host
//   table    pm_setup_nonperiodic_kernel (:371-438, 500-558): -erf(u)/r on GRID^3, D2Z, CIC deconvolution
//   force    pmforce_nonperiodic(0) (:576-1175): range check, CIC deposit, D2Z, product with the table, Z2D,
//            4-point gradient, CIC read-out; then the tail of long_range_force (longrange.c:117-138)
//   potential  pmpotential_nonperiodic(0) (:1354-1750): the same up to Z2D, CIC read-out of the potential
//
// Particles of the allowed region land in cells [2, GRID/2 - 2): the mass occupies the lower octant only.  It
// is deposited into a compact PMGRID^3 array -- the block a shard sends, 1/8 of the padded mesh -- and
// scattered into the padded GRID^3 mesh, whose other seven octants are zero.  The force components are kept for
// the lower octant only (3 PMGRID^3 doubles); cells outside [2, GRID/2 - 2), which the reference leaves
// unwritten (:1005-1008), are zero.
//
// Every mesh index is formed only after its coordinate was found inside [0, PMGRID - 1) IN DOUBLE; a
// particle that fails this after it passed the range check (an inconsistent region) is skipped and raises
// GHIP_ERRW_PM.  A coordinate that is not a number fails the range check (the reference's comparisons let it
// pass, :622).
//
// The mass assignment uses fp64 atomic adds, as the periodic mesh does: the summation order on a mesh point is
// not fixed, so the result is reproducible to rounding, not bitwise.  Equal-cell runs are merged inside the
// wavefront before the atomics (k_pmnp_deposit), as k_decomp_hist does.  Kept because it does not lose to the
// plain form (one atomic per particle and corner), measured on an MI355X with 2 x 64^3 clustered particles,
// ms_pm of the whole call, least of 10: PMGRID 32 0.19 ms against 0.33 ms in curve order and 0.12 against 0.24
// in file order; PMGRID 128 0.752 against 0.757 and 0.709 against 0.709, where the transforms dominate.
// =============================================================================================
#define PMNP_ASMTH 1.25   // allvars.h:122
#define PMNP_RCUT 4.5     // allvars.h:128
#define PMNP_MIN_GRID 8
#define PMNP_MAX_GRID 512
// status word behind the octant of a shard's block
#define PMNP_ST_OK 0.0
#define PMNP_ST_RANGE 1.0   // a particle outside the allowed region
#define PMNP_ST_LOCAL 2.0   // this shard's own pass failed

struct PmnpGeo
{
  double c[3];   // Corner
  double fac;    // to_slab_fac = GRID / TotalMeshSize (:609)
  int M;         // PMGRID: the octant
  int G;         // GRID: the padded mesh
};

static PmnpGeo pmnp_geo(const ghip_pm_region &r)
{
  PmnpGeo g;
  for(int j = 0; j < 3; j++)
    g.c[j] = r.Corner[j];
  g.M = r.pmgrid;
  g.G = 2 * r.pmgrid;
  g.fac = g.G / r.TotalMeshSize;
  return g;
}

// :614-647 -- one pass, no host read of positions
__global__ void k_pmnp_range(int n, const double *__restrict__ pos, double lo0, double lo1, double lo2, double hi0,
                             double hi1, double hi2, int *__restrict__ err)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  const double x = pos[i], y = pos[(size_t) n + i], z = pos[2 * (size_t) n + i];
  if(!(x >= lo0 && x <= hi0 && y >= lo1 && y <= hi1 && z >= lo2 && z <= hi2))
    atomicOr(err, 1);
}

// the cell of particle i in the octant (:766-772); false: outside the octant, no index formed
__device__ __forceinline__ bool d_pmnp_cell(const PmnpGeo &g, int n, int i, const double *__restrict__ pos, CicCell &c)
{
  bool ok = true;
  for(int j = 0; j < 3; j++)
    {
      const double p = g.fac * (pos[(size_t) j * n + i] - g.c[j]);
      if(p >= 0.0 && p < (double) (g.M - 1))
        {
          c.s[j] = (int) p;
          c.d[j] = p - c.s[j];
        }
      else
        {
          c.s[j] = 0;
          c.d[j] = 0;
          ok = false;
        }
    }
  return ok;
}

// mesh point of corner (xx, yy, zz) of an open cell in an array of side `side` (the octant M, the padded mesh G):
// no wrap, d_pmnp_cell keeps the +1 corner inside
__device__ __forceinline__ size_t d_pmnp_corner(int side, const CicCell &c, int xx, int yy, int zz)
{
  return ((size_t) (c.s[0] + xx) * side + (c.s[1] + yy)) * side + (c.s[2] + zz);
}

// :757-790 into the compact octant oct[M][M][M].  Lanes whose particle has the same base cell as their
// neighbour's form runs (particles in curve order); the eight weights of a run are summed inside the wavefront
// (a segmented scan, skipped when the wavefront holds no run) and its last lane issues the eight atomics.
__global__ void __launch_bounds__(256)
k_pmnp_deposit(int n, PmnpGeo g, const double *__restrict__ pos, const double *__restrict__ mass,
               double *__restrict__ oct, int *__restrict__ errw)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  CicCell c = {{0, 0, 0}, {0, 0, 0}};
  const bool ok = i < n && d_pmnp_cell(g, n, i, pos, c);
  if(i < n && !ok)
    *errw = 1;
  const int M = g.M;
  // (whole wavefronts arrive here: the shuffles need all 64 lanes)
  const int lane = threadIdx.x & (GHIP_WAVE - 1);
  const unsigned int cell = ok ? (unsigned int) ((c.s[0] * M + c.s[1]) * M + c.s[2]) : 0xffffffffu - (unsigned int) lane;
  const double m = ok ? mass[i] : 0.0;
  double w[8];
  for(int xx = 0; xx < 2; xx++)
    for(int yy = 0; yy < 2; yy++)
      for(int zz = 0; zz < 2; zz++)
        w[xx * 4 + yy * 2 + zz] = d_cic_weight(m, c, xx, yy, zz);
  bool issue = ok;
  const unsigned int before = __shfl_up(cell, 1, GHIP_WAVE), after = __shfl_down(cell, 1, GHIP_WAVE);
  const bool head = lane == 0 || before != cell, tail = lane == GHIP_WAVE - 1 || after != cell;
  const unsigned long long heads = __ballot(head);
  if(heads != ~0ULL)
    {
      const int first = 63 - __clzll((long long) (heads & (~0ULL >> (63 - lane))));
      const int dist = lane - first;
      for(int off = 1; off < GHIP_WAVE; off <<= 1)
        for(int k = 0; k < 8; k++)
          {
            const double o = __shfl_up(w[k], off, GHIP_WAVE);
            if(dist >= off)
              w[k] += o;
          }
      issue = ok && tail;
    }
  if(issue)
    for(int xx = 0; xx < 2; xx++)
      for(int yy = 0; yy < 2; yy++)
        for(int zz = 0; zz < 2; zz++)
          atomicAdd(&oct[d_pmnp_corner(M, c, xx, yy, zz)], w[xx * 4 + yy * 2 + zz]);
}

// the octant into the padded mesh, zeros everywhere else (:785-787)
__global__ void k_pmnp_scatter(int M, int G, const double *__restrict__ oct, double *__restrict__ rho)
{
  size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
  if(idx >= (size_t) G * G * G)
    return;
  const int z = (int) (idx % G), y = (int) ((idx / G) % G), x = (int) (idx / ((size_t) G * G));
  rho[idx] = (x < M && y < M && z < M) ? oct[((size_t) x * M + y) * M + z] : 0.0;
}

// :396-430: the real-space kernel, coordinates in mesh units folded at 0.5
__global__ void k_pmnp_table_fill(int G, double *__restrict__ kern)
{
  size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
  if(idx >= (size_t) G * G * G)
    return;
  const int z = (int) (idx % G), y = (int) ((idx / G) % G), x = (int) (idx / ((size_t) G * G));
  double xx = ((double) x) / G, yy = ((double) y) / G, zz = ((double) z) / G;
  if(xx >= 0.5)
    xx -= 1.0;
  if(yy >= 0.5)
    yy -= 1.0;
  if(zz >= 0.5)
    zz -= 1.0;
  const double r = sqrt(xx * xx + yy * yy + zz * zz);
  const double u = 0.5 * r / (((double) PMNP_ASMTH) / G);
  const double fac = 1 - erfc(u);
  kern[idx] = r > 0 ? -fac / r : -1 / (sqrt(M_PI) * (((double) PMNP_ASMTH) / G));
}

// :500-558 on hipFFT's layout [x][y][z = 0..G/2]: the CIC deconvolution, twice; k = 0 is left as it is
__global__ void k_pmnp_table_deconv(int G, double2 *__restrict__ fk)
{
  const int nz = G / 2 + 1;
  size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
  if(idx >= (size_t) G * G * nz)
    return;
  const int z = (int) (idx % nz), y = (int) ((idx / nz) % G), x = (int) (idx / ((size_t) nz * G));
  const double kx = x > G / 2 ? x - G : x, ky = y > G / 2 ? y - G : y, kz = z > G / 2 ? z - G : z;
  if(kx * kx + ky * ky + kz * kz > 0)
    {
      const double ff = d_cic_deconv(kx, ky, kz, G);
      double2 v = fk[idx];
      v.x *= ff;
      v.y *= ff;
      fk[idx] = v;
    }
}

// :860-891
__global__ void k_pmnp_multiply(size_t nk, const double2 *__restrict__ table, double2 *__restrict__ fk)
{
  size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
  if(idx >= nk)
    return;
  const double2 a = fk[idx], b = table[idx];
  double2 v;
  v.x = a.x * b.x - a.y * b.y;
  v.y = a.x * b.y + a.y * b.x;
  fk[idx] = v;
}

// :1000-1051 for the lower octant: force[dim][M][M][M] from the padded potential phi[G][G][G]
__global__ void k_pmnp_gradient(int M, int G, double fac, const double *__restrict__ phi, double *__restrict__ force)
{
  size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
  const size_t m3 = (size_t) M * M * M;
  if(idx >= m3)
    return;
  const int z = (int) (idx % M), y = (int) ((idx / M) % M), x = (int) (idx / ((size_t) M * M));
  const bool inner = x >= 2 && x < M - 2 && y >= 2 && y < M - 2 && z >= 2 && z < M - 2;
  const size_t c = ((size_t) x * G + y) * G + z;
  for(int dim = 0; dim < 3; dim++)
    {
      double v = 0;   // (a cell the reference does not write)
      if(inner)       // (c - 2 stride .. c + 2 stride stay inside the octant)
        {
          const size_t st = dim == 0 ? (size_t) G * G : dim == 1 ? (size_t) G : 1;
          v = fac * ((4.0 / 3) * (phi[c - st] - phi[c + st]) - (1.0 / 6) * (phi[c - 2 * st] - phi[c + 2 * st]));
        }
      force[(size_t) dim * m3 + idx] = v;
    }
}

// :1134-1153 in the reference's corner order, and the tail of long_range_force (longrange.c:117-138):
// GravPM = (0 + acc) + tailfac * Pos -- the zeroing of longrange.c:63 is this store
__global__ void k_pmnp_interpolate(int n, PmnpGeo g, double tailfac, const double *__restrict__ pos,
                                   const double *__restrict__ force, double *__restrict__ gravpm,
                                   int *__restrict__ errw)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  CicCell c;
  double acc[3] = {0, 0, 0};
  if(d_pmnp_cell(g, n, i, pos, c))
    {
      const int M = g.M;
      const size_t m3 = (size_t) M * M * M;
      for(int xx = 0; xx < 2; xx++)
        for(int yy = 0; yy < 2; yy++)
          for(int zz = 0; zz < 2; zz++)
            {
              const size_t at = d_pmnp_corner(M, c, xx, yy, zz);
              for(int dim = 0; dim < 3; dim++)
                acc[dim] += d_cic_weight(force[(size_t) dim * m3 + at], c, xx, yy, zz);
            }
    }
  else
    *errw = 1;
  for(int dim = 0; dim < 3; dim++)
    gravpm[(size_t) dim * n + i] = acc[dim] + tailfac * pos[(size_t) dim * n + i];
}

// :1713-1732 with the fac of :1378.  (The fork computes fac and never applies it, the same slip as in
// pmpotential_periodic; without it the mesh potential is not in the units of the tree potential, so it is
// applied here, as for the periodic mesh -- DESIGN.md 4.13.)
__global__ void k_pmnp_pot_readout(int n, PmnpGeo g, double fac, const double *__restrict__ pos,
                                   const double *__restrict__ phi, double *__restrict__ pot, int *__restrict__ errw)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  CicCell c;
  if(!d_pmnp_cell(g, n, i, pos, c))
    {
      *errw = 1;
      return;
    }
  const int G = g.G;
  double v = 0;
  for(int xx = 0; xx < 2; xx++)
    for(int yy = 0; yy < 2; yy++)
      for(int zz = 0; zz < 2; zz++)
        v += d_cic_weight(phi[d_pmnp_corner(G, c, xx, yy, zz)], c, xx, yy, zz);
  pot[i] += fac * v;
}

// Deliberate difference: the symmetrisation of :133-134, (xmin + xmax) / 2 - ext / 2 and + ext, is rounded three
// times, so a bound can come out one unit in the last place INSIDE the very particle that defines the extent.
// The reference's comparison (:622) then refuses that particle, pm_init_regionsize gives the same region again
// and the run stops with endrun(68687).  The range check here allows 4 DBL_EPSILON max(|Xmintot|, |Xmaxtot|)
// along each axis -- twice the bound of those three roundings, and 1e-7 of the 1e-9 extent that must be refused
// for coordinates of the size of the extent.  The region itself is stored as the reference computes it.
static double pmnp_range_slack(const ghip_pm_region &r, int j)
{
  const double a = fabs(r.Xmintot[j]), b = fabs(r.Xmaxtot[j]);
  return 4 * DBL_EPSILON * (a > b ? a : b);
}

static int pmnp_check_grid(ghip_ctx *ctx, int pmgrid, const char *who)
{
  if(pmgrid < PMNP_MIN_GRID || pmgrid > PMNP_MAX_GRID || (pmgrid & 1))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: PMGRID %d is not an even number in [%d, %d]", who, pmgrid, PMNP_MIN_GRID,
                     PMNP_MAX_GRID);
  return GHIP_OK;
}

// pm_init_regionsize :121-159 from the extremes of all particles, operation for operation in double (every
// rank gets the same bytes: no contraction of a product into the sum that follows it)
static int pmnp_region_from_extremes(ghip_ctx *ctx, int pmgrid, unsigned long long err, int bad,
                                     unsigned long long ntot, const double xmin[3], const double xmax[3],
                                     ghip_pm_region *out, const char *who)
{
#pragma clang fp contract(off)
  if(err & EXTENT_ERR_POS)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: a position that is not finite (first on shard %d); nothing stored", who,
                     bad);
  if(ntot == 0)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: no particle at all; nothing stored", who);
  const int GRID = 2 * pmgrid;
  ghip_pm_region r;
  r.pmgrid = pmgrid;
  double tms = xmax[0] - xmin[0];                              // :123-125
  tms = tms > xmax[1] - xmin[1] ? tms : xmax[1] - xmin[1];
  tms = tms > xmax[2] - xmin[2] ? tms : xmax[2] - xmin[2];
  if(!(tms > 0) || !(tms <= DBL_MAX))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: the extent of the particles has length %g; nothing stored", who, tms);
  for(int i = 0; i < 3; i++)                                   // :131-135
    {
      r.Xmintot[i] = (xmin[i] + xmax[i]) / 2 - tms / 2;
      r.Xmaxtot[i] = r.Xmintot[i] + tms;
    }
  tms *= 2.001 * (GRID) / ((double) (GRID - 2 - 8));           // :144
  r.TotalMeshSize = tms;
  for(int i = 0; i < 3; i++)                                   // :152-153
    {
      r.Corner[i] = r.Xmintot[i] - 2.0005 * tms / GRID;
      r.UpperCorner[i] = r.Corner[i] + (GRID / 2 - 1) * (tms / GRID);
    }
  r.Asmth = PMNP_ASMTH * tms / GRID;                           // :158-159
  r.Rcut = PMNP_RCUT * r.Asmth;
  if(!(r.TotalMeshSize <= DBL_MAX))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: the mesh size is not finite; nothing stored", who);
  ctx->pm_region = r;
  ctx->pm_region_set = true;
  if(out)
    *out = r;
  return GHIP_OK;
}

extern "C" int ghip_pm_find_region(ghip_ctx *ctx, int pmgrid, ghip_pm_region *out)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  GCHK(pmnp_check_grid(ctx, pmgrid, "ghip_pm_find_region"));
  if(ctx->dd.on)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_pm_find_region: on a multi-GPU shard use GHIP_DD_PM_REGION");
  if(ctx->n > 0 && !ctx->f[GHIP_F_POS].p)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_pm_find_region: particle field %d not set", (int) GHIP_F_POS);
  GCHK(ghip_extent_pass(ctx, ctx->dd.dc_own, 0));   // (the block of the shard operations: idle here, dd is off)
  unsigned long long blk[EXTENT_WORDS], ntot;
  HIPCHK(hipMemcpyAsync(blk, ctx->dd.dc_own.p, sizeof(blk), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  double xmin[3], xmax[3];
  int bmin, bmax, bad;
  const unsigned long long err = ghip_extent_reduce(blk, 1, xmin, xmax, &ntot, &bmin, &bmax, &bad);
  return pmnp_region_from_extremes(ctx, pmgrid, err, bad, ntot, xmin, xmax, out, "ghip_pm_find_region");
}

extern "C" int ghip_pm_set_region(ghip_ctx *ctx, const ghip_pm_region *r)
{
  if(!ctx || !r)
    return GHIP_EINVAL;
  GCHK(pmnp_check_grid(ctx, r->pmgrid, "ghip_pm_set_region"));
  const int GRID = 2 * r->pmgrid;
  bool ok = r->TotalMeshSize > 0 && r->TotalMeshSize <= DBL_MAX && r->Asmth > 0 && r->Rcut > 0;
  for(int j = 0; j < 3 && ok; j++)
    {
      // [Xmintot, Xmaxtot] has to land in cells [2, GRID/2 - 2) with both CIC neighbours
      const double fac = GRID / r->TotalMeshSize;
      const double lo = fac * (r->Xmintot[j] - r->Corner[j]), hi = fac * (r->Xmaxtot[j] - r->Corner[j]);
      ok = r->Xmaxtot[j] > r->Xmintot[j] && lo >= 2.0 && hi < (double) (GRID / 2 - 3) && fabs(r->UpperCorner[j]) <= DBL_MAX;
    }
  if(!ok)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_pm_set_region: the region does not place [Xmintot, Xmaxtot] into cells "
                     "[2, GRID/2 - 2) of a mesh of TotalMeshSize > 0 (or Asmth, Rcut are not > 0); nothing stored");
  ctx->pm_region = *r;
  ctx->pm_region_set = true;
  return GHIP_OK;
}

extern "C" int ghip_pm_get_region(const ghip_ctx *ctx, ghip_pm_region *out)
{
  if(!ctx || !out || !ctx->pm_region_set)
    return GHIP_EINVAL;
  *out = ctx->pm_region;
  return GHIP_OK;
}

static int pmnp_need_region(ghip_ctx *ctx, int pmgrid, const char *who)
{
  if(!ctx->pm_region_set)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: no region: call ghip_pm_find_region (GHIP_DD_PM_REGION) or "
                     "ghip_pm_set_region first", who);
  if(ctx->pm_region.pmgrid != pmgrid)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: PMGRID %d, but the region in force was made for PMGRID %d", who, pmgrid,
                     ctx->pm_region.pmgrid);
  return GHIP_OK;
}

// the block a shard sends: the octant and its status word
static size_t pmnp_block_bytes(int pmgrid) { return ((size_t) pmgrid * pmgrid * pmgrid + 1) * sizeof(double); }

// Plans, buffers and the Green's function table for PMGRID = M.  The table depends on PMGRID only (ASMTH / GRID
// is in mesh units, :413): it is keyed on M and survives every change of the region that keeps M.
static int pmnp_prepare(ghip_ctx *ctx, int M)
{
  hipStream_t st = ctx->stream;
  PmMesh::Open &o = ctx->pm.open;
  const int G = 2 * M;
  const size_t g3 = (size_t) G * G * G, nk = (size_t) G * G * (G / 2 + 1), m3 = (size_t) M * M * M;
  if(o.fft.n != G)
    ghip_renew(o);   // (the table and the octant go with the plans)
  auto buffers = [&]() -> int {
    GCHK(pm_fft_prepare(ctx, o.fft, G));
    GCHK(ghip_ensure(ctx, o.table, nk * sizeof(double2)));
    GCHK(ghip_ensure(ctx, o.force, 3 * m3 * sizeof(double)));
    GCHK(ghip_ensure(ctx, o.oct, pmnp_block_bytes(M)));
    if(o.table_n != M)
      {
        double *kern = P<double>(o.fft.rho);
        double2 *table = P<double2>(o.table);
        k_pmnp_table_fill<<<cdiv((long long) g3, 256), 256, 0, st>>>(G, kern);
        HIPCHK(hipGetLastError());
        FFTCHK(hipfftExecD2Z((hipfftHandle) o.fft.fwd, kern, reinterpret_cast<hipfftDoubleComplex *>(table)));
        k_pmnp_table_deconv<<<cdiv((long long) nk, 256), 256, 0, st>>>(G, table);
        HIPCHK(hipGetLastError());
        o.table_n = M;
      }
    return GHIP_OK;
  };
  const int rc = buffers();
  if(rc != GHIP_OK)
    {
      const std::string msg = ctx->err;
      (void) hipStreamSynchronize(st);
      ghip_renew(o);
      ctx->err = msg;
    }
  return rc;
}

// range check (:614-647) and, if every particle is inside, the deposit into the (zeroed) octant; the status word
// behind the octant says which.  One host read: the error word.
static int pmnp_check_and_deposit(ghip_ctx *ctx, int *outside)
{
  hipStream_t st = ctx->stream;
  const ghip_pm_region &r = ctx->pm_region;
  const int M = r.pmgrid, n = ctx->n;
  const size_t m3 = (size_t) M * M * M;
  double *oct = P<double>(ctx->pm.open.oct);
  int *errw = &ghip_words(ctx)->pm_err;
  int flag = 0;
  *outside = 0;
  HIPCHK(hipMemsetAsync(oct, 0, (m3 + 1) * sizeof(double), st));   // (status PMNP_ST_OK)
  if(n > 0)
    {
      HIPCHK(hipMemsetAsync(errw, 0, sizeof(int), st));
      double lo[3], hi[3];
      for(int j = 0; j < 3; j++)
        {
          const double tol = pmnp_range_slack(r, j);
          lo[j] = r.Xmintot[j] - tol;
          hi[j] = r.Xmaxtot[j] + tol;
        }
      k_pmnp_range<<<cdiv(n, 256), 256, 0, st>>>(n, P<double>(ctx->f[GHIP_F_POS]), lo[0], lo[1], lo[2], hi[0], hi[1],
                                                 hi[2], errw);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(&flag, errw, sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
    }
  if(flag)
    {
      const double s = PMNP_ST_RANGE;
      HIPCHK(hipMemcpyAsync(oct + m3, &s, sizeof(double), hipMemcpyHostToDevice, st));
      HIPCHK(ghip_stream_sync(ctx, st));   // (`s` lives on this frame)
      *outside = 1;
      return GHIP_OK;
    }
  if(n > 0)
    {
      k_pmnp_deposit<<<cdiv(n, 256), 256, 0, st>>>(n, pmnp_geo(r), P<double>(ctx->f[GHIP_F_POS]),
                                                   P<double>(ctx->f[GHIP_F_MASS]), oct, ghip_errword(ctx, GHIP_ERRW_PM));
      HIPCHK(hipGetLastError());
    }
  return GHIP_OK;
}

// all != nullptr: the status words of the nranks gathered blocks; *outside: a shard met a particle outside
// the region, *failed: the first shard whose own pass failed (-1: none)
static int pmnp_read_status(ghip_ctx *ctx, int M, int nranks, const double *all, int *outside, int *failed)
{
  const size_t m3 = (size_t) M * M * M;
  double st[GHIP_MAXRANKS];
  *outside = 0;
  *failed = -1;
  for(int r = 0; r < nranks; r++)
    HIPCHK(hipMemcpyAsync(&st[r], all + (size_t) r * (m3 + 1) + m3, sizeof(double), hipMemcpyDeviceToHost,
                          ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  for(int r = 0; r < nranks; r++)
    {
      if(st[r] == PMNP_ST_LOCAL && *failed < 0)
        *failed = r;
      if(st[r] == PMNP_ST_RANGE)
        *outside = 1;
    }
  return GHIP_OK;
}

// the octant (all != nullptr: the sum of the gathered ones, in rank order) -> the padded mesh -> the potential
// mesh in open.rho
static int pmnp_solve(ghip_ctx *ctx, int nranks, const double *all)
{
  hipStream_t st = ctx->stream;
  PmMesh::Open &o = ctx->pm.open;
  const int G = o.fft.n, M = G / 2;
  const size_t g3 = (size_t) G * G * G, nk = (size_t) G * G * (G / 2 + 1), m3 = (size_t) M * M * M;
  double *rho = P<double>(o.fft.rho), *oct = P<double>(o.oct);
  double2 *fk = P<double2>(o.fft.k);
  if(all)
    {
      k_pm_sum_meshes<<<cdiv((long long) m3, 256), 256, 0, st>>>(m3, m3 + 1, nranks, all, oct);
      HIPCHK(hipGetLastError());
    }
  k_pmnp_scatter<<<cdiv((long long) g3, 256), 256, 0, st>>>(M, G, oct, rho);
  HIPCHK(hipGetLastError());
  FFTCHK(hipfftExecD2Z((hipfftHandle) o.fft.fwd, rho, reinterpret_cast<hipfftDoubleComplex *>(fk)));
  k_pmnp_multiply<<<cdiv((long long) nk, 256), 256, 0, st>>>(nk, P<double2>(o.table), fk);
  HIPCHK(hipGetLastError());
  FFTCHK(hipfftExecZ2D((hipfftHandle) o.fft.inv, reinterpret_cast<hipfftDoubleComplex *>(fk), rho));
  return GHIP_OK;
}

// potential mesh -> force components of the octant -> GRAVPM of this context's particles, with the tail
static int pmnp_force(ghip_ctx *ctx, const ghip_pmnp_params *p)
{
  hipStream_t st = ctx->stream;
  PmMesh::Open &o = ctx->pm.open;
  const ghip_pm_region &r = ctx->pm_region;
  const int G = o.fft.n, M = G / 2, n = ctx->n;
  const size_t m3 = (size_t) M * M * M;
  const double tms = r.TotalMeshSize;
  double fac = p->G / pow(tms, 4) * pow(tms / G, 3);   // :606
  fac *= 1 / (2 * tms / G);                             // :607
  // longrange.c:117-138
  const double tailfac = p->comoving ? 0.5 * p->Hubble * p->Hubble * p->Omega0 : p->OmegaLambda * p->Hubble * p->Hubble;
  k_pmnp_gradient<<<cdiv((long long) m3, 256), 256, 0, st>>>(M, G, fac, P<double>(o.fft.rho), P<double>(o.force));
  HIPCHK(hipGetLastError());
  if(n > 0)
    {
      k_pmnp_interpolate<<<cdiv(n, 256), 256, 0, st>>>(n, pmnp_geo(r), tailfac, P<double>(ctx->f[GHIP_F_POS]),
                                                       P<double>(o.force), P<double>(ctx->f[GHIP_F_GRAVPM]),
                                                       ghip_errword(ctx, GHIP_ERRW_PM));
      HIPCHK(hipGetLastError());
    }
  return GHIP_OK;
}

static int pmnp_check_params(ghip_ctx *ctx, const ghip_pmnp_params *p, const char *who)
{
  GCHK(pmnp_check_grid(ctx, p->pmgrid, who));
  if(!(fabs(p->G) <= DBL_MAX) || !(fabs(p->Hubble) <= DBL_MAX) || !(fabs(p->Omega0) <= DBL_MAX) ||
     !(fabs(p->OmegaLambda) <= DBL_MAX))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: G, Hubble, Omega0, OmegaLambda must be finite", who);
  return GHIP_OK;
}

static int pmnp_need_fields(ghip_ctx *ctx, const char *who)
{
  for(int f : {GHIP_F_POS, GHIP_F_MASS, GHIP_F_GRAVPM})
    if(ctx->n > 0 && !ctx->f[f].p)
      return ghip_fail(ctx, GHIP_EINVAL, "%s: particle field %d not set", who, f);
  return GHIP_OK;
}

static int pmnp_outside(ghip_ctx *ctx, const char *who)
{
  return ghip_fail(ctx, GHIP_EREGION, "%s: a particle lies outside the allowed region of the mesh; nothing was "
                   "written.  Find the region again (ghip_pm_find_region / GHIP_DD_PM_REGION) and repeat the call", who);
}

// What the deposits left: GHIP_OK to go on and solve.  Else the call ends here, on every shard alike: `failed`
// is the first shard whose own pass failed (-1: none), `outside` says that a particle lies outside the region.
// force: the call is one of the force's, whose end event closes ms_pm and which promises that nothing was written
static int pmnp_verdict(ghip_ctx *ctx, const char *who, int outside, int failed, bool force)
{
  if(!outside && failed < 0)
    return GHIP_OK;
  if(force)
    HIPCHK(hipEventRecord(ctx->evp[15], ctx->stream));
  if(failed >= 0)
    return ghip_dd_raise(ctx, failed, "%s: the deposit failed on shard %d (its own message says why); every shard "
                         "stops here%s", who, failed, force ? ", nothing was written" : "");
  return pmnp_outside(ctx, who);
}

extern "C" int ghip_pm_nonperiodic(ghip_ctx *ctx, const ghip_pmnp_params *p)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !p)
    return GHIP_EINVAL;
  const char *who = "ghip_pm_nonperiodic";
  GCHK(pmnp_check_params(ctx, p, who));
  if(ctx->dd.on)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_pm_nonperiodic: on a multi-GPU shard use GHIP_DD_PM_NONPERIODIC");
  if(ctx->n == 0)
    return GHIP_OK;
  GCHK(pmnp_need_region(ctx, p->pmgrid, who));
  GCHK(pmnp_need_fields(ctx, who));
  hipStream_t st = ctx->stream;
  GCHK(pmnp_prepare(ctx, p->pmgrid));
  HIPCHK(hipEventRecord(ctx->evp[14], st));
  int outside = 0;
  GCHK(pmnp_check_and_deposit(ctx, &outside));
  GCHK(pmnp_verdict(ctx, who, outside, -1, true));
  GCHK(pmnp_solve(ctx, 1, nullptr));
  GCHK(pmnp_force(ctx, p));
  HIPCHK(hipEventRecord(ctx->evp[15], st));
  return GHIP_OK;
}

// the open mesh's potential: (all != nullptr: the statuses of the gathered blocks first) solve, pot[i] += the
// mesh potential at particle i
static int pmnp_potential(ghip_ctx *ctx, const ghip_pm_params *pm, int nranks, const double *all, double *pot)
{
  const ghip_pm_region &r = ctx->pm_region;
  const int n = ctx->n;
  if(all)
    {
      int outside = 0, failed = -1;
      GCHK(pmnp_read_status(ctx, pm->pmgrid, nranks, all, &outside, &failed));
      GCHK(pmnp_verdict(ctx, "the non-periodic mesh potential", outside, failed, false));
    }
  GCHK(pmnp_solve(ctx, nranks, all));
  const double tms = r.TotalMeshSize;
  const double fac = pm->G / pow(tms, 4) * pow(tms / (2 * pm->pmgrid), 3);   // :1378
  if(n > 0)
    {
      k_pmnp_pot_readout<<<cdiv(n, 256), 256, 0, ctx->stream>>>(n, pmnp_geo(r), fac, P<double>(ctx->f[GHIP_F_POS]),
                                                                P<double>(ctx->pm.open.fft.rho), pot,
                                                                ghip_errword(ctx, GHIP_ERRW_PM));
      HIPCHK(hipGetLastError());
    }
  return GHIP_OK;
}

// ---- GHIP_DD_PM_REGION: phase 0 reduces this shard's positions and posts the all-gather of the extent blocks,
// phase 1 evaluates all blocks in rank order (the MPI_Allreduce of :118-119) and stores the region ----
int ghip_dd_pmreg_begin(ghip_ctx *ctx, int, const void *params, int)
{
  GHIP_JOIN(ctx);
  ctx->dd.pmreg_grid = *reinterpret_cast<const int *>(params);
  GCHK(pmnp_check_grid(ctx, ctx->dd.pmreg_grid, "GHIP_DD_PM_REGION"));
  if(ctx->n > 0 && !ctx->f[GHIP_F_POS].p)
    return ghip_fail(ctx, GHIP_EINVAL, "GHIP_DD_PM_REGION: particle field %d not set", (int) GHIP_F_POS);
  return GHIP_OK;
}

int ghip_dd_pmreg_step(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  enum { EXTENT, REGION };
  if(D.phase == EXTENT)
    {
      // (a failure of this shard's own pass is marked in the block: its peers stop with it in REGION)
      if(ghip_dd_hold(ctx, ghip_extent_pass(ctx, D.dc_own, 0)) && !D.dc_own.p)
        return D.held.rc;   // (without the block there is nothing to send)
      ghip_dd_set_allgather(D, D.dc_own.p, EXTENT_WORDS * 8, &D.dc_all);
      D.phase = REGION;
      return 1;
    }
  if(D.phase == REGION)
    {
      std::vector<unsigned long long> all((size_t) D.nranks * EXTENT_WORDS);
      HIPCHK(hipMemcpyAsync(all.data(), D.dc_all.p, all.size() * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      double xmin[3], xmax[3];
      unsigned long long ntot;
      int bmin, bmax, bad;
      const unsigned long long err = ghip_extent_reduce(all.data(), D.nranks, xmin, xmax, &ntot, &bmin, &bmax, &bad);
      if(err & EXTENT_ERR_LOCAL)
        return ghip_dd_raise(ctx, bad, "%s: the pass over the positions failed on shard %d (its own message says "
                             "why); nothing stored", "GHIP_DD_PM_REGION", bad);
      const int rc = pmnp_region_from_extremes(ctx, D.pmreg_grid, err, bad, ntot, xmin, xmax, nullptr,
                                               "GHIP_DD_PM_REGION");
      return rc == GHIP_OK ? 0 : rc;
    }
  return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: the mesh region has no phase %d", D.phase);
}

// ---- GHIP_DD_PM_NONPERIODIC: phase 0 checks the range, deposits and posts the all-gather of the compact
// octants with their status words; phase 1 reads every status (all shards stop together), adds the octants in
// rank order, solves and reads out ----
int ghip_dd_pmnp_begin(ghip_ctx *ctx, int, const void *params, int)
{
  GHIP_JOIN(ctx);
  ctx->dd.pmnp = *reinterpret_cast<const ghip_pmnp_params *>(params);
  const char *who = "GHIP_DD_PM_NONPERIODIC";
  GCHK(pmnp_check_params(ctx, &ctx->dd.pmnp, who));
  GCHK(pmnp_need_region(ctx, ctx->dd.pmnp.pmgrid, who));
  return pmnp_need_fields(ctx, who);
}

int ghip_dd_pmnp_step(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  const ghip_pmnp_params *p = &D.pmnp;
  hipStream_t st = ctx->stream;
  const int M = p->pmgrid;
  const size_t m3 = (size_t) M * M * M;
  enum { DEPOSIT, SOLVE };
  if(D.phase == DEPOSIT)
    {
      GCHK(pmnp_prepare(ctx, M));
      HIPCHK(hipEventRecord(ctx->evp[14], st));
      int outside = 0;
      if(ghip_dd_hold(ctx, pmnp_check_and_deposit(ctx, &outside)))
        {
          const double s = PMNP_ST_LOCAL;
          HIPCHK(hipMemcpy(P<double>(ctx->pm.open.oct) + m3, &s, sizeof(double), hipMemcpyHostToDevice));
        }
      ghip_dd_set_allgather(D, ctx->pm.open.oct.p, pmnp_block_bytes(M), &D.pm_all);
      D.phase = SOLVE;
      return 1;
    }
  if(D.phase == SOLVE)
    {
      int outside = 0, failed = -1;
      GCHK(pmnp_read_status(ctx, M, D.nranks, P<double>(D.pm_all), &outside, &failed));
      GCHK(pmnp_verdict(ctx, "GHIP_DD_PM_NONPERIODIC", outside, failed, true));
      GCHK(pmnp_solve(ctx, D.nranks, P<double>(D.pm_all)));
      GCHK(pmnp_force(ctx, p));
      HIPCHK(hipEventRecord(ctx->evp[15], st));
      return 0;
    }
  return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: the non-periodic mesh force has no phase %d", D.phase);
}

// ---- the mesh part of the potential (ghip_potential.hip calls these three, with pm.pmgrid != 0): with
// grav.periodic pmpotential_periodic, else pmpotential_nonperiodic(0).  GRAVPM is not touched. ----
int ghip_pm_pot_check(ghip_ctx *ctx, const ghip_pot_params *p, const char *who)
{
  const ghip_grav_params &g = p->grav;
  const ghip_pm_params &pm = p->pm;
  if(g.periodic)
    {
      if(pm.pmgrid < 4 || pm.pmgrid > 2048 || (pm.pmgrid & 1) || !(pm.BoxSize > 0) || !(pm.Asmth > 0))
        return ghip_fail(ctx, GHIP_EINVAL, "%s: need an even PMGRID in [4, 2048], pm.BoxSize > 0, "
                         "pm.Asmth > 0", who);
      if(pm.BoxSize != g.BoxSize)
        return ghip_fail(ctx, GHIP_EINVAL, "%s: pm.BoxSize %g differs from grav.BoxSize %g", who,
                         pm.BoxSize, g.BoxSize);
      if(!(g.Rcut > 0 && g.Asmth > 0))
        return ghip_fail(ctx, GHIP_EINVAL, "%s: a PM potential needs Rcut, Asmth > 0", who);
      return GHIP_OK;
    }
  // a region is set, of this PMGRID, and the walk is cut where the region says (pm.BoxSize is not read: there is no box)
  GCHK(pmnp_check_grid(ctx, pm.pmgrid, who));
  GCHK(pmnp_need_region(ctx, pm.pmgrid, who));
  const ghip_pm_region &r = ctx->pm_region;
  if(!(g.Asmth == pm.Asmth && pm.Asmth == r.Asmth))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: grav.Asmth %.17g, pm.Asmth %.17g and the region's Asmth %.17g must be "
                     "equal (ghip_pm_get_region)", who, g.Asmth, pm.Asmth, r.Asmth);
  if(!(g.Rcut == r.Rcut))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: grav.Rcut %.17g differs from the region's Rcut %.17g (ghip_pm_get_region)",
                     who, g.Rcut, r.Rcut);
  if(!(fabs(pm.G) <= DBL_MAX))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: pm.G must be finite", who);
  return GHIP_OK;
}

int ghip_pm_pot_deposit(ghip_ctx *ctx, const ghip_pot_params *p, PmBlock *b)
{
  const int N = p->pm.pmgrid;
  b->outside = 0;
  if(p->grav.periodic)
    {
      GCHK(pm_prepare(ctx, N));
      GCHK(pm_deposit(ctx, &p->pm, false));
      b->p = ctx->pm.fft.rho.p;
      b->bytes = (size_t) N * N * N * sizeof(double);
      return GHIP_OK;
    }
  GCHK(pmnp_need_region(ctx, N, "the non-periodic mesh potential"));
  GCHK(pmnp_prepare(ctx, N));
  GCHK(pmnp_check_and_deposit(ctx, &b->outside));
  b->p = ctx->pm.open.oct.p;
  b->bytes = pmnp_block_bytes(N);
  return GHIP_OK;
}

int ghip_pm_pot_solve(ghip_ctx *ctx, const ghip_pot_params *p, int nranks, const double *all, double *pot)
{
  return p->grav.periodic ? pm_potential(ctx, &p->pm, nranks, all, pot)
                          : pmnp_potential(ctx, &p->pm, nranks, all, pot);
}

void ghip_pm_release(ghip_ctx *ctx)
{
  if(ctx)
    ghip_renew(ctx->pm);
}
