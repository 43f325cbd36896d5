// ghip_fof.hip -- friends-of-friends groups on the resident state (fof_fof, fof.c:94-333, without the group
// files and SUBFIND).  One call:
//
//   k_fof_classify     per sorted index of the gravity tree: ID, kind (primary / secondary), parent = itself
//   ghip_select_flagged  the sorted indices of the primaries and of the secondaries           -> 2 words read
//   k_fof_mass_*       LinkL <= 0: mass and number of the primaries in a fixed order, LinkL      -> 1 word read
//   k_fof_link         one wavefront per bucket of 64 consecutive primaries: a wave-uniform traversal of the
//                      tree (a node is opened when any lane's sphere overlaps it), candidates staged in LDS 64 at a time, every
//                      lane tests its own primary against each staged primary of smaller sorted index and
//                      unites the two in a lock-free union-find (fof_find_groups, fof.c:337-706)
//   k_fof_flatten      parent = root for everybody, then the smallest ID of each root (integer atomicMin)
//   k_fof_label        the primaries' labels
//   k_fof_nearest      one thread per secondary, per round; h doubles for those that found nobody  -> 1 word / round
//   sort by (label, ID), segment heads, a scan: the candidate groups; sort of the groups by (Len desc, MinID asc);
//   a scan of Len: Offset; k_fof_members: the ID list; k_fof_props: one wavefront per kept group, lane-strided
//   partial sums in member order and a fixed butterfly: no floating-point atomics             -> 4 words read
//
// The union-find (sorted indices; a root has parent[x] == x, and parent[x] <= x always):
//   find    follows parents, which only ever decrease: every step goes to a strictly smaller index, so it ends
//           after at most x steps.  Parents are read with agent-scope atomic loads, so that no lane keeps reading a
//           stale line of its CU's L1.
//   union   finds both roots, hooks the LARGER root under the smaller with atomicCAS(parent[a], a, b).  A CAS fails
//           only when another lane has hooked a meanwhile: parent[a] < a then, and the next find from a ends at a
//           strictly smaller index.  The larger root of the pair strictly decreases with every retry and is bounded
//           below by 0, so the loop ends; no lane waits for another lane's progress and nothing is locked.
// The partition is that of the link relation whatever the order of the unions; only who is root depends on it,
// and the label is the smallest ID of the component, which does not.
#include <cfloat>
#include <climits>

#include "ghip_ngb.h"
#include "ghip_prim.h"

#define FOF_LEAF 64        // a node of at most this many particles is swept flat (one LDS stage)
#define FOF_NEAR_LEAF 8    // ... in the per-thread search of the secondaries
#define FOF_RED_BLOCK 256

struct FofWords
{
  int nprim, nsec, left, ngroups, largest, nseg;
  unsigned long long nids;
  double linkl, masstot;
  long long ndm;
  int changed;   // the collective form: a label fell in this round
};

__device__ __forceinline__ int d_fof_sum_i32(int v)
{
  for(int off = 32; off > 0; off >>= 1)
    v += __shfl_xor(v, off, 64);
  return v;
}

// fof_periodic, fof.c:2273-2280
__device__ __forceinline__ double d_fof_periodic(double x, const BoxK b)
{
  if(x >= b.boxhalf)
    x -= b.boxsize;
  if(x < -b.boxhalf)
    x += b.boxsize;
  return x;
}

__device__ __forceinline__ int d_fof_load(const int *p)
{
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ends: every step reads a parent < x (a root has parent == x and stops the loop)
__device__ __forceinline__ int d_fof_find(int *parent, int x)
{
  int p = d_fof_load(parent + x);
  while(p != x)
    {
      const int g = d_fof_load(parent + p);
      if(g != p)
        atomicMin(parent + x, g);   // halve the path: g is an ancestor of x, and parents still only decrease
      x = p;
      p = g;
    }
  return x;
}

// ends: a failed CAS means parent[a] < a now, so the larger root found next is strictly smaller (see the top)
__device__ __forceinline__ void d_fof_union(int *parent, int a, int b)
{
  for(;;)
    {
      a = d_fof_find(parent, a);
      b = d_fof_find(parent, b);
      if(a == b)
        return;
      if(a < b)
        {
          const int t = a;
          a = b;
          b = t;
        }
      if(atomicCAS(parent + a, a, b) == a)
        return;
    }
}

__global__ void k_fof_classify(int n, const int *__restrict__ perm, const int *__restrict__ type,
                               const int *__restrict__ id, int pmask, int smask, int *__restrict__ sid,
                               int *__restrict__ sflag, int *__restrict__ parent, int *__restrict__ rootmin,
                               int *__restrict__ slabel, int *__restrict__ isprim, int *__restrict__ issec)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if(p >= n)
    return;
  const int j = perm[p];
  const int ty = type[j];
  const bool inrange = (unsigned int) ty < 6u;
  const bool prim = inrange && ((pmask >> ty) & 1);
  const bool sec = inrange && !prim && ((smask >> ty) & 1);
  sid[p] = id[j];
  slabel[p] = id[j];
  sflag[p] = prim ? 1 : (sec ? 2 : 0);
  isprim[p] = prim;
  issec[p] = sec;
  parent[p] = p;
  rootmin[p] = INT_MAX;
}

// LINKLENGTH rule (fof.c:112-124): block sums in index order, then one block adds them in block order
__global__ void __launch_bounds__(FOF_RED_BLOCK)
k_fof_mass_blocks(int n, const int *__restrict__ type, const double *__restrict__ mass, int pmask,
                  double *__restrict__ part)
{
  __shared__ double sm[FOF_RED_BLOCK];
  const int j = blockIdx.x * FOF_RED_BLOCK + threadIdx.x;
  double m = 0;
  if(j < n)
    {
      const int ty = type[j];
      if((unsigned int) ty < 6u && ((pmask >> ty) & 1))
        m = mass[j];
    }
  sm[threadIdx.x] = m;
  __syncthreads();
  for(int s = FOF_RED_BLOCK / 2; s > 0; s >>= 1)
    {
      if(threadIdx.x < s)
        sm[threadIdx.x] += sm[threadIdx.x + s];
      __syncthreads();
    }
  if(threadIdx.x == 0)
    part[blockIdx.x] = sm[0];
}

__global__ void __launch_bounds__(FOF_RED_BLOCK)
k_fof_linkl(int nblk, const double *__restrict__ part, double linklength, double rhodm, FofWords *w)
{
  __shared__ double sm[FOF_RED_BLOCK];
  double m = 0;
  for(int b = threadIdx.x; b < nblk; b += FOF_RED_BLOCK)
    m += part[b];
  sm[threadIdx.x] = m;
  __syncthreads();
  for(int s = FOF_RED_BLOCK / 2; s > 0; s >>= 1)
    {
      if(threadIdx.x < s)
        sm[threadIdx.x] += sm[threadIdx.x + s];
      __syncthreads();
    }
  if(threadIdx.x == 0)
    {
      w->masstot = sm[0];
      w->linkl = w->nprim > 0 ? linklength * pow(sm[0] / w->nprim / rhodm, 1.0 / 3) : 0.0;
    }
}

// One wavefront per bucket of 64 consecutive primaries (plist ascending in sorted, i.e. curve order).  The element
// index e is the same in all lanes.  A linked pair (p, q) is found by the bucket of the larger sorted index only:
// nodes whose first particle lies behind the bucket's last primary are skipped, and a lane tests q < p.
__global__ void __launch_bounds__(64)
k_fof_link(int nprim, const int *__restrict__ plist, int nelem, const int4 *__restrict__ lk,
           const double4 *__restrict__ cl, const double *__restrict__ sx, const double *__restrict__ sy,
           const double *__restrict__ sz, const int *__restrict__ sflag, double linkl, BoxK b,
           int *__restrict__ parent)
{
  __shared__ double cx[64], cy[64], cz[64];
  const int lane = threadIdx.x;
  const int k = blockIdx.x * 64 + lane;
  const bool valid = k < nprim;
  const int p = plist[valid ? k : nprim - 1];   // (the bucket exists: nprim > 64 blockIdx.x)
  const double px = sx[p], py = sy[p], pz = sz[p];
  const int pmax = d_wave_max_i32(p);
  const double l2 = linkl * linkl;
  int e = 0;
  while(e < nelem)
    {
      const int4 kk = lk[e];
      int first = kk.y, count = 1, next = e + 1;   // a particle element
      if(kk.y < 0)
        {
          // opened when the search sphere of any lane's primary overlaps it (the node test of
          // ngb_treefind_fof_primary, ngb.c:336-349, per lane; one vote).  Not a test against a sphere around
          // the whole bucket: 64 consecutive primaries of the curve can lie half a box apart, and such a
          // bucket would sweep the whole tree
          const double4 c = cl[e];
          const bool open = kk.z <= pmax && __any(valid && d_node_overlaps(c, linkl, px, py, pz, b));
          first = kk.z;
          count = (open && kk.w <= FOF_LEAF) ? kk.w : 0;
          next = (open && kk.w > FOF_LEAF) ? e + 1 : kk.x;
        }
      e = next;
      if(count == 0 || first > pmax)
        continue;
      // stage the candidates (count <= 64): positions and who is a primary no later than the bucket's last
      const int q = first + lane;
      const bool cand = lane < count && q <= pmax && sflag[q] == 1;
      __syncthreads();   // the previous stage has been read
      if(cand)
        {
          cx[lane] = sx[q];
          cy[lane] = sy[q];
          cz[lane] = sz[q];
        }
      __syncthreads();
      unsigned long long m = __ballot(cand);
      while(m)
        {
          const int i = __ffsll((long long) m) - 1;
          m &= m - 1;
          const int qi = first + i;
          const double dx = d_wrap(px - cx[i], b), dy = d_wrap(py - cy[i], b), dz = d_wrap(pz - cz[i], b);
          const double r2 = dx * dx + dy * dy + dz * dz;
          if(valid && qi < p && !(r2 > l2))   // ngb.c:351-368 continues on r2 > LinkL^2: equality links
            d_fof_union(parent, p, qi);
        }
    }
}

__global__ void k_fof_flatten(int n, const int *__restrict__ sflag, const int *__restrict__ sid, int *parent,
                              int *__restrict__ rootmin)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if(p >= n || sflag[p] != 1)
    return;
  // no union runs any more: the roots are final, every value met on the way is an ancestor
  int r = p, q;
  while((q = d_fof_load(parent + r)) != r)
    r = q;
  __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // (the minimum only decreases: a lane whose ID is not below the value in place has nothing to add, which spares
  // a percolating group its hundreds of thousands of atomics on one word)
  const int id = sid[p];
  if(id < d_fof_load(rootmin + r))
    atomicMin(rootmin + r, id);
}

__global__ void k_fof_label(int n, const int *__restrict__ sflag, const int *__restrict__ parent,
                            const int *__restrict__ rootmin, int *__restrict__ slabel)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if(p < n && sflag[p] == 1)
    slabel[p] = rootmin[parent[p]];
}

__global__ void k_fof_hinit(int nsec, const int *__restrict__ slist, const int *__restrict__ perm,
                            const int *__restrict__ type, const double *__restrict__ hsml, const FofWords *w,
                            double *__restrict__ hcur)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if(k >= nsec)
    return;
  const int j = perm[slist[k]];
  hcur[k] = type[j] == 0 ? hsml[j] : 0.1 * w->linkl;   // fof.c:1454-1457
}

// fof_find_nearest_dmparticle_evaluate (fof.c:1672-1776) for one secondary per thread; hcur < 0: done
__global__ void k_fof_nearest(int nsec, const int *__restrict__ slist, int nelem, const int4 *__restrict__ lk,
                              const double4 *__restrict__ cl, const double *__restrict__ sx,
                              const double *__restrict__ sy, const double *__restrict__ sz,
                              const int *__restrict__ sflag, const int *__restrict__ sid, BoxK b,
                              double *__restrict__ hcur, int *__restrict__ slabel, int *__restrict__ left)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if(k >= nsec)
    return;
  const double h = hcur[k];
  if(h < 0)
    return;
  const int s = slist[k];
  const double px = sx[s], py = sy[s], pz = sz[s];
  const double h2 = h * h;
  double best = 1.0e30 * 1.0e30;
  int bestid = INT_MAX, bestq = -1;
  d_ngb_walk_thread<FOF_NEAR_LEAF>(GravElems{lk, cl}, nelem, px, py, pz, h, b, [&](int q) {
    if(sflag[q] != 1)
      return;
    const double dx = d_wrap(px - sx[q], b), dy = d_wrap(py - sy[q], b), dz = d_wrap(pz - sz[q], b);
    const double r2 = dx * dx + dy * dy + dz * dz;
    if(!(r2 < h2))
      return;
    const int qid = sid[q];
    if(r2 < best || (r2 == best && qid < bestid))
      {
        best = r2;
        bestid = qid;
        bestq = q;
      }
  });
  if(bestq >= 0)
    {
      slabel[s] = slabel[bestq];   // (a primary's label: final before the first round)
      hcur[k] = -1.0;
    }
  else
    {
      hcur[k] = 2.0 * h;   // fof.c:1625
      atomicAdd(left, 1);
    }
}

__global__ void k_fof_keys(int n, const int *__restrict__ perm, const int *__restrict__ slabel,
                           const int *__restrict__ sid, int *__restrict__ label, unsigned long long *__restrict__ key,
                           int *__restrict__ val)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if(p >= n)
    return;
  const int j = perm[p];
  label[j] = slabel[p];
  // signed order of (label, ID) as an unsigned key
  key[j] = ((unsigned long long) ((unsigned int) slabel[p] ^ 0x80000000u) << 32) | ((unsigned int) sid[p] ^ 0x80000000u);
  val[j] = j;
}

__global__ void k_fof_heads(int n, const unsigned long long *__restrict__ skey, int *__restrict__ head)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if(k < n)
    head[k] = (k == 0 || (skey[k] >> 32) != (skey[k - 1] >> 32)) ? 1 : 0;
}

// segof = exclusive sum of head: for a head its segment, else (segment + 1)
__global__ void k_fof_segstart(int n, const int *__restrict__ head, int *__restrict__ segof, int *__restrict__ segstart,
                               FofWords *w)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if(k >= n)
    return;
  const int s = segof[k] + head[k] - 1;
  segof[k] = s;
  if(head[k])
    segstart[s] = k;
  if(k == n - 1)
    {
      segstart[s + 1] = n;
      w->nseg = s + 1;
    }
}

__global__ void k_fof_groupkeys(const int *__restrict__ segstart, const unsigned long long *__restrict__ skey,
                                int minlen, unsigned long long *__restrict__ gkey, int *__restrict__ gval,
                                int *__restrict__ glen, FofWords *w)
{
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if(s >= w->nseg)
    return;
  const int len = segstart[s + 1] - segstart[s];
  const bool keep = len >= minlen;
  const unsigned int lab = (unsigned int) (skey[segstart[s]] >> 32);   // the label, sign bit flipped
  // Len descending, MinID ascending; a group that is not kept goes behind all kept ones
  gkey[s] = keep ? (((unsigned long long) (0xFFFFFFFEu - (unsigned int) len) << 32) | lab) : ~0ull;
  gval[s] = s;
  glen[s] = len;
  if(keep)
    {
      atomicAdd(&w->ngroups, 1);
      atomicAdd(&w->nids, (unsigned long long) len);
      atomicMax(&w->largest, len);
    }
}

// in the groups' order r: the segment's GrNr and the Len of the kept ones (0 behind them) for the scan
__global__ void k_fof_rank(const int *__restrict__ gorder, const int *__restrict__ glen, int *__restrict__ grnr,
                           int *__restrict__ rlen, const FofWords *w)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if(r >= w->nseg)
    return;
  const int s = gorder[r];
  const bool kept = r < w->ngroups;
  grnr[s] = kept ? r : -1;
  rlen[r] = kept ? glen[s] : 0;
}

__global__ void k_fof_members(int n, const int *__restrict__ sval, const unsigned long long *__restrict__ skey,
                              const int *__restrict__ segof, const int *__restrict__ segstart,
                              const int *__restrict__ grnr, const int *__restrict__ goff, int *__restrict__ pgrnr,
                              int *__restrict__ ids)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if(k >= n)
    return;
  const int s = segof[k];
  const int g = grnr[s];
  pgrnr[sval[k]] = g;
  if(g >= 0)
    ids[goff[g] + (k - segstart[s])] = (int) ((unsigned int) skey[k] ^ 0x80000000u);
}

// fof_compute_group_properties / fof_finish_group_properties (fof.c:900-974, 1081-1119): one wavefront per kept
// group.  Lane l adds members l, l + 64, ... of the (GrNr, ID)-sorted list in that order; the butterflies of
// d_wave_sum_f64 combine the 64 partial sums in a fixed order.
__global__ void __launch_bounds__(64)
k_fof_props(const int *__restrict__ gorder, const int *__restrict__ segstart, const int *__restrict__ goff,
            const int *__restrict__ sval, const unsigned long long *__restrict__ skey, int n, int ngas,
            const double *__restrict__ pos, const double *__restrict__ vel, const double *__restrict__ mass,
            const int *__restrict__ type, const double *__restrict__ dens, BoxK b, ghip_fof_group *__restrict__ out)
{
  const int r = blockIdx.x, lane = threadIdx.x;
  const int s = gorder[r];
  const int k0 = segstart[s], len = segstart[s + 1] - k0;
  const int jref = sval[k0];   // the member that carries MinID: the list is sorted by ID within the group
  const double rx = pos[jref], ry = pos[(size_t) n + jref], rz = pos[2 * (size_t) n + jref];
  double mt[6] = {0, 0, 0, 0, 0, 0}, cm[3] = {0, 0, 0}, mv[3] = {0, 0, 0};
  int lt[6] = {0, 0, 0, 0, 0, 0};
  double maxd = 0;
  int imax = INT_MAX;
  for(int k = k0 + lane; k < k0 + len; k += 64)
    {
      const int j = sval[k];
      const int ty = type[j];
      const double m = mass[j];
      for(int t = 0; t < 6; t++)
        if(ty == t)
          {
            lt[t]++;
            mt[t] += m;
          }
      double x = pos[j], y = pos[(size_t) n + j], z = pos[2 * (size_t) n + j];
      if(b.periodic)
        {
          x = d_fof_periodic(x - rx, b);   // fof.c:968
          y = d_fof_periodic(y - ry, b);
          z = d_fof_periodic(z - rz, b);
        }
      cm[0] += m * x;
      cm[1] += m * y;
      cm[2] += m * z;
      mv[0] += m * vel[j];
      mv[1] += m * vel[(size_t) n + j];
      mv[2] += m * vel[2 * (size_t) n + j];
      if(ty == 0 && j < ngas)
        {
          const double d = dens[j];
          if(d > maxd || (d == maxd && d > 0 && j < imax))   // fof.c:955 starts from MaxDens = 0
            {
              maxd = d;
              imax = j;
            }
        }
    }
  double Mass = 0;
  ghip_fof_group G;
  for(int t = 0; t < 6; t++)
    {
      G.MassType[t] = d_wave_sum_f64(mt[t]);
      G.LenType[t] = d_fof_sum_i32(lt[t]);
    }
  for(int t = 0; t < 6; t++)
    Mass += G.MassType[t];
  for(int c = 0; c < 3; c++)
    {
      cm[c] = d_wave_sum_f64(cm[c]);
      mv[c] = d_wave_sum_f64(mv[c]);
    }
  const double dmax = d_wave_max_f64(maxd);
  const int ibest = d_wave_min_i32((maxd == dmax && dmax > 0) ? imax : INT_MAX);
  if(lane != 0)
    return;
  G.Len = len;
  G.Offset = goff[r];
  G.MinID = (int) ((unsigned int) (skey[k0] >> 32) ^ 0x80000000u);
  G.GrNr = r;
  G.Mass = Mass;
  const double ref[3] = {rx, ry, rz};
  for(int c = 0; c < 3; c++)
    {
      double x = cm[c] / Mass;
      if(b.periodic)
        {
          x += ref[c];   // fof.c:1096, fof_periodic_wrap (fof.c:2283-2290): about the reference position, into the box
          while(x >= b.boxsize)
            x -= b.boxsize;
          while(x < 0)
            x += b.boxsize;
        }
      G.CM[c] = x;
      G.Vel[c] = mv[c] / Mass;
    }
  G.MaxDens = dmax > 0 ? dmax : 0;
  G.index_maxdens = dmax > 0 ? ibest : -1;
  // (the record was cleared before the launch, so its padding is zero: two calls give the same bytes)
  ghip_fof_group *o = out + r;
  o->Len = G.Len;
  o->Offset = G.Offset;
  o->MinID = G.MinID;
  o->GrNr = G.GrNr;
  for(int t = 0; t < 6; t++)
    {
      o->LenType[t] = G.LenType[t];
      o->MassType[t] = G.MassType[t];
    }
  o->Mass = G.Mass;
  for(int c = 0; c < 3; c++)
    {
      o->CM[c] = G.CM[c];
      o->Vel[c] = G.Vel[c];
    }
  o->MaxDens = G.MaxDens;
  o->index_maxdens = G.index_maxdens;
}

static int fof_events(ghip_ctx *ctx)
{
  for(int i = 0; i < 5; i++)
    if(!ctx->fof.ev[i])
      HIPCHK(hipEventCreate(&ctx->fof.ev[i]));
  return GHIP_OK;
}

static int fof_read_words(ghip_ctx *ctx, FofWords *h)
{
  HIPCHK(hipMemcpyAsync(h, ctx->fof.words.p, sizeof(FofWords), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  return GHIP_OK;
}

extern "C" size_t ghip_fof_params_size(void) { return sizeof(ghip_fof_params); }
extern "C" size_t ghip_fof_group_size(void) { return sizeof(ghip_fof_group); }

extern "C" int ghip_fof(ghip_ctx *ctx, const ghip_fof_params *p, ghip_fof_result *out)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !p || !out)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_fof: NULL argument");
  FofState &F = ctx->fof;
  F.n = -1;
  F.dd = false;
  if(ctx->dd.on || ctx->shard_n > 1)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_fof: not on a multi-GPU shard: groups that span shards need an exchange "
                     "of labels between the shards, which the collective form does (GHIP_DD_GLOBAL_QUANTITIES begun "
                     "with walk = GHIP_FOF_FORM and a ghip_dd_fof_args)");
  if(!ctx->gt.built)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_fof: call ghip_tree_build first (the groups are found on the gravity "
                     "tree of the current positions)");
  if(!ctx->id_given)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_fof: the ID field was never set (ghip_set_field(GHIP_F_ID)): groups are "
                     "labelled with their smallest ID");
  if((p->primary_types & 63) == 0)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_fof: primary_types selects no particle type");
  if(p->LinkL != p->LinkL || (p->LinkL <= 0 && !(p->linklength > 0 && p->rhodm > 0)))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_fof: LinkL <= 0 asks for the LINKLENGTH rule, which needs linklength > 0 "
                     "and rhodm > 0");
  if(p->periodic && !(p->BoxSize > 0))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_fof: a periodic box needs BoxSize > 0");
  GCHK(ghip_tree_verify(ctx));
  TreeDev &t = ctx->gt;
  const int n = ctx->n;
  if(t.n != n || n <= 0)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_fof: the gravity tree holds %d sources, the context %d particles", t.n, n);
  hipStream_t st = ctx->stream;
  GCHK(fof_events(ctx));
  const BoxK b = make_box(p->BoxSize, p->periodic);
  const int pmask = p->primary_types & 63, smask = p->secondary_types & 63;
  const int minlen = p->group_min_len > 1 ? p->group_min_len : 1;
  const size_t n4 = (size_t) n * 4, n8 = (size_t) n * 8;
  for(DevBuf *d : {&F.sid, &F.sflag, &F.parent, &F.rootmin, &F.slabel, &F.plist, &F.slist, &F.label, &F.val,
                   &F.sval, &F.head, &F.segof, &F.gval, &F.gorder, &F.glen, &F.goff, &F.grnr, &F.pgrnr, &F.ids})
    GCHK(ghip_ensure(ctx, *d, n4));
  GCHK(ghip_ensure(ctx, F.segstart, n4 + 4));
  for(DevBuf *d : {&F.key, &F.skey, &F.gkey, &F.gskey})
    GCHK(ghip_ensure(ctx, *d, n8));
  GCHK(ghip_ensure(ctx, F.words, sizeof(FofWords)));
  FofWords *w = P<FofWords>(F.words);
  HIPCHK(hipMemsetAsync(w, 0, sizeof(FofWords), st));
  const int nb = cdiv(n, 256);
  const int *perm = P<int>(t.perm), *type = P<int>(ctx->f[GHIP_F_TYPE]);
  const double *sx = P<double>(ctx->sx), *sy = P<double>(ctx->sy), *sz = P<double>(ctx->sz);
  const int4 *lk = P<int4>(t.lk);
  const double4 *cl = P<double4>(t.cl);

  // ---- who is what; the two lists (head and segof serve as the flag arrays here) ----
  k_fof_classify<<<nb, 256, 0, st>>>(n, perm, type, P<int>(ctx->f[GHIP_F_ID]), pmask, smask, P<int>(F.sid),
                                     P<int>(F.sflag), P<int>(F.parent), P<int>(F.rootmin), P<int>(F.slabel), P<int>(F.head),
                                     P<int>(F.segof));
  HIPCHK(hipGetLastError());
  GCHK(ghip_select_flagged(ctx, nullptr, P<int>(F.head), P<int>(F.plist), &w->nprim, n, st));
  GCHK(ghip_select_flagged(ctx, nullptr, P<int>(F.segof), P<int>(F.slist), &w->nsec, n, st));
  double linkl = p->LinkL;
  if(!(linkl > 0))
    {
      GCHK(ghip_ensure(ctx, F.part, (size_t) nb * 8));
      k_fof_mass_blocks<<<nb, FOF_RED_BLOCK, 0, st>>>(n, type, P<double>(ctx->f[GHIP_F_MASS]), pmask, P<double>(F.part));
      k_fof_linkl<<<1, FOF_RED_BLOCK, 0, st>>>(nb, P<double>(F.part), p->linklength, p->rhodm, w);
      HIPCHK(hipGetLastError());
    }
  FofWords hw;
  GCHK(fof_read_words(ctx, &hw));
  const int nprim = hw.nprim, nsec = hw.nsec;
  if(nprim < 0 || nsec < 0 || nprim + nsec > n)
    return ghip_fail(ctx, GHIP_EDEVICE, "ghip_fof: the selection gave %d primaries and %d secondaries of %d", nprim, nsec, n);
  if(nprim == 0)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_fof: no particle has a primary type (mask %d)", pmask);
  if(!(linkl > 0))
    {
      linkl = hw.linkl;
      if(!(linkl > 0) || linkl > DBL_MAX)
        return ghip_fail(ctx, GHIP_EINVAL, "ghip_fof: the LINKLENGTH rule gave LinkL = %g (mass of the primaries %g)",
                         linkl, hw.masstot);
    }
  else
    {
      hw.linkl = linkl;
      HIPCHK(hipMemcpyAsync(&w->linkl, &hw.linkl, 8, hipMemcpyHostToDevice, st));
    }

  // ---- linking ----
  HIPCHK(hipEventRecord(F.ev[0], st));
  k_fof_link<<<cdiv(nprim, 64), 64, 0, st>>>(nprim, P<int>(F.plist), t.nelem, lk, cl, sx, sy, sz, P<int>(F.sflag),
                                             linkl, b, P<int>(F.parent));
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(F.ev[1], st));
  k_fof_flatten<<<nb, 256, 0, st>>>(n, P<int>(F.sflag), P<int>(F.sid), P<int>(F.parent), P<int>(F.rootmin));
  k_fof_label<<<nb, 256, 0, st>>>(n, P<int>(F.sflag), P<int>(F.parent), P<int>(F.rootmin), P<int>(F.slabel));
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(F.ev[2], st));

  // ---- secondaries ----
  int iter = 0;
  if(nsec > 0)
    {
      GCHK(ghip_ensure(ctx, F.hcur, (size_t) nsec * 8));
      k_fof_hinit<<<cdiv(nsec, 256), 256, 0, st>>>(nsec, P<int>(F.slist), perm, type, P<double>(ctx->f[GHIP_F_HSML]), w,
                                                  P<double>(F.hcur));
      for(;;)
        {
          HIPCHK(hipMemsetAsync(&w->left, 0, 4, st));
          k_fof_nearest<<<cdiv(nsec, 64), 64, 0, st>>>(nsec, P<int>(F.slist), t.nelem, lk, cl, sx, sy, sz,
                                                       P<int>(F.sflag), P<int>(F.sid), b, P<double>(F.hcur),
                                                       P<int>(F.slabel), &w->left);
          HIPCHK(hipGetLastError());
          int left = 0;
          HIPCHK(hipMemcpyAsync(&left, &w->left, 4, hipMemcpyDeviceToHost, st));
          HIPCHK(ghip_stream_sync(ctx, st));
          if(left == 0)
            break;
          iter++;   // fof.c:1638-1653
          if(iter > p->MaxIter)
            return ghip_fail(ctx, GHIP_ENOCONV, "ghip_fof: failed to converge in fof-nearest: %d particles of a "
                             "secondary type found no primary after %d doublings (endrun(1159))", left, iter - 1);
        }
    }
  HIPCHK(hipEventRecord(F.ev[3], st));

  // ---- catalogue ----
  k_fof_keys<<<nb, 256, 0, st>>>(n, perm, P<int>(F.slabel), P<int>(F.sid), P<int>(F.label),
                                 P<unsigned long long>(F.key), P<int>(F.val));
  HIPCHK(hipGetLastError());
  GCHK((ghip_sort_pairs<unsigned long long, int>(ctx, P<unsigned long long>(F.key), P<unsigned long long>(F.skey),
                                                 P<int>(F.val), P<int>(F.sval), n, 64, st)));
  k_fof_heads<<<nb, 256, 0, st>>>(n, P<unsigned long long>(F.skey), P<int>(F.head));
  HIPCHK(hipGetLastError());
  GCHK(ghip_scan<int>(ctx, P<int>(F.head), P<int>(F.segof), n, st));
  k_fof_segstart<<<nb, 256, 0, st>>>(n, P<int>(F.head), P<int>(F.segof), P<int>(F.segstart), w);
  // (the number of segments stays on the device: the kernels over segments are launched for n and read it there)
  k_fof_groupkeys<<<nb, 256, 0, st>>>(P<int>(F.segstart), P<unsigned long long>(F.skey), minlen,
                                      P<unsigned long long>(F.gkey), P<int>(F.gval), P<int>(F.glen), w);
  HIPCHK(hipGetLastError());
  GCHK(fof_read_words(ctx, &hw));
  const int nseg = hw.nseg, ng = hw.ngroups;
  if(nseg < 1 || nseg > n || ng < 0 || ng > nseg || hw.nids > (unsigned long long) n)
    return ghip_fail(ctx, GHIP_EDEVICE, "ghip_fof: %d groups of %d candidates with %llu members of %d particles", ng,
                     nseg, hw.nids, n);
  GCHK((ghip_sort_pairs<unsigned long long, int>(ctx, P<unsigned long long>(F.gkey), P<unsigned long long>(F.gskey),
                                                 P<int>(F.gval), P<int>(F.gorder), nseg, 64, st)));
  // head is free again: the Len of the groups in their order, for the scan that gives Offset
  k_fof_rank<<<cdiv(nseg, 256), 256, 0, st>>>(P<int>(F.gorder), P<int>(F.glen), P<int>(F.grnr), P<int>(F.head), w);
  HIPCHK(hipGetLastError());
  GCHK(ghip_scan<int>(ctx, P<int>(F.head), P<int>(F.goff), nseg, st));
  k_fof_members<<<nb, 256, 0, st>>>(n, P<int>(F.sval), P<unsigned long long>(F.skey), P<int>(F.segof),
                                    P<int>(F.segstart), P<int>(F.grnr), P<int>(F.goff), P<int>(F.pgrnr),
                                    P<int>(F.ids));
  HIPCHK(hipGetLastError());
  if(ng > 0)
    {
      GCHK(ghip_ensure(ctx, F.groups, (size_t) ng * sizeof(ghip_fof_group)));
      HIPCHK(hipMemsetAsync(F.groups.p, 0, (size_t) ng * sizeof(ghip_fof_group), st));
      k_fof_props<<<ng, 64, 0, st>>>(P<int>(F.gorder), P<int>(F.segstart), P<int>(F.goff), P<int>(F.sval),
                                     P<unsigned long long>(F.skey), n, ctx->ngas, P<double>(ctx->f[GHIP_F_POS]),
                                     P<double>(ctx->f[GHIP_F_VEL]), P<double>(ctx->f[GHIP_F_MASS]), type,
                                     P<double>(ctx->f[GHIP_F_DENSITY]), b, P<ghip_fof_group>(F.groups));
      HIPCHK(hipGetLastError());
    }
  HIPCHK(hipEventRecord(F.ev[4], st));
  HIPCHK(ghip_stream_sync(ctx, st));
  for(int i = 0; i < 4; i++)
    {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, F.ev[i], F.ev[i + 1]));
      F.ms[i] = ms;
    }
  GCHK(ghip_check_device_errors(ctx));
  F.n = n;
  F.ngroups = ng;
  F.nids = (long long) hw.nids;
  out->Ngroups = ng;
  out->Nids = F.nids;
  out->largest = hw.largest;
  out->LinkL = linkl;
  out->nearest_iterations = iter;
  return GHIP_OK;
}

static int fof_have(ghip_ctx *ctx, const char *who)
{
  if(ctx->fof.n < 0 || ctx->fof.n != ctx->n)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: no catalogue: the last ghip_fof of this particle set did not succeed", who);
  return GHIP_OK;
}

extern "C" int ghip_fof_get_groups(ghip_ctx *ctx, ghip_fof_group *groups)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx)
    return GHIP_EINVAL;
  GCHK(fof_have(ctx, "ghip_fof_get_groups"));
  if(ctx->fof.ngroups == 0)
    return GHIP_OK;
  if(!groups)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_fof_get_groups: NULL argument");
  HIPCHK(hipMemcpyAsync(groups, ctx->fof.groups.p, (size_t) ctx->fof.ngroups * sizeof(ghip_fof_group),
                        hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  return GHIP_OK;
}

extern "C" int ghip_fof_get_ids(ghip_ctx *ctx, int *ids)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx)
    return GHIP_EINVAL;
  GCHK(fof_have(ctx, "ghip_fof_get_ids"));
  if(ctx->fof.nids == 0)
    return GHIP_OK;
  if(!ids)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_fof_get_ids: NULL argument");
  HIPCHK(hipMemcpyAsync(ids, ctx->fof.ids.p, (size_t) ctx->fof.nids * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  return GHIP_OK;
}

extern "C" int ghip_fof_get_labels(ghip_ctx *ctx, int *minid, int *grnr)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx)
    return GHIP_EINVAL;
  GCHK(fof_have(ctx, "ghip_fof_get_labels"));
  const size_t bytes = (size_t) ctx->n * 4;
  if(bytes == 0)
    return GHIP_OK;   // (a shard without particles after the collective form)
  if(minid)
    HIPCHK(hipMemcpyAsync(minid, ctx->fof.label.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  if(grnr)
    HIPCHK(hipMemcpyAsync(grnr, ctx->fof.pgrnr.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  return GHIP_OK;
}

extern "C" int ghip_fof_get_timing(ghip_ctx *ctx, double ms[4])
{
  if(!ctx || !ms)
    return GHIP_EINVAL;
  GCHK(fof_have(ctx, "ghip_fof_get_timing"));
  for(int i = 0; i < 4; i++)
    ms[i] = ctx->fof.ms[i];
  return GHIP_OK;
}

extern "C" int ghip_fof_get_maxdens_task(ghip_ctx *ctx, int *task)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx)
    return GHIP_EINVAL;
  GCHK(fof_have(ctx, "ghip_fof_get_maxdens_task"));
  const int ng = ctx->fof.ngroups;
  if(ng == 0)
    return GHIP_OK;
  if(!task)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_fof_get_maxdens_task: NULL argument");
  if(ctx->fof.dd)
    {
      HIPCHK(hipMemcpyAsync(task, ctx->fof.task.p, (size_t) ng * 4, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ghip_stream_sync(ctx, ctx->stream));
      return GHIP_OK;
    }
  std::vector<ghip_fof_group> g((size_t) ng);
  HIPCHK(hipMemcpyAsync(g.data(), ctx->fof.groups.p, (size_t) ng * sizeof(ghip_fof_group), hipMemcpyDeviceToHost,
                        ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  for(int r = 0; r < ng; r++)
    task[r] = g[r].index_maxdens >= 0 ? 0 : -1;
  return GHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// The groups of all shards (DESIGN.md 4.17 "On shards"): GHIP_DD_GLOBAL_QUANTITIES begun with walk = GHIP_FOF_FORM.
// The reference's multi-rank fof.c is the specification: labels are the pair (MinID, MinIDTask) (fof.c:159-192),
// cross links are repeated until link_across_tot == 0 (fof.c:416-583), secondaries are exported (fof.c:1434-1776),
// partial group records go to MinIDTask and are combined about FirstPos (fof.c:977-1119).  Phases, each ending in
// one of the two pending exchanges:
//   CLASSIFY   own primaries / secondaries of the merged tree (imports are neither)      -> all-gather {mass, counts}
//   LINK       LinkL from the sums in rank order; k_fof_link over the own primaries; group boxes  -> all-gather
//   BORDER     primaries within LinkL of another shard's boxes, (x, y, z, label)          -> all-to-all-v
//   CROSS      imports behind the tree's sources in the union-find, k_fof_dd_link_import; roots and their labels
//   LABEL_*    labels along the same lists (all-to-all-v), integer atomicMin on the root, "did any fall"
//              (one-word all-gather), repeated until nobody's did
//   SEC_*      per round: own search, queries (x, y, z, h) to the shards whose boxes the sphere reaches
//              (all-to-all-v), answers (r2, ID, label) back along the same routes (all-to-all-v), the smallest
//              (r2, ID) wins, h doubles where no shard found anything, "how many are left" (one-word all-gather)
//   CAT_*      local (label, ID) sort and segments; each segment asks its MinIDTask for the group's FirstPos and gets
//              it back (two all-to-all-v of 8 and 24 bytes: the reference shifts each partial centre of mass as a
//              whole, fof.c:1062-1066, which differs from the one-GPU sum where a group is longer than half the box;
//              summed about one position the result does not depend on the decomposition); a partial record per
//              segment to its MinIDTask (all-to-all-v, the owner's own among them at its rank's place); the owner
//              adds them in rank order, drops the short groups; the kept records reach every shard as an all-to-all-v whose send block is the same for
//              every destination; one sort, one scan, a look-up of GrNr by MinID
// ---------------------------------------------------------------------------------------------
int ghip_dd_fof_groups(ghip_ctx *ctx, const int *plist, int nprim);   // ghip_dd.hip
int ghip_dd_fof_status(ghip_ctx *ctx, const char *what);
int ghip_dd_fof_select(ghip_ctx *ctx, int nitem, const int *items, const double *hs, double h0, double boxsize,
                       int periodic, DevBuf &mask, DevBuf &list, int *scount, int *soff, int *total);
int ghip_dd_select_ranks(ghip_ctx *ctx, int n, const unsigned long long *mask, DevBuf &list, int *scount, int *soff,
                         int *total);

#define FOF_NOLABEL (~0ULL)
#define FOF_FAR (1.0e30 * 1.0e30)

struct FofBorder   // an exported primary; a secondary's query carries h in place of the label
{
  double x, y, z;
  union
  {
    unsigned long long lab;
    double h;
  };
};

struct FofAnswer
{
  double r2;
  long long id;
  unsigned long long lab;
};

struct FofPart   // a segment's share of struct group_properties (fof.c:900-974), sums about its own FirstPos
{
  unsigned long long lab;
  int Len, src;
  int LenType[6];
  double MassType[6];
  double cm[3], mv[3], first[3];
  double maxdens;
  int imax, pad;
};

struct FofKept
{
  ghip_fof_group g;
  int task, pad;
};

__device__ __forceinline__ unsigned long long d_fof_word(int id, int task)
{
  return ((unsigned long long) ((unsigned int) id ^ 0x80000000u) << 32) | (unsigned int) task;
}
__device__ __forceinline__ int d_fof_word_id(unsigned long long w) { return (int) ((unsigned int) (w >> 32) ^ 0x80000000u); }

// k_fof_classify on the merged tree: sources with perm >= n (imported particles and pruned nodes) are neither kind
__global__ void k_fof_dd_classify(int nt, int n, const int *__restrict__ perm, const int *__restrict__ type,
                                  const int *__restrict__ id, int pmask, int smask, int rank, int *__restrict__ sid,
                                  int *__restrict__ sflag, int *__restrict__ parent, int *__restrict__ slabel,
                                  unsigned long long *__restrict__ plab, int *__restrict__ isprim,
                                  int *__restrict__ issec)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if(p >= nt)
    return;
  const int j = perm[p];
  parent[p] = p;
  if(j >= n)
    {
      sid[p] = INT_MAX;
      slabel[p] = INT_MAX;
      sflag[p] = 0;
      isprim[p] = 0;
      issec[p] = 0;
      plab[p] = FOF_NOLABEL;
      return;
    }
  const int ty = type[j];
  const bool inrange = (unsigned int) ty < 6u;
  const bool prim = inrange && ((pmask >> ty) & 1);
  const bool sec = inrange && !prim && ((smask >> ty) & 1);
  sid[p] = id[j];
  slabel[p] = id[j];
  sflag[p] = prim ? 1 : (sec ? 2 : 0);
  isprim[p] = prim;
  issec[p] = sec;
  plab[p] = d_fof_word(id[j], rank);
}

__global__ void k_fof_dd_pack_border(int nrec, const int *__restrict__ list, const double *__restrict__ sx,
                                     const double *__restrict__ sy, const double *__restrict__ sz,
                                     const unsigned long long *__restrict__ plab, FofBorder *__restrict__ out)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nrec)
    return;
  const int s = list[a];
  FofBorder r;
  r.x = sx[s];
  r.y = sy[s];
  r.z = sz[s];
  r.lab = plab[s];
  out[a] = r;
}

__global__ void k_fof_dd_extend(int nt, int nimp, int *__restrict__ parent)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a < nimp)
    parent[nt + a] = nt + a;
}

// Imported primary a is element nt + a of the union-find.  One thread walks the own tree for it and unites it with
// every own primary at r2 <= LinkL^2: the pair test of k_fof_link (d_wrap is odd, so both shards of a pair compute
// the same r2 from the same two positions and decide alike).
__global__ void __launch_bounds__(64)
k_fof_dd_link_import(int nimp, const FofBorder *__restrict__ imp, int nt, int nelem, const int4 *__restrict__ lk,
                     const double4 *__restrict__ cl, const double *__restrict__ sx, const double *__restrict__ sy,
                     const double *__restrict__ sz, const int *__restrict__ sflag, double linkl, BoxK b,
                     int *__restrict__ parent)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nimp)
    return;
  const double px = imp[a].x, py = imp[a].y, pz = imp[a].z;
  const double l2 = linkl * linkl;
  d_ngb_walk_thread<FOF_NEAR_LEAF>(GravElems{lk, cl}, nelem, px, py, pz, linkl, b, [&](int q) {
    if(sflag[q] != 1)
      return;
    const double dx = d_wrap(px - sx[q], b), dy = d_wrap(py - sy[q], b), dz = d_wrap(pz - sz[q], b);
    const double r2 = dx * dx + dy * dy + dz * dz;
    if(!(r2 > l2))
      d_fof_union(parent, nt + a, q);
  });
}

// parent = root for the own primaries and the imports; the label of a root: the smallest word of its own primaries
// (integer atomicMin; rlab starts as FOF_NOLABEL everywhere)
__global__ void k_fof_dd_flatten(int nt, int ntot, const int *__restrict__ sflag,
                                 const unsigned long long *__restrict__ plab, int *parent,
                                 unsigned long long *__restrict__ rlab)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if(p >= ntot || (p < nt && sflag[p] != 1))
    return;
  int r = p, q;
  while((q = d_fof_load(parent + r)) != r)
    r = q;
  __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if(p < nt)
    atomicMin(rlab + r, plab[p]);
}

__global__ void k_fof_dd_label_send(int nrec, const int *__restrict__ list, const int *__restrict__ parent,
                                    const unsigned long long *__restrict__ rlab, unsigned long long *__restrict__ out)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a < nrec)
    out[a] = rlab[parent[list[a]]];
}

// the label round: the root of import a takes the sender's label if that is lower (fof.c:475, 686)
__global__ void k_fof_dd_label_round(int nimp, int nt, const int *__restrict__ parent,
                                     const unsigned long long *__restrict__ in, unsigned long long *__restrict__ rlab,
                                     int *__restrict__ changed)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nimp)
    return;
  const int r = parent[nt + a];
  if(r >= nt)
    return;   // linked to no own primary: nobody reads this root
  const unsigned long long v = in[a];
  if(v < atomicMin(rlab + r, v))
    atomicOr(changed, 1);
}

__global__ void k_fof_dd_final_labels(int nt, const int *__restrict__ sflag, const int *__restrict__ parent,
                                      const unsigned long long *__restrict__ rlab, int *__restrict__ slabel,
                                      unsigned long long *__restrict__ plab)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if(p >= nt || sflag[p] != 1)
    return;
  const unsigned long long w = rlab[parent[p]];
  plab[p] = w;
  slabel[p] = d_fof_word_id(w);
}

__global__ void k_fof_dd_hinit(int nsec, const int *__restrict__ slist, const int *__restrict__ perm,
                               const int *__restrict__ type, const double *__restrict__ hsml, double linkl,
                               double *__restrict__ hs)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if(k >= nsec)
    return;
  const int s = slist[k];
  const int j = perm[s];
  hs[s] = type[j] == 0 ? hsml[j] : 0.1 * linkl;   // fof.c:1454-1457
}

// the nearest own primary with r2 < h^2 of the point (px, py, pz): the search of k_fof_nearest
__device__ __forceinline__ FofAnswer d_fof_dd_nearest(double px, double py, double pz, double h, int nelem,
                                                      const int4 *__restrict__ lk, const double4 *__restrict__ cl,
                                                      const double *__restrict__ sx, const double *__restrict__ sy,
                                                      const double *__restrict__ sz, const int *__restrict__ sflag,
                                                      const int *__restrict__ sid,
                                                      const unsigned long long *__restrict__ plab, BoxK b)
{
  const double h2 = h * h;
  double best = FOF_FAR;
  int bestid = INT_MAX, bestq = -1;
  d_ngb_walk_thread<FOF_NEAR_LEAF>(GravElems{lk, cl}, nelem, px, py, pz, h, b, [&](int q) {
    if(sflag[q] != 1)
      return;
    const double dx = d_wrap(px - sx[q], b), dy = d_wrap(py - sy[q], b), dz = d_wrap(pz - sz[q], b);
    const double r2 = dx * dx + dy * dy + dz * dz;
    if(!(r2 < h2))
      return;
    const int qid = sid[q];
    if(r2 < best || (r2 == best && qid < bestid))
      {
        best = r2;
        bestid = qid;
        bestq = q;
      }
  });
  FofAnswer A;
  A.r2 = best;
  A.id = bestid;
  A.lab = bestq >= 0 ? plab[bestq] : FOF_NOLABEL;
  return A;
}

// per round, the unsettled secondaries against the own tree: the candidate (r2, ID, label) by tree index
__global__ void __launch_bounds__(64)
k_fof_dd_nearest_own(int nsec, const int *__restrict__ slist, int nelem, const int4 *__restrict__ lk,
                     const double4 *__restrict__ cl, const double *__restrict__ sx, const double *__restrict__ sy,
                     const double *__restrict__ sz, const int *__restrict__ sflag, const int *__restrict__ sid,
                     const unsigned long long *__restrict__ plab, BoxK b, const double *__restrict__ hs,
                     double *__restrict__ cr2, int *__restrict__ cid, unsigned long long *__restrict__ clab)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if(k >= nsec)
    return;
  const int s = slist[k];
  const double h = hs[s];
  if(h < 0)
    return;
  const FofAnswer A = d_fof_dd_nearest(sx[s], sy[s], sz[s], h, nelem, lk, cl, sx, sy, sz, sflag, sid, plab, b);
  cr2[s] = A.r2;
  cid[s] = (int) A.id;
  clab[s] = A.lab;
}

__global__ void k_fof_dd_pack_query(int nrec, const int *__restrict__ list, const double *__restrict__ sx,
                                    const double *__restrict__ sy, const double *__restrict__ sz,
                                    const double *__restrict__ hs, FofBorder *__restrict__ out)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nrec)
    return;
  const int s = list[a];
  FofBorder r;
  r.x = sx[s];
  r.y = sy[s];
  r.z = sz[s];
  r.h = hs[s];
  out[a] = r;
}

// the remote answer: another shard's secondary against this shard's primaries
__global__ void __launch_bounds__(64)
k_fof_dd_answer(int nq, const FofBorder *__restrict__ q, int nelem, const int4 *__restrict__ lk,
                const double4 *__restrict__ cl, const double *__restrict__ sx, const double *__restrict__ sy,
                const double *__restrict__ sz, const int *__restrict__ sflag, const int *__restrict__ sid,
                const unsigned long long *__restrict__ plab, BoxK b, FofAnswer *__restrict__ out)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nq)
    return;
  out[a] = d_fof_dd_nearest(q[a].x, q[a].y, q[a].z, q[a].h, nelem, lk, cl, sx, sy, sz, sflag, sid, plab, b);
}

// home takes the smallest r2, ties to the smaller ID (one destination's answers per launch: no two threads share s)
__global__ void k_fof_dd_merge(int nrec, const int *__restrict__ list, const FofAnswer *__restrict__ ans,
                               double *__restrict__ cr2, int *__restrict__ cid, unsigned long long *__restrict__ clab)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nrec)
    return;
  const FofAnswer A = ans[a];
  if(A.lab == FOF_NOLABEL)
    return;
  const int s = list[a];
  if(A.r2 < cr2[s] || (A.r2 == cr2[s] && (int) A.id < cid[s]))
    {
      cr2[s] = A.r2;
      cid[s] = (int) A.id;
      clab[s] = A.lab;
    }
}

__global__ void k_fof_dd_settle(int nsec, const int *__restrict__ slist, const unsigned long long *__restrict__ clab,
                                double *__restrict__ hs, int *__restrict__ slabel, unsigned long long *__restrict__ plab,
                                int *__restrict__ left)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if(k >= nsec)
    return;
  const int s = slist[k];
  const double h = hs[s];
  if(h < 0)
    return;
  const unsigned long long w = clab[s];
  if(w != FOF_NOLABEL)
    {
      plab[s] = w;
      slabel[s] = d_fof_word_id(w);
      hs[s] = -1.0;
    }
  else
    {
      hs[s] = 2.0 * h;   // fof.c:1625: no shard found anything
      atomicAdd(left, 1);
    }
}

// k_fof_keys on the merged tree (imports have no host index), with the label word in host order
__global__ void k_fof_dd_keys(int nt, int n, const int *__restrict__ perm, const int *__restrict__ slabel,
                              const int *__restrict__ sid, const unsigned long long *__restrict__ plab,
                              int *__restrict__ label, unsigned long long *__restrict__ key, int *__restrict__ val,
                              unsigned long long *__restrict__ plabh)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if(p >= nt)
    return;
  const int j = perm[p];
  if(j >= n)
    return;
  label[j] = slabel[p];
  key[j] = ((unsigned long long) ((unsigned int) slabel[p] ^ 0x80000000u) << 32) | ((unsigned int) sid[p] ^ 0x80000000u);
  val[j] = j;
  plabh[j] = plab[p];
}

__global__ void k_fof_dd_segmask(int nseg, const int *__restrict__ segstart, const int *__restrict__ sval,
                                 const unsigned long long *__restrict__ plabh, int nranks,
                                 unsigned long long *__restrict__ smask)
{
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if(s >= nseg)
    return;
  const unsigned int task = (unsigned int) plabh[sval[segstart[s]]];
  smask[s] = task < (unsigned int) nranks ? 1ULL << task : 0ULL;
}

__global__ void k_fof_dd_seg_requests(int nseg, const int *__restrict__ seglist, const int *__restrict__ segstart,
                                      const int *__restrict__ sval, const unsigned long long *__restrict__ plabh,
                                      unsigned long long *__restrict__ out)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a < nseg)
    out[a] = plabh[sval[segstart[seglist[a]]]];
}

// the owner's answer to "about which position is group `lab` summed": FirstPos, the position of its own member with
// the smallest ID (the segments are in label order: a binary search); a label it does not hold is counted
__global__ void k_fof_dd_refpos(int nreq, const unsigned long long *__restrict__ req, int nseg,
                                const int *__restrict__ segstart, const int *__restrict__ sval,
                                const unsigned long long *__restrict__ skey, int n, const double *__restrict__ pos,
                                double *__restrict__ out, int *__restrict__ missing)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nreq)
    return;
  const unsigned int lab = (unsigned int) (req[a] >> 32);
  int lo = 0, hi = nseg;
  while(lo < hi)
    {
      const int mid = (lo + hi) >> 1;
      if((unsigned int) (skey[segstart[mid]] >> 32) < lab)
        lo = mid + 1;
      else
        hi = mid;
    }
  if(lo < nseg && (unsigned int) (skey[segstart[lo]] >> 32) == lab)
    {
      const int j = sval[segstart[lo]];
      out[3 * (size_t) a] = pos[j];
      out[3 * (size_t) a + 1] = pos[(size_t) n + j];
      out[3 * (size_t) a + 2] = pos[2 * (size_t) n + j];
    }
  else
    {
      out[3 * (size_t) a] = out[3 * (size_t) a + 1] = out[3 * (size_t) a + 2] = 0;
      atomicAdd(missing, 1);
    }
}

// One wavefront per local segment, in the order its owner's list names them: the sums of k_fof_props about the
// group's FirstPos as its owner gave it (refpos, in list order), so that every member of a group -- wherever it is
// resident -- is wrapped about the same position, as on one GPU.  The record was cleared before the launch.
__global__ void __launch_bounds__(64)
k_fof_dd_partial(const int *__restrict__ seglist, const int *__restrict__ segstart, const int *__restrict__ sval,
                 const unsigned long long *__restrict__ plabh, const double *__restrict__ refpos, int n, int ngas,
                 int me, const double *__restrict__ pos, const double *__restrict__ vel,
                 const double *__restrict__ mass, const int *__restrict__ type, const double *__restrict__ dens,
                 BoxK b, FofPart *__restrict__ out)
{
  const int a = blockIdx.x, lane = threadIdx.x;
  const int s = seglist[a];
  const int k0 = segstart[s], len = segstart[s + 1] - k0;
  const int jref = sval[k0];
  const double rx = refpos[3 * (size_t) a], ry = refpos[3 * (size_t) a + 1], rz = refpos[3 * (size_t) a + 2];
  double mt[6] = {0, 0, 0, 0, 0, 0}, cm[3] = {0, 0, 0}, mv[3] = {0, 0, 0};
  int lt[6] = {0, 0, 0, 0, 0, 0};
  double maxd = 0;
  int imax = INT_MAX;
  for(int k = k0 + lane; k < k0 + len; k += 64)
    {
      const int j = sval[k];
      const int ty = type[j];
      const double m = mass[j];
      for(int t = 0; t < 6; t++)
        if(ty == t)
          {
            lt[t]++;
            mt[t] += m;
          }
      double x = pos[j], y = pos[(size_t) n + j], z = pos[2 * (size_t) n + j];
      if(b.periodic)
        {
          x = d_fof_periodic(x - rx, b);
          y = d_fof_periodic(y - ry, b);
          z = d_fof_periodic(z - rz, b);
        }
      cm[0] += m * x;
      cm[1] += m * y;
      cm[2] += m * z;
      mv[0] += m * vel[j];
      mv[1] += m * vel[(size_t) n + j];
      mv[2] += m * vel[2 * (size_t) n + j];
      if(ty == 0 && j < ngas && dens)   // (no GHIP_F_DENSITY on this shard: no densest member)
        {
          const double d = dens[j];
          if(d > maxd || (d == maxd && d > 0 && j < imax))
            {
              maxd = d;
              imax = j;
            }
        }
    }
  for(int t = 0; t < 6; t++)
    {
      mt[t] = d_wave_sum_f64(mt[t]);
      lt[t] = d_fof_sum_i32(lt[t]);
    }
  for(int c = 0; c < 3; c++)
    {
      cm[c] = d_wave_sum_f64(cm[c]);
      mv[c] = d_wave_sum_f64(mv[c]);
    }
  const double dmax = d_wave_max_f64(maxd);
  const int ibest = d_wave_min_i32((maxd == dmax && dmax > 0) ? imax : INT_MAX);
  if(lane != 0)
    return;
  FofPart *o = out + a;
  o->lab = plabh[jref];
  o->Len = len;
  o->src = me;
  for(int t = 0; t < 6; t++)
    {
      o->LenType[t] = lt[t];
      o->MassType[t] = mt[t];
    }
  for(int c = 0; c < 3; c++)
    {
      o->cm[c] = cm[c];
      o->mv[c] = mv[c];
    }
  o->first[0] = rx;
  o->first[1] = ry;
  o->first[2] = rz;
  o->maxdens = dmax > 0 ? dmax : 0;
  o->imax = dmax > 0 ? ibest : -1;
}

// the partials an owner received: (MinID, arrival slot) -- arrival is source-rank major, so this is rank order
__global__ void k_fof_dd_partkeys(int nrec, const FofPart *__restrict__ rec, unsigned long long *__restrict__ key,
                                  int *__restrict__ val)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nrec)
    return;
  key[a] = (rec[a].lab & 0xFFFFFFFF00000000ULL) | (unsigned int) a;
  val[a] = a;
}

// One thread per owned group: its partials rank by rank in ascending order, the owner's own at its rank's place
// (fof.c:1044-1075).  All of them were summed about the owner's FirstPos, so the shift of fof.c:1062-1066,
// nearest(CM_p / M_p + FirstPos_p - FirstPos), moves nothing and the sums are added as they are; then
// fof_finish_group_properties (fof.c:1081-1119).  MaxDens:
// ties to the lower rank (a later partial replaces only when larger), within a rank to the smaller index.
// The record was cleared before the launch.
__global__ void k_fof_dd_combine(int nown, const int *__restrict__ segstart, const int *__restrict__ psval,
                                 const FofPart *__restrict__ rec, int me, int minlen, BoxK b,
                                 FofKept *__restrict__ out, int *__restrict__ keep)
{
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if(g >= nown)
    return;
  const int k0 = segstart[g], k1 = segstart[g + 1];
  int io = psval[k0];
  for(int k = k0; k < k1; k++)
    if(rec[psval[k]].src == me)
      io = psval[k];
  const double fx[3] = {rec[io].first[0], rec[io].first[1], rec[io].first[2]};
  ghip_fof_group G;
  G.Len = 0;
  for(int t = 0; t < 6; t++)
    {
      G.LenType[t] = 0;
      G.MassType[t] = 0;
    }
  double cm[3] = {0, 0, 0}, mv[3] = {0, 0, 0}, maxd = 0;
  int imax = -1, task = -1;
  for(int k = k0; k < k1; k++)
    {
      const FofPart &R = rec[psval[k]];
      G.Len += R.Len;
      for(int t = 0; t < 6; t++)
        {
          G.LenType[t] += R.LenType[t];
          G.MassType[t] += R.MassType[t];
        }
      for(int c = 0; c < 3; c++)
        {
          mv[c] += R.mv[c];
          cm[c] += R.cm[c];
        }
      if(R.maxdens > maxd)
        {
          maxd = R.maxdens;
          imax = R.imax;
          task = R.src;
        }
    }
  double Mass = 0;
  for(int t = 0; t < 6; t++)
    Mass += G.MassType[t];
  FofKept *o = out + g;
  o->g.Len = G.Len;
  o->g.MinID = d_fof_word_id(rec[io].lab);
  for(int t = 0; t < 6; t++)
    {
      o->g.LenType[t] = G.LenType[t];
      o->g.MassType[t] = G.MassType[t];
    }
  o->g.Mass = Mass;
  for(int c = 0; c < 3; c++)
    {
      double x = cm[c] / Mass;
      if(b.periodic)
        {
          x += fx[c];
          while(x >= b.boxsize)
            x -= b.boxsize;
          while(x < 0)
            x += b.boxsize;
        }
      o->g.CM[c] = x;
      o->g.Vel[c] = mv[c] / Mass;
    }
  o->g.MaxDens = maxd;
  o->g.index_maxdens = imax;
  o->task = task;
  keep[g] = G.Len >= minlen ? 1 : 0;
}

__global__ void k_fof_dd_gather_kept(int nk, const int *__restrict__ klist, const FofKept *__restrict__ own,
                                     FofKept *__restrict__ out)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a < nk)
    out[a] = own[klist[a]];
}

// the kept groups of all shards: Len descending, MinID ascending (the key of k_fof_groupkeys)
__global__ void k_fof_dd_orderkeys(int ng, const FofKept *__restrict__ all, unsigned long long *__restrict__ gkey,
                                   int *__restrict__ gval)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= ng)
    return;
  gkey[a] = ((unsigned long long) (0xFFFFFFFEu - (unsigned int) all[a].g.Len) << 32) |
            ((unsigned int) all[a].g.MinID ^ 0x80000000u);
  gval[a] = a;
}

__global__ void k_fof_dd_lens(int ng, const int *__restrict__ gorder, const FofKept *__restrict__ all,
                              int *__restrict__ rlen)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if(r < ng)
    rlen[r] = all[gorder[r]].g.Len;
}

// the catalogue in its order (the records were cleared before the launch), the tasks, and (MinID, GrNr) for the look-up
__global__ void k_fof_dd_catalogue(int ng, const int *__restrict__ gorder, const int *__restrict__ goff,
                                   const FofKept *__restrict__ all, ghip_fof_group *__restrict__ out,
                                   int *__restrict__ task, unsigned int *__restrict__ mkey, int *__restrict__ mval)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if(r >= ng)
    return;
  const FofKept &K = all[gorder[r]];
  ghip_fof_group *o = out + r;
  o->Len = K.g.Len;
  o->Offset = goff[r];
  o->MinID = K.g.MinID;
  o->GrNr = r;
  for(int t = 0; t < 6; t++)
    {
      o->LenType[t] = K.g.LenType[t];
      o->MassType[t] = K.g.MassType[t];
    }
  o->Mass = K.g.Mass;
  for(int c = 0; c < 3; c++)
    {
      o->CM[c] = K.g.CM[c];
      o->Vel[c] = K.g.Vel[c];
    }
  o->MaxDens = K.g.MaxDens;
  o->index_maxdens = K.g.index_maxdens;
  task[r] = K.task;
  mkey[r] = (unsigned int) K.g.MinID ^ 0x80000000u;
  mval[r] = r;
}

// GrNr of the own particles from a look-up by MinID (k: the local (label, ID) order); the (GrNr, ID) key of a member
__global__ void k_fof_dd_members(int n, const int *__restrict__ sval, const unsigned long long *__restrict__ skey,
                                 int ng, const unsigned int *__restrict__ msk, const int *__restrict__ msv,
                                 int *__restrict__ pgrnr, unsigned long long *__restrict__ key2,
                                 unsigned long long *__restrict__ nkept)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if(k >= n)
    return;
  const unsigned int lab = (unsigned int) (skey[k] >> 32);
  int lo = 0, hi = ng;
  while(lo < hi)
    {
      const int mid = (lo + hi) >> 1;
      if(msk[mid] < lab)
        lo = mid + 1;
      else
        hi = mid;
    }
  const int g = (lo < ng && msk[lo] == lab) ? msv[lo] : -1;
  pgrnr[sval[k]] = g;
  key2[k] = g >= 0 ? (((unsigned long long) (unsigned int) g << 32) | (unsigned int) skey[k]) : ~0ULL;
  if(g >= 0)
    atomicAdd(nkept, 1ULL);
}

__global__ void k_fof_dd_ids(int nk, const unsigned long long *__restrict__ skey2, int *__restrict__ ids)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if(k < nk)
    ids[k] = (int) ((unsigned int) skey2[k] ^ 0x80000000u);
}

extern "C" size_t ghip_dd_fof_args_size(void) { return sizeof(ghip_dd_fof_args); }

int ghip_dd_fof_begin(ghip_ctx *ctx, int, const void *params, int)
{
  GHIP_JOIN(ctx);
  const char *who = "GHIP_DD_GLOBAL_QUANTITIES (GHIP_FOF_FORM)";
  FofState &F = ctx->fof;
  F.a = *reinterpret_cast<const ghip_dd_fof_args *>(params);
  if(!F.a.p || !F.a.out)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: params (a ghip_dd_fof_args) needs p and out", who);
  F.p = *F.a.p;
  const ghip_fof_params *p = &F.p;
  if((p->primary_types & 63) == 0)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: primary_types selects no particle type", who);
  if(p->LinkL != p->LinkL || (p->LinkL <= 0 && !(p->linklength > 0 && p->rhodm > 0)))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: LinkL <= 0 asks for the LINKLENGTH rule, which needs linklength > 0 and "
                     "rhodm > 0", who);
  if(p->periodic && !(p->BoxSize > 0))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: a periodic box needs BoxSize > 0", who);
  if(!ctx->id_given && ctx->n > 0)   // (a shard without particles has no field to set)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: the ID field was never set (ghip_set_field(GHIP_F_ID)): groups are "
                     "labelled with their smallest ID", who);
  if(!ctx->gt.built && !ctx->dd.geom_kept)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: run GHIP_DD_GRAVITY of this step first (the groups are found on its "
                     "merged tree; none is built here)", who);
  if(ctx->dd.gt_is_pot)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: the tree in place is the one GHIP_DD_POTENTIAL built: run GHIP_DD_GRAVITY "
                     "first", who);
  F.n = -1;
  F.dd = false;
  if(F.a.counts)
    for(int k = 0; k < 8; k++)
      F.a.counts[k] = 0;
  return GHIP_OK;
}

// device time of a stage, exchanges excluded: tic before the kernels of a phase, toc behind them
static int fof_tic(ghip_ctx *ctx)
{
  HIPCHK(hipEventRecord(ctx->fof.ev[0], ctx->stream));
  return GHIP_OK;
}
static int fof_toc(ghip_ctx *ctx, int stage)
{
  HIPCHK(hipEventRecord(ctx->fof.ev[1], ctx->stream));
  HIPCHK(ghip_event_sync(ctx, ctx->fof.ev[1]));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->fof.ev[0], ctx->fof.ev[1]));
  ctx->fof.ms[stage] += ms;
  return GHIP_OK;
}

// a one-word all-gather: post, and read the shards' words in rank order
static int fof_post_word(ghip_ctx *ctx, unsigned long long v)
{
  FofState &F = ctx->fof;
  GCHK(ghip_ensure(ctx, F.word_own, 8));
  HIPCHK(hipMemcpyAsync(F.word_own.p, &v, 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));   // (`v` lives on this frame)
  ghip_dd_set_allgather(ctx->dd, F.word_own.p, 8, &F.word_all);
  return GHIP_OK;
}
static int fof_read_shard_words(ghip_ctx *ctx, unsigned long long *all)
{
  HIPCHK(hipMemcpyAsync(all, ctx->fof.word_all.p, (size_t) ctx->dd.nranks * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  return GHIP_OK;
}

enum
{
  FOF_CLASSIFY,
  FOF_LINK,
  FOF_BORDER,
  FOF_CROSS,
  FOF_LABEL_RECV,
  FOF_LABEL_CHECK,
  FOF_SEC_ANSWER,
  FOF_SEC_MERGE,
  FOF_SEC_CHECK,
  FOF_CAT_REFPOS,
  FOF_CAT_PARTIAL,
  FOF_CAT_COMBINE,
  FOF_CAT_ORDER
};

struct FofTree   // the merged tree as the kernels read it
{
  int nelem;
  const int4 *lk;
  const double4 *cl;
  const double *sx, *sy, *sz;
  const int *perm;
};
static FofTree fof_tree(ghip_ctx *ctx)
{
  const TreeDev &t = ctx->gt;
  const FofTree T = {t.nelem, P<int4>(t.lk), P<double4>(t.cl), P<double>(ctx->sx), P<double>(ctx->sy),
                     P<double>(ctx->sz), P<int>(t.perm)};
  return T;
}

// a label round's first half: the current label of each exported primary, along the lists of FOF_BORDER
static int fof_post_labels(ghip_ctx *ctx)
{
  FofState &F = ctx->fof;
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  GCHK(fof_tic(ctx));
  HIPCHK(hipMemsetAsync(&P<FofWords>(F.words)->changed, 0, 4, st));
  GCHK(ghip_ensure(ctx, F.lsend, (size_t) (F.nexp > 0 ? F.nexp : 1) * 8));
  if(F.nexp > 0)
    {
      k_fof_dd_label_send<<<cdiv(F.nexp, 256), 256, 0, st>>>(F.nexp, P<int>(F.xlist), P<int>(F.parent),
                                                            P<unsigned long long>(F.rlab),
                                                            P<unsigned long long>(F.lsend));
      HIPCHK(hipGetLastError());
    }
  GCHK(fof_toc(ctx, 1));
  ghip_dd_set_alltoallv(D, F.lsend.p, 8, F.x_scount, F.x_soff, &F.lrecv);
  D.phase = FOF_LABEL_RECV;
  return 1;
}

// a secondary round's first half: the own search, then the queries to the shards whose primaries a sphere reaches
static int fof_post_queries(ghip_ctx *ctx)
{
  FofState &F = ctx->fof;
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  const FofTree T = fof_tree(ctx);
  const BoxK b = make_box(F.p.BoxSize, F.p.periodic);
  GCHK(fof_tic(ctx));
  if(F.nsec > 0)
    {
      k_fof_dd_nearest_own<<<cdiv(F.nsec, 64), 64, 0, st>>>(
        F.nsec, P<int>(F.slist), T.nelem, T.lk, T.cl, T.sx, T.sy, T.sz, P<int>(F.sflag), P<int>(F.sid),
        P<unsigned long long>(F.plab), b, P<double>(F.hs), P<double>(F.cr2), P<int>(F.cid),
        P<unsigned long long>(F.clab));
      HIPCHK(hipGetLastError());
    }
  int total = 0;
  GCHK(ghip_dd_fof_select(ctx, F.nsec, P<int>(F.slist), P<double>(F.hs), 0.0, F.p.BoxSize, F.p.periodic, F.xmask,
                          F.qlist, F.q_scount, F.q_soff, &total));
  GCHK(ghip_ensure(ctx, F.qsend, (size_t) (total > 0 ? total : 1) * sizeof(FofBorder)));
  if(total > 0)
    {
      k_fof_dd_pack_query<<<cdiv(total, 256), 256, 0, st>>>(total, P<int>(F.qlist), T.sx, T.sy, T.sz, P<double>(F.hs),
                                                           P<FofBorder>(F.qsend));
      HIPCHK(hipGetLastError());
    }
  GCHK(fof_toc(ctx, 2));
  F.queries += total;
  ghip_dd_set_alltoallv(D, F.qsend.p, sizeof(FofBorder), F.q_scount, F.q_soff, &F.qrecv);
  D.phase = FOF_SEC_ANSWER;
  return 1;
}

// the catalogue's first part: local segments, and a question to the owner of each: about which position is it summed
static int fof_post_partials(ghip_ctx *ctx)
{
  FofState &F = ctx->fof;
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  const FofTree T = fof_tree(ctx);
  const BoxK b = make_box(F.p.BoxSize, F.p.periodic);
  const int n = ctx->n, nt = F.nt, P_ = D.nranks;
  FofWords *w = P<FofWords>(F.words);
  int *sc = F.p_scount, *so = F.p_soff;
  for(int r = 0; r < GHIP_MAXRANKS; r++)
    sc[r] = so[r] = 0;
  GCHK(fof_tic(ctx));
  F.nseg = 0;
  GCHK(ghip_ensure(ctx, F.rqsend, 8));
  if(n > 0)
    {
      const size_t n4 = (size_t) n * 4, n8 = (size_t) n * 8;
      for(DevBuf *d : {&F.label, &F.val, &F.sval, &F.head, &F.segof, &F.pgrnr, &F.ids})
        GCHK(ghip_ensure(ctx, *d, n4));
      GCHK(ghip_ensure(ctx, F.segstart, n4 + 4));
      for(DevBuf *d : {&F.key, &F.skey, &F.plabh, &F.smask, &F.key2, &F.skey2})
        GCHK(ghip_ensure(ctx, *d, n8));
      const int nb = cdiv(n, 256);
      k_fof_dd_keys<<<cdiv(nt, 256), 256, 0, st>>>(nt, n, T.perm, P<int>(F.slabel), P<int>(F.sid),
                                                   P<unsigned long long>(F.plab), P<int>(F.label),
                                                   P<unsigned long long>(F.key), P<int>(F.val),
                                                   P<unsigned long long>(F.plabh));
      HIPCHK(hipGetLastError());
      GCHK((ghip_sort_pairs<unsigned long long, int>(ctx, P<unsigned long long>(F.key), P<unsigned long long>(F.skey),
                                                     P<int>(F.val), P<int>(F.sval), n, 64, st)));
      k_fof_heads<<<nb, 256, 0, st>>>(n, P<unsigned long long>(F.skey), P<int>(F.head));
      HIPCHK(hipGetLastError());
      GCHK(ghip_scan<int>(ctx, P<int>(F.head), P<int>(F.segof), n, st));
      k_fof_segstart<<<nb, 256, 0, st>>>(n, P<int>(F.head), P<int>(F.segof), P<int>(F.segstart), w);
      HIPCHK(hipGetLastError());
      FofWords hw;
      GCHK(fof_read_words(ctx, &hw));
      const int nseg = hw.nseg;
      if(nseg < 1 || nseg > n)
        return ghip_fail(ctx, GHIP_EDEVICE, "ghip_dd fof: %d candidate groups of %d particles", nseg, n);
      F.nseg = nseg;
      k_fof_dd_segmask<<<cdiv(nseg, 256), 256, 0, st>>>(nseg, P<int>(F.segstart), P<int>(F.sval),
                                                       P<unsigned long long>(F.plabh), P_,
                                                       P<unsigned long long>(F.smask));
      HIPCHK(hipGetLastError());
      int total = 0;
      GCHK(ghip_dd_select_ranks(ctx, nseg, P<unsigned long long>(F.smask), F.seglist, sc, so, &total));
      if(total != nseg)
        return ghip_fail(ctx, GHIP_EDEVICE, "ghip_dd fof: %d of %d candidate groups have an owner among the %d "
                         "shards", total, nseg, P_);
      GCHK(ghip_ensure(ctx, F.rqsend, (size_t) nseg * 8));
      k_fof_dd_seg_requests<<<cdiv(nseg, 256), 256, 0, st>>>(nseg, P<int>(F.seglist), P<int>(F.segstart),
                                                            P<int>(F.sval), P<unsigned long long>(F.plabh),
                                                            P<unsigned long long>(F.rqsend));
      HIPCHK(hipGetLastError());
    }
  GCHK(fof_toc(ctx, 3));
  F.parts_sent = (long long) F.nseg - sc[D.rank];
  ghip_dd_set_alltoallv(D, F.rqsend.p, 8, sc, so, &F.rqrecv);
  D.phase = FOF_CAT_REFPOS;
  return 1;
}

// after the labels are final: the secondaries if any shard has one, else the catalogue
static int fof_after_labels(ghip_ctx *ctx)
{
  FofState &F = ctx->fof;
  hipStream_t st = ctx->stream;
  const FofTree T = fof_tree(ctx);
  const int nt = F.nt;
  GCHK(fof_tic(ctx));
  if(nt > 0)
    {
      k_fof_dd_final_labels<<<cdiv(nt, 256), 256, 0, st>>>(nt, P<int>(F.sflag), P<int>(F.parent),
                                                          P<unsigned long long>(F.rlab), P<int>(F.slabel),
                                                          P<unsigned long long>(F.plab));
      HIPCHK(hipGetLastError());
    }
  GCHK(fof_toc(ctx, 1));
  F.iter = 0;
  if(F.totsec == 0)
    return fof_post_partials(ctx);
  GCHK(fof_tic(ctx));
  const size_t t8 = (size_t) (nt > 0 ? nt : 1) * 8;
  for(DevBuf *d : {&F.hs, &F.cr2, &F.clab})
    GCHK(ghip_ensure(ctx, *d, t8));
  GCHK(ghip_ensure(ctx, F.cid, t8 / 2));
  if(F.nsec > 0)
    {
      k_fof_dd_hinit<<<cdiv(F.nsec, 256), 256, 0, st>>>(F.nsec, P<int>(F.slist), T.perm, P<int>(ctx->f[GHIP_F_TYPE]),
                                                       P<double>(ctx->f[GHIP_F_HSML]), F.linkl, P<double>(F.hs));
      HIPCHK(hipGetLastError());
    }
  GCHK(fof_toc(ctx, 2));
  return fof_post_queries(ctx);
}

int ghip_dd_fof_step(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  FofState &F = ctx->fof;
  const ghip_fof_params *p = &F.p;
  hipStream_t st = ctx->stream;
  const char *who = "GHIP_DD_GLOBAL_QUANTITIES (GHIP_FOF_FORM)";
  const int P_ = D.nranks, me = D.rank, n = ctx->n;
  const BoxK b = make_box(p->BoxSize, p->periodic);
  const int pmask = p->primary_types & 63, smask = p->secondary_types & 63;
  const int minlen = p->group_min_len > 1 ? p->group_min_len : 1;
  if(D.phase == FOF_CLASSIFY)
    {
      GCHK(ghip_tree_verify(ctx));
      GCHK(fof_events(ctx));
      const TreeDev &t = ctx->gt;
      const int nt = t.n;
      F.nt = nt;
      F.nprim = F.nsec = F.nimp = F.nexp = F.nseg = F.nown = F.nkept = F.iter = F.rounds = 0;
      F.queries = F.parts_sent = 0;
      for(int i = 0; i < 4; i++)
        F.ms[i] = 0;
      GCHK(ghip_ensure(ctx, F.words, sizeof(FofWords)));
      FofWords *w = P<FofWords>(F.words);
      HIPCHK(hipMemsetAsync(w, 0, sizeof(FofWords), st));
      bool bad = false;
      if(nt < n)
        bad = ghip_dd_hold(ctx, ghip_fail(ctx, GHIP_EINVAL, "%s: the gravity tree holds %d sources, the shard %d "
                                          "particles: run GHIP_DD_GRAVITY of this step first", who, nt, n));
      FofWords hw;
      memset(&hw, 0, sizeof(hw));
      if(!bad && nt > 0)
        {
          const size_t t4 = (size_t) nt * 4;
          for(DevBuf *d : {&F.sid, &F.sflag, &F.parent, &F.slabel, &F.plist, &F.slist, &F.head, &F.segof})
            GCHK(ghip_ensure(ctx, *d, t4));
          GCHK(ghip_ensure(ctx, F.plab, 2 * t4));
          const FofTree T = fof_tree(ctx);
          const int *type = P<int>(ctx->f[GHIP_F_TYPE]);
          k_fof_dd_classify<<<cdiv(nt, 256), 256, 0, st>>>(nt, n, T.perm, type, P<int>(ctx->f[GHIP_F_ID]), pmask, smask,
                                                          me, P<int>(F.sid), P<int>(F.sflag), P<int>(F.parent),
                                                          P<int>(F.slabel), P<unsigned long long>(F.plab),
                                                          P<int>(F.head), P<int>(F.segof));
          HIPCHK(hipGetLastError());
          GCHK(ghip_select_flagged(ctx, nullptr, P<int>(F.head), P<int>(F.plist), &w->nprim, nt, st));
          GCHK(ghip_select_flagged(ctx, nullptr, P<int>(F.segof), P<int>(F.slist), &w->nsec, nt, st));
          if(!(p->LinkL > 0) && n > 0)
            {
              const int nb = cdiv(n, FOF_RED_BLOCK);
              GCHK(ghip_ensure(ctx, F.part, (size_t) nb * 8));
              k_fof_mass_blocks<<<nb, FOF_RED_BLOCK, 0, st>>>(n, type, P<double>(ctx->f[GHIP_F_MASS]), pmask,
                                                              P<double>(F.part));
              k_fof_linkl<<<1, FOF_RED_BLOCK, 0, st>>>(nb, P<double>(F.part), p->linklength, p->rhodm, w);
              HIPCHK(hipGetLastError());
            }
          GCHK(fof_read_words(ctx, &hw));
          if(hw.nprim < 0 || hw.nsec < 0 || (long long) hw.nprim + hw.nsec > n)
            bad = ghip_dd_hold(ctx, ghip_fail(ctx, GHIP_EDEVICE, "%s: the selection gave %d primaries and %d "
                                              "secondaries of %d", who, hw.nprim, hw.nsec, n));
        }
      F.nprim = bad ? 0 : hw.nprim;
      F.nsec = bad ? 0 : hw.nsec;
      const double mine[4] = {hw.masstot, (double) F.nprim, (double) F.nsec, bad ? 1.0 : 0.0};
      GCHK(ghip_ensure(ctx, F.stat_own, sizeof(mine)));
      HIPCHK(hipMemcpyAsync(F.stat_own.p, mine, sizeof(mine), hipMemcpyHostToDevice, st));
      HIPCHK(ghip_stream_sync(ctx, st));   // (`mine` lives on this frame)
      ghip_dd_set_allgather(D, F.stat_own.p, sizeof(mine), &F.stat_all);
      D.phase = FOF_LINK;
      return 1;
    }
  if(D.phase == FOF_LINK)
    {
      double all[4 * GHIP_MAXRANKS];
      HIPCHK(hipMemcpyAsync(all, F.stat_all.p, (size_t) P_ * 32, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      double masstot = 0;
      long long np = 0, ns = 0;
      int failed = -1;
      for(int r = 0; r < P_; r++)   // in rank order: every shard computes the same LinkL bytes
        {
          masstot += all[4 * r];
          np += (long long) all[4 * r + 1];
          ns += (long long) all[4 * r + 2];
          if(all[4 * r + 3] != 0 && failed < 0)
            failed = r;
        }
      GCHK(ghip_dd_raise(ctx, failed, "%s: shard %d reported an error while it classified its particles (its own "
                         "message says what); every shard stops here", who, failed));
      F.totprim = np;
      F.totsec = ns;
      if(np == 0)
        return ghip_fail(ctx, GHIP_EINVAL, "%s: no particle of any shard has a primary type (mask %d)", who, pmask);
      double linkl = p->LinkL;
      if(!(linkl > 0))
        {
          linkl = p->linklength * pow(masstot / (double) np / p->rhodm, 1.0 / 3);   // fof.c:112-124
          if(!(linkl > 0) || linkl > DBL_MAX)
            return ghip_fail(ctx, GHIP_EINVAL, "%s: the LINKLENGTH rule gave LinkL = %g (mass of the primaries %g)",
                             who, linkl, masstot);
        }
      F.linkl = linkl;
      const FofTree T = fof_tree(ctx);
      if(F.nprim > 0)
        {
          GCHK(fof_tic(ctx));
          k_fof_link<<<cdiv(F.nprim, 64), 64, 0, st>>>(F.nprim, P<int>(F.plist), T.nelem, T.lk, T.cl, T.sx, T.sy, T.sz,
                                                       P<int>(F.sflag), linkl, b, P<int>(F.parent));
          HIPCHK(hipGetLastError());
          GCHK(fof_toc(ctx, 0));
        }
      D.phase = FOF_BORDER;
      return ghip_dd_fof_groups(ctx, P<int>(F.plist), F.nprim);
    }
  if(D.phase == FOF_BORDER)
    {
      GCHK(ghip_dd_fof_status(ctx, who));
      const FofTree T = fof_tree(ctx);
      int total = 0;
      GCHK(ghip_dd_fof_select(ctx, F.nprim, P<int>(F.plist), nullptr, F.linkl, p->BoxSize, p->periodic, F.xmask,
                              F.xlist, F.x_scount, F.x_soff, &total));
      F.nexp = total;
      GCHK(ghip_ensure(ctx, F.xsend, (size_t) (total > 0 ? total : 1) * sizeof(FofBorder)));
      if(total > 0)
        {
          k_fof_dd_pack_border<<<cdiv(total, 256), 256, 0, st>>>(total, P<int>(F.xlist), T.sx, T.sy, T.sz,
                                                                P<unsigned long long>(F.plab), P<FofBorder>(F.xsend));
          HIPCHK(hipGetLastError());
        }
      ghip_dd_set_alltoallv(D, F.xsend.p, sizeof(FofBorder), F.x_scount, F.x_soff, &F.xrecv);
      D.phase = FOF_CROSS;
      return 1;
    }
  if(D.phase == FOF_CROSS)
    {
      const FofTree T = fof_tree(ctx);
      const int nt = F.nt, nimp = D.x.rtotal, ntot = nt + nimp;
      F.nimp = nimp;
      for(int r = 0; r < P_; r++)
        F.x_rcount[r] = D.x.rcount[r];
      GCHK(fof_tic(ctx));
      if(nimp > 0)
        {
          // the union-find grows by the imports (parents are kept: a block that grows is a new block)
          GCHK(ghip_ensure(ctx, F.parent2, (size_t) ntot * 4));
          if(nt > 0)
            HIPCHK(hipMemcpyAsync(F.parent2.p, F.parent.p, (size_t) nt * 4, hipMemcpyDeviceToDevice, st));
          HIPCHK(ghip_stream_sync(ctx, st));
          F.parent.swap(F.parent2);
          k_fof_dd_extend<<<cdiv(nimp, 256), 256, 0, st>>>(nt, nimp, P<int>(F.parent));
          if(F.nprim > 0)
            k_fof_dd_link_import<<<cdiv(nimp, 64), 64, 0, st>>>(nimp, P<FofBorder>(F.xrecv), nt, T.nelem, T.lk, T.cl,
                                                               T.sx, T.sy, T.sz, P<int>(F.sflag), F.linkl, b,
                                                               P<int>(F.parent));
          HIPCHK(hipGetLastError());
        }
      GCHK(fof_toc(ctx, 0));
      GCHK(fof_tic(ctx));
      GCHK(ghip_ensure(ctx, F.rlab, (size_t) (ntot > 0 ? ntot : 1) * 8));
      if(ntot > 0)
        {
          HIPCHK(hipMemsetAsync(F.rlab.p, 0xFF, (size_t) ntot * 8, st));
          k_fof_dd_flatten<<<cdiv(ntot, 256), 256, 0, st>>>(nt, ntot, P<int>(F.sflag), P<unsigned long long>(F.plab),
                                                           P<int>(F.parent), P<unsigned long long>(F.rlab));
          HIPCHK(hipGetLastError());
        }
      GCHK(fof_toc(ctx, 1));
      return fof_post_labels(ctx);
    }
  if(D.phase == FOF_LABEL_RECV)
    {
      for(int r = 0; r < P_; r++)
        if(D.x.rcount[r] != F.x_rcount[r])
          return ghip_fail(ctx, GHIP_ECOMM, "%s: %d labels came from rank %d, %d primaries had come", who,
                           D.x.rcount[r], r, F.x_rcount[r]);
      int changed = 0;
      if(F.nimp > 0)
        {
          GCHK(fof_tic(ctx));
          FofWords *w = P<FofWords>(F.words);
          k_fof_dd_label_round<<<cdiv(F.nimp, 256), 256, 0, st>>>(F.nimp, F.nt, P<int>(F.parent),
                                                                 P<unsigned long long>(F.lrecv),
                                                                 P<unsigned long long>(F.rlab), &w->changed);
          HIPCHK(hipGetLastError());
          GCHK(fof_toc(ctx, 1));
          HIPCHK(hipMemcpyAsync(&changed, &w->changed, 4, hipMemcpyDeviceToHost, st));
          HIPCHK(ghip_stream_sync(ctx, st));
        }
      // one word: did a label fall here, and how many primaries this shard exports (the cap of the rounds)
      GCHK(fof_post_word(ctx, ((unsigned long long) F.nexp << 1) | (changed ? 1ULL : 0ULL)));
      D.phase = FOF_LABEL_CHECK;
      return 1;
    }
  if(D.phase == FOF_LABEL_CHECK)
    {
      unsigned long long all[GHIP_MAXRANKS];
      GCHK(fof_read_shard_words(ctx, all));
      long long totexp = 0;
      bool any = false;
      for(int r = 0; r < P_; r++)
        {
          totexp += (long long) (all[r] >> 1);
          any = any || (all[r] & 1ULL);
        }
      F.rounds++;
      if(!any)   // link_across_tot == 0 (fof.c:560-583)
        return fof_after_labels(ctx);
      if(F.rounds > totexp + 1)
        return ghip_fail(ctx, GHIP_EDEVICE, "%s: labels still fall after %d rounds with %lld exported primaries "
                         "(labels only fall: this cannot be)", who, F.rounds, totexp);
      return fof_post_labels(ctx);
    }
  if(D.phase == FOF_SEC_ANSWER)
    {
      const FofTree T = fof_tree(ctx);
      const int nq = D.x.rtotal;
      GCHK(fof_tic(ctx));
      GCHK(ghip_ensure(ctx, F.asend, (size_t) (nq > 0 ? nq : 1) * sizeof(FofAnswer)));
      if(nq > 0)
        {
          k_fof_dd_answer<<<cdiv(nq, 64), 64, 0, st>>>(nq, P<FofBorder>(F.qrecv), T.nelem, T.lk, T.cl, T.sx, T.sy, T.sz,
                                                      P<int>(F.sflag), P<int>(F.sid), P<unsigned long long>(F.plab), b,
                                                      P<FofAnswer>(F.asend));
          HIPCHK(hipGetLastError());
        }
      GCHK(fof_toc(ctx, 2));
      int sc[GHIP_MAXRANKS], so[GHIP_MAXRANKS];
      for(int r = 0; r < P_; r++)
        {
          sc[r] = D.x.rcount[r];
          so[r] = D.x.roff[r];
        }
      ghip_dd_set_alltoallv(D, F.asend.p, sizeof(FofAnswer), sc, so, &F.arecv);
      D.phase = FOF_SEC_MERGE;
      return 1;
    }
  if(D.phase == FOF_SEC_MERGE)
    {
      for(int r = 0; r < P_; r++)
        if(D.x.rcount[r] != (r == me ? 0 : F.q_scount[r]))
          return ghip_fail(ctx, GHIP_ECOMM, "%s: %d answers came back from rank %d, %d queries went there", who,
                           D.x.rcount[r], r, F.q_scount[r]);
      int left = 0;
      if(F.nsec > 0)
        {
          GCHK(fof_tic(ctx));
          FofWords *w = P<FofWords>(F.words);
          HIPCHK(hipMemsetAsync(&w->left, 0, 4, st));
          for(int r = 0; r < P_; r++)
            if(r != me && F.q_scount[r] > 0)
              k_fof_dd_merge<<<cdiv(F.q_scount[r], 256), 256, 0, st>>>(
                F.q_scount[r], P<int>(F.qlist) + F.q_soff[r], P<FofAnswer>(F.arecv) + D.x.roff[r], P<double>(F.cr2),
                P<int>(F.cid), P<unsigned long long>(F.clab));
          k_fof_dd_settle<<<cdiv(F.nsec, 256), 256, 0, st>>>(F.nsec, P<int>(F.slist), P<unsigned long long>(F.clab),
                                                            P<double>(F.hs), P<int>(F.slabel),
                                                            P<unsigned long long>(F.plab), &w->left);
          HIPCHK(hipGetLastError());
          GCHK(fof_toc(ctx, 2));
          HIPCHK(hipMemcpyAsync(&left, &w->left, 4, hipMemcpyDeviceToHost, st));
          HIPCHK(ghip_stream_sync(ctx, st));
        }
      GCHK(fof_post_word(ctx, (unsigned long long) left));
      D.phase = FOF_SEC_CHECK;
      return 1;
    }
  if(D.phase == FOF_SEC_CHECK)
    {
      unsigned long long all[GHIP_MAXRANKS];
      GCHK(fof_read_shard_words(ctx, all));
      long long left = 0;
      for(int r = 0; r < P_; r++)
        left += (long long) all[r];
      if(left == 0)
        return fof_post_partials(ctx);
      F.iter++;   // fof.c:1638-1653
      if(F.iter > p->MaxIter)
        return ghip_fail(ctx, GHIP_ENOCONV, "%s: failed to converge in fof-nearest: %lld particles of a secondary "
                         "type found no primary on any shard after %d doublings (endrun(1159))", who, left, F.iter - 1);
      return fof_post_queries(ctx);
    }
  if(D.phase == FOF_CAT_REFPOS)
    {
      // the owner answers with FirstPos of each group it was asked about, along the routes the questions came
      const int nreq = D.x.rtotal;
      FofWords *w = P<FofWords>(F.words);
      GCHK(fof_tic(ctx));
      GCHK(ghip_ensure(ctx, F.rpsend, (size_t) (nreq > 0 ? nreq : 1) * 24));
      int missing = 0;
      if(nreq > 0)
        {
          HIPCHK(hipMemsetAsync(&w->left, 0, 4, st));
          k_fof_dd_refpos<<<cdiv(nreq, 256), 256, 0, st>>>(nreq, P<unsigned long long>(F.rqrecv), F.nseg,
                                                          P<int>(F.segstart), P<int>(F.sval),
                                                          P<unsigned long long>(F.skey), n,
                                                          P<double>(ctx->f[GHIP_F_POS]), P<double>(F.rpsend), &w->left);
          HIPCHK(hipGetLastError());
          HIPCHK(hipMemcpyAsync(&missing, &w->left, 4, hipMemcpyDeviceToHost, st));
        }
      GCHK(fof_toc(ctx, 3));
      if(missing != 0)
        return ghip_fail(ctx, GHIP_EDEVICE, "%s: %d groups name this shard as MinIDTask, which holds no particle of "
                         "theirs", who, missing);
      int sc[GHIP_MAXRANKS], so[GHIP_MAXRANKS];
      for(int r = 0; r < P_; r++)
        {
          sc[r] = D.x.rcount[r];
          so[r] = D.x.roff[r];
        }
      ghip_dd_set_alltoallv(D, F.rpsend.p, 24, sc, so, &F.rprecv);
      D.phase = FOF_CAT_PARTIAL;
      return 1;
    }
  if(D.phase == FOF_CAT_PARTIAL)
    {
      // a partial record of each local segment to its owner, the owner's own among them
      for(int r = 0; r < P_; r++)
        if(D.x.rcount[r] != F.p_scount[r])
          return ghip_fail(ctx, GHIP_ECOMM, "%s: %d positions came back from rank %d, %d groups were asked about", who,
                           D.x.rcount[r], r, F.p_scount[r]);
      const int nseg = F.nseg;
      GCHK(fof_tic(ctx));
      GCHK(ghip_ensure(ctx, F.psend, (size_t) (nseg > 0 ? nseg : 1) * sizeof(FofPart)));
      if(nseg > 0)
        {
          HIPCHK(hipMemsetAsync(F.psend.p, 0, (size_t) nseg * sizeof(FofPart), st));
          k_fof_dd_partial<<<nseg, 64, 0, st>>>(P<int>(F.seglist), P<int>(F.segstart), P<int>(F.sval),
                                                P<unsigned long long>(F.plabh), P<double>(F.rprecv), n, ctx->ngas, me,
                                                P<double>(ctx->f[GHIP_F_POS]), P<double>(ctx->f[GHIP_F_VEL]),
                                                P<double>(ctx->f[GHIP_F_MASS]), P<int>(ctx->f[GHIP_F_TYPE]),
                                                P<double>(ctx->f[GHIP_F_DENSITY]), b, P<FofPart>(F.psend));
          HIPCHK(hipGetLastError());
        }
      GCHK(fof_toc(ctx, 3));
      ghip_dd_set_alltoallv(D, F.psend.p, sizeof(FofPart), F.p_scount, F.p_soff, &F.precv);
      D.phase = FOF_CAT_COMBINE;
      return 1;
    }
  if(D.phase == FOF_CAT_COMBINE)
    {
      const int nrec = D.x.rtotal;
      FofWords *w = P<FofWords>(F.words);
      int sc[GHIP_MAXRANKS], so[GHIP_MAXRANKS];
      GCHK(fof_tic(ctx));
      int nown = 0, nk = 0;
      GCHK(ghip_ensure(ctx, F.ksend, sizeof(FofKept)));
      if(nrec > 0)
        {
          const size_t r4 = (size_t) nrec * 4;
          for(DevBuf *d : {&F.pval, &F.psval, &F.phead, &F.psegof, &F.keep, &F.klist})
            GCHK(ghip_ensure(ctx, *d, r4));
          GCHK(ghip_ensure(ctx, F.psegstart, r4 + 4));
          for(DevBuf *d : {&F.pkey, &F.pskey})
            GCHK(ghip_ensure(ctx, *d, 2 * r4));
          const int nb = cdiv(nrec, 256);
          k_fof_dd_partkeys<<<nb, 256, 0, st>>>(nrec, P<FofPart>(F.precv), P<unsigned long long>(F.pkey), P<int>(F.pval));
          HIPCHK(hipGetLastError());
          GCHK((ghip_sort_pairs<unsigned long long, int>(ctx, P<unsigned long long>(F.pkey),
                                                         P<unsigned long long>(F.pskey), P<int>(F.pval),
                                                         P<int>(F.psval), nrec, 64, st)));
          k_fof_heads<<<nb, 256, 0, st>>>(nrec, P<unsigned long long>(F.pskey), P<int>(F.phead));
          HIPCHK(hipGetLastError());
          GCHK(ghip_scan<int>(ctx, P<int>(F.phead), P<int>(F.psegof), nrec, st));
          k_fof_segstart<<<nb, 256, 0, st>>>(nrec, P<int>(F.phead), P<int>(F.psegof), P<int>(F.psegstart), w);
          HIPCHK(hipGetLastError());
          FofWords hw;
          GCHK(fof_read_words(ctx, &hw));
          nown = hw.nseg;
          if(nown < 1 || nown > nrec)
            return ghip_fail(ctx, GHIP_EDEVICE, "ghip_dd fof: %d groups of %d partial records", nown, nrec);
          GCHK(ghip_ensure(ctx, F.own, (size_t) nown * sizeof(FofKept)));
          HIPCHK(hipMemsetAsync(F.own.p, 0, (size_t) nown * sizeof(FofKept), st));
          k_fof_dd_combine<<<cdiv(nown, 64), 64, 0, st>>>(nown, P<int>(F.psegstart), P<int>(F.psval),
                                                         P<FofPart>(F.precv), me, minlen, b, P<FofKept>(F.own),
                                                         P<int>(F.keep));
          HIPCHK(hipGetLastError());
          GCHK(ghip_select_flagged(ctx, nullptr, P<int>(F.keep), P<int>(F.klist), &w->ngroups, nown, st));
          GCHK(fof_read_words(ctx, &hw));
          nk = hw.ngroups;
          if(nk < 0 || nk > nown)
            return ghip_fail(ctx, GHIP_EDEVICE, "ghip_dd fof: %d kept of %d owned groups", nk, nown);
          if(nk > 0)
            {
              GCHK(ghip_ensure(ctx, F.ksend, (size_t) nk * sizeof(FofKept)));
              k_fof_dd_gather_kept<<<cdiv(nk, 256), 256, 0, st>>>(nk, P<int>(F.klist), P<FofKept>(F.own),
                                                                 P<FofKept>(F.ksend));
              HIPCHK(hipGetLastError());
            }
        }
      GCHK(fof_toc(ctx, 3));
      F.nown = nown;
      F.nkept = nk;
      // an all-gather of unequal blocks: the same block for every destination, this shard's own at its rank's place
      for(int r = 0; r < GHIP_MAXRANKS; r++)
        {
          sc[r] = r < P_ ? nk : 0;
          so[r] = 0;
        }
      ghip_dd_set_alltoallv(D, F.ksend.p, sizeof(FofKept), sc, so, &F.kall);
      D.phase = FOF_CAT_ORDER;
      return 1;
    }
  if(D.phase == FOF_CAT_ORDER)
    {
      const int ng = D.x.rtotal;
      FofWords *w = P<FofWords>(F.words);
      GCHK(fof_tic(ctx));
      ghip_fof_group gfirst, glast;
      memset(&gfirst, 0, sizeof(gfirst));
      memset(&glast, 0, sizeof(glast));
      GCHK(ghip_ensure(ctx, F.mkey, 4));
      GCHK(ghip_ensure(ctx, F.msk, 4));
      GCHK(ghip_ensure(ctx, F.msv, 4));
      if(ng > 0)
        {
          const size_t g4 = (size_t) ng * 4;
          for(DevBuf *d : {&F.gval, &F.gorder, &F.glen, &F.goff, &F.task, &F.mkey, &F.msk, &F.mval, &F.msv})
            GCHK(ghip_ensure(ctx, *d, g4));
          for(DevBuf *d : {&F.gkey, &F.gskey})
            GCHK(ghip_ensure(ctx, *d, 2 * g4));
          GCHK(ghip_ensure(ctx, F.groups, (size_t) ng * sizeof(ghip_fof_group)));
          const int nb = cdiv(ng, 256);
          k_fof_dd_orderkeys<<<nb, 256, 0, st>>>(ng, P<FofKept>(F.kall), P<unsigned long long>(F.gkey), P<int>(F.gval));
          HIPCHK(hipGetLastError());
          GCHK((ghip_sort_pairs<unsigned long long, int>(ctx, P<unsigned long long>(F.gkey),
                                                         P<unsigned long long>(F.gskey), P<int>(F.gval),
                                                         P<int>(F.gorder), ng, 64, st)));
          k_fof_dd_lens<<<nb, 256, 0, st>>>(ng, P<int>(F.gorder), P<FofKept>(F.kall), P<int>(F.glen));
          HIPCHK(hipGetLastError());
          GCHK(ghip_scan<int>(ctx, P<int>(F.glen), P<int>(F.goff), ng, st));
          HIPCHK(hipMemsetAsync(F.groups.p, 0, (size_t) ng * sizeof(ghip_fof_group), st));
          k_fof_dd_catalogue<<<nb, 256, 0, st>>>(ng, P<int>(F.gorder), P<int>(F.goff), P<FofKept>(F.kall),
                                                 P<ghip_fof_group>(F.groups), P<int>(F.task),
                                                 P<unsigned int>(F.mkey), P<int>(F.mval));
          HIPCHK(hipGetLastError());
          GCHK((ghip_sort_pairs<unsigned int, int>(ctx, P<unsigned int>(F.mkey), P<unsigned int>(F.msk), P<int>(F.mval),
                                                   P<int>(F.msv), ng, 32, st)));
          HIPCHK(hipMemcpyAsync(&gfirst, F.groups.p, sizeof(gfirst), hipMemcpyDeviceToHost, st));
          HIPCHK(hipMemcpyAsync(&glast, P<ghip_fof_group>(F.groups) + (ng - 1), sizeof(glast), hipMemcpyDeviceToHost, st));
        }
      long long nmine = 0;
      if(n > 0)
        {
          HIPCHK(hipMemsetAsync(&w->nids, 0, 8, st));
          k_fof_dd_members<<<cdiv(n, 256), 256, 0, st>>>(n, P<int>(F.sval), P<unsigned long long>(F.skey), ng,
                                                         P<unsigned int>(F.msk), P<int>(F.msv), P<int>(F.pgrnr),
                                                         P<unsigned long long>(F.key2), &w->nids);
          HIPCHK(hipGetLastError());
          GCHK(ghip_sort_keys(ctx, P<unsigned long long>(F.key2), P<unsigned long long>(F.skey2), n, 64, st));
          FofWords hw;
          GCHK(fof_read_words(ctx, &hw));
          nmine = (long long) hw.nids;
          if(nmine < 0 || nmine > n)
            return ghip_fail(ctx, GHIP_EDEVICE, "ghip_dd fof: %lld members of kept groups among %d particles", nmine, n);
          if(nmine > 0)
            {
              k_fof_dd_ids<<<cdiv(nmine, 256), 256, 0, st>>>((int) nmine, P<unsigned long long>(F.skey2), P<int>(F.ids));
              HIPCHK(hipGetLastError());
            }
        }
      GCHK(fof_toc(ctx, 3));
      HIPCHK(ghip_stream_sync(ctx, st));
      GCHK(ghip_check_device_errors(ctx));
      F.n = n;
      F.dd = true;
      F.ngroups = ng;
      F.nids = nmine;
      ghip_fof_result *out = F.a.out;
      out->Ngroups = ng;
      out->Nids = ng > 0 ? (long long) glast.Offset + glast.Len : 0;
      out->largest = ng > 0 ? gfirst.Len : 0;
      out->LinkL = F.linkl;
      out->nearest_iterations = F.iter;
      if(F.a.counts)
        {
          long long *c = F.a.counts;
          c[0] = nmine;
          c[1] = F.nexp;
          c[2] = F.nimp;
          c[3] = F.rounds;
          c[4] = F.queries;
          c[5] = F.parts_sent;
          c[6] = D.bytes_sent[D.op];
          c[7] = F.nkept;
        }
      return 0;
    }
  return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: the group finder has no phase %d", D.phase);
}
