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
  if(ctx->dd.on || ctx->shard_n > 1)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_fof: not on a multi-GPU shard: groups that span shards are not built "
                     "(they need an exchange of labels between the shards)");
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
