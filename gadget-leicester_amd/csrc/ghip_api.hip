// ghip_api.hip -- C-ABI entry points: context lifetime, the field table with ghip_set_field /
// ghip_get_field, the active list, tree build and dumps, run statistics.  (Whole P[] / SphP[] records
// move through ghip_records.hip.)
// See include/ghip.h for what each entry point replaces in the reference.
#include <cstdarg>

#include <atomic>
#include <dlfcn.h>
#include <mutex>

#include "ghip_internal.h"

// ---------------------------------------------------------------------------------------------
// Launch counter.  Every `kernel<<<...>>>` of this library -- its own kernels and the rocPRIM /
// hipCUB ones it calls -- ends in hipLaunchKernel.  The library carries a LOCAL definition of that
// symbol (the export map keeps it out of the dynamic symbol table, so nobody else's calls are
// touched) that counts and forwards to the runtime's.  bench.py reports launches per step from it.
// ---------------------------------------------------------------------------------------------
static std::atomic<long long> g_launches{0};
typedef hipError_t (*launch_fn)(const void *, dim3, dim3, void **, size_t, hipStream_t);
// Process-wide state, made once by the first ghip_create (process_init) and kept until the process
// ends: the runtime's hipLaunchKernel and the device error words.  Kernels are only launched on behalf
// of a context, so both exist wherever they are used.
static launch_fn g_real_launch = nullptr;
static int *g_errwords = nullptr;
static std::once_flag g_process_once;

static launch_fn find_real_launch(void)
{
  void *p = dlvsym(RTLD_NEXT, "hipLaunchKernel", "hip_4.2");
  if(!p)
    p = dlsym(RTLD_NEXT, "hipLaunchKernel");
  if(!p)
    {
      // the runtime this library is linked against, found through one of its other symbols
      Dl_info info;
      if(dladdr((void *) &hipMemsetAsync, &info) && info.dli_fname)
        {
          void *h = dlopen(info.dli_fname, RTLD_LAZY | RTLD_NOLOAD);
          if(h)
            p = dlsym(h, "hipLaunchKernel");
        }
    }
  return (launch_fn) p;
}
extern "C" hipError_t hipLaunchKernel(const void *function_address, dim3 numBlocks, dim3 dimBlocks,
                                      void **args, size_t sharedMemBytes, hipStream_t stream)
{
  if(!g_real_launch)
    return hipErrorNotInitialized;   // (no context was ever made)
  g_launches.fetch_add(1, std::memory_order_relaxed);
  return g_real_launch(function_address, numBlocks, dimBlocks, args, sharedMemBytes, stream);
}
long long ghip_launch_count(void) { return g_launches.load(std::memory_order_relaxed); }

// ---------------------------------------------------------------------------------------------
// Device memory: a DevBuf owns its block.  The bytes held are counted, so that a test can tell that
// a destroyed context has given everything back.
// ---------------------------------------------------------------------------------------------
static std::atomic<long long> g_device_bytes{0};
extern "C" long long ghip_device_bytes_in_use(void) { return g_device_bytes.load(std::memory_order_relaxed); }

hipError_t DevBuf::alloc(size_t bytes)
{
  hipError_t e = hipMalloc(&p, bytes);
  if(e != hipSuccess)
    {
      p = nullptr;
      return e;
    }
  cap = bytes;
  g_device_bytes.fetch_add((long long) bytes, std::memory_order_relaxed);
  return hipSuccess;
}

hipError_t DevBuf::release()
{
  hipError_t e = hipSuccess;
  if(p)
    {
      e = hipFree(p);
      g_device_bytes.fetch_sub((long long) cap, std::memory_order_relaxed);
    }
  p = nullptr;
  cap = 0;
  return e;
}

int ghip_fail(ghip_ctx *ctx, int code, const char *fmt, ...)
{
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if(ctx)
    ctx->err = buf;
  return code;
}

int ghip_ensure(ghip_ctx *ctx, DevBuf &b, size_t bytes)
{
  if(bytes == 0)
    bytes = 8;
  if(b.cap >= bytes)
    return GHIP_OK;
  // grow with slack so that per-step size jitter does not reallocate
  size_t want = bytes + bytes / 8 + 256;
  if(b.p)
    {
      // (nothing may still be using the old block: the walks of a gravity pair run on streams of
      // their own, and the host no longer waits for them at the end of every step)
      HIPCHK(ghip_stream_sync(ctx, ctx->stream));
      if(ctx->stream2)
        HIPCHK(ghip_stream_sync(ctx, ctx->stream2));
      if(ctx->stream3)
        HIPCHK(ghip_stream_sync(ctx, ctx->stream3));
      HIPCHK(b.release());
    }
  hipError_t e = b.alloc(want);
  if(e != hipSuccess)
    return ghip_fail(ctx, GHIP_ENOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
  return GHIP_OK;
}

int ghip_join_pair(ghip_ctx *ctx)
{
  if(ctx && ctx->grav_pending)
    {
      ctx->grav_pending = false;
      HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->evx[2], 0));
    }
  return GHIP_OK;
}

int ghip_join(ghip_ctx *ctx)
{
  // (first: a tree built without waiting for its sizes is verified -- and, if it turned out bad,
  // rebuilt with the gravity calls made since replayed -- before anything else relies on it)
  if(ctx)
    GCHK(ghip_tree_verify(ctx));
  GCHK(ghip_join_pair(ctx));
  if(!ctx)
    return GHIP_OK;
  GCHK(ghip_finish_gas_tree(ctx));
  return ghip_gas_verify(ctx);
}

int *ghip_errwords(void) { return g_errwords; }

static void process_init(void)
{
  g_real_launch = find_real_launch();
  void *p = nullptr;
  if(hipHostMalloc(&p, 256, hipHostMallocDefault) == hipSuccess)
    {
      memset(p, 0, 256);
      g_errwords = reinterpret_cast<int *>(p);
    }
}

// call after a stream synchronisation: has a kernel reported a broken invariant?
int ghip_check_device_errors(ghip_ctx *ctx)
{
  if(!ctx)
    return GHIP_OK;
  static const char *what[GHIP_ERRW_COUNT] = {
    "the wavefront plan of a gravity walk exceeded its grid (ghip_walk.h, k_plan_fill)",
    "a target had to open a pruned node of an imported (other shard's) tree: the locally "
    "essential tree was incomplete",
    "tree emission outside the element list, a malformed imported element (3), paths deeper than "
    "GHIP_TREE_MAXLEVEL (7: ghip_set_rnd_table), a particle outside its "
    "shard's key range (5: migrate first, or allow guests with ghip_dd_set_guests) or outside the domain cube (6: ghip_dd_set_domain with a fresh extent)",
    "a particle that passed the range check of the non-periodic mesh fell outside its lower octant (nothing was "
    "written for it): the region in force is inconsistent",
    "drift", "timestep", "", ""};
  for(int w = 0; w < GHIP_ERRW_COUNT; w++)
    {
      volatile int *e = ghip_errword(ctx, w);
      if(*e != 0)
        {
          int v = *e;
          *e = 0;
          // what an asynchronous ghip_drift / ghip_advance_timesteps would have returned itself
          if(w == GHIP_ERRW_DRIFT)
            return ghip_fail(ctx, GHIP_EINVAL, "ghip_drift: a particle is ahead of time1 (reference: "
                             "endrun(12), predict.c:148)");
          if(w == GHIP_ERRW_TIMESTEP)
            {
              ctx->timestep_endrun = v;
              return ghip_fail(ctx, GHIP_ETIMESTEP, "ghip_advance_timesteps: the reference stops here with "
                               "endrun(%d) (timestep.c:171/1082: 888, :1119: 818, :1233: 112313)", v);
            }
          return ghip_fail(ctx, GHIP_EDEVICE, "device invariant %d broken (%d): %s", w, v, what[w]);
        }
    }
  return GHIP_OK;
}

extern "C" const char *ghip_version(void)
{
  return "ghip 0.3 (gfx950)";
}

extern "C" int ghip_create(int device, ghip_ctx **out)
{
  if(!out)
    return GHIP_EINVAL;
  *out = nullptr;
  int ndev = 0;
  if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return GHIP_ENODEVICE;
  if(device < 0 || device >= ndev)
    return GHIP_ENODEVICE;
  std::call_once(g_process_once, process_init);
  if(!g_real_launch)
    {
      fprintf(stderr, "ghip_create: the HIP runtime's hipLaunchKernel was not found\n");
      return GHIP_EHIP;
    }
  if(!g_errwords)
    {
      fprintf(stderr, "ghip_create: the device error words could not be pinned\n");
      return GHIP_ENOMEM;
    }
  ghip_ctx *ctx = new(std::nothrow) ghip_ctx();
  if(!ctx)
    return GHIP_ENOMEM;
  ctx->device = device;
  memset(&ctx->stats, 0, sizeof(ctx->stats));
  // the main stream gets the highest priority, the two streams of a gravity pair the lowest: what
  // is enqueued underneath the walks (SPH phases, the deferred gas-tree work) consists of short
  // kernels that must not queue behind two chip-filling ones
  int prio_least = 0, prio_greatest = 0;
  if(hipSetDevice(device) != hipSuccess ||
     hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess ||
     hipStreamCreateWithPriority(&ctx->stream, hipStreamDefault, prio_greatest) != hipSuccess)
    {
      delete ctx;
      return GHIP_ENODEVICE;
    }
  for(int i = 0; i < 16; i++)
    if(hipEventCreate(&ctx->ev[i]) != hipSuccess)
      {
        delete ctx;
        return GHIP_EHIP;
      }
  ctx->evp = ctx->ev;
  if(hipEventCreateWithFlags(&ctx->ev_side, hipEventDisableTiming) != hipSuccess ||
     hipEventCreateWithFlags(&ctx->ev_sizes, hipEventDisableTiming) != hipSuccess ||
     hipEventCreateWithFlags(&ctx->ev_sizes_gas, hipEventDisableTiming) != hipSuccess)
    {
      delete ctx;
      return GHIP_EHIP;
    }
  ctx->tree_async_ok = !(getenv("GHIP_TREE_SYNC") && atoi(getenv("GHIP_TREE_SYNC")) == 1);
  if(hipStreamCreateWithPriority(&ctx->stream2, hipStreamDefault, prio_least) != hipSuccess ||
     hipStreamCreateWithPriority(&ctx->stream3, hipStreamDefault, prio_least) != hipSuccess)
    {
      delete ctx;
      return GHIP_EHIP;
    }
  for(int i = 0; i < 4; i++)
    if(hipEventCreateWithFlags(&ctx->evx[i], hipEventDisableTiming) != hipSuccess)
      {
        delete ctx;
        return GHIP_EHIP;
      }
  for(int i = 0; i < 2; i++)
    if(hipEventCreateWithFlags(&ctx->evt[i], hipEventDisableTiming) != hipSuccess)
      {
        delete ctx;
        return GHIP_EHIP;
      }
  // the scratch words start at zero (hipMalloc does not clear)
  if(ghip_ensure(ctx, ctx->words, sizeof(DevWords)) != GHIP_OK ||
     hipMemset(ctx->words.p, 0, ctx->words.cap) != hipSuccess)
    {
      delete ctx;
      return GHIP_ENOMEM;
    }
  if(ghip_ensure(ctx, ctx->cslots, GHIP_CBUF_BYTES) != GHIP_OK ||
     ghip_ensure(ctx, ctx->rslots, GHIP_CBUF_BYTES) != GHIP_OK ||
     hipMemset(ctx->cslots.p, 0, GHIP_CBUF_BYTES) != hipSuccess ||
     hipMemset(ctx->rslots.p, 0, GHIP_CBUF_BYTES) != hipSuccess)
    {
      delete ctx;
      return GHIP_ENOMEM;
    }
  // pinned, device-visible host words
  void *pin = nullptr;
  if(hipHostMalloc(&pin, sizeof(PinnedWords), hipHostMallocDefault) != hipSuccess)
    {
      delete ctx;
      return GHIP_ENOMEM;
    }
  memset(pin, 0, sizeof(PinnedWords));
  ctx->pinned = reinterpret_cast<PinnedWords *>(pin);
  // the trees' sizes: on the device and mirrored in pinned memory
  ctx->gt.hsz = &ctx->pinned->sizes[0];
  ctx->st.hsz = &ctx->pinned->sizes[1];
  if(ghip_ensure(ctx, ctx->gt.dsz, sizeof(TreeSizes)) != GHIP_OK ||
     ghip_ensure(ctx, ctx->st.dsz, sizeof(TreeSizes)) != GHIP_OK ||
     hipMemset(ctx->gt.dsz.p, 0, sizeof(TreeSizes)) != hipSuccess ||
     hipMemset(ctx->st.dsz.p, 0, sizeof(TreeSizes)) != hipSuccess)
    {
      delete ctx;
      return GHIP_ENOMEM;
    }
  // make every event "recorded" so that elapsed-time queries never fault
  for(int i = 0; i < 16; i++)
    (void) hipEventRecord(ctx->ev[i], ctx->stream);
  (void) hipStreamSynchronize(ctx->stream);
  *out = ctx;
  return GHIP_OK;
}

ghip_ctx::~ghip_ctx()
{
  (void) hipSetDevice(device);
  for(hipStream_t s : {stream, stream2, stream3})
    if(s)
      (void) hipStreamSynchronize(s);
  ghip_dd_release(this);   // (the communicator and the hipFFT plans go while the streams exist)
  ghip_pm_release(this);
  if(pinned)
    (void) hipHostFree(pinned);
  for(void *p : host_pins)
    (void) hipHostUnregister(p);
  auto destroy = [](hipEvent_t *e, int count) {
    for(int i = 0; i < count; i++)
      if(e[i])
        (void) hipEventDestroy(e[i]);
  };
  destroy(ev, 16);
  destroy(&pc_ev[0][0], 16);
  destroy(&ev_side, 1);
  destroy(&ev_sizes, 1);
  destroy(&ev_sizes_gas, 1);
  destroy(ev_ring.data(), (int) ev_ring.size());
  destroy(evx, 4);
  destroy(evt, 2);
  destroy(wind_ev, 8);
  for(hipStream_t s : {stream2, stream3, stream})
    if(s)
      (void) hipStreamDestroy(s);
}

extern "C" void ghip_destroy(ghip_ctx *ctx)
{
  delete ctx;
}

extern "C" const char *ghip_last_error(const ghip_ctx *ctx)
{
  return ctx ? ctx->err.c_str() : "null context";
}

extern "C" void *ghip_stream(ghip_ctx *ctx)
{
  if(ctx)
    (void) ghip_join(ctx);
  return ctx ? (void *) ctx->stream : nullptr;
}

extern "C" int ghip_sync(ghip_ctx *ctx)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx)
    return GHIP_EINVAL;
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  return ghip_check_device_errors(ctx);
}

// ---------------------------------------------------------------------------------------------
// field table
// ---------------------------------------------------------------------------------------------
struct FieldInfo
{
  int gas;    // 1: sized ngas, 0: sized numpart
  int ncomp;  // 1 or 3
  int isint;
};

static const FieldInfo kField[GHIP_F_COUNT] = {
  /* POS */ {0, 3, 0},        /* VEL */ {0, 3, 0},       /* MASS */ {0, 1, 0},
  /* TYPE */ {0, 1, 1},       /* OLDACC */ {0, 1, 0},    /* HSML */ {0, 1, 0},
  /* TIMEBIN */ {0, 1, 1},    /* TI_BEGSTEP */ {0, 1, 1}, /* VELPRED */ {1, 3, 0},
  /* ENTROPY */ {1, 1, 0},    /* DTENTROPY */ {1, 1, 0}, /* GRAVACCEL */ {0, 3, 0},
  /* GRAVCOST */ {0, 1, 1},   /* NUMNGB */ {1, 1, 0},    /* DENSITY */ {1, 1, 0},
  /* DHSMLFAC */ {1, 1, 0},   /* DIVVEL */ {1, 1, 0},    /* CURLVEL */ {1, 1, 0},
  /* PRESSURE */ {1, 1, 0},   /* HYDROACCEL */ {1, 3, 0}, /* MAXSIGNALVEL */ {1, 1, 0},
  /* TI_CURRENT */ {0, 1, 1}, /* GRAVPM */ {0, 3, 0}, /* ID */ {0, 1, 1}};

// the same table for the migration of ghip_dd.hip and the record members of ghip_records.hip
void ghip_field_info(int f, int *gas, int *ncomp, int *isint)
{
  *gas = kField[f].gas;
  *ncomp = kField[f].ncomp;
  *isint = kField[f].isint;
}

static size_t field_count(const ghip_ctx *ctx, int f)
{
  return (size_t) (kField[f].gas ? ctx->ngas : ctx->n);
}

static size_t field_bytes(const ghip_ctx *ctx, int f)
{
  return field_count(ctx, f) * kField[f].ncomp * (kField[f].isint ? 4 : 8);
}

extern "C" int ghip_set_counts(ghip_ctx *ctx, int numpart, int ngas)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || numpart < 0 || ngas < 0 || ngas > numpart)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_set_counts: need 0 <= ngas <= numpart");
  HIPCHK(hipSetDevice(ctx->device));
  bool changed = (numpart != ctx->n || ngas != ctx->ngas);
  if(changed)
    {
      ctx->pot_n = -1;      // (the potential of ghip_potential belongs to the particle set it was made for)
      ctx->visc_ngas = -1;  // (... and alpha / Dtalpha of ghip_visc_set_alpha too)
      ctx->id_given = false;
      if(ctx->sk.on)
        ctx->sk.stale = true;   // (the sink table: refused until given again)
      if(ctx->wk.on)
        ctx->wk.stale = true;   // (the wind table, keyed by particle index, too)
      ctx->sfr_ncand = -1;      // (the candidates of ghip_sfr_cooling are particle indices of the old counts)
    }
  ctx->n = numpart;
  ctx->ngas = ngas;
  for(int f = 0; f < GHIP_F_COUNT; f++)
    {
      size_t before = ctx->f[f].cap;
      GCHK(ghip_ensure(ctx, ctx->f[f], field_bytes(ctx, f)));
      if(ctx->f[f].cap != before)
        HIPCHK(hipMemsetAsync(ctx->f[f].p, 0, ctx->f[f].cap, ctx->stream));
    }
  if(changed)
    {
      ctx->gt.built = false;
      ctx->st.built = false;
      ctx->dd.geom_kept = false;
      ctx->nactive = -1;
      ctx->lists_dirty = ctx->gas_list_dirty = true;
    }
  return GHIP_OK;
}

// [n][ncomp] (host layout, in `stage`) <-> SoA with pitch n (device layout)
template <class T>
__global__ void k_aos_to_soa(size_t n, int ncomp, const T *__restrict__ src, T *__restrict__ dst)
{
  size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  for(int c = 0; c < ncomp; c++)
    dst[(size_t) c * n + i] = src[i * ncomp + c];
}

template <class T>
__global__ void k_soa_to_aos(size_t n, int ncomp, const T *__restrict__ src, T *__restrict__ dst)
{
  size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  for(int c = 0; c < ncomp; c++)
    dst[i * ncomp + c] = src[(size_t) c * n + i];
}

// is every record of the gas block [0, ngas) still gas?  (allvars.h:1384 holds after a
// rearrange_particle_sequence(); a particle converted since keeps its place with another Type)
__global__ void k_check_gas_types(int ngas, const int *__restrict__ type, int *word)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i < ngas && type[i] != 0)
    *word = 1;
}

int ghip_check_gas_types(ghip_ctx *ctx)
{
  bool mixed = false;
  if(ctx->ngas > 0)
    {
      int *w = ghip_gas_mixed_word(ctx);
      *w = 0;
      k_check_gas_types<<<cdiv(ctx->ngas, 256), 256, 0, ctx->stream>>>(ctx->ngas, P<int>(ctx->f[GHIP_F_TYPE]), w);
      HIPCHK(hipGetLastError());
      HIPCHK(ghip_stream_sync(ctx, ctx->stream));
      mixed = *reinterpret_cast<volatile int *>(w) != 0;
    }
  if(mixed != ctx->gas_mixed)
    {
      ctx->gas_mixed = mixed;
      ctx->st.built = false;
      ctx->gas_list_dirty = true;
    }
  return GHIP_OK;
}

extern "C" int ghip_set_field(ghip_ctx *ctx, int field, const void *host)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || field < 0 || field >= GHIP_F_COUNT)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_set_field: bad field %d", field);
  if(field == GHIP_F_POS || field == GHIP_F_MASS || field == GHIP_F_TYPE)
    ctx->pot_n = -1;   // (what ghip_potential computed no longer belongs to this state)
  size_t cnt = field_count(ctx, field), bytes = field_bytes(ctx, field);
  if(cnt == 0)
    return GHIP_OK;
  if(!host)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_set_field: null host pointer");
  hipStream_t st = ctx->stream;
  if(kField[field].ncomp == 1)
    HIPCHK(hipMemcpyAsync(ctx->f[field].p, host, bytes, hipMemcpyHostToDevice, st));
  else
    {
      GCHK(ghip_ensure(ctx, ctx->stage, bytes));
      HIPCHK(hipMemcpyAsync(ctx->stage.p, host, bytes, hipMemcpyHostToDevice, st));
      k_aos_to_soa<double><<<cdiv((long long) cnt, 256), 256, 0, st>>>(
        cnt, 3, P<double>(ctx->stage), P<double>(ctx->f[field]));
      HIPCHK(hipGetLastError());
    }
  HIPCHK(ghip_stream_sync(ctx, st));
  if(field == GHIP_F_ID)
    ctx->id_given = true;
  if(field == GHIP_F_POS || field == GHIP_F_MASS || field == GHIP_F_TYPE)
    {
      ctx->gt.built = false;
      ctx->st.built = false;
      ctx->dd.geom_kept = false;
    }
  if(field == GHIP_F_TYPE)
    GCHK(ghip_check_gas_types(ctx));
  return GHIP_OK;
}

extern "C" int ghip_get_field(ghip_ctx *ctx, int field, void *host)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || field < 0 || field >= GHIP_F_COUNT)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_get_field: bad field %d", field);
  size_t cnt = field_count(ctx, field), bytes = field_bytes(ctx, field);
  if(cnt == 0)
    return GHIP_OK;
  if(!host)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_get_field: null host pointer");
  hipStream_t st = ctx->stream;
  if(kField[field].ncomp == 1)
    HIPCHK(hipMemcpyAsync(host, ctx->f[field].p, bytes, hipMemcpyDeviceToHost, st));
  else
    {
      GCHK(ghip_ensure(ctx, ctx->stage, bytes));
      k_soa_to_aos<double><<<cdiv((long long) cnt, 256), 256, 0, st>>>(
        cnt, 3, P<double>(ctx->f[field]), P<double>(ctx->stage));
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(host, ctx->stage.p, bytes, hipMemcpyDeviceToHost, st));
    }
  HIPCHK(ghip_stream_sync(ctx, st));
  return ghip_check_device_errors(ctx);
}

// ---------------------------------------------------------------------------------------------
// active list / shard / tree / stats
// ---------------------------------------------------------------------------------------------
extern "C" int ghip_set_active(ghip_ctx *ctx, const int *idx, int nactive)
{
  // "everybody" while everybody already is: nothing changes, and a gravity pair in flight (whose
  // target lists this call would otherwise rebuild) need not be waited for
  if(ctx && !idx && ctx->nactive < 0 && (nactive == 0 || nactive == ctx->n))
    return GHIP_OK;
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || nactive < 0)
    return GHIP_EINVAL;
  if(!idx)
    {
      if(nactive != 0 && nactive != ctx->n)
        return ghip_fail(ctx, GHIP_EINVAL, "ghip_set_active: NULL list means all particles");
      ctx->nactive = (nactive == 0 && ctx->n != 0) ? -1 : -1;
      ctx->lists_dirty = ctx->gas_list_dirty = true;
      return GHIP_OK;
    }
  for(int a = 0; a < nactive; a++)
    if(idx[a] < 0 || idx[a] >= ctx->n)
      return ghip_fail(ctx, GHIP_EINVAL, "ghip_set_active: index %d out of range", idx[a]);
  GCHK(ghip_ensure(ctx, ctx->act_host_idx, (size_t) nactive * 4));
  if(nactive > 0)
    {
      HIPCHK(hipMemcpyAsync(ctx->act_host_idx.p, idx, (size_t) nactive * 4, hipMemcpyHostToDevice,
                            ctx->stream));
      HIPCHK(ghip_stream_sync(ctx, ctx->stream));
    }
  ctx->nactive = nactive;
  ctx->lists_dirty = ctx->gas_list_dirty = true;
  return GHIP_OK;
}

extern "C" int ghip_set_shard(ghip_ctx *ctx, int rank, int nranks)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || nranks < 1 || nranks > GHIP_MAXRANKS || rank < 0 || rank >= nranks)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_set_shard: need 0 <= rank < nranks <= %d",
                     GHIP_MAXRANKS);
  if(nranks != ctx->shard_n)
    ctx->lists_dirty = ctx->gas_list_dirty = true;   // the stored list order is rank-major
  ctx->shard_rank = rank;
  ctx->shard_n = nranks;
  return GHIP_OK;
}

extern "C" int ghip_tree_build(ghip_ctx *ctx, const double corner[3], const double center[3],
                               double len, const double soft[6])
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !corner || !center || !soft || !(len > 0))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_tree_build: bad arguments");
  HIPCHK(hipSetDevice(ctx->device));
  for(int j = 0; j < 3; j++)
    {
      ctx->corner[j] = corner[j];
      ctx->center[j] = center[j];
    }
  ctx->dlen = len;
  for(int j = 0; j < 6; j++)
    ctx->soft[j] = soft[j];
  ctx->dyn_use = false;
  GCHK(ghip_tree_build_impl(ctx));
  // a full build (TreeReconstructFlag): with ghip_set_dynamic_tree the tree sub-steps will drift
  if(ctx->dyn_on)
    GCHK(ghip_dyn_capture(ctx));
  return GHIP_OK;
}

extern "C" int ghip_set_massless_gas_rule(ghip_ctx *ctx, int on)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  const int rule = on == 1 ? 1 : (on ? 3 : 0);
  if(ctx->skip_massless != rule)
    ctx->st.built = false;   // the rule is baked into the gas records
  ctx->skip_massless = rule;
  return GHIP_OK;
}

extern "C" int ghip_set_adaptive_gravsoft(ghip_ctx *ctx, int on)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  if(ctx->adaptive_gravsoft != (on != 0))
    ctx->gt.built = false;   // particle and node softenings are baked into the element records
  ctx->adaptive_gravsoft = (on != 0);
  return GHIP_OK;
}

extern "C" int ghip_set_rnd_table(ghip_ctx *ctx, const double *table, int ntable)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  if(ntable < 0 || (table && ntable > 0x3fffffff))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_set_rnd_table: bad table size %d", ntable);
  HIPCHK(hipSetDevice(ctx->device));
  ctx->gt.built = false;   // the tree in place follows the old rule
  ctx->st.built = false;
  ctx->gas_pending = false;
  if(!table || ntable == 0)
    {
      ctx->rnd_n = 0;
      return GHIP_OK;
    }
  ctx->rnd_n = 0;
  GCHK(ghip_ensure(ctx, ctx->rnd_table, (size_t) ntable * 8));
  HIPCHK(hipMemcpyAsync(ctx->rnd_table.p, table, (size_t) ntable * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));   // (the table is the caller's)
  ctx->rnd_n = ntable;
  return GHIP_OK;
}

extern "C" int ghip_tree_max_level(void)
{
  return GHIP_TREE_MAXLEVEL;
}

int ghip_read_slots(ghip_ctx *ctx, DevBuf &buf, unsigned long long out[GHIP_CK_COUNT][2])
{
  std::vector<unsigned long long> h((size_t) GHIP_CK_COUNT * GHIP_CKIND_U64);
  HIPCHK(hipMemcpy(h.data(), buf.p, GHIP_CBUF_BYTES, hipMemcpyDeviceToHost));
  for(int k = 0; k < GHIP_CK_COUNT; k++)
    for(int w = 0; w < 2; w++)
      {
        unsigned long long t = 0;
        for(int s = 0; s < GHIP_CSLOTS; s++)
          t += h[(size_t) k * GHIP_CKIND_U64 + (size_t) s * GHIP_CSLOT_U64 + w];
        out[k][w] = t;
      }
  return GHIP_OK;
}

extern "C" int ghip_get_stats(const ghip_ctx *cctx, ghip_stats *out)
{
  ghip_ctx *ctx = const_cast<ghip_ctx *>(cctx);
  if(!ctx || !out)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  ghip_stats &S = ctx->stats;
  if(ctx->cslots.p)
    {
      unsigned long long c[GHIP_CK_COUNT][2];
      GCHK(ghip_read_slots(ctx, ctx->cslots, c));
      S.grav_wave_steps = (long long) c[GHIP_CK_NEWTON][1];
      S.ewald_wave_steps = (long long) c[GHIP_CK_EWALD][1];
      S.grav_interactions = (long long) c[GHIP_CK_NEWTON][0];
      S.ewald_interactions = (long long) c[GHIP_CK_EWALD][0];
      S.dens_neighbours = (long long) c[GHIP_CK_DENS][0];
      S.hydro_pairs = (long long) c[GHIP_CK_HYDRO][0];
    }
  auto el = [&](int a, int b) {
    float ms = 0;
    if(hipEventElapsedTime(&ms, ctx->evp[a], ctx->evp[b]) != hipSuccess)
      ms = 0;
    return ms;
  };
  S.ms_tree = el(0, 1);
  S.ms_grav = el(2, 3);
  S.ms_ewald = el(4, 5);
  S.ms_dens = el(6, 7);
  S.ms_hmax = el(8, 9);
  S.ms_hydro = el(10, 11);
  S.ms_kick = el(12, 13);
  S.ms_pm = el(14, 15);
  *out = S;
  return ghip_check_device_errors(ctx);
}

extern "C" int ghip_set_async(ghip_ctx *ctx, int on)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  if(!on && ctx->async)
    {
      // leaving asynchronous mode: whatever was deferred is reported now
      HIPCHK(ghip_stream_sync(ctx, ctx->stream));
      ctx->async = false;
      return ghip_check_device_errors(ctx);
    }
  ctx->async = (on != 0);
  return GHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// statistics of a run of steps without a host synchronisation per step
// ---------------------------------------------------------------------------------------------
#define RUN_EV (GHIP_NEV + 2)   // events per ring slot: the phase events + step begin / end marks

extern "C" int ghip_run_begin(ghip_ctx *ctx, int max_steps)
{
  if(!ctx || max_steps < 1)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  const size_t want = (size_t) max_steps * RUN_EV;
  while(ctx->ev_ring.size() < want)
    {
      hipEvent_t e;
      HIPCHK(hipEventCreate(&e));
      ctx->ev_ring.push_back(e);
    }
  ctx->ring_slots = max_steps;
  ctx->ring_cur = -1;
  ctx->run_steps = 0;
  ctx->run_dens_iter = 0;
  ctx->run_syncs0 = ctx->n_syncs;
  ctx->run_launches0 = ghip_launch_count();
  // (the walks and the SPH kernels add to the run's counter slots themselves)
  HIPCHK(hipMemsetAsync(ctx->rslots.p, 0, GHIP_CBUF_BYTES, ctx->stream));
  return GHIP_OK;
}

extern "C" int ghip_step_begin(ghip_ctx *ctx)
{
  if(!ctx || ctx->ring_slots <= 0)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_step_begin: call ghip_run_begin first");
  ctx->ring_cur++;
  ctx->evp = &ctx->ev_ring[(size_t) (ctx->ring_cur % ctx->ring_slots) * RUN_EV];
  // (on the main stream, which is in order: after the previous step's end mark)
  HIPCHK(hipEventRecord(ctx->evp[GHIP_NEV], ctx->stream));
  return GHIP_OK;
}

extern "C" int ghip_step_end(ghip_ctx *ctx)
{
  if(!ctx || ctx->ring_slots <= 0 || ctx->ring_cur < 0)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_step_end: no step in progress");
  GCHK(ghip_join_pair(ctx));   // (a gravity pair still in flight belongs to this step)
  HIPCHK(hipEventRecord(ctx->evp[GHIP_NEV + 1], ctx->stream));
  ctx->run_steps++;
  ctx->run_dens_iter += ctx->stats.dens_iterations;
  return GHIP_OK;
}

extern "C" int ghip_run_end(ghip_ctx *ctx, ghip_run_stats *out)
{
  if(!ctx || !out || ctx->ring_slots <= 0)
    return GHIP_EINVAL;
  memset(out, 0, sizeof(*out));
  out->launches = ghip_launch_count() - ctx->run_launches0;
  out->blocking_syncs = ctx->n_syncs - ctx->run_syncs0;
  GHIP_JOIN(ctx);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  unsigned long long acc[GHIP_CK_COUNT][2];
  GCHK(ghip_read_slots(ctx, ctx->rslots, acc));
  out->steps = ctx->run_steps;
  out->grav_interactions = (long long) acc[GHIP_CK_NEWTON][0];
  out->ewald_interactions = (long long) acc[GHIP_CK_EWALD][0];
  out->dens_neighbours = (long long) acc[GHIP_CK_DENS][0];
  out->hydro_pairs = (long long) acc[GHIP_CK_HYDRO][0];
  out->grav_wave_steps = (long long) acc[GHIP_CK_NEWTON][1];
  out->ewald_wave_steps = (long long) acc[GHIP_CK_EWALD][1];
  out->dens_extra_iterations = ctx->run_dens_iter;
  auto el = [](hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    if(hipEventElapsedTime(&ms, a, b) != hipSuccess)
      ms = 0;   // (a phase that did not run in that step)
    return (double) ms;
  };
  const long long timed = ctx->run_steps < ctx->ring_slots ? ctx->run_steps : ctx->ring_slots;
  out->steps_timed = timed;
  const long long first = ctx->run_steps - timed;
  hipEvent_t *prev = nullptr, *e0 = nullptr;
  for(long long k = first; k < ctx->run_steps; k++)
    {
      hipEvent_t *e = &ctx->ev_ring[(size_t) (k % ctx->ring_slots) * RUN_EV];
      out->ms_tree += el(e[0], e[1]);
      out->ms_grav += el(e[2], e[3]);
      out->ms_ewald += el(e[4], e[5]);
      out->ms_dens += el(e[6], e[7]);
      out->ms_hmax += el(e[8], e[9]);
      out->ms_hydro += el(e[10], e[11]);
      out->ms_kick += el(e[12], e[13]);
      out->ms_steps_device += el(e[GHIP_NEV], e[GHIP_NEV + 1]);
      if(prev)
        out->ms_between_steps += el(prev[GHIP_NEV + 1], e[GHIP_NEV]);
      else
        e0 = e;
      prev = e;
    }
  if(e0 && prev)
    out->ms_first_to_last = el(e0[GHIP_NEV], prev[GHIP_NEV + 1]);
  ctx->evp = ctx->ev;   // back to the fixed event set of ghip_get_stats
  ctx->ring_slots = 0;
  ctx->ring_cur = -1;
  return ghip_check_device_errors(ctx);
}

extern "C" int ghip_tree_dump(ghip_ctx *ctx, int which, int *nelem, double *xm4, double *cl4,
                              int *lk4, double *aux, int *perm)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !nelem || which < 0 || which > 1)
    return GHIP_EINVAL;
  TreeDev &t = which ? ctx->st : ctx->gt;
  if(!t.built)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_tree_dump: tree not built");
  *nelem = t.nelem;
  if(t.n == 0)
    return GHIP_OK;
  hipStream_t st = ctx->stream;
  size_t ne = (size_t) t.nelem;
  if(xm4)
    HIPCHK(hipMemcpyAsync(xm4, t.xm.p, ne * 32, hipMemcpyDeviceToHost, st));
  if(cl4)
    HIPCHK(hipMemcpyAsync(cl4, t.cl.p, ne * 32, hipMemcpyDeviceToHost, st));
  if(lk4)
    HIPCHK(hipMemcpyAsync(lk4, t.lk.p, ne * 16, hipMemcpyDeviceToHost, st));
  if(aux)
    HIPCHK(hipMemcpyAsync(aux, t.aux.p, ne * 8, hipMemcpyDeviceToHost, st));
  if(perm)
    HIPCHK(hipMemcpyAsync(perm, t.perm.p, (size_t) t.n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  return GHIP_OK;
}
