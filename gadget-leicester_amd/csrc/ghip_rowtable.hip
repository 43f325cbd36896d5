// ghip_rowtable.hip -- the operations of the keyed row table (ghip_rowtable.h): the image sorted into
// a table, rows dropped by flags, growth, and the refusals every entry point with a table shares.  Integer and copy
// code only: a row is nc opaque doubles here.
#include "ghip_rowtable.h"

__global__ void __launch_bounds__(256) k_rt_iota(int m, int *__restrict__ v)
{
  const int r = blockIdx.x * 256 + threadIdx.x;
  if(r < m)
    v[r] = r;
}

// dst row r = src row from[r].  key_from != nullptr: key_to[r] = key_from[from[r]].  words != nullptr: key_to is the
// sorted column, and two equal neighbours raise the duplicate words
__global__ void __launch_bounds__(256) k_rt_gather(int m, int nc, const int *__restrict__ from,
                                                   const double *__restrict__ src, double *__restrict__ dst,
                                                   const unsigned int *__restrict__ key_from, unsigned int *key_to,
                                                   int *__restrict__ words)
{
  const long long e = (long long) blockIdx.x * 256 + threadIdx.x;
  if(e >= (long long) m * nc)
    return;
  const int r = (int) (e / nc), c = (int) (e % nc);
  dst[e] = src[(size_t) from[r] * nc + c];
  if(c != 0)
    return;
  if(key_from)
    key_to[r] = key_from[from[r]];
  if(words && r + 1 < m && key_to[r] == key_to[r + 1])
    {
      words[RTW_DUP] = 1;
      atomicMax(reinterpret_cast<unsigned int *>(words + RTW_DUPKEY), key_to[r]);
    }
}

int ghip_rt_work(ghip_ctx *ctx, RowTable &T, size_t na, size_t nrow, RtWork &W, bool zero)
{
  const size_t head = RTW_WORDS * 4 + RT_REPORT_BYTES;
  if(na == 0)
    na = 1;
  GCHK(ghip_ensure(ctx, T.work, head + (3 * na + nrow) * 4 + 64));
  char *base = P<char>(T.work);
  W.words = reinterpret_cast<int *>(base);
  W.report = base + RTW_WORDS * 4;
  W.a = reinterpret_cast<int *>(base + head);
  W.b = W.a + na;
  W.c = W.b + na;
  W.row = W.c + na;
  if(zero)
    HIPCHK(hipMemsetAsync(base, 0, head, ctx->stream));
  return GHIP_OK;
}

int ghip_rt_need(ghip_ctx *ctx, const RowTable &T, const char *who, bool must_exist)
{
  if(T.on && T.stale)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: the %s table was given for other counts: give it again after "
                     "ghip_set_counts (%s)", who, T.what, T.setter);
  if(must_exist && !T.on)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: no %s table (%s)", who, T.what, T.setter);
  return GHIP_OK;
}

void ghip_rt_open_empty(RowTable &T)
{
  if(!T.on)
    {
      T.on = true;
      T.n = 0;
      T.stale = false;
    }
}

int ghip_rt_stage(ghip_ctx *ctx, RowTable &T, int m, bool keep_front)
{
  GCHK(ghip_ensure(ctx, T.tmp_key, (size_t) m * 4));
  GCHK(ghip_ensure(ctx, T.tmp_rows, (size_t) m * T.nc * 8));
  if(keep_front && T.n > 0)
    {
      HIPCHK(hipMemcpyAsync(T.tmp_key.p, T.key.p, (size_t) T.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
      HIPCHK(hipMemcpyAsync(T.tmp_rows.p, T.rows.p, (size_t) T.n * T.nc * 8, hipMemcpyDeviceToDevice, ctx->stream));
    }
  return GHIP_OK;
}

int ghip_rt_stage_host(ghip_ctx *ctx, RowTable &T, int m, const unsigned int *key, const double *rows)
{
  if(m <= 0)
    return GHIP_OK;
  GCHK(ghip_rt_stage(ctx, T, m, false));
  HIPCHK(hipMemcpyAsync(T.tmp_key.p, key, (size_t) m * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(T.tmp_rows.p, rows, (size_t) m * T.nc * 8, hipMemcpyHostToDevice, ctx->stream));
  return GHIP_OK;
}

int ghip_rt_install(ghip_ctx *ctx, RowTable &T, int m, const char *who, bool zeroed, int *hw)
{
  hipStream_t st = ctx->stream;
  T.on = false;
  T.n = 0;
  T.stale = false;
  if(m > 0)
    {
      RtWork W;
      GCHK(ghip_rt_work(ctx, T, (size_t) m, 0, W, !zeroed));
      GCHK(ghip_ensure(ctx, T.key, (size_t) m * 4));
      GCHK(ghip_ensure(ctx, T.rows, (size_t) m * T.nc * 8));
      k_rt_iota<<<cdiv(m, 256), 256, 0, st>>>(m, W.a);
      HIPCHK(hipGetLastError());
      GCHK(ghip_sort_pairs(ctx, P<unsigned int>(T.tmp_key), P<unsigned int>(T.key), W.a, W.b, m, 32, st));
      k_rt_gather<<<cdiv((long long) m * T.nc, 256), 256, 0, st>>>(m, T.nc, W.b, P<double>(T.tmp_rows),
                                                                  P<double>(T.rows), nullptr, P<unsigned int>(T.key),
                                                                  W.words);
      HIPCHK(hipGetLastError());
      if(hw)
        {
          HIPCHK(hipMemcpyAsync(hw, W.words, RTW_WORDS * 4, hipMemcpyDeviceToHost, st));
          HIPCHK(ghip_stream_sync(ctx, st));
          T.last_dup = (unsigned int) hw[RTW_DUPKEY];
          if(hw[RTW_DUP])
            return ghip_fail(ctx, GHIP_EINVAL, "%s: two rows of the %s table have the %s %u (the context holds no "
                             "table now)", who, T.what, T.key_what, T.last_dup);
        }
    }
  T.on = true;
  T.n = m;
  return GHIP_OK;
}

int ghip_rt_compact(ghip_ctx *ctx, RowTable &T, const char *who, RtWork &W, const int *keep,
                    const unsigned int *newkey, int extra, int *kept_out)
{
  hipStream_t st = ctx->stream;
  const int m = T.n;
  int kept = 0;
  if(m > 0)
    {
      GCHK(ghip_select_flagged(ctx, nullptr, keep, W.b, W.words + RTW_KEPT, m, st));
      HIPCHK(hipMemcpyAsync(&kept, W.words + RTW_KEPT, 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      if(kept < 0 || kept > m)
        return ghip_fail(ctx, GHIP_EDEVICE, "%s: %d of %d rows of the %s table kept", who, kept, m, T.what);
    }
  *kept_out = kept;
  const bool in_place = !newkey && extra == 0;
  if(in_place && kept == m)
    return GHIP_OK;
  if(kept + extra > 0)
    GCHK(ghip_rt_stage(ctx, T, kept + extra, false));
  if(kept > 0)
    {
      k_rt_gather<<<cdiv((long long) kept * T.nc, 256), 256, 0, st>>>(kept, T.nc, W.b, P<double>(T.rows),
                                                                     P<double>(T.tmp_rows),
                                                                     newkey ? newkey : P<unsigned int>(T.key),
                                                                     P<unsigned int>(T.tmp_key), nullptr);
      HIPCHK(hipGetLastError());
    }
  if(in_place)
    {
      if(kept > 0)
        {
          T.key.swap(T.tmp_key);   // (ascending still: the selection keeps the order)
          T.rows.swap(T.tmp_rows);
        }
      T.n = kept;
    }
  return GHIP_OK;
}

int ghip_rt_reserve(ghip_ctx *ctx, RowTable &T, int extra, unsigned int **key_tail, double **rows_tail)
{
  ghip_rt_open_empty(T);
  const size_t m = (size_t) T.n + (size_t) (extra > 0 ? extra : 0);
  if(T.key.cap < m * 4 || T.rows.cap < m * T.nc * 8)   // into a larger block, which then becomes the table
    {
      GCHK(ghip_rt_stage(ctx, T, (int) m, true));
      T.key.swap(T.tmp_key);
      T.rows.swap(T.tmp_rows);
    }
  *key_tail = P<unsigned int>(T.key) + T.n;
  *rows_tail = P<double>(T.rows) + (size_t) T.n * T.nc;
  return GHIP_OK;
}

void ghip_rt_appended(RowTable &T, int extra)
{
  T.n += extra;
}

int ghip_rt_get(ghip_ctx *ctx, const RowTable &T, int *n, unsigned int *key, double *rows)
{
  *n = T.n;
  if(T.n > 0 && (key || rows))
    {
      if(key)
        HIPCHK(hipMemcpyAsync(key, T.key.p, (size_t) T.n * 4, hipMemcpyDeviceToHost, ctx->stream));
      if(rows)
        HIPCHK(hipMemcpyAsync(rows, T.rows.p, (size_t) T.n * T.nc * 8, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ghip_stream_sync(ctx, ctx->stream));
    }
  return GHIP_OK;
}

int ghip_rt_clear(ghip_ctx *ctx, RowTable &T)
{
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  for(DevBuf *b : {&T.key, &T.rows, &T.tmp_key, &T.tmp_rows, &T.work})
    (void) b->release();
  T.n = 0;
  T.on = T.stale = false;
  T.last_dup = 0;
  return GHIP_OK;
}
