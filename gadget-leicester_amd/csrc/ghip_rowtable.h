// ghip_rowtable.h -- the keyed row table (struct RowTable, ghip_internal.h) under the resident sink
// table (ghip_accretion.hip) and the resident wind table (ghip_wind.hip): the device find, the layout of the work
// block, and the host operations of ghip_rowtable.hip.  What a table's rows mean, who may have one and which
// particles select a row stay with the two owners.
#pragma once
#include "ghip_prim.h"

// ints at the front of RowTable::work
enum
{
  RTW_COUNT = 0,   // particles that a pass of the owner selected
  RTW_ERR,         // the owner's error: a selected particle without a row, a key that names the wrong particle
  RTW_ERRKEY,      // ... the largest such key
  RTW_DUP,         // two rows with the same key (ghip_rt_install)
  RTW_DUPKEY,      // ... the largest such key
  RTW_KEPT,        // rows kept by ghip_rt_compact
  RTW_WORDS = 16
};
#define RT_REPORT_BYTES 1024   // room for a pass's report behind the words
static_assert(sizeof(ghip_bh_accretion_report) <= RT_REPORT_BYTES && sizeof(ghip_sfr_form_report) <= RT_REPORT_BYTES &&
              sizeof(ghip_wind_result) <= RT_REPORT_BYTES, "the report block of RowTable::work");

struct RtWork
{
  int *words;
  char *report;
  int *a, *b, *c;   // i32[na] each: flags, selections, sort values, new keys
  int *row;         // i32[nrow]
};

// the row of `key` in the ascending list keys[0, n), -1: none
__device__ __forceinline__ int d_rt_find(int n, const unsigned int *__restrict__ keys, unsigned int key)
{
  int lo = 0, hi = n;
  while(lo < hi)
    {
      const int mid = (lo + hi) >> 1;
      if(keys[mid] < key)
        lo = mid + 1;
      else
        hi = mid;
    }
  return (lo < n && keys[lo] == key) ? lo : -1;
}

// Every operation runs on ctx->stream; `who` is the entry point in messages.  Which of them wait for the device is
// said at each (the counts per entry point: DESIGN.md 4.21).
//
// The work block for na-word arrays and nrow row slots (the same sizes give the same block); zero: the words and
// the report are cleared on the stream.  No wait.
int ghip_rt_work(ghip_ctx *ctx, RowTable &T, size_t na, size_t nrow, RtWork &W, bool zero);
// The stale table ("given for other counts") is refused; must_exist: so is the missing one ("no ... table").  No wait.
int ghip_rt_need(ghip_ctx *ctx, const RowTable &T, const char *who, bool must_exist);
// A context without a table gets one of 0 rows.
void ghip_rt_open_empty(RowTable &T);
// The image has room for m rows; keep_front: the table's own n rows stand at its front.  No wait.
int ghip_rt_stage(ghip_ctx *ctx, RowTable &T, int m, bool keep_front);
// ... and holds the caller's m rows (host arrays), copied on the stream.  No wait.
int ghip_rt_stage_host(ghip_ctx *ctx, RowTable &T, int m, const unsigned int *key, const double *rows);
// The m rows of the image, in any order, become the table: sorted by key, two equal keys raise RTW_DUP on the
// device.  zeroed: the caller cleared the words (ghip_rt_work) and may have raised RTW_ERR since.  hw == nullptr:
// no wait, nothing is read.  Otherwise the RTW_WORDS words are read into hw (one wait) and a duplicate is refused:
// the context then holds no table, and T.last_dup is the key.
int ghip_rt_install(ghip_ctx *ctx, RowTable &T, int m, const char *who, bool zeroed, int *hw);
// The rows r with keep[r] != 0 stay, in their order; W is the caller's block with na >= T.n and cleared words
// (keep may be W.a, newkey W.c; W.b is used).  One wait, for their number -> *kept.  newkey == nullptr and
// extra == 0: the table is compacted in place of itself (no sort: the order is kept).  Otherwise the kept rows, under
// newkey[r] if given, go to the front of an image with room for kept + extra rows, for the ghip_rt_install that
// follows; the table itself is as it was.
int ghip_rt_compact(ghip_ctx *ctx, RowTable &T, const char *who, RtWork &W, const int *keep,
                    const unsigned int *newkey, int extra, int *kept);
// Room for `extra` rows behind the table's own (opened empty if there is none): the tails to fill, and, once they
// are filled, the rows counted in.  No wait.
int ghip_rt_reserve(ghip_ctx *ctx, RowTable &T, int extra, unsigned int **key_tail, double **rows_tail);
void ghip_rt_appended(RowTable &T, int extra);
// *n = the rows; key / rows != nullptr: copied to the host (one wait when there is a row).
int ghip_rt_get(ghip_ctx *ctx, const RowTable &T, int *n, unsigned int *key, double *rows);
// Everything the table holds goes back; the context holds no table.  Waits for the stream.
int ghip_rt_clear(ghip_ctx *ctx, RowTable &T);
