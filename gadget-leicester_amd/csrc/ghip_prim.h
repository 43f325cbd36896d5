// ghip_prim.h -- device scans, radix sorts and order-preserving selections (ghip_prim.hip, the only translation
// unit that sees the scan / sort library).  Every primitive runs on the stream it is given.
#pragma once
#include "ghip_internal.h"

// Scratch of the primitives that run on stream st: the main stream, stream2 and a distinct stream3 have a
// block each (two streams that shared one would race); every primitive below looks its block up here.
DevBuf &ghip_prim_scratch(ghip_ctx *ctx, hipStream_t st);

// ---- library-backed: size query, scratch and run in one call; instantiated for the types the tree uses ----
// exclusive sum of int or unsigned long long; scratch != nullptr: that block, not the stream's (build_plan)
template <class T>
int ghip_scan(ghip_ctx *ctx, const T *in, T *out, int n, hipStream_t st, DevBuf *scratch = nullptr);
// stable, on key bits [0, end_bit): (unsigned int, int), (unsigned long long, int), (unsigned long long, double)
template <class K, class V>
int ghip_sort_pairs(ghip_ctx *ctx, const K *kin, K *kout, const V *vin, V *vout, int n, int end_bit, hipStream_t st);
int ghip_sort_keys(ghip_ctx *ctx, const unsigned long long *kin, unsigned long long *kout, int n, int end_bit,
                   hipStream_t st);
// out = the in[a] with flags[a] != 0, in order; their number -> *dcount (device).  in == nullptr: the indices a
int ghip_select_flagged(ghip_ctx *ctx, const int *in, const int *flags, int *out, int *dcount, int n, hipStream_t st);
// A list of particles (a pass's grains, wind particles, ...) in the order of the gravity tree: ord[t] = the list
// slot whose particle idx[slot] stands t-th in the tree, a sort of gt.iperm[idx[slot]].  All pointers on the
// device, n words each; key, key2 and slot are scratch
int ghip_tree_order(ghip_ctx *ctx, int n, const int *idx, unsigned int *key, unsigned int *key2, int *slot, int *ord,
                    hipStream_t st);
// slot[idx[a]] = a for the n particles of a list: the list slot by particle index
int ghip_list_slots(ghip_ctx *ctx, int n, const int *idx, int *slot, hipStream_t st);

// ---- out of one-wavefront workgroups (why: ghip_prim.hip), PRIM_BLOCK items each ----
#define PRIM_ITEMS 16
#define PRIM_BLOCK (64 * PRIM_ITEMS)
int ghip_wscan_i32(ghip_ctx *ctx, const int *in, int *out, int n, hipStream_t st);
// the tree build's exclusive sum: one-wavefront on the main stream underneath a gravity pair, else the library's
int ghip_scan_i32_under_pair(ghip_ctx *ctx, const int *in, int *out, int n, hipStream_t st);
// rows x nblk counts -> exclusive offsets per row, in place; total != nullptr: total[row] = the row's sum
int ghip_block_offsets(ghip_ctx *ctx, int rows, int nblk, int *cnt, int *total, hipStream_t st);
// selection in two halves: the flagged items per block -> blockoff[cdiv(n, PRIM_BLOCK)] as offsets, their number
// -> *total (two launches); then out = the in[a] with flags[a] != 0, in order (one launch)
int ghip_wsel_count(ghip_ctx *ctx, int n, const int *flags, int *blockoff, int *total, hipStream_t st);
int ghip_wsel_scatter(ghip_ctx *ctx, int n, const int *in, const int *flags, const int *blockoff, int *out,
                      hipStream_t st);
