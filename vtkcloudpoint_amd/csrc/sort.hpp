// sort.hpp -- the library's one use of rocPRIM: a stable LSD radix sort of (key, value) pairs.
#pragma once
#include <string.h>  // rocprim's texture_cache_iterator.hpp calls ::memset without including it

#include <rocprim/rocprim.hpp>

#include "vcp_ctx.hpp"

// smallest number of key bits that holds every value in [0, maxval] (at least 1)
inline int vcp_bits_for(uint64_t maxval) {
  int b = 1;
  while (b < 64 && (maxval >> b)) b++;
  return b;
}

// (kin, vin) [n] -> (kout, vout) sorted on the low `bits` bits of the key, stable; tmp is grown to rocPRIM's temporary
// storage.  Enqueued on the context's stream.
template <class K, class V>
int vcp_sort_pairs(vcp_ctx* ctx, DevBuf& tmp, K* kin, K* kout, V* vin, V* vout, size_t n, int bits,
                   bool tmp_listed = true) {
  size_t tb = 0;
  VCP_HIP(ctx, rocprim::radix_sort_pairs(nullptr, tb, kin, kout, vin, vout, n, 0, bits, ctx->stream));
  VCP_TRY(vcp_ensure(ctx, tmp, tb + 64, tmp_listed));
  VCP_HIP(ctx, rocprim::radix_sort_pairs(tmp.p, tb, kin, kout, vin, vout, n, 0, bits, ctx->stream));
  return VCP_OK;
}

// Group m list entries by cluster label (group.hip).  Entry t is point i = order ? order[t] : t with label labels[i];
// a label outside 0..K adds one to *bad and counts as label 0.  The entries are put in (label, t) order by a stable sort
// (keys / vals: workspace, 2 (m + 1) words each; tmp: the sort's): *sorted = the points in that order,
// segstart[k] = the first sorted slot of label k (segstart[K + 1] = m), counts[k] = entries with label k.  The caller
// zeroes segstart [K + 2] and *bad beforehand.
int vcp_group_by_label(vcp_ctx* ctx, const int32_t* d_labels, const int64_t* d_order, int64_t m, int32_t K,
                       DevBuf& keys, DevBuf& vals, DevBuf& tmp, uint32_t* segstart, uint32_t* counts, uint32_t* bad,
                       const uint32_t** sorted);
