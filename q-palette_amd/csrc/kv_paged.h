// Paged KV cache: the row address of a position in a pool [num_pages][nkv][page_size][HD], page_size = 1 << shift,
// shared by attn_batch.hip and attn_prefill.hip, and the host-side checks of the paged entry points.
#pragma once
#include <hip/hip_runtime.h>

#include "qpal_common.h"

namespace qpal {

// element offset of position n of kv head kh, whose page (entry n >> shift of the sequence's block-table row) is `page`
template <int HD>
__device__ __forceinline__ long paged_row(int page, int nkv, int kh, int shift, long n) {
    return ((((long)page * nkv + kh) << shift) + (n & ((1L << shift) - 1))) * HD;
}

// the guard: an entry outside the pool is read as page 0 and never stored through
__device__ __forceinline__ bool page_ok(int page, int num_pages) { return (unsigned)page < (unsigned)num_pages; }

struct PageArgs {
    const int *table;  // int32 [B][ld_table] (prefill: one row, [max_pages])
    long ld_table;
    int num_pages, page_size, max_pages;
};

// the paged-only argument checks that come before the geometry; sets shift = log2(page_size) and max_len = max_pages * page_size
inline int paged_shape(const PageArgs &a, int kv_fmt, int &shift, long &max_len) {
    shift = 0, max_len = 0;
    if (a.page_size != 16 && a.page_size != 32 && a.page_size != 64 && a.page_size != 128 && a.page_size != 256) return QPAL_E_SHAPE;
    if (a.num_pages < 1 || a.max_pages < 1 || a.ld_table < a.max_pages || (kv_fmt != 0 && kv_fmt != 1)) return QPAL_E_SHAPE;
    while ((1 << shift) < a.page_size) shift++;
    max_len = (long)a.max_pages * a.page_size;
    return QPAL_OK;
}

}  // namespace qpal
