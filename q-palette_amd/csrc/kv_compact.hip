// qpal_kv_compact: behind a tree step's accept, the accepted node of depth k sits at cache slot pos0 + path[k],
// rotated for position pos0 + k.  ONE launch moves the K and V rows of every layer, kv head and slot from slot pos0 + path[k] to
// slot pos0 + k, k = 1 .. n_acc, where path[k] != k; afterwards slots pos0 .. pos0 + n_acc hold the sequential cache.
//
// A row is hd elements of 2 bytes (fp16) or 1 byte (e4m3): a byte copy in 16-byte pieces.  A thread owns ONE 16-byte column of the
// K or the V row of one kv head, for all of the slot's <= 15 moves: it loads every source piece into registers, then stores them.
// path[k] > k and the path rises, so a destination pos0 + k is never a LATER move's source; it can be an EARLIER move's (path (0, 2,
// 3, 5): k = 1 reads slot 2, k = 2 writes it).  Moves in rising k would therefore be safe one by one; loading all sources first
// does not lean on that, is right for any path a caller hands in, and keeps up to 15 loads in flight.  Columns are disjoint, so no
// thread reads what another writes and no barrier is needed.
// Grid: (pieces of a layer's K | V rows over all kv heads / 256, slots, layers).  pos0, path and n_acc are the draft's and the
// accept's device tensors; the host reads nothing, so the launch is capturable.  Moves that would leave the cache — n_acc outside
// 0 .. 15, path[k] outside (k, 32), a slot at or past max_len, a page entry outside the pool (§17's guard) — are skipped.
#include <hip/hip_runtime.h>

#include "kv_paged.h"
#include "qpal_common.h"

namespace qpal {

namespace {

constexpr int kCompactMoves = 15, kCompactRows = 32, kCompactThreads = 256;

struct KvCompactParams {
    unsigned char *const *kptr, *const *vptr;  // [L] device pointers: the layers' caches [B][nkv][max_len][row] or pools
    const long *pos0;                          // int64 [B]
    const int *path;                           // int32 [B][16]
    const int *n_acc;                          // int32 [B]
    int nkv, cpr;                              // kv heads; 16-byte pieces of a row
    long max_len;
    const int *table;  // PAGED: int32 [B][ld_table]
    long ld_table;
    int num_pages, page_shift;
};

template <bool PAGED>
__global__ __launch_bounds__(kCompactThreads) void kv_compact_kernel(const KvCompactParams p) {
    const int b = blockIdx.y, layer = blockIdx.z;
    const int item = blockIdx.x * kCompactThreads + threadIdx.x;  // (kv head, K | V, piece)
    const int m = p.n_acc[b];
    const long pos0 = p.pos0[b];
    if (item >= p.nkv * 2 * p.cpr || m < 1 || m > kCompactMoves || pos0 < 0 || pos0 >= p.max_len) return;
    const int kh = item / (2 * p.cpr), isv = (item / p.cpr) & 1, ch = item % p.cpr;
    unsigned char *const base = isv ? p.vptr[layer] : p.kptr[layer];
    const long row = 16l * p.cpr;
    // byte offset of the piece at cache position n of this slot and kv head, or -1: not to be touched
    auto at = [&](long n) -> long {
        if (n >= p.max_len) return -1;
        if constexpr (PAGED) {
            const int pg = p.table[(long)b * p.ld_table + (n >> p.page_shift)];
            if (!page_ok(pg, p.num_pages)) return -1;
            return ((((long)pg * p.nkv + kh) << p.page_shift) + (n & ((1l << p.page_shift) - 1))) * row + 16l * ch;
        } else {
            return (((long)b * p.nkv + kh) * p.max_len + n) * row + 16l * ch;
        }
    };
    const int *path = p.path + b * (kCompactMoves + 1);
    u32x4 regs[kCompactMoves];
    long dst[kCompactMoves];
#pragma unroll
    for (int k = 1; k <= kCompactMoves; k++) {  // every load ...
        dst[k - 1] = -1;
        if (k <= m) {
            const int j = path[k];
            const long s = j > k && j < kCompactRows ? at(pos0 + j) : -1;
            if (s >= 0) {
                regs[k - 1] = *reinterpret_cast<const u32x4 *>(base + s);
                dst[k - 1] = at(pos0 + k);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kCompactMoves; k++)  // ... before any store
        if (dst[k] >= 0) *reinterpret_cast<u32x4 *>(base + dst[k]) = regs[k];
}

}  // namespace

}  // namespace qpal

using namespace qpal;

extern "C" int qpal_kv_compact(void *const *kptrs, void *const *vptrs, int layers, const long *pos0, const int *path, const int *n_acc,
                               const int *block_table, long ld_table, int num_pages, int page_size, int max_pages, int kv_fmt, int B,
                               int nkv, int hd, long max_len, void *stream) {
    if (!kptrs || !vptrs || !pos0 || !path || !n_acc) return QPAL_E_NULL;
    if (kv_fmt != 0 && kv_fmt != 1) return QPAL_E_SHAPE;
    if (layers < 1 || layers > 65535 || B < 1 || B > 128 || nkv < 1 || (hd != 64 && hd != 128 && hd != 256)) return QPAL_E_SHAPE;
    int shift = 0;
    if (block_table) {
        const PageArgs pg{block_table, ld_table, num_pages, page_size, max_pages};
        const int rc = paged_shape(pg, kv_fmt, shift, max_len);
        if (rc != QPAL_OK) return rc;
    }
    if (max_len < 4 || max_len % 4 || max_len >= (1L << 30)) return QPAL_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(kptrs) | reinterpret_cast<uintptr_t>(vptrs) | reinterpret_cast<uintptr_t>(pos0)) & 7) return QPAL_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(path) | reinterpret_cast<uintptr_t>(n_acc) | reinterpret_cast<uintptr_t>(block_table)) & 3)
        return QPAL_E_ALIGN;
    const int cpr = hd * (kv_fmt == 1 ? 1 : 2) / 16;
    KvCompactParams p{reinterpret_cast<unsigned char *const *>(kptrs), reinterpret_cast<unsigned char *const *>(vptrs), pos0, path, n_acc,
                      nkv, cpr, max_len, block_table, ld_table, num_pages, shift};
    const dim3 grid((nkv * 2 * cpr + kCompactThreads - 1) / kCompactThreads, B, layers);
    if (block_table) hipLaunchKernelGGL(kv_compact_kernel<true>, grid, dim3(kCompactThreads), 0, static_cast<hipStream_t>(stream), p);
    else hipLaunchKernelGGL(kv_compact_kernel<false>, grid, dim3(kCompactThreads), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}
