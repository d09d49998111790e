// Shared-prefix decode attention: the ONE membership rule both launches of qpal_attn_rope_decode_batch_shared follow
// (attn_prefix.hip: the prefix phase; attn_batch.hip: the suffix phase), the host-side geometry of the prefix phase and the layout
// of the workspace the two launches share.
#pragma once
#include <hip/hip_runtime.h>

#include "qpal_common.h"

namespace qpal {

constexpr int kPxMaxGroups = 16;  // G of a launch
constexpr int kPxRows = 64;       // query rows (slot, query head) of a prefix workgroup: four waves of 16
constexpr int kPxMaxSplit = 8;    // key chunks of a prefix (ONE workgroup merges a tile's chunks: more of them cost more there than they save)
constexpr long kPxMinChunk = 128; // a chunk holds at least this many keys

// the three device tensors that describe sharing for one launch
struct SharedPrefixArgs {
    const int *row_group;  // int32 [B]: the group of slot b, or -1
    const int *grp_slot;   // int32 [G]: a live member whose table row addresses the group's shared pages
    const int *grp_len;    // int32 [G]: the shared positions, a positive multiple of page_size
    int G;
};

// THE rule.  The shared length of slot b at position pos (> 0) and its group in g where b is served as a member; 0 and g = -1
// where it is an ordinary slot, served exactly as the plain paged launch serves it.
__device__ __forceinline__ int shared_prefix_len(const SharedPrefixArgs &s, int b, long pos, int B, int page_shift, long max_len, int &g) {
    g = -1;
    if (pos < 0 || pos >= max_len) return 0;  // inactive
    const int gg = s.row_group[b];
    if ((unsigned)gg >= (unsigned)s.G) return 0;
    const int gs = s.grp_slot[gg], len = s.grp_len[gg];
    if ((unsigned)gs >= (unsigned)B) return 0;
    if (len <= 0 || (len & ((1 << page_shift) - 1)) != 0) return 0;
    if ((long)len > pos) return 0;
    g = gg;
    return len;
}

// Geometry of the prefix phase from (B, G, heads, max_len) alone: the group lengths are read on the device.  A workgroup is (kv
// head, tile of kPxRows rows of ONE group, key chunk); the groups of a launch have at most ceil(B rep / kPxRows) + min(G, B) tiles
// between them.  The partials of a row are addressed by the row itself (slot, query head): a slot is in one group at most.
struct PrefixGeometry {
    int nsplit, ntile;
    size_t tickets, part, pre;  // floats: ticket words [nkv][ntile] | chunk partials [nsplit][B nq][hd + 2] | merged [B nq][hd + 2]
};

inline void prefix_geometry(int B, int G, int nq, int nkv, int hd, long max_len, PrefixGeometry &g) {
    const int rep = nq / nkv;
    const long full = ((long)B * rep + kPxRows - 1) / kPxRows;  // tiles of one group that holds every slot
    long cap = max_len / kPxMinChunk;                           // chunks the longest prefix can feed
    if (cap < 1) cap = 1;
    if (cap > kPxMaxSplit) cap = kPxMaxSplit;
    long ns = (kNumCU + full * nkv - 1) / (full * nkv);         // ~one workgroup per compute unit for that group
    if (ns > cap) ns = cap;
    g.nsplit = (int)ns;
    g.ntile = (int)(full + (G < B ? G : B));
    g.tickets = (size_t)nkv * g.ntile;
    g.part = (size_t)g.nsplit * B * nq * (hd + 2);
    g.pre = (size_t)B * nq * (hd + 2);
}

// what the prefix launch is given, the cache element type apart (kv_fmt: 0 fp16, 1 e4m3fn)
struct PrefixLaunch {
    const float *q;
    long ld_qkv;
    const void *kpool, *vpool;
    const long *pos;
    const float *inv_freq;
    SharedPrefixArgs sp;
    const int *table;
    long ld_table;
    int num_pages, page_shift;
    int B, nkv;
    long max_len;
    float scale;
    unsigned *tickets;
    float *part, *pre;
    int nsplit, ntile;
};

// attn_prefix.hip
int launch_attn_prefix(const PrefixLaunch &a, int kv_fmt, int hd, int rep, void *stream);

}  // namespace qpal
