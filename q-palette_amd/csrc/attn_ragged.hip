// Ragged prefill attention (qpal_attn_rope_prefill_ragged, qpal_attn_rope_prefill_ragged_paged): ONE launch for R
// <= 128 rows of q | k | v cut into S <= 128 segments, segment s = rows row0[s] .. row0[s + 1] - 1 of sequence seq[s] at positions
// pos0[s] ..  Per segment the launch is attn_prefill.hip's launch of T = row0[s + 1] - row0[s] rows on that sequence's cache: the
// same body (attn_prefill.h), with the per-sequence values — pos0, T, the q / k / v / out row base, the cache base or the block-
// table row — found per workgroup instead of read from the arguments.
//
// seq, row0 and pos0 live on the device and the host never reads them: the grid is fixed from (R, S, heads, max_len).  A query
// tile never straddles two segments (tile j of a segment starts at its row j * TQ), so a launch has at most ntile = min(R, (R +
// S (TQ - 1)) / TQ) tiles per kv head, and workgroup (kv head, tile jg, chunk) finds the segment that holds tile jg: thread s counts
// the tiles of segment s (none if it is inactive), sums the counts before it out of LDS, and the one thread whose range holds jg
// publishes (s, jg - first tile of s).  No such segment: the workgroup leaves.  Tickets and partials are indexed by (kv head, jg);
// the tickets sit at kh * 128 + jg in front of the partials, whatever this launch's ntile, so that one zero-filled workspace serves
// launches of different (R, S): every launch finds every ticket word at zero and leaves it there.
#include "attn_prefill.h"

namespace qpal {

namespace {

// Launch geometry from (R, S, heads, max_len) only: ntile bounds the sum over segments of ceil(T_s / TQ) for segments that share R
// rows; chunks and workspace by prefill_split with nkv * kPfRaggedTiles tickets.  ws_bytes is monotone in R, S and max_len.
// window > 0: the chunks are sized for the longest span a query tile can have (prefill_window_positions) instead of max_len.
int ragged_geometry(int R, int S, int nq, int nkv, int hd, long max_len, PrefillGeometry &g, long window = 0) {
    g = PrefillGeometry{0, 0, 0};
    const int rc = attn_shape(R, nq, nkv, hd, max_len);
    if (rc != QPAL_OK) return rc;
    if (S < 1 || S > kPfMaxT) return QPAL_E_SHAPE;
    const int tq = 16 * pf_qs(nq / nkv);
    const long bound = ((long)R + (long)S * (tq - 1)) / tq, ntile = bound < R ? bound : R;
    prefill_split(ntile, (long)nkv * kPfRaggedTiles, nq, nkv, hd,
                  window > 0 ? prefill_window_positions(window, nq / nkv, max_len) : max_len, g);
    return QPAL_OK;
}

// the two per-row tensors of a TREE launch
struct TreeArgs {
    const int *depth;
    const unsigned *anc;
};

// The ragged family of attn_launch (c.rows = R, c.pos = pos0 [S]); TREE: the _tree entry points, without windows or score modifiers
// SC: the soft cap and the sinks; a launch without a window runs the windowed body with window = max_len
template <bool TREE>
struct Ragged {
    static constexpr bool kContig = true, kMods = !TREE;
    const int *seq, *row0;
    int S, B;
    TreeArgs tree;  // TREE only

    bool any_null() const { return !seq || !row0 || (TREE && (!tree.depth || !tree.anc)); }

    template <class CT, bool PAGED, bool WIN, bool SC>
    int launch(const AttnCall &c, const AttnVariant &v, int shift, long max_len) const {
        const int R = c.rows;
        const long window = SC && v.window == 0 ? max_len : v.window;
        PrefillGeometry g;
        int rc = ragged_geometry(R, S, c.nq, c.nkv, c.hd, max_len, g, WIN ? window : 0);
        if (rc != QPAL_OK) return rc;
        if (B < 1) return QPAL_E_SHAPE;
        rc = attn_args(c, v, g.ws_bytes);
        if (rc != QPAL_OK) return rc;
        if ((reinterpret_cast<uintptr_t>(seq) | reinterpret_cast<uintptr_t>(row0)) & 3) return QPAL_E_ALIGN;
        if constexpr (TREE) {
            if ((reinterpret_cast<uintptr_t>(tree.depth) | reinterpret_cast<uintptr_t>(tree.anc)) & 3) return QPAL_E_ALIGN;
        }
        float *wsf = static_cast<float *>(c.ws);
        AttnRaggedParams<CT> p{};
        static_cast<AttnPrefillParams<CT> &>(p) = AttnPrefillParams<CT>{
            c.q, c.k, c.v, c.ld_qkv, static_cast<CT *>(c.kcache), static_cast<CT *>(c.vcache), static_cast<uint16_t *>(c.out_f16), c.ld_out,
            c.pos, c.inv_freq, R, c.nkv, max_len, c.scale, g.ws_bytes ? reinterpret_cast<unsigned *>(wsf) : nullptr,
            g.ws_bytes ? wsf + (long)c.nkv * kPfRaggedTiles : nullptr, g.nsplit, g.ntile};
        p.seq = seq, p.row0 = row0, p.S = S, p.B = B;
        if constexpr (PAGED) p.table = v.pg.table, p.num_pages = v.pg.num_pages, p.page_shift = shift, p.ld_table = v.pg.ld_table;
        if constexpr (WIN) p.window = window;
        if constexpr (SC)
            p.softcap = v.mods.softcap, p.inv_softcap = v.mods.softcap != 0.f ? 1.f / v.mods.softcap : 0.f, p.sinks = v.mods.sinks;
        if constexpr (TREE) p.depth = tree.depth, p.anc = tree.anc;
        const int grid = c.nkv * g.ntile * g.nsplit;
        return for_hd_rep(c.hd, c.nq / c.nkv, [&](auto HD, auto REP) {
            hipLaunchKernelGGL((attn_prefill_kernel<CT, PAGED, true, HD(), REP(), WIN, SC, TREE>), dim3(grid), dim3(64 * REP() * pf_qs(REP())),
                               0, static_cast<hipStream_t>(c.stream), p);
            return (int)hipGetLastError();
        });
    }
};

}  // namespace

}  // namespace qpal

using namespace qpal;

extern "C" long qpal_attn_ragged_ws_bytes(int R, int S, int nq, int nkv, int hd, long max_len) {
    PrefillGeometry g;
    if (ragged_geometry(R, S, nq, nkv, hd, max_len, g) != QPAL_OK) return 0;
    return (long)g.ws_bytes;
}

extern "C" int qpal_attn_rope_prefill_ragged(const float *q, const float *k, const float *v, long ld_qkv, void *kcache, void *vcache,
                                             void *out_f16, long ld_out, const int *seq, const int *row0, const long *pos0,
                                             const float *inv_freq, int kv_fmt, int R, int S, int B, int nq, int nkv, int hd, long max_len,
                                             float scale, void *ws, long ws_bytes, void *stream) {
    return attn_launch({q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, pos0, inv_freq, R, nq, nkv, hd, scale, ws, ws_bytes, stream},
                       {.kv_fmt = kv_fmt, .max_len = max_len}, Ragged<false>{seq, row0, S, B});
}

extern "C" int qpal_attn_rope_prefill_ragged_paged(const float *q, const float *k, const float *v, long ld_qkv, void *kpool, void *vpool,
                                                   void *out_f16, long ld_out, const int *seq, const int *row0, const long *pos0,
                                                   const float *inv_freq, const int *block_table, long ld_table, int num_pages,
                                                   int page_size, int max_pages, int kv_fmt, int R, int S, int B, int nq, int nkv, int hd,
                                                   float scale, void *ws, long ws_bytes, void *stream) {
    return attn_launch({q, k, v, ld_qkv, kpool, vpool, out_f16, ld_out, pos0, inv_freq, R, nq, nkv, hd, scale, ws, ws_bytes, stream},
                       {.pg = {block_table, ld_table, num_pages, page_size, max_pages}, .need_table = true, .kv_fmt = kv_fmt},
                       Ragged<false>{seq, row0, S, B});
}

// Draft trees: the two launches above with depth int32 [R] and anc uint32 [R] behind pos0
extern "C" int qpal_attn_rope_prefill_ragged_tree(const float *q, const float *k, const float *v, long ld_qkv, void *kcache, void *vcache,
                                                  void *out_f16, long ld_out, const int *seq, const int *row0, const long *pos0,
                                                  const int *depth, const unsigned *anc, const float *inv_freq, int kv_fmt, int R, int S,
                                                  int B, int nq, int nkv, int hd, long max_len, float scale, void *ws, long ws_bytes,
                                                  void *stream) {
    return attn_launch({q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, pos0, inv_freq, R, nq, nkv, hd, scale, ws, ws_bytes, stream},
                       {.kv_fmt = kv_fmt, .max_len = max_len}, Ragged<true>{seq, row0, S, B, {depth, anc}});
}

extern "C" int qpal_attn_rope_prefill_ragged_tree_paged(const float *q, const float *k, const float *v, long ld_qkv, void *kpool,
                                                        void *vpool, void *out_f16, long ld_out, const int *seq, const int *row0,
                                                        const long *pos0, const int *depth, const unsigned *anc, const float *inv_freq,
                                                        const int *block_table, long ld_table, int num_pages, int page_size, int max_pages,
                                                        int kv_fmt, int R, int S, int B, int nq, int nkv, int hd, float scale, void *ws,
                                                        long ws_bytes, void *stream) {
    return attn_launch({q, k, v, ld_qkv, kpool, vpool, out_f16, ld_out, pos0, inv_freq, R, nq, nkv, hd, scale, ws, ws_bytes, stream},
                       {.pg = {block_table, ld_table, num_pages, page_size, max_pages}, .need_table = true, .kv_fmt = kv_fmt},
                       Ragged<true>{seq, row0, S, B, {depth, anc}});
}

extern "C" int qpal_attn_rope_prefill_ragged_window(const float *q, const float *k, const float *v, long ld_qkv, void *kcache, void *vcache,
                                                    void *out_f16, long ld_out, const int *seq, const int *row0, const long *pos0,
                                                    const float *inv_freq, const int *block_table, long ld_table, int num_pages,
                                                    int page_size, int max_pages, int kv_fmt, int R, int S, int B, int nq, int nkv, int hd,
                                                    long max_len, float scale, long window, void *ws, long ws_bytes, void *stream) {
    return attn_launch({q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, pos0, inv_freq, R, nq, nkv, hd, scale, ws, ws_bytes, stream},
                       {.pg = {block_table, ld_table, num_pages, page_size, max_pages}, .kv_fmt = kv_fmt, .max_len = max_len, .window = window},
                       Ragged<false>{seq, row0, S, B});
}

extern "C" int qpal_attn_rope_prefill_ragged_score(const float *q, const float *k, const float *v, long ld_qkv, void *kcache, void *vcache,
                                                   void *out_f16, long ld_out, const int *seq, const int *row0, const long *pos0,
                                                   const float *inv_freq, const int *block_table, long ld_table, int num_pages,
                                                   int page_size, int max_pages, int kv_fmt, int R, int S, int B, int nq, int nkv, int hd,
                                                   long max_len, float scale, long window, float softcap, const float *sinks, void *ws,
                                                   long ws_bytes, void *stream) {
    return attn_launch({q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, pos0, inv_freq, R, nq, nkv, hd, scale, ws, ws_bytes, stream},
                       {.pg = {block_table, ld_table, num_pages, page_size, max_pages}, .kv_fmt = kv_fmt, .max_len = max_len, .window = window,
                        .mods = {softcap, sinks}},
                       Ragged<false>{seq, row0, S, B});
}
