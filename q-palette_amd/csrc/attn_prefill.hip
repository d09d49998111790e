// Prompt prefill attention of ONE sequence (qpal_attn_rope_prefill): T new tokens at positions *pos0 .. *pos0 + T - 1 in one
// launch — rotary embedding of their q and k (qpal_rope_kv's convention: rotate_half, cos / sin of pos * inv_freq rounded to fp16,
// fp16 arithmetic), k and v appended to the cache at rows *pos0 + t, and causal attention of row t over positions 0 .. *pos0 + t.
// *pos0 < 0 or *pos0 + T > max_len: the launch does nothing.
//
// Shape: flash attention with the keys on the M side of the matrix pipe.  Workgroup = (kv head, tile of TQ query rows, chunk of
// that tile's keys); wave = (one query head of the group, 16 query rows).  The keys 0 .. *pos0 + (last row of the tile) are cut
// evenly into at most `nsplit` chunks on the device (the host fixes the grid from (T, nkv, max_len) alone: *pos0 is never read
// on the host).  A chunk walks its keys in tiles of 32: K and V rows go through LDS ONCE per workgroup — rows below *pos0 from
// the cache (prefetched into registers one tile ahead), new rows rotated from the fp32 k / v inputs, so nothing the launch reads
// from the cache was written by it; the workgroup whose query tile holds a new row also stores it to the cache.  Per tile and wave:
//   S^T[key][query] = K Q^T      v_mfma_f32_16x16x32_f16, A = 16 K rows from LDS (ds_read_b128), B = the wave's Q rows (registers)
//   online softmax per query     a query is a COLUMN of S^T = one lane & 15: maxima / sums over 8 registers and lanes ^ 16, ^ 32
//   O^T[d][query] += V^T P^T     the same instruction: B = P^T straight from the S^T registers (the k slots of the product are
//                                the keys 4 (lane >> 4) + 0..3 of both 16-key halves), A = V^T by ds_read_b64_tr_b16 from the
//                                row-major V image
// Chunks of one (kv head, query tile) leave (max, sum, unnormalised out) per row in the workspace and take a ticket; the last to
// arrive merges them in chunk order (bitwise reproducible, no float atomics) and resets the ticket: attn_batch.hip's pattern.
//
// The cache element type CT is a template parameter: uint16_t = fp16 (qpal_attn_rope_prefill), uint8_t = OCP e4m3fn
// (qpal_attn_rope_prefill_kv8, kv8.h).  The e4m3 instantiation keeps the fp16 LDS image and everything that reads
// it; the register prefetch holds bytes (cached rows as loaded, new rows quantised by the thread that rotates them, which also
// stores them where its tile owns them) and the bytes are converted exactly on their way into LDS — a new row takes part at its
// stored value.  Workspace and grid do not depend on CT.
//
// PAGED (qpal_attn_rope_prefill_paged, kv_paged.h): the caches are pools [num_pages][nkv][page_size][HD] and position
// n lives in page block_row[n / page_size].  Only the address of a cache row differs: a 32-key tile starts at a multiple of 32, so
// its two 16-key halves have one page id each, workgroup-uniform and fetched one tile ahead of the rows.
#include "attn_prefill.h"

namespace qpal {

namespace {

// Launch geometry from (T, heads, max_len) only.  ws_bytes is an upper bound of what ANY launch with at most T rows and at most
// max_len positions needs (monotone in both): one workspace serves every smaller launch of the same heads.
// window > 0: the chunks are sized for the longest span a query tile can have (prefill_window_positions) instead of max_len — never
// more chunks, never a larger workspace
int prefill_geometry(int T, int nq, int nkv, int hd, long max_len, PrefillGeometry &g, long window = 0) {
    g = PrefillGeometry{0, 0, 0};
    const int rc = attn_shape(T, nq, nkv, hd, max_len);
    if (rc != QPAL_OK) return rc;
    const int tq = 16 * pf_qs(nq / nkv);
    prefill_split((T + tq - 1) / tq, (long)nkv * kPfMaxTiles, nq, nkv, hd,
                  window > 0 ? prefill_window_positions(window, nq / nkv, max_len) : max_len, g);
    return QPAL_OK;
}

// the entry points: the same checks, geometry and launch, the cache element type and the row addressing apart (PAGED: kcache /
// vcache are the pools, `pg` the sequence's block-table row, max_len = max_pages * page_size)
// mods: SC — the soft cap and the sinks; a launch without a window runs the windowed body with window = max_len
template <class CT, bool PAGED, bool WIN = false, bool SC = false>
int attn_rope_prefill(const float *q, const float *k, const float *v, long ld_qkv, void *kcache, void *vcache, void *out_f16,
                      long ld_out, const long *pos0, const float *inv_freq, int T, int nq, int nkv, int hd, long max_len, float scale,
                      void *ws, long ws_bytes, void *stream, const PageArgs *pg = nullptr, int shift = 0, long window = 0,
                      const ScoreMods *mods = nullptr) {
    if (!q || !k || !v || !kcache || !vcache || !out_f16 || !pos0 || !inv_freq) return QPAL_E_NULL;
    if constexpr (SC) {
        if (window == 0) window = max_len;
    }
    PrefillGeometry g;
    int rc = prefill_geometry(T, nq, nkv, hd, max_len, g, WIN ? window : 0);
    if (rc != QPAL_OK) return rc;
    rc = attn_args(q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, pos0, inv_freq, nq, hd, g.ws_bytes, ws, ws_bytes,
                   (PAGED ? reinterpret_cast<uintptr_t>(pg->table) : 0) | (SC ? reinterpret_cast<uintptr_t>(mods->sinks) : 0));
    if (rc != QPAL_OK) return rc;
    float *wsf = static_cast<float *>(ws);
    AttnPrefillParams<CT> p{q, k, v, ld_qkv, static_cast<CT *>(kcache), static_cast<CT *>(vcache),
                            static_cast<uint16_t *>(out_f16), ld_out, pos0, inv_freq, T, nkv, max_len, scale,
                            g.ws_bytes ? reinterpret_cast<unsigned *>(wsf) : nullptr, g.ws_bytes ? wsf + (long)nkv * kPfMaxTiles : nullptr,
                            g.nsplit, g.ntile};
    if constexpr (PAGED) p.table = pg->table, p.num_pages = pg->num_pages, p.page_shift = shift;
    if constexpr (WIN) p.window = window;
    if constexpr (SC) p.softcap = mods->softcap, p.inv_softcap = mods->softcap != 0.f ? 1.f / mods->softcap : 0.f, p.sinks = mods->sinks;
    const int grid = nkv * g.ntile * g.nsplit, rep = nq / nkv;
    return for_hd_rep(hd, rep, [&](auto HD, auto REP) {
        hipLaunchKernelGGL((attn_prefill_kernel<CT, PAGED, false, HD(), REP(), WIN, SC>), dim3(grid), dim3(64 * REP() * pf_qs(REP())), 0,
                           static_cast<hipStream_t>(stream), p);
        return (int)hipGetLastError();
    });
}

}  // namespace

}  // namespace qpal

using namespace qpal;

extern "C" long qpal_attn_prefill_ws_bytes(int T, int nq, int nkv, int hd, long max_len) {
    PrefillGeometry g;
    if (prefill_geometry(T, nq, nkv, hd, max_len, g) != QPAL_OK) return 0;
    return (long)g.ws_bytes;
}

extern "C" int qpal_attn_rope_prefill(const float *q, const float *k, const float *v, long ld_qkv, void *kcache_f16, void *vcache_f16,
                                      void *out_f16, long ld_out, const long *pos0, const float *inv_freq, int T, int nq, int nkv,
                                      int hd, long max_len, float scale, void *ws, long ws_bytes, void *stream) {
    return attn_rope_prefill<uint16_t, false>(q, k, v, ld_qkv, kcache_f16, vcache_f16, out_f16, ld_out, pos0, inv_freq, T, nq, nkv, hd, max_len,
                                       scale, ws, ws_bytes, stream);
}

extern "C" int qpal_attn_rope_prefill_kv8(const float *q, const float *k, const float *v, long ld_qkv, void *kcache_e4m3,
                                          void *vcache_e4m3, void *out_f16, long ld_out, const long *pos0, const float *inv_freq, int T,
                                          int nq, int nkv, int hd, long max_len, float scale, void *ws, long ws_bytes, void *stream) {
    return attn_rope_prefill<uint8_t, false>(q, k, v, ld_qkv, kcache_e4m3, vcache_e4m3, out_f16, ld_out, pos0, inv_freq, T, nq, nkv, hd, max_len,
                                      scale, ws, ws_bytes, stream);
}

extern "C" int qpal_attn_rope_prefill_paged(const float *q, const float *k, const float *v, long ld_qkv, void *kpool, void *vpool,
                                            void *out_f16, long ld_out, const long *pos0, const float *inv_freq, const int *block_row,
                                            int num_pages, int page_size, int max_pages, int kv_fmt, int T, int nq, int nkv, int hd,
                                            float scale, void *ws, long ws_bytes, void *stream) {
    const PageArgs pg{block_row, max_pages, num_pages, page_size, max_pages};
    const bool any_null = !block_row || !q || !k || !v || !kpool || !vpool || !out_f16 || !pos0 || !inv_freq;
    return paged_entry(any_null, pg, kv_fmt, [&](auto ct, int shift, long max_len) {
        return attn_rope_prefill<decltype(ct), true>(q, k, v, ld_qkv, kpool, vpool, out_f16, ld_out, pos0, inv_freq, T, nq, nkv, hd, max_len,
                                                     scale, ws, ws_bytes, stream, &pg, shift);
    });
}

extern "C" int qpal_attn_rope_prefill_window(const float *q, const float *k, const float *v, long ld_qkv, void *kcache, void *vcache,
                                             void *out_f16, long ld_out, const long *pos0, const float *inv_freq, const int *block_row,
                                             int num_pages, int page_size, int max_pages, int kv_fmt, int T, int nq, int nkv, int hd,
                                             long max_len, float scale, long window, void *ws, long ws_bytes, void *stream) {
    if (!q || !k || !v || !kcache || !vcache || !out_f16 || !pos0 || !inv_freq) return QPAL_E_NULL;
    if (window < 0) return QPAL_E_PARAM;
    if (kv_fmt != 0 && kv_fmt != 1) return QPAL_E_SHAPE;
    auto launch = [&](auto ct, auto paged, auto win, long len, const PageArgs *pg, int shift) {
        return attn_rope_prefill<decltype(ct), paged(), win()>(q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, pos0, inv_freq, T, nq, nkv, hd,
                                                              len, scale, ws, ws_bytes, stream, pg, shift, window);
    };
    using Y = std::true_type;
    using N = std::false_type;
    if (!block_row) {  // a contiguous cache [nkv][max_len][hd]
        return for_kv_fmt(kv_fmt, [&](auto ct) {
            return window ? launch(ct, N{}, Y{}, max_len, nullptr, 0) : launch(ct, N{}, N{}, max_len, nullptr, 0);
        });
    }
    const PageArgs pg{block_row, max_pages, num_pages, page_size, max_pages};
    return paged_entry(false, pg, kv_fmt, [&](auto ct, int shift, long len) {
        return window ? launch(ct, Y{}, Y{}, len, &pg, shift) : launch(ct, Y{}, N{}, len, &pg, shift);
    });
}

extern "C" int qpal_attn_rope_prefill_score(const float *q, const float *k, const float *v, long ld_qkv, void *kcache, void *vcache,
                                            void *out_f16, long ld_out, const long *pos0, const float *inv_freq, const int *block_row,
                                            int num_pages, int page_size, int max_pages, int kv_fmt, int T, int nq, int nkv, int hd,
                                            long max_len, float scale, long window, float softcap, const float *sinks, void *ws,
                                            long ws_bytes, void *stream) {
    if (!q || !k || !v || !kcache || !vcache || !out_f16 || !pos0 || !inv_freq) return QPAL_E_NULL;
    if (window < 0 || !score_mods_ok(softcap)) return QPAL_E_PARAM;
    if (softcap == 0.f && !sinks)
        return qpal_attn_rope_prefill_window(q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, pos0, inv_freq, block_row, num_pages,
                                             page_size, max_pages, kv_fmt, T, nq, nkv, hd, max_len, scale, window, ws, ws_bytes, stream);
    if (kv_fmt != 0 && kv_fmt != 1) return QPAL_E_SHAPE;
    const ScoreMods mods{softcap, sinks};
    auto launch = [&](auto ct, auto paged, long len, const PageArgs *pg, int shift) {
        return attn_rope_prefill<decltype(ct), paged(), true, true>(q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, pos0, inv_freq, T, nq,
                                                                   nkv, hd, len, scale, ws, ws_bytes, stream, pg, shift, window, &mods);
    };
    if (!block_row)  // a contiguous cache [nkv][max_len][hd]
        return for_kv_fmt(kv_fmt, [&](auto ct) { return launch(ct, std::false_type{}, max_len, nullptr, 0); });
    const PageArgs pg{block_row, max_pages, num_pages, page_size, max_pages};
    return paged_entry(false, pg, kv_fmt, [&](auto ct, int shift, long len) { return launch(ct, std::true_type{}, len, &pg, shift); });
}
