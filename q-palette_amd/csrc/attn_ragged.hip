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

// mods: SC — the soft cap and the sinks; a launch without a window runs the windowed body with window = max_len
template <class CT, bool PAGED, bool WIN = false, bool SC = false>
int attn_rope_ragged(const float *q, const float *k, const float *v, long ld_qkv, void *kcache, void *vcache, void *out_f16, long ld_out,
                     const int *seq, const int *row0, const long *pos0, const float *inv_freq, int R, int S, int B, int nq, int nkv, int hd,
                     long max_len, float scale, void *ws, long ws_bytes, void *stream, const PageArgs *pg = nullptr, int shift = 0,
                     long window = 0, const ScoreMods *mods = nullptr) {
    if constexpr (SC) {
        if (window == 0) window = max_len;
    }
    PrefillGeometry g;
    int rc = ragged_geometry(R, S, nq, nkv, hd, max_len, g, WIN ? window : 0);
    if (rc != QPAL_OK) return rc;
    if (B < 1) return QPAL_E_SHAPE;
    rc = attn_args(q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, pos0, inv_freq, nq, hd, g.ws_bytes, ws, ws_bytes,
                   (PAGED ? reinterpret_cast<uintptr_t>(pg->table) : 0) | (SC ? reinterpret_cast<uintptr_t>(mods->sinks) : 0));
    if (rc != QPAL_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(seq) | reinterpret_cast<uintptr_t>(row0)) & 3) return QPAL_E_ALIGN;
    float *wsf = static_cast<float *>(ws);
    AttnRaggedParams<CT> p{};
    static_cast<AttnPrefillParams<CT> &>(p) = AttnPrefillParams<CT>{
        q, k, v, ld_qkv, static_cast<CT *>(kcache), static_cast<CT *>(vcache), static_cast<uint16_t *>(out_f16), ld_out, pos0, inv_freq,
        R, nkv, max_len, scale, g.ws_bytes ? reinterpret_cast<unsigned *>(wsf) : nullptr,
        g.ws_bytes ? wsf + (long)nkv * kPfRaggedTiles : nullptr, g.nsplit, g.ntile};
    p.seq = seq, p.row0 = row0, p.S = S, p.B = B;
    if constexpr (PAGED) p.table = pg->table, p.num_pages = pg->num_pages, p.page_shift = shift, p.ld_table = pg->ld_table;
    if constexpr (WIN) p.window = window;
    if constexpr (SC) p.softcap = mods->softcap, p.inv_softcap = mods->softcap != 0.f ? 1.f / mods->softcap : 0.f, p.sinks = mods->sinks;
    const int grid = nkv * g.ntile * g.nsplit, rep = nq / nkv;
    return for_hd_rep(hd, rep, [&](auto HD, auto REP) {
        hipLaunchKernelGGL((attn_prefill_kernel<CT, PAGED, true, HD(), REP(), WIN, SC>), dim3(grid), dim3(64 * REP() * pf_qs(REP())), 0,
                           static_cast<hipStream_t>(stream), p);
        return (int)hipGetLastError();
    });
}

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
    if (!q || !k || !v || !kcache || !vcache || !out_f16 || !seq || !row0 || !pos0 || !inv_freq) return QPAL_E_NULL;
    if (kv_fmt != 0 && kv_fmt != 1) return QPAL_E_SHAPE;
    return for_kv_fmt(kv_fmt, [&](auto ct) {
        return attn_rope_ragged<decltype(ct), false>(q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, seq, row0, pos0, inv_freq, R, S, B, nq,
                                                     nkv, hd, max_len, scale, ws, ws_bytes, stream);
    });
}

extern "C" int qpal_attn_rope_prefill_ragged_paged(const float *q, const float *k, const float *v, long ld_qkv, void *kpool, void *vpool,
                                                   void *out_f16, long ld_out, const int *seq, const int *row0, const long *pos0,
                                                   const float *inv_freq, const int *block_table, long ld_table, int num_pages,
                                                   int page_size, int max_pages, int kv_fmt, int R, int S, int B, int nq, int nkv, int hd,
                                                   float scale, void *ws, long ws_bytes, void *stream) {
    const PageArgs pg{block_table, ld_table, num_pages, page_size, max_pages};
    const bool any_null = !block_table || !q || !k || !v || !kpool || !vpool || !out_f16 || !seq || !row0 || !pos0 || !inv_freq;
    return paged_entry(any_null, pg, kv_fmt, [&](auto ct, int shift, long max_len) {
        return attn_rope_ragged<decltype(ct), true>(q, k, v, ld_qkv, kpool, vpool, out_f16, ld_out, seq, row0, pos0, inv_freq, R, S, B, nq, nkv,
                                                    hd, max_len, scale, ws, ws_bytes, stream, &pg, shift);
    });
}

extern "C" int qpal_attn_rope_prefill_ragged_window(const float *q, const float *k, const float *v, long ld_qkv, void *kcache, void *vcache,
                                                    void *out_f16, long ld_out, const int *seq, const int *row0, const long *pos0,
                                                    const float *inv_freq, const int *block_table, long ld_table, int num_pages,
                                                    int page_size, int max_pages, int kv_fmt, int R, int S, int B, int nq, int nkv, int hd,
                                                    long max_len, float scale, long window, void *ws, long ws_bytes, void *stream) {
    if (!q || !k || !v || !kcache || !vcache || !out_f16 || !seq || !row0 || !pos0 || !inv_freq) return QPAL_E_NULL;
    if (window < 0) return QPAL_E_PARAM;
    if (kv_fmt != 0 && kv_fmt != 1) return QPAL_E_SHAPE;
    auto launch = [&](auto ct, auto paged, auto win, long len, const PageArgs *pg, int shift) {
        return attn_rope_ragged<decltype(ct), paged(), win()>(q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, seq, row0, pos0, inv_freq, R, S, B,
                                                             nq, nkv, hd, len, scale, ws, ws_bytes, stream, pg, shift, window);
    };
    using Y = std::true_type;
    using N = std::false_type;
    if (!block_table) {  // contiguous caches [B][nkv][max_len][hd]
        return for_kv_fmt(kv_fmt, [&](auto ct) {
            return window ? launch(ct, N{}, Y{}, max_len, nullptr, 0) : launch(ct, N{}, N{}, max_len, nullptr, 0);
        });
    }
    const PageArgs pg{block_table, ld_table, num_pages, page_size, max_pages};
    return paged_entry(false, pg, kv_fmt, [&](auto ct, int shift, long len) {
        return window ? launch(ct, Y{}, Y{}, len, &pg, shift) : launch(ct, Y{}, N{}, len, &pg, shift);
    });
}

extern "C" int qpal_attn_rope_prefill_ragged_score(const float *q, const float *k, const float *v, long ld_qkv, void *kcache, void *vcache,
                                                   void *out_f16, long ld_out, const int *seq, const int *row0, const long *pos0,
                                                   const float *inv_freq, const int *block_table, long ld_table, int num_pages,
                                                   int page_size, int max_pages, int kv_fmt, int R, int S, int B, int nq, int nkv, int hd,
                                                   long max_len, float scale, long window, float softcap, const float *sinks, void *ws,
                                                   long ws_bytes, void *stream) {
    if (!q || !k || !v || !kcache || !vcache || !out_f16 || !seq || !row0 || !pos0 || !inv_freq) return QPAL_E_NULL;
    if (window < 0 || !score_mods_ok(softcap)) return QPAL_E_PARAM;
    if (softcap == 0.f && !sinks)
        return qpal_attn_rope_prefill_ragged_window(q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, seq, row0, pos0, inv_freq, block_table,
                                                    ld_table, num_pages, page_size, max_pages, kv_fmt, R, S, B, nq, nkv, hd, max_len, scale,
                                                    window, ws, ws_bytes, stream);
    if (kv_fmt != 0 && kv_fmt != 1) return QPAL_E_SHAPE;
    const ScoreMods mods{softcap, sinks};
    auto launch = [&](auto ct, auto paged, long len, const PageArgs *pg, int shift) {
        return attn_rope_ragged<decltype(ct), paged(), true, true>(q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, seq, row0, pos0, inv_freq, R,
                                                                  S, B, nq, nkv, hd, len, scale, ws, ws_bytes, stream, pg, shift, window,
                                                                  &mods);
    };
    if (!block_table)  // contiguous caches [B][nkv][max_len][hd]
        return for_kv_fmt(kv_fmt, [&](auto ct) { return launch(ct, std::false_type{}, max_len, nullptr, 0); });
    const PageArgs pg{block_table, ld_table, num_pages, page_size, max_pages};
    return paged_entry(false, pg, kv_fmt, [&](auto ct, int shift, long len) { return launch(ct, std::true_type{}, len, &pg, shift); });
}
