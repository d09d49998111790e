// qpal_spec_draft / qpal_spec_accept: the two ends of a speculative decode step (DESIGN.md §19 has the contracts word for word).
//
// The step in between is a ragged prefill step (§18): slot b contributes its pending token and up to K guessed tokens as ONE
// segment, the sampler draws at every row the token the model would have drawn at that position, and accept keeps the guesses that
// equal those draws.  Everything lives on the device and the host reads nothing: a captured step is replayed while the state moves.
//
//   spec_search_kernel   one workgroup (4 waves) per slot: how many drafts the slot proposes and where they start.  Prompt lookup is
//                        ONE pass over the history: for every end position e the length m(e) <= gmax of the common suffix of
//                        hist[0 .. e) and hist[0 .. n), and a max-reduction of the key (m(e), e) — the longest gram wins, the most
//                        recent occurrence among its matches (what "g = gmax down to gmin, largest j" selects).
//   spec_pack_kernel     one workgroup: the prefix sum over <= 128 slots in LDS, the cut at R rows, and every output array.
//   spec_accept_kernel   one workgroup, one thread per slot: <= 16 rows each.
// Two launches for the draft: a slot's first row depends on every earlier slot's count, and the only single-launch forms are a
// last-arriver ticket (a global atomic and a word of workspace) or 128 serial searches in one workgroup.  Between the two launches
// n_draft[b] holds the slot's uncut draft count and pos0[b] the history index its drafts start at; the pack launch overwrites both.
// No atomics, one writer per output word, vector stores only: two launches on one state are bitwise equal.
#include <hip/hip_runtime.h>

#include "qpal_common.h"

namespace qpal {

constexpr int kSpecMaxSlots = 128, kSpecMaxDraft = 15, kSpecMaxGram = 8, kSpecSearchThreads = 256;

struct SpecDraftParams {
    const int *hist;
    long ld_hist;
    const long *n_tok, *limit;
    const long *ext_draft;
    const int *ext_n;
    int B, K, gmin, gmax, R;
    long max_len;
    long *tokens;
    int *seq, *row0;
    long *pos0;
    int *row_slot;
    long *row_ctr;
    int *n_draft;
};

// the slot rule of both kernels: 1 <= n_tok < limit, n_tok <= max_len, n_tok <= ld_hist
__device__ __forceinline__ bool spec_active(long n, long lim, long max_len, long ld_hist) {
    return n >= 1 && n < lim && n <= max_len && n <= ld_hist;
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
    return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(kSpecSearchThreads) void spec_search_kernel(const SpecDraftParams p) {
    __shared__ unsigned long long red[kSpecSearchThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long n = p.n_tok[b], lim = p.limit[b];
    int nd = 0;
    long src = 0;
    if (spec_active(n, lim, p.max_len, p.ld_hist)) {  // (uniform in the workgroup)
        long dm = lim - n - 1 < p.max_len - n ? lim - n - 1 : p.max_len - n;
        const int d_max = (int)(dm < 0 ? 0 : (dm > p.K ? p.K : dm));
        if (p.ext_draft) {
            if (tid == 0) {
                const int en = p.ext_n[b] < d_max ? p.ext_n[b] : d_max;
                const long *e = p.ext_draft + (long)b * p.K;
                while (nd < en && e[nd] >= 0 && e[nd] < (1l << 30)) nd++;
            }
        } else if (d_max > 0 && n >= 2) {
            const int *h = p.hist + (long)b * p.ld_hist;
            const bool vec = (reinterpret_cast<uintptr_t>(h) & 15) == 0;
            const int nn = (int)n;  // n <= ld_hist < 2^31
            int s[kSpecMaxGram];    // the suffix, last token first
#pragma unroll
            for (int i = 0; i < kSpecMaxGram; i++) s[i] = i < nn ? h[nn - 1 - i] : 0;
            // candidates: the match's last token p in [0, n - 2] (drafts start at e = p + 1 < n); a thread takes four at a time,
            // p = 4 q + c, and the 12 tokens 4 q - 8 .. 4 q + 3 they look back on
            unsigned long long best = 0ull;
            const int nquad = (nn - 1 + 3) >> 2;
            for (int q = tid; q < nquad; q += kSpecSearchThreads) {
                int w[12];
                const int i0 = 4 * q - 8;
#pragma unroll
                for (int v = 0; v < 3; v++) {
                    const int at = i0 + 4 * v;
                    if (at < 0) {
                        w[4 * v] = w[4 * v + 1] = w[4 * v + 2] = w[4 * v + 3] = 0;  // (never compared: p - i >= 0 is tested)
                    } else if (vec && at + 4 <= nn) {
                        const int4 t = *reinterpret_cast<const int4 *>(h + at);
                        w[4 * v] = t.x; w[4 * v + 1] = t.y; w[4 * v + 2] = t.z; w[4 * v + 3] = t.w;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; e++) w[4 * v + e] = at + e < nn ? h[at + e] : 0;
                    }
                }
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const int pp = 4 * q + c;
                    if (pp > nn - 2) continue;
                    int m = 0;
                    bool run = true;
#pragma unroll
                    for (int i = 0; i < kSpecMaxGram; i++) {
                        run = run && i < p.gmax && pp - i >= 0 && w[8 + c - i] == s[i];
                        m += run ? 1 : 0;
                    }
                    const unsigned long long key = ((unsigned long long)m << 32) | (uint32_t)pp;
                    if (m >= p.gmin && key > best) best = key;
                }
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const unsigned long long o = shfl_xor_u64(best, m);
                best = o > best ? o : best;
            }
            if ((tid & 63) == 0) red[tid >> 6] = best;
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < kSpecSearchThreads / 64; w++) best = red[w] > best ? red[w] : best;
                if (best != 0ull) {
                    src = (long)(uint32_t)best + 1;
                    const long left = n - src;
                    nd = (int)(left < d_max ? left : d_max);
                }
            }
        }
    }
    if (tid == 0) {
        p.n_draft[b] = nd;
        p.pos0[b] = src;
    }
}

__global__ __launch_bounds__(kSpecMaxSlots) void spec_pack_kernel(const SpecDraftParams p) {
    __shared__ int sc_act[kSpecMaxSlots], sc_d[kSpecMaxSlots];
    const int t = threadIdx.x, B = p.B, R = p.R;
    long n = 0;
    bool act = false;
    int d = 0;
    long src = 0;
    if (t < B) {
        n = p.n_tok[t];
        act = spec_active(n, p.limit[t], p.max_len, p.ld_hist);
        d = act ? p.n_draft[t] : 0;
        d = d < 0 ? 0 : (d > p.K ? p.K : d);
        src = p.pos0[t];
        if (!p.ext_draft) {  // what the search launch left, held to the history whatever it is: no read past hist[n - 1]
            if (src < 1 || src >= n) d = 0;
            else if (n - src < d) d = (int)(n - src);
        }
    }
    sc_act[t] = act ? 1 : 0;
    sc_d[t] = d;
    __syncthreads();
#pragma unroll 1
    for (int off = 1; off < kSpecMaxSlots; off <<= 1) {  // inclusive scans of both counts
        const int a = t >= off ? sc_act[t - off] : 0, dd = t >= off ? sc_d[t - off] : 0;
        __syncthreads();
        sc_act[t] += a;
        sc_d[t] += dd;
        __syncthreads();
    }
    // drafts are handed out in slot order from what the pending rows leave of R: slot b gets clamp(E - (drafts before it), 0, d)
    const int E = R - sc_act[kSpecMaxSlots - 1];  // >= 0: R >= B
    const int a_incl = sc_act[t], d_incl = sc_d[t];
    const int a_before = a_incl - (act ? 1 : 0), d_before = d_incl - d;
    const int given_before = d_before < E ? d_before : E;
    int given = E - d_before;
    given = given < 0 ? 0 : (given > d ? d : given);
    const int r0 = a_before + given_before;
    const int d_all = sc_d[kSpecMaxSlots - 1];
    const int total = sc_act[kSpecMaxSlots - 1] + (d_all < E ? d_all : E);
    if (t < B) {
        const int rows = act ? 1 + given : 0;
        if (t == 0) p.row0[0] = 0;
        p.row0[t + 1] = r0 + rows;
        p.seq[t] = act ? t : -1;
        p.pos0[t] = n - 1;
        p.n_draft[t] = given;
        if (act) {
            const int *h = p.hist + (long)t * p.ld_hist;
            p.tokens[r0] = h[n - 1];
            for (int i = 0; i < given; i++)
                p.tokens[r0 + 1 + i] = p.ext_draft ? p.ext_draft[(long)t * p.K + i] : (long)h[src + i];
            for (int i = 0; i < rows; i++) {
                p.row_slot[r0 + i] = t;
                p.row_ctr[r0 + i] = n - 1 + i;
            }
        }
    }
    for (int r = total + t; r < R; r += kSpecMaxSlots) {
        p.tokens[r] = 0;
        p.row_slot[r] = -1;
        p.row_ctr[r] = -1;
    }
}

struct SpecAcceptParams {
    const long *tokens, *drawn;
    const int *seq, *row0;
    int *hist;
    long ld_hist;
    long *n_tok, *limit;
    const long *eos;
    int B, K, R;
    long *out_tok;
    int *n_out, *n_acc;
};

__global__ __launch_bounds__(kSpecMaxSlots) void spec_accept_kernel(const SpecAcceptParams p) {
    const int b = threadIdx.x;
    if (b >= p.B) return;
    const int r = p.row0[b], T = p.row0[b + 1] - r;
    const long n = p.n_tok[b], lim = p.limit[b];
    int m = 0, cnt = 0;
    // an active segment: the draft kernel's (seq[b] = b, 1 .. K + 1 rows inside R) on a slot that can still grow
    if (p.seq[b] == b && T >= 1 && T <= p.K + 1 && r >= 0 && r + T <= p.R && n >= 1 && n < lim) {
        while (m < T - 1 && p.tokens[r + m + 1] == p.drawn[r + m]) m++;
        cnt = m + 1;
        if (lim - n < cnt) cnt = (int)(lim - n);
        const long stop = p.eos[b];
        bool hit = false;
        int *h = p.hist + (long)b * p.ld_hist;
        for (int i = 0; i < cnt; i++) {
            const long tok = p.drawn[r + i];
            p.out_tok[(long)b * (p.K + 1) + i] = tok;
            if (n + i < p.ld_hist) h[n + i] = (int)tok;
            if (stop >= 0 && tok == stop) {
                cnt = i + 1;
                hit = true;
            }
        }
        p.n_tok[b] = n + cnt;
        if (hit) p.limit[b] = n + cnt;
    }
    p.n_out[b] = cnt;
    p.n_acc[b] = m;
}

}  // namespace qpal

using namespace qpal;

static inline bool misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

extern "C" int qpal_spec_draft(const int *hist, long ld_hist, const long *n_tok, const long *limit, const long *ext_draft,
                               const int *ext_n, int B, int K, int gmin, int gmax, int R, long max_len, long *tokens, int *seq,
                               int *row0, long *pos0, int *row_slot, long *row_ctr, int *n_draft, void *stream) {
    if (!hist || !n_tok || !limit || !tokens || !seq || !row0 || !pos0 || !row_slot || !row_ctr || !n_draft) return QPAL_E_NULL;
    if (ext_draft && !ext_n) return QPAL_E_NULL;
    if (B < 1 || B > kSpecMaxSlots || K < 0 || K > kSpecMaxDraft || gmin < 1 || gmax > kSpecMaxGram || gmin > gmax || R < B ||
        R > 128 || max_len < 1 || ld_hist < 1 || ld_hist > 0x7fffffffl)
        return QPAL_E_SHAPE;
    if (misaligned(hist, 4) || misaligned(n_tok, 8) || misaligned(limit, 8) || misaligned(ext_draft, 8) || misaligned(ext_n, 4) ||
        misaligned(tokens, 8) || misaligned(seq, 4) || misaligned(row0, 4) || misaligned(pos0, 8) || misaligned(row_slot, 4) ||
        misaligned(row_ctr, 8) || misaligned(n_draft, 4))
        return QPAL_E_ALIGN;
    SpecDraftParams p{hist, ld_hist, n_tok, limit, ext_draft, ext_n, B, K, gmin, gmax, R, max_len, tokens, seq, row0, pos0, row_slot,
                      row_ctr, n_draft};
    hipLaunchKernelGGL(spec_search_kernel, dim3(B), dim3(kSpecSearchThreads), 0, static_cast<hipStream_t>(stream), p);
    hipLaunchKernelGGL(spec_pack_kernel, dim3(1), dim3(kSpecMaxSlots), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

extern "C" int qpal_spec_accept(const long *tokens, const long *drawn, const int *seq, const int *row0, int *hist, long ld_hist,
                                long *n_tok, long *limit, const long *eos, int B, int K, int R, long *out_tok, int *n_out, int *n_acc,
                                void *stream) {
    if (!tokens || !drawn || !seq || !row0 || !hist || !n_tok || !limit || !eos || !out_tok || !n_out || !n_acc) return QPAL_E_NULL;
    if (B < 1 || B > kSpecMaxSlots || K < 0 || K > kSpecMaxDraft || R < B || R > 128 || ld_hist < 1 || ld_hist > 0x7fffffffl)
        return QPAL_E_SHAPE;
    if (misaligned(tokens, 8) || misaligned(drawn, 8) || misaligned(seq, 4) || misaligned(row0, 4) || misaligned(hist, 4) ||
        misaligned(n_tok, 8) || misaligned(limit, 8) || misaligned(eos, 8) || misaligned(out_tok, 8) || misaligned(n_out, 4) ||
        misaligned(n_acc, 4))
        return QPAL_E_ALIGN;
    SpecAcceptParams p{tokens, drawn, seq, row0, hist, ld_hist, n_tok, limit, eos, B, K, R, out_tok, n_out, n_acc};
    hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(kSpecMaxSlots), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}
