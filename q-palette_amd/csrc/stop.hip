// Stop conditions on the device: stop strings (a byte-level Aho-Corasick automaton per stop set), stop token ids, token budgets and
// the context limit, judged by ONE launch at the end of a step (DESIGN.md §33 has the contract word for word;
// stop.reference_stop_advance / reference_stop_mask restate it in numpy and the kernels equal them bit for bit).
//
//   stop_advance_kernel  grid = slots, ONE wave per slot.  The wave first fetches what the walk will read: four lanes per token load
//                        the token id and its two offsets and copy the first 64 bytes of the token into LDS (a token's bytes sit
//                        anywhere in tok_bytes: byte loads), sixteen lanes load the slot's stop ids.  Behind one barrier lane 0
//                        judges the tokens in order: the walk through trans is a chain of dependent loads, one per byte, which no
//                        second lane could shorten.  Bytes past a token's first 64 are read where they lie.  Lane 0 is the one
//                        writer of every word of the slot; no workspace, no atomics: equal launches leave equal bits.
//   stop_mask_kernel     one workgroup of 256 threads, thread (r, i) writes -inf at stop id i of row r's slot while the slot is
//                        below its min_tokens: at most 16 words per row.  The logits are not read.
// Every index read from device memory (set id, number of states, automaton state, token id, token offsets, the next state out of
// the table, stop ids, slot) is compared with its range before it addresses anything.
#include <hip/hip_runtime.h>

#include "qpal.h"
#include "qpal_common.h"

namespace qpal {

constexpr int kStopMaxSlots = 128, kStopMaxRows = 128, kStopMaxWidth = 16, kStopMaxSets = 256, kStopMaxIds = 16;
constexpr int kStopMaxStates = 65535;
constexpr int kStopWave = 64, kStopTokLanes = kStopWave / kStopMaxWidth;  // four lanes fetch one token
constexpr int kStopStage = 64;                                            // bytes of a token that the wave copies into LDS
constexpr int kStopMaskThreads = 256;
enum { kStopRunning = 0, kStopId = 1, kStopString = 2, kStopMaxTokens = 3, kStopContext = 4 };

struct StopAdvanceParams {
    qpal_stop_bank k;
    const int *tok_off;              // [vocab + 1]
    const unsigned char *tok_bytes;  // [total]
    int vocab, total, width;
    const long *tokens;  // [slots][width]
    int *n_out;          // [slots], speculative mode; null: decode mode
    long *n_tok, *limit;  // [slots], speculative mode
    long *tok, *pos;      // [slots], decode mode
    long max_len;
};

__global__ __launch_bounds__(kStopWave) void stop_advance_kernel(const StopAdvanceParams p) {
    __shared__ unsigned char s_bytes[kStopMaxWidth * kStopStage];
    __shared__ long s_tok[kStopMaxWidth];
    __shared__ int s_off[kStopMaxWidth], s_len[kStopMaxWidth];  // s_len -1: the id is no token of the vocabulary
    __shared__ int s_ids[kStopMaxIds];
    const int b = blockIdx.x, lane = threadIdx.x;
    const bool spec = p.n_out != nullptr;
    // ---- which tokens (uniform in the wave: every lane reads the same words)
    int m;
    long next0;  // the position the first token would be fed at
    if (spec) {
        m = p.n_out[b];
        m = m < 0 ? 0 : (m > p.width ? p.width : m);
        next0 = p.n_tok[b] - m;
    } else {
        const long pos = p.pos[b];
        m = (pos >= 0 && pos < p.max_len) ? 1 : 0;
        next0 = pos + 1;
    }
    if (m == 0) return;
    // ---- the wave's fetch: ids, offsets, the first bytes of every token, the slot's stop ids
    {
        const int j = lane / kStopTokLanes, q = lane % kStopTokLanes;
        if (j < m) {
            const long t = p.tokens[(long)b * p.width + j];
            int o0 = 0, len = -1;
            if (t >= 0 && t < p.vocab) {
                o0 = p.tok_off[t];
                const int o1 = p.tok_off[t + 1];
                len = (o0 < 0 || o1 > p.total || o1 < o0) ? 0 : o1 - o0;  // offsets that describe no bytes of the table: none
            }
            const int staged = len < kStopStage ? len : kStopStage;
            for (int i = q; i < staged; i += kStopTokLanes) s_bytes[j * kStopStage + i] = p.tok_bytes[o0 + i];
            if (q == 0) {
                s_tok[j] = t;
                s_off[j] = o0;
                s_len[j] = len;
            }
        }
        if (lane < kStopMaxIds) s_ids[lane] = lane < p.k.id_slots ? p.k.stop_ids[(long)b * p.k.id_slots + lane] : -1;
    }
    __syncthreads();
    if (lane != 0) return;
    // ---- lane 0: the slot's automaton and criteria
    int S = 0;
    const int g = p.k.set_id[b];
    if (g >= 0 && g < p.k.sets) {
        S = p.k.n_states[g];
        if (S < 1 || S > p.k.max_states) S = 0;
    }
    const unsigned short *trans = p.k.trans + (long)(S ? g : 0) * p.k.max_states * 256;
    const unsigned short *out_len = p.k.out_len + (long)(S ? g : 0) * p.k.max_states;
    int nid = p.k.n_ids[b];
    nid = nid < 0 ? 0 : (nid > p.k.id_slots ? p.k.id_slots : nid);
    const int max_tokens = p.k.max_tokens[b], min_tokens = p.k.min_tokens[b];
    int n = p.k.n_gen[b];
    long bytes = p.k.gen_bytes[b];
    int s = p.k.ac_state[b];
    if (s < 0 || s >= S) s = 0;
    bool walked = false;
    int reason = kStopRunning, hit = 0, j = 0;
    long text_len = 0, t = 0;
    for (; j < m; j++) {
        t = s_tok[j];
        n++;
        if (n >= 1 && n <= p.k.cap) p.k.out[(long)b * p.k.cap + (n - 1)] = t;
        const bool exempt = n < min_tokens;
        bool is_id = false;
        if (!exempt)
            for (int i = 0; i < nid; i++) is_id |= (long)s_ids[i] == t;
        const int len = s_len[j];
        if (is_id) {
            reason = kStopId;
            text_len = bytes;
        } else if (len >= 0) {
            if (S == 0) {
                bytes += len;
            } else {
                walked = true;
                const unsigned char *rest = p.tok_bytes + s_off[j];
                for (int i = 0; i < len; i++) {
                    const unsigned c = i < kStopStage ? s_bytes[j * kStopStage + i] : rest[i];
                    const unsigned nx = trans[(long)s * 256 + c];
                    s = nx < (unsigned)S ? (int)nx : 0;
                    bytes++;
                    if (!exempt) {
                        const int ol = out_len[s];
                        if (ol > 0) {
                            reason = kStopString;
                            text_len = bytes - ol;
                            hit = s;
                            break;
                        }
                    }
                }
            }
        }
        if (reason == kStopRunning && max_tokens > 0 && n >= max_tokens) {
            reason = kStopMaxTokens;
            text_len = bytes;
        }
        if (reason == kStopRunning && next0 + j >= p.max_len) {
            reason = kStopContext;
            text_len = bytes;
        }
        if (reason != kStopRunning) break;
    }
    // ---- the slot's words, each written here and nowhere else
    p.k.n_gen[b] = n;
    p.k.gen_bytes[b] = bytes;
    if (walked) p.k.ac_state[b] = s;
    if (reason != kStopRunning) {
        p.k.reason[b] = reason;
        p.k.text_len[b] = text_len;
        if (reason == kStopString) p.k.hit[b] = hit;
        p.k.end_pos[b] = next0 + j;
    }
    if (spec) {
        if (reason != kStopRunning) {
            p.n_out[b] = j + 1;
            p.n_tok[b] = next0 + j + 1;
            p.limit[b] = next0 + j + 1;
        }
    } else if (reason != kStopRunning) {
        p.pos[b] = -1;
    } else {
        p.tok[b] = t;
        p.pos[b] = next0;
    }
}

struct StopMaskParams {
    float *logits;
    long ld;
    int rows, vocab;
    const int *row_slot;
    const long *ctr;
    const int *row0;  // [slots + 1] or null: every row is the first of its slot
    const int *stop_ids;
    int id_slots;
    const int *n_ids, *min_tokens, *n_gen;
    int slots;
};

__global__ __launch_bounds__(kStopMaskThreads) void stop_mask_kernel(const StopMaskParams p) {
    for (int idx = threadIdx.x; idx < p.rows * kStopMaxIds; idx += kStopMaskThreads) {
        const int r = idx / kStopMaxIds, i = idx % kStopMaxIds;
        const int b = p.row_slot[r];
        if (p.ctr[r] < 0 || b < 0 || b >= p.slots) continue;
        long j = 0;
        if (p.row0) {
            const int first = p.row0[b];
            j = (long)r - first;
            if (first < 0 || j < 0 || j >= kStopMaxWidth) continue;
        }
        if ((long)p.n_gen[b] + j >= (long)p.min_tokens[b]) continue;
        int nid = p.n_ids[b];
        nid = nid > p.id_slots ? p.id_slots : nid;
        if (i >= nid) continue;
        const int id = p.stop_ids[(long)b * p.id_slots + i];
        if (id >= 0 && id < p.vocab) p.logits[(long)r * p.ld + id] = kNegInf;
    }
}

}  // namespace qpal

using namespace qpal;

static inline bool misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

extern "C" int qpal_stop_advance(const qpal_stop_bank *bank, const int *tok_off, const unsigned char *tok_bytes, int vocab,
                                 int total_bytes, int slots, const long *tokens, int width, int *n_out, long *n_tok, long *limit,
                                 long *tok, long *pos, long max_len, void *stream) {
    if (!bank || !tok_off || !tok_bytes || !tokens) return QPAL_E_NULL;
    const qpal_stop_bank &k = *bank;
    if (!k.trans || !k.out_len || !k.n_states || !k.set_id || !k.ac_state || !k.stop_ids || !k.n_ids || !k.max_tokens || !k.min_tokens ||
        !k.n_gen || !k.gen_bytes || !k.out || !k.reason || !k.text_len || !k.hit || !k.end_pos)
        return QPAL_E_NULL;
    if (n_out ? (!n_tok || !limit) : (!tok || !pos)) return QPAL_E_NULL;
    if (slots < 1 || slots > kStopMaxSlots || width < 1 || width > kStopMaxWidth || k.sets < 1 || k.sets > kStopMaxSets ||
        k.max_states < 1 || k.max_states > kStopMaxStates || k.id_slots < 1 || k.id_slots > kStopMaxIds || k.cap < 1 || vocab < 1 ||
        vocab > (1 << 30) || total_bytes < 0 || max_len < 1)
        return QPAL_E_SHAPE;
    if (!n_out && width != 1) return QPAL_E_PARAM;  // decode mode judges one token per slot
    if (misaligned(k.trans, 2) || misaligned(k.out_len, 2) || misaligned(k.n_states, 4) || misaligned(k.set_id, 4) ||
        misaligned(k.ac_state, 4) || misaligned(k.stop_ids, 4) || misaligned(k.n_ids, 4) || misaligned(k.max_tokens, 4) ||
        misaligned(k.min_tokens, 4) || misaligned(k.n_gen, 4) || misaligned(k.gen_bytes, 8) || misaligned(k.out, 8) ||
        misaligned(k.reason, 4) || misaligned(k.text_len, 8) || misaligned(k.hit, 4) || misaligned(k.end_pos, 8) ||
        misaligned(tok_off, 4) || misaligned(tokens, 8) || misaligned(n_out, 4) || misaligned(n_tok, 8) || misaligned(limit, 8) ||
        misaligned(tok, 8) || misaligned(pos, 8))
        return QPAL_E_ALIGN;
    StopAdvanceParams p{k, tok_off, tok_bytes, vocab, total_bytes, width, tokens, n_out, n_tok, limit, tok, pos, max_len};
    hipLaunchKernelGGL(stop_advance_kernel, dim3((unsigned)slots), dim3(kStopWave), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

extern "C" int qpal_stop_mask(float *logits, long ld_logits, int rows, int vocab, const int *row_slot, const long *ctr,
                              const int *row0, const int *stop_ids, int id_slots, const int *n_ids, const int *min_tokens,
                              const int *n_gen, int slots, void *stream) {
    if (!logits || !row_slot || !ctr || !stop_ids || !n_ids || !min_tokens || !n_gen) return QPAL_E_NULL;
    if (rows < 1 || rows > kStopMaxRows || vocab < 1 || vocab > (1 << 30) || ld_logits < vocab || id_slots < 1 ||
        id_slots > kStopMaxIds || slots < 1 || slots > kStopMaxSlots)
        return QPAL_E_SHAPE;
    if (misaligned(logits, 4) || misaligned(row_slot, 4) || misaligned(ctr, 8) || misaligned(row0, 4) || misaligned(stop_ids, 4) ||
        misaligned(n_ids, 4) || misaligned(min_tokens, 4) || misaligned(n_gen, 4))
        return QPAL_E_ALIGN;
    StopMaskParams p{logits, ld_logits, rows, vocab, row_slot, ctr, row0, stop_ids, id_slots, n_ids, min_tokens, n_gen, slots};
    hipLaunchKernelGGL(stop_mask_kernel, dim3(1), dim3(kStopMaskThreads), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}
