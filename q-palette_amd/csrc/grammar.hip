// Grammar-constrained decoding: a byte-level deterministic automaton per slot, followed on the device (DESIGN.md §24 has the
// contracts word for word; grammar.reference_allow / reference_rows / reference_mask / reference_advance restate them in numpy and
// the kernels equal them bit for bit).
//
//   grammar_compile_kernel  grid (ceil(vocab / 256), ceil((S + 1) / 8)), 256 threads: a thread owns ONE token and walks its bytes
//                           from each of the workgroup's 8 states (a walk mostly ends at its first byte: the automaton is trimmed);
//                           a wave's 64 verdicts are one ballot = TWO mask words (tokens 64 w .. 64 w + 31 and 64 w + 32 .. 64 w +
//                           63), written by lane 0.  A word has one writer; integer work only: equal launches leave equal bits.
//                           Runs once per load, never in a step.
//   grammar_rows_kernel     one workgroup of 128 threads: thread r first marks row r dead, then (after a barrier) thread b walks
//                           slot b's segment: row first + j gets the state after the j guessed tokens in front of it.
//   grammar_mask_kernel     grid (ceil(vocab / 4096), rows), 256 threads, logit_process_kernel's tile: four groups of four
//                           consecutive tokens per thread.  It reads NO logit: a group whose four bits are clear is one 16-byte
//                           store of -inf where the row base allows, clear bits elsewhere are single stores, set bits are nothing.
//   grammar_advance_kernel  one workgroup of 128 threads, thread b folds slot b's emitted tokens into state[b].
// Every index read from device memory (slot, grammar id, number of states, state, token id, token offsets, the next state out of
// the table) is compared with its range before it addresses anything; out of range means "skip" or "dead", as the contract says.
#include <hip/hip_runtime.h>

#include "qpal_common.h"

namespace qpal {

constexpr int kGramDead = -1;
constexpr int kGramMaxStates = 65534, kGramMaxSlots = 128, kGramMaxRows = 128, kGramMaxWidth = 16, kGramMaxGrammars = 1024;
constexpr int kCompileThreads = 256, kCompileStates = 8;
constexpr int kMaskThreads = 256, kMaskGroups = 4, kMaskTile = kMaskThreads * 4 * kMaskGroups;  // 4096 tokens = 128 mask words
constexpr int kStepThreads = 128;

// the vocabulary as the kernels see it
struct GramVocab {
    const int *tok_off;            // [vocab + 1]
    const unsigned char *tok_bytes;  // [total]
    int vocab, total, eos;
};

// the bytes of token t from state s < S of one automaton: the state they lead to, or kGramDead (an empty token, offsets that do
// not describe bytes of the table, a byte without a transition)
__device__ __forceinline__ int gram_walk(const unsigned short *trans, int S, const GramVocab &v, int s, int t) {
    const int o0 = v.tok_off[t], o1 = v.tok_off[t + 1];
    if (o0 < 0 || o1 > v.total || o1 <= o0) return kGramDead;
    for (int o = o0; o < o1; o++) {
        const unsigned nx = trans[(long)s * 256 + v.tok_bytes[o]];
        if (nx >= (unsigned)S) return kGramDead;  // (0xFFFF: no transition, or no state of this automaton)
        s = (int)nx;
    }
    return s;
}

// one token from state s of an automaton of S states (S: the finished state); the contract's reference_step
__device__ __forceinline__ int gram_step(const unsigned short *trans, const unsigned char *accept, int S, const GramVocab &v, int s,
                                         long t) {
    if (s < 0 || s > S) return kGramDead;
    if (s == S) return t == v.eos ? S : kGramDead;
    if (t == v.eos) return accept[s] ? S : kGramDead;
    if (t < 0 || t >= v.vocab) return kGramDead;
    return gram_walk(trans, S, v, s, (int)t);
}

// ---------------------------------------------------------------------------------------------------------------- compile

struct GramCompileParams {
    const unsigned short *trans;  // [S][256]
    const unsigned char *accept;  // [S]
    int S, words;
    GramVocab v;
    uint32_t *allow;  // [S + 1][ld_allow]
    long ld_allow;
};

__global__ __launch_bounds__(kCompileThreads) void grammar_compile_kernel(const GramCompileParams p) {
    const int t = blockIdx.x * kCompileThreads + threadIdx.x, lane = threadIdx.x & 63;
    const int w0 = (blockIdx.x * kCompileThreads + (threadIdx.x & ~63)) >> 5;  // the wave's first word
    const bool tok = t < p.v.vocab;
    int o0 = 0, o1 = 0;
    if (tok) {
        o0 = p.v.tok_off[t];
        o1 = p.v.tok_off[t + 1];
        if (o0 < 0 || o1 > p.v.total || o1 <= o0) o0 = o1 = 0;  // an empty token, or offsets that describe no bytes: never allowed
    }
    const bool is_eos = tok && t == p.v.eos;
    const int s_end = min(p.S + 1, (int)(blockIdx.y + 1) * kCompileStates);
    for (int s0 = blockIdx.y * kCompileStates; s0 < s_end; s0++) {
        bool ok;
        if (s0 == p.S) {
            ok = is_eos;  // the finished state: eos and nothing else
        } else if (is_eos) {
            ok = p.accept[s0] != 0;  // whatever bytes eos has
        } else {
            ok = o1 > o0;
            int s = s0;
            for (int o = o0; ok && o < o1; o++) {
                const unsigned nx = p.trans[(long)s * 256 + p.v.tok_bytes[o]];
                ok = nx < (unsigned)p.S;
                s = (int)nx;
            }
        }
        const unsigned long long bal = __ballot(ok);  // 64 lanes: two words of the table
        if (lane == 0) {
            uint32_t *row = p.allow + (long)s0 * p.ld_allow;
            if (w0 < p.words) row[w0] = (uint32_t)bal;
            if (w0 + 1 < p.words) row[w0 + 1] = (uint32_t)(bal >> 32);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the bank

// the automata of a bank and the slots' choice among them
struct GramBank {
    const unsigned short *trans;  // [grammars][max_states][256]
    const unsigned char *accept;  // [grammars][max_states]
    const int *n_states;          // [grammars]
    int grammars, max_states;
    const int *gram;  // [slots]; -1: no grammar
    int slots;
};

// slot b's automaton: its number of states S (0: the slot has none, or what the device holds describes none) and its tables
__device__ __forceinline__ int gram_of_slot(const GramBank &k, int b, const unsigned short *&trans, const unsigned char *&accept, int &g) {
    g = k.gram[b];
    if (g < 0 || g >= k.grammars) return 0;
    const int S = k.n_states[g];
    if (S < 1 || S > k.max_states) return 0;
    trans = k.trans + (long)g * k.max_states * 256;
    accept = k.accept + (long)g * k.max_states;
    return S;
}

// ---------------------------------------------------------------------------------------------------------------- rows

struct GramRowsParams {
    GramBank k;
    GramVocab v;
    const int *state;    // [slots]
    const long *tokens;  // [rows]
    const int *row0;     // [slots + 1]
    int rows;
    int *row_state;  // [rows]
};

__global__ __launch_bounds__(kStepThreads) void grammar_rows_kernel(const GramRowsParams p) {
    const int tid = threadIdx.x;
    if (tid < p.rows) p.row_state[tid] = kGramDead;
    __syncthreads();  // the walks below overwrite what this workgroup has just stored
    if (tid >= p.k.slots) return;
    const int first = p.row0[tid], end = p.row0[tid + 1];
    if (first < 0 || end > p.rows || end <= first || end - first > kGramMaxWidth) return;  // no rows, or no segment of a step
    const unsigned short *trans = nullptr;
    const unsigned char *accept = nullptr;
    int g;
    const int S = gram_of_slot(p.k, tid, trans, accept, g);
    if (S == 0) return;
    int s = p.state[tid];
    if (s < 0 || s > S) return;
    p.row_state[first] = s;
    for (int r = first + 1; r < end; r++) {
        s = gram_step(trans, accept, S, p.v, s, p.tokens[r]);
        if (s == kGramDead) return;  // the rows behind stay dead
        p.row_state[r] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------- mask

struct GramMaskParams {
    GramBank k;
    float *logits;
    long ld;
    int rows, vocab;
    const int *row_slot;
    const long *ctr;
    const int *row_state;
    const uint32_t *allow;  // [grammars][max_states + 1][ld_allow]
    long ld_allow;
};

__global__ __launch_bounds__(kMaskThreads) void grammar_mask_kernel(const GramMaskParams p) {
    const int r = blockIdx.y, tid = threadIdx.x, vocab = p.vocab;
    const int base = blockIdx.x * kMaskTile;  // < vocab: the grid has ceil(vocab / tile) tiles
    // ---- the row (uniform in the workgroup)
    const int b = p.row_slot[r];
    if (p.ctr[r] < 0 || b < 0 || b >= p.k.slots) return;
    const int g = p.k.gram[b];
    if (g < 0 || g >= p.k.grammars) return;
    const int S = p.k.n_states[g];
    if (S < 1 || S > p.k.max_states) return;
    const int s = p.row_state[r];
    if (s < 0 || s > S) return;  // dead, or no state of the automaton: the row keeps every bit
    const uint32_t *bits = p.allow + ((long)g * (p.k.max_states + 1) + s) * p.ld_allow;
    float *out = p.logits + (long)r * p.ld;
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    // ---- the four bits of every group, all loads in flight before the stores
    uint32_t nib[kMaskGroups];
#pragma unroll
    for (int q = 0; q < kMaskGroups; q++) {
        const int i0 = base + q * (kMaskThreads * 4) + 4 * tid;
        nib[q] = i0 < vocab ? (bits[i0 >> 5] >> (i0 & 31)) & 0xFu : 0xFu;  // i0 % 4 == 0: the four bits lie in one word
    }
#pragma unroll
    for (int q = 0; q < kMaskGroups; q++) {
        const int i0 = base + q * (kMaskThreads * 4) + 4 * tid;
        if (nib[q] == 0xFu) continue;
        if (nib[q] == 0u && vec && i0 + 4 <= vocab) {
            *reinterpret_cast<float4 *>(out + i0) = make_float4(kNegInf, kNegInf, kNegInf, kNegInf);
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (!((nib[q] >> e) & 1u) && i0 + e < vocab) out[i0 + e] = kNegInf;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- advance

struct GramAdvanceParams {
    GramBank k;
    GramVocab v;
    int *state;          // [slots]
    const long *tokens;  // [slots][width]
    int width;
    const int *n;        // [slots] or null: width tokens
    const long *active;  // [slots] or null
};

__global__ __launch_bounds__(kStepThreads) void grammar_advance_kernel(const GramAdvanceParams p) {
    const int b = threadIdx.x;
    if (b >= p.k.slots || (p.active && p.active[b] < 0)) return;
    const unsigned short *trans = nullptr;
    const unsigned char *accept = nullptr;
    int g;
    const int S = gram_of_slot(p.k, b, trans, accept, g);
    if (S == 0) return;
    int n = p.n ? p.n[b] : p.width;
    n = n < 0 ? 0 : (n > p.width ? p.width : n);
    int s = p.state[b];
    if (s < kGramDead || s > S) s = kGramDead;
    for (int i = 0; i < n && s != kGramDead; i++) s = gram_step(trans, accept, S, p.v, s, p.tokens[(long)b * p.width + i]);
    if (n > 0) p.state[b] = s;
}

}  // namespace qpal

using namespace qpal;

static inline bool misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

static inline bool bad_vocab(int vocab, int total_bytes, int eos) {
    return vocab < 1 || vocab > (1 << 30) || total_bytes < 0 || eos < 0 || eos >= vocab;
}

static inline bool bad_bank(int grammars, int max_states, int slots) {
    return grammars < 1 || grammars > kGramMaxGrammars || max_states < 1 || max_states > kGramMaxStates || slots < 1 ||
           slots > kGramMaxSlots;
}

extern "C" int qpal_grammar_compile(const unsigned short *trans, const unsigned char *accept, int n_states, const int *tok_off,
                                    const unsigned char *tok_bytes, int vocab, int total_bytes, int eos, unsigned *allow,
                                    long ld_allow, void *stream) {
    if (!trans || !accept || !tok_off || !tok_bytes || !allow) return QPAL_E_NULL;
    if (n_states < 1 || n_states > kGramMaxStates || bad_vocab(vocab, total_bytes, eos) || ld_allow < (vocab + 31) / 32)
        return QPAL_E_SHAPE;
    if (misaligned(trans, 2) || misaligned(tok_off, 4) || misaligned(allow, 4)) return QPAL_E_ALIGN;
    GramCompileParams p{trans, accept, n_states, (vocab + 31) / 32, {tok_off, tok_bytes, vocab, total_bytes, eos}, allow, ld_allow};
    const dim3 grid((unsigned)((vocab + kCompileThreads - 1) / kCompileThreads), (unsigned)((n_states + 1 + kCompileStates - 1) / kCompileStates));
    hipLaunchKernelGGL(grammar_compile_kernel, grid, dim3(kCompileThreads), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

extern "C" int qpal_grammar_rows(const unsigned short *trans, const unsigned char *accept, const int *n_states, int grammars,
                                 int max_states, const int *tok_off, const unsigned char *tok_bytes, int vocab, int total_bytes,
                                 int eos, const int *gram, const int *state, int slots, const long *tokens, const int *row0, int rows,
                                 int *row_state, void *stream) {
    if (!trans || !accept || !n_states || !tok_off || !tok_bytes || !gram || !state || !tokens || !row0 || !row_state) return QPAL_E_NULL;
    if (bad_bank(grammars, max_states, slots) || bad_vocab(vocab, total_bytes, eos) || rows < 1 || rows > kGramMaxRows) return QPAL_E_SHAPE;
    if (misaligned(trans, 2) || misaligned(n_states, 4) || misaligned(tok_off, 4) || misaligned(gram, 4) || misaligned(state, 4) ||
        misaligned(tokens, 8) || misaligned(row0, 4) || misaligned(row_state, 4))
        return QPAL_E_ALIGN;
    GramRowsParams p{{trans, accept, n_states, grammars, max_states, gram, slots}, {tok_off, tok_bytes, vocab, total_bytes, eos},
                     state, tokens, row0, rows, row_state};
    hipLaunchKernelGGL(grammar_rows_kernel, dim3(1), dim3(kStepThreads), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

extern "C" int qpal_grammar_mask(float *logits, long ld_logits, int rows, int vocab, const int *row_slot, const long *ctr,
                                 const int *row_state, const int *gram, int slots, const int *n_states, int grammars, int max_states,
                                 const unsigned *allow, long ld_allow, void *stream) {
    if (!logits || !row_slot || !ctr || !row_state || !gram || !n_states || !allow) return QPAL_E_NULL;
    if (bad_bank(grammars, max_states, slots) || rows < 1 || rows > kGramMaxRows || vocab < 1 || vocab > (1 << 30) || ld_logits < vocab ||
        ld_allow < (vocab + 31) / 32)
        return QPAL_E_SHAPE;
    if (misaligned(logits, 4) || misaligned(row_slot, 4) || misaligned(ctr, 8) || misaligned(row_state, 4) || misaligned(gram, 4) ||
        misaligned(n_states, 4) || misaligned(allow, 4))
        return QPAL_E_ALIGN;
    GramMaskParams p{{nullptr, nullptr, n_states, grammars, max_states, gram, slots}, logits, ld_logits, rows, vocab, row_slot, ctr,
                     row_state, allow, ld_allow};
    const dim3 grid((unsigned)(((long)vocab + kMaskTile - 1) / kMaskTile), (unsigned)rows);
    hipLaunchKernelGGL(grammar_mask_kernel, grid, dim3(kMaskThreads), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

extern "C" int qpal_grammar_advance(const unsigned short *trans, const unsigned char *accept, const int *n_states, int grammars,
                                    int max_states, const int *tok_off, const unsigned char *tok_bytes, int vocab, int total_bytes,
                                    int eos, const int *gram, int *state, int slots, const long *tokens, int width, const int *n,
                                    const long *active, void *stream) {
    if (!trans || !accept || !n_states || !tok_off || !tok_bytes || !gram || !state || !tokens) return QPAL_E_NULL;
    if (bad_bank(grammars, max_states, slots) || bad_vocab(vocab, total_bytes, eos) || width < 1 || width > kGramMaxWidth) return QPAL_E_SHAPE;
    if (misaligned(trans, 2) || misaligned(n_states, 4) || misaligned(tok_off, 4) || misaligned(gram, 4) || misaligned(state, 4) ||
        misaligned(tokens, 8) || misaligned(n, 4) || misaligned(active, 8))
        return QPAL_E_ALIGN;
    GramAdvanceParams p{{trans, accept, n_states, grammars, max_states, gram, slots}, {tok_off, tok_bytes, vocab, total_bytes, eos},
                        state, tokens, width, n, active};
    hipLaunchKernelGGL(grammar_advance_kernel, dim3(1), dim3(kStepThreads), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}
