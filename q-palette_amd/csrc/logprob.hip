// qpal_token_logprob: log-softmax of up to 128 rows of fp32 logits, each evaluated at ONE token — the log-probability a sampler
// reports for the token it drew and the per-position term of a cross-entropy (decoder.Score); with it the row's log-sum-exp and
// the token's rank (include/qpal.h and DESIGN.md §15 have the contract word for word).  The distribution is the plain softmax of
// the raw logits: temperature 1, no top-k / top-p.
//
// Workgroup = one row, 16 waves, as in sample.hip: a 128 k row (513 KB) does not fit LDS and is read from L2 once per pass.
//   pass 1   the row maximum (NaN reads as -inf)
//   pass 2   sum of expf(l - max) and the count of logits strictly above the token's
// Every sum has a fixed order — at most 128 serial adds per lane, the wave's DPP tree, a tree over the 16 waves — so two launches
// are bitwise equal.  The count compares raw fp32 values and is exact.  One thread combines max, log(sum) and the token's logit in
// fp64, so the result is rounded once at the magnitude of the logits.  No atomics, no workspace, vector stores only.
#include <hip/hip_runtime.h>

#include "qpal_common.h"

namespace qpal {

struct LogprobParams {
    const float *logits;
    long ld;
    int rows, vocab;
    const long long *token, *active;
    float *logprob, *lse;
    int *rank;
};

__global__ __launch_bounds__(1024) void token_logprob_kernel(const LogprobParams p) {
    __shared__ float redf[16];
    __shared__ int redi[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long tok = p.token[b];
    if (tok < 0 || tok >= p.vocab || (p.active && p.active[b] < 0)) return;  // inactive row: no output is written
    const int vocab = p.vocab;
    const float *row = p.logits + (long)b * p.ld;
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    float lt = row[tok];
    if (lt != lt) lt = kNegInf;

    float mx = kNegInf;
    row_pass4(row, vocab, vec, [&](int, int n, const float (&v)[4]) {
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (e < n && v[e] > mx) mx = v[e];  // (a NaN is never above)
    });
    mx = wave_max(mx);
    if (lane == 0) redf[wave] = mx;
    __syncthreads();
    mx = redf[0];
#pragma unroll
    for (int w = 1; w < 16; w++) mx = fmaxf(mx, redf[w]);
    __syncthreads();  // (redf is rewritten below)

    float s = 0.f;
    int above = 0;
    row_pass4(row, vocab, vec, [&](int, int n, const float (&v)[4]) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (e >= n) continue;
            above += v[e] > lt;
            const float d = v[e] - mx;  // NaN: a NaN logit (weight 0), or inf - inf (+inf rows: the +inf entries share the mass)
            s += d == d ? expf(d) : (v[e] == mx ? 1.0f : 0.f);
        }
    });
    s = wave_sum(s);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) above += __shfl_xor(above, m, 64);
    if (lane == 0) {
        redf[wave] = s;
        redi[wave] = above;
    }
    __syncthreads();
    if (tid != 0) return;
    float part[16];
#pragma unroll
    for (int w = 0; w < 16; w++) part[w] = redf[w];
#pragma unroll
    for (int st = 1; st < 16; st <<= 1)
#pragma unroll
        for (int w = 0; w < 16; w += 2 * st) part[w] += part[w + st];
    above = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) above += redi[w];
    float lp, ls;
    if (mx == kNegInf) {  // no logit above -inf: nothing has a probability (above == 0)
        lp = ls = kNegInf;
    } else if (mx == -kNegInf) {
        ls = mx;
        lp = lt == mx ? -logf(part[0]) : kNegInf;
    } else {
        const double lg = (double)logf(part[0]);  // part[0] >= 1: the maximum's own term
        ls = (float)((double)mx + lg);
        lp = (float)(((double)lt - (double)mx) - lg);
    }
    p.logprob[b] = lp;
    if (p.lse) p.lse[b] = ls;
    if (p.rank) p.rank[b] = above;
}

}  // namespace qpal

using namespace qpal;

extern "C" int qpal_token_logprob(const float *logits_f32, long ld_logits, int rows, int vocab, const long long *token, float *logprob,
                                  float *lse, int *rank, const long long *active, void *stream) {
    if (!logits_f32 || !token || !logprob) return QPAL_E_NULL;
    if (rows < 1 || rows > 128 || vocab < 1 || vocab > (1 << 30) || ld_logits < vocab) return QPAL_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(logits_f32) & 3) || (reinterpret_cast<uintptr_t>(token) & 7) || (reinterpret_cast<uintptr_t>(logprob) & 3) ||
        (reinterpret_cast<uintptr_t>(lse) & 3) || (reinterpret_cast<uintptr_t>(rank) & 3) || (reinterpret_cast<uintptr_t>(active) & 7))
        return QPAL_E_ALIGN;
    LogprobParams p{logits_f32, ld_logits, rows, vocab, token, active, logprob, lse, rank};
    hipLaunchKernelGGL(token_logprob_kernel, dim3(rows), dim3(1024), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}
