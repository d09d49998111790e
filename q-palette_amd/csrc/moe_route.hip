// Mixture-of-experts routing for the step classes: qpal_moe_route — RMSNorm of the fp32 stream rows, router
// logits, softmax, top-k, gate weights and the expert-sorted layout of the routed pairs, one launch — and qpal_moe_combine, the
// gate-weighted sum of the experts' outputs back into the stream.  qpal_moe_route_ex is the same kernel with the second
// router (sigmoid or softmax scores, a selection-only bias, group-limited top-k, a routed scale, a per-row shared-expert gate) in
// wave 0's selection, and qpal_moe_combine_shared the same combine with a shared expert's rows folded in.
//
// Route: one workgroup (16 waves) per row.  Every expert's logit is accumulated in the same order of operations (a lane's chain over its
// columns, then the wave's fixed tree), so two identical router rows give bitwise equal logits and the tie rule (lower expert id)
// is testable.  The row's chosen experts go out in ascending expert id.  The LAST workgroup to arrive (a ticket: the order of
// arrival decides who sorts, never what comes out) builds the layout of reference_layout (qpalette_amd/moe.py): a counting sort of
// the pairs by (expert, pair id) in LDS — thread e owns expert e and walks the pairs in pair order, so the sort is stable without
// atomics — and the table of groups of at most 8 consecutive positions of one expert, the work items of qpal_moe_gemv.
#include "attn_common.h"

namespace qpal {

namespace {

constexpr int kMoeMaxRows = 128, kMoeMaxExperts = 256, kMoeMaxTopK = 8;
constexpr int kMoeMaxPairs = kMoeMaxRows * kMoeMaxTopK;
constexpr int kMoeMaxH = 8192;  // x̂ of a row in LDS (fp32)
constexpr int kRouteThreads = 1024, kRouteWaves = kRouteThreads / 64;
constexpr int kRouteBatch = 4;  // experts a wave has in flight: their loads are requested together, their sums reduced one by one

struct MoeRouteParams {
    const float *h;
    long ld_h;
    const uint16_t *rms_w;
    float eps;
    const uint16_t *router_w;
    const float *router_bias;
    const long long *active;
    int n, H, E, top_k, renorm, max_groups;
    int *sel;
    float *gate;
    int *order, *inv, *x_index, *group_expert, *group_first, *group_count, *ngroups;
    unsigned *ticket;
    qpal_moe_router rt;  // (read by moe_route_kernel<true> only)
};

__device__ __forceinline__ void st_agent_i(int *p, int v) {
    __hip_atomic_store(as_global(reinterpret_cast<unsigned *>(p)), (unsigned)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_agent_i(const int *p) {
    return (int)__hip_atomic_load(as_global(reinterpret_cast<const unsigned *>(p)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// `rounds` rounds of arg-max over the values a wave holds as v[j] of id lane + 64 j (ids whose `valid` bit j is clear never
// compete): the largest wins, ties to the lower id.  -> the bits j of this lane's winners.  The order of moe_route_kernel's own
// top-k rounds.
__device__ __forceinline__ unsigned route_rounds(const float (&v)[4], unsigned valid, int rounds, int lane) {
    unsigned chosen = 0u;
    for (int t = 0; t < rounds; t++) {
        float b = kNegInf;
        int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int e = lane + 64 * j;
            if (((valid & ~chosen) >> j) & 1u)
                if (v[j] > b || (v[j] == b && e < bi)) b = v[j], bi = e;
        }
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) {
            const float ob = __shfl_xor(b, sh, 64);
            const int oi = __shfl_xor(bi, sh, 64);
            if (ob > b || (ob == b && oi < bi)) b = ob, bi = oi;
        }
        if (bi != 0x7fffffff && (bi & 63) == lane) chosen |= 1u << (bi >> 6);
    }
    return chosen;
}

// EX = false: qpal_moe_route.  EX = true: qpal_moe_route_ex — the shared gate's weight row is one more "expert" of the logit loop,
// and wave 0 selects by the contract of reference_route_ex.
template <bool EX>
__global__ __launch_bounds__(kRouteThreads) void moe_route_kernel(const MoeRouteParams p) {
    __shared__ __attribute__((aligned(16))) float xh[kMoeMaxH];
    __shared__ float logit[kMoeMaxExperts + 1];  // (EX: entry E is the shared gate's dot product)
    __shared__ float red[kRouteThreads / 64];
    __shared__ int sel_s[kMoeMaxTopK];
    __shared__ float prob_s[kMoeMaxTopK];
    __shared__ float key_s[EX ? kMoeMaxExperts : 1];
    __shared__ unsigned char gallow_s[EX ? kMoeMaxExperts : 1];
    __shared__ unsigned flag;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x;
    const bool live = !p.active || p.active[r] >= 0;
    if (live) {  // (workgroup-uniform)
        // ---- RMSNorm in fp32: a thread's chain over its columns, the wave's tree, the sixteen waves in order
        const float *hr = p.h + (long)r * p.ld_h;
        float ss = 0.f;
        for (int i = tid; i < p.H; i += kRouteThreads) {
            const float v = hr[i];
            xh[i] = v;
            ss += v * v;
        }
        ss = wave_sum(ss);
        if (lane == 0) red[wave] = ss;
        __syncthreads();
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < kRouteWaves; w++) tot += red[w];
        const float rs = 1.0f / sqrtf(tot / (float)p.H + p.eps);
        for (int i = tid; i < p.H; i += kRouteThreads) {
            float v = xh[i] * rs;
            if (p.rms_w) v *= (float)__builtin_bit_cast(_Float16, p.rms_w[i]);
            xh[i] = v;
        }
        __syncthreads();
        // ---- logits: wave w takes experts w, w + 16, ..., kRouteBatch of them at a time (one memory round trip for the batch);
        // lane l the 8-column pieces l, l + 64, ... (H % 8 == 0).  Every expert: the same chain of FMAs per lane, the same tree.
        const int npiece = p.H >> 3;
        const int ET = p.E + (EX && p.rt.shared_gate_f16 ? 1 : 0);
        for (int e0 = wave; e0 < ET; e0 += kRouteWaves * kRouteBatch) {
            float a[kRouteBatch];
#pragma unroll
            for (int u = 0; u < kRouteBatch; u++) a[u] = 0.f;
            for (int c = lane; c < npiece; c += 64) {
                u32x4 wv[kRouteBatch];
#pragma unroll
                for (int u = 0; u < kRouteBatch; u++) {
                    const int e = e0 + u * kRouteWaves;
                    const int er = e < ET ? e : e0;  // (past the end: a re-read, unused)
                    const uint16_t *wr = EX && er == p.E ? static_cast<const uint16_t *>(p.rt.shared_gate_f16) : p.router_w + (long)er * p.H;
                    wv[u] = *reinterpret_cast<const u32x4 *>(wr + 8 * c);
                }
                const float4 x0 = *reinterpret_cast<const float4 *>(xh + 8 * c);
                const float4 x1 = *reinterpret_cast<const float4 *>(xh + 8 * c + 4);
                const float xx[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
                for (int u = 0; u < kRouteBatch; u++) {
                    const uint32_t ww[4] = {wv[u].x, wv[u].y, wv[u].z, wv[u].w};
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        a[u] = fmaf((float)__builtin_bit_cast(_Float16, (uint16_t)(ww[j] & 0xffffu)), xx[2 * j], a[u]);
                        a[u] = fmaf((float)__builtin_bit_cast(_Float16, (uint16_t)(ww[j] >> 16)), xx[2 * j + 1], a[u]);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < kRouteBatch; u++) {
                const int e = e0 + u * kRouteWaves;
                float v = wave_sum(a[u]);
                if (e < p.E) {  // (wave-uniform)
                    if (p.router_bias) v += p.router_bias[e];
                    if (lane == 0) logit[e] = v == v ? v : kNegInf;  // (a NaN logit is never chosen)
                } else if (EX && e == p.E && ET > p.E) {
                    if (lane == 0) logit[e] = v;
                }
            }
        }
        __syncthreads();
    }
    // ---- softmax over all experts, top-k (ties to the lower id), gates: wave 0, expert e = lane + 64 j
    if (wave == 0) {
        if (live) {
            float v[4], mx = kNegInf;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int e = lane + 64 * j;
                v[j] = e < p.E ? logit[e] : kNegInf;
                mx = fmaxf(mx, v[j]);
            }
            unsigned chosen = 0u;
            float score[4];  // (EX: the gate of a chosen expert; else ex[j] / sum below)
            float ex[4], sum = 0.f;
            if (!EX || p.rt.scoring == QPAL_MOE_SOFTMAX) {
                mx = wave_max(mx);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    ex[j] = lane + 64 * j < p.E ? expf(v[j] - mx) : 0.f;
                    sum += ex[j];
                }
                sum = wave_sum(sum);
            }
            if constexpr (!EX) {
                for (int t = 0; t < p.top_k; t++) {
                    float b = kNegInf;
                    int bi = 0x7fffffff;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int e = lane + 64 * j;
                        if (e < p.E && !((chosen >> j) & 1u) && (v[j] > b || (v[j] == b && e < bi))) b = v[j], bi = e;
                    }
#pragma unroll
                    for (int sh = 32; sh >= 1; sh >>= 1) {
                        const float ob = __shfl_xor(b, sh, 64);
                        const int oi = __shfl_xor(bi, sh, 64);
                        if (ob > b || (ob == b && oi < bi)) b = ob, bi = oi;
                    }
                    if ((bi & 63) == lane && bi < p.E) chosen |= 1u << (bi >> 6);
                }
#pragma unroll
                for (int j = 0; j < 4; j++) score[j] = ex[j] / sum;
            } else {
                // ---- scores and keys: key = score + select_bias decides who is chosen, the score alone becomes the gate
                float key[4];
                unsigned allowed = 0u;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int e = lane + 64 * j;
                    score[j] = p.rt.scoring == QPAL_MOE_SOFTMAX ? ex[j] / sum : 1.0f / (1.0f + expf(-v[j]));
                    key[j] = kNegInf;
                    if (e < p.E) {
                        key[j] = v[j] == kNegInf ? kNegInf : (p.rt.select_bias ? score[j] + p.rt.select_bias[e] : score[j]);
                        if (!(key[j] == key[j])) key[j] = kNegInf;  // (a NaN key is never preferred)
                        allowed |= 1u << j;
                    }
                }
                if (p.rt.n_group > 1) {
                    // ---- group scores: group g = experts g S .. g S + S - 1, its score in register g >> 6 of lane g & 63
                    const int G = p.rt.n_group, S = p.E / G;
                    const bool top2 = p.rt.group_score == QPAL_MOE_GROUP_TOP2;
                    float gs[4] = {kNegInf, kNegInf, kNegInf, kNegInf};
                    if (S <= G) {  // short groups: lane g walks its own members (S steps)
#pragma unroll
                        for (int j = 0; j < 4; j++) key_s[lane + 64 * j] = key[j];
                        __builtin_amdgcn_wave_barrier();
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const int g = lane + 64 * j;
                            if (g < G) {
                                float m1 = kNegInf, m2 = kNegInf;
                                for (int i = 0; i < S; i++) {
                                    const float k = key_s[g * S + i];
                                    m2 = fmaxf(m2, fminf(m1, k));
                                    m1 = fmaxf(m1, k);
                                }
                                gs[j] = top2 ? m1 + m2 : m1;
                            }
                        }
                    } else {  // few groups: one wave reduction each (G steps); a lane's members of g are at most its four registers
                        for (int g = 0; g < G; g++) {
                            float m1 = kNegInf, m2 = kNegInf;
#pragma unroll
                            for (int j = 0; j < 4; j++) {
                                const int e = lane + 64 * j;
                                if (e >= g * S && e < g * S + S) {
                                    m2 = fmaxf(m2, fminf(m1, key[j]));
                                    m1 = fmaxf(m1, key[j]);
                                }
                            }
#pragma unroll
                            for (int sh = 32; sh >= 1; sh >>= 1) {  // (the two sets are disjoint: equal keys count twice)
                                const float o1 = __shfl_xor(m1, sh, 64), o2 = __shfl_xor(m2, sh, 64);
                                m2 = fmaxf(fminf(m1, o1), fmaxf(m2, o2));
                                m1 = fmaxf(m1, o1);
                            }
                            const float sc = top2 ? m1 + m2 : m1;
#pragma unroll
                            for (int j = 0; j < 4; j++)
                                if (g == lane + 64 * j) gs[j] = sc;
                        }
                    }
                    // ---- the topk_group best groups (ties to the lower group id), then the mask of their experts
                    unsigned gvalid = 0u;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if (lane + 64 * j < G) gvalid |= 1u << j;
                        if (!(gs[j] == gs[j])) gs[j] = kNegInf;
                    }
                    const unsigned gsel = route_rounds(gs, gvalid, p.rt.topk_group, lane);
#pragma unroll
                    for (int j = 0; j < 4; j++) gallow_s[lane + 64 * j] = (unsigned char)((gsel >> j) & 1u);
                    __builtin_amdgcn_wave_barrier();
                    unsigned in_group = 0u;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int e = lane + 64 * j;
                        if (e < p.E && gallow_s[e / S]) in_group |= 1u << j;
                    }
                    allowed &= in_group;
                }
                chosen = route_rounds(key, allowed, p.top_k, lane);
            }
            // ascending expert id: the position of a chosen expert is the number of chosen ones below it
            int below = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const unsigned long long m = __ballot((chosen >> j) & 1u);
                if ((chosen >> j) & 1u) {
                    const int pos = below + __popcll(m & ((1ull << lane) - 1ull));
                    sel_s[pos] = lane + 64 * j;
                    prob_s[pos] = score[j];
                }
                below += __popcll(m);
            }
        }
        __builtin_amdgcn_wave_barrier();  // (one wave: its LDS writes above stay in front of the reads below)
        if (lane < p.top_k) {
            int s = -1;
            float g = 0.f;
            if (live) {
                s = sel_s[lane];
                g = prob_s[lane];
                if (p.renorm) {
                    float den = 0.f;
                    for (int j = 0; j < p.top_k; j++) den += prob_s[j];
                    g = g / den;
                }
                if constexpr (EX) g = g * p.rt.routed_scale;
            }
            st_agent_i(p.sel + r * p.top_k + lane, s);
            p.gate[r * p.top_k + lane] = g;
        }
        if constexpr (EX)
            if (lane == 0 && p.rt.shared_gate_out)  // sigmoid(x̂ · shared_gate), 1 without a gate, 0 on an inactive row
                p.rt.shared_gate_out[r] = !live ? 0.f : (p.rt.shared_gate_f16 ? 1.0f / (1.0f + expf(-logit[p.E])) : 1.0f);
    }
    if (!ticket_last<__ATOMIC_ACQ_REL>(p.ticket, (unsigned)p.n, &flag, tid)) return;

    // ---- the last workgroup to arrive: layout of the P = n * top_k pairs
    __shared__ short pair_e[kMoeMaxPairs];
    __shared__ int cnt[kMoeMaxExperts], start[kMoeMaxExperts], gstart[kMoeMaxExperts];
    __shared__ int totals[2];
    const int P = p.n * p.top_k;
    for (int i = tid; i < P; i += kRouteThreads) {
        const int e = ld_agent_i(p.sel + i);
        pair_e[i] = (short)((unsigned)e < (unsigned)p.E ? e : -1);
    }
    __syncthreads();
    {
        int c = 0;
        if (tid < p.E)
            for (int i = 0; i < P; i++) c += pair_e[i] == tid;
        if (tid < kMoeMaxExperts) cnt[tid] = c;  // (zero above E)
    }
    __syncthreads();
    if (wave == 0) {  // exclusive scans of the counts and of the group counts: lane l owns experts 4 l .. 4 l + 3
        int c[4], g[4], cs = 0, gs = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            c[j] = cnt[4 * lane + j];
            g[j] = (c[j] + 7) >> 3;
            cs += c[j];
            gs += g[j];
        }
        int ci = cs, gi = gs;
#pragma unroll
        for (int sh = 1; sh < 64; sh <<= 1) {
            const int oc = __shfl_up(ci, sh, 64), og = __shfl_up(gi, sh, 64);
            if (lane >= sh) ci += oc, gi += og;
        }
        int c0 = ci - cs, g0 = gi - gs;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            start[4 * lane + j] = c0;
            gstart[4 * lane + j] = g0;
            c0 += c[j];
            g0 += g[j];
        }
        if (lane == 63) totals[0] = ci, totals[1] = gi;
    }
    __syncthreads();
    const int routed = totals[0], ng = totals[1];
    if (tid < p.E) {
        int pos = start[tid];
        for (int i = 0; i < P; i++)
            if (pair_e[i] == tid) {
                p.order[pos] = i;
                p.x_index[pos] = i / p.top_k;
                p.inv[i] = pos;
                pos++;
            }
        const int c = cnt[tid];
        for (int j = 0, g = gstart[tid]; 8 * j < c; j++, g++)
            if (g < p.max_groups) {  // (never false: max_groups bounds ngroups)
                p.group_expert[g] = tid;
                p.group_first[g] = start[tid] + 8 * j;
                p.group_count[g] = c - 8 * j < 8 ? c - 8 * j : 8;
            }
    }
    for (int i = tid; i < P; i += kRouteThreads) {
        if (pair_e[i] < 0) p.inv[i] = -1;
        if (i >= routed) p.order[i] = -1, p.x_index[i] = -1;
    }
    for (int g = ng + tid; g < p.max_groups; g += kRouteThreads) p.group_expert[g] = -1, p.group_first[g] = 0, p.group_count[g] = 0;
    if (tid == 0) {
        *p.ngroups = ng < p.max_groups ? ng : p.max_groups;
        __hip_atomic_store(as_global(p.ticket), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct MoeCombineParams {
    float *out;
    long ld_out;
    const float *y;
    long ld_y;
    const float *gate;
    const int *inv;
    int n, top_k, H, P, accumulate;
    const float *ys;  // (moe_combine_kernel<true> only: the shared expert's rows and their gates)
    long ld_ys;
    const float *sgate;
};

// out[r][c] (+)= sum_j gate[r][j] * y[inv[r][j]][c], j ascending: each product rounded to fp32, added in j order.  SHARED: then
// + fp32(sgate[r] * ys[r][c]) behind the routed sum (alone where the row has no routed pair); a row with sgate[r] == 0 reads no ys
template <bool SHARED>
__global__ __launch_bounds__(256) void moe_combine_kernel(const MoeCombineParams p) {
#pragma clang fp contract(off)  // (a product and the add behind it stay two roundings: the contract's order)
    const int r = blockIdx.y;
    float g[kMoeMaxTopK];
    int src[kMoeMaxTopK];
#pragma unroll
    for (int j = 0; j < kMoeMaxTopK; j++) {
        src[j] = -1, g[j] = 0.f;
        if (j < p.top_k) {
            const int s = p.inv[r * p.top_k + j];
            if ((unsigned)s < (unsigned)p.P) src[j] = s, g[j] = p.gate[r * p.top_k + j];
        }
    }
    float sg = 0.f;
    if constexpr (SHARED) sg = p.sgate[r];
    const bool shared = SHARED && sg != 0.f;  // (an inactive row's gate is exactly 0: whatever ys holds stays out of the stream)
    for (int c = blockIdx.x * 256 + threadIdx.x; c < p.H; c += gridDim.x * 256) {
        float *o = p.out + (long)r * p.ld_out + c;
        float acc = 0.f;
        bool any = false;
#pragma unroll
        for (int j = 0; j < kMoeMaxTopK; j++)
            if (src[j] >= 0) {
                const float t = g[j] * p.y[(long)src[j] * p.ld_y + c];
                acc = any ? acc + t : t;
                any = true;
            }
        if (shared) {
            const float t = sg * p.ys[(long)r * p.ld_ys + c];
            acc = any ? acc + t : t;
            any = true;
        }
        if (p.accumulate) {
            if (any) *o = *o + acc;
        } else {
            *o = acc;
        }
    }
}

// Upper bound of the group count: the largest sum_e ceil(c_e / 8) over 0 <= c_e <= n, sum_e c_e = n * top_k.  N groups over
// a = min(E, N) experts in use (more experts in use never hurt) exist iff N <= a G and 8 N - 7 a <= P <= 8 N - t f, with
// n = 8 G - t and f = max(0, N - a (G - 1)) experts that must hold G groups.  Exact: tests/test_moe_contract.py.
int moe_max_groups(int n, int E, int top_k) {
    if (n < 1 || n > kMoeMaxRows || E < 1 || E > kMoeMaxExperts || top_k < 1 || top_k > kMoeMaxTopK || top_k > E) return 0;
    const int P = n * top_k, G = (n + 7) / 8, t = 8 * G - n;
    int best = 0;
    for (int N = 1; N <= P && N <= E * G; N++) {
        const int a = E < N ? E : N;
        const int f = N - a * (G - 1) > 0 ? N - a * (G - 1) : 0;
        if (N <= a * G && 8 * N - 7 * a <= P && P <= 8 * N - t * f) best = N;
    }
    return best;
}

}  // namespace

}  // namespace qpal

using namespace qpal;

extern "C" int qpal_moe_max_groups(int n, int E, int top_k) { return moe_max_groups(n, E, top_k); }

extern "C" long qpal_moe_route_ws_bytes(int n, int E, int top_k) {
    const int mg = moe_max_groups(n, E, top_k);
    if (!mg) return 0;
    // ticket (16 bytes) | sel, gate, order, inv, x_index [n top_k] | group_expert, group_first, group_count [max_groups] | ngroups
    return 16 + 4L * (5L * n * top_k + 3L * mg + 1);
}

static int moe_route_launch(const float *h_f32, long ld_h, const void *rms_w_f16, float rms_eps, const void *router_w_f16,
                              const float *router_bias, const long long *active, int n, int H, int E, int top_k, int renorm,
                              int *sel, float *gate, int *order, int *inv, int *x_index, int *group_expert, int *group_first,
                              int *group_count, int *ngroups, int max_groups, unsigned *ticket, const qpal_moe_router *router,
                              void *stream) {
    if (!h_f32 || !router_w_f16 || !sel || !gate || !order || !inv || !x_index || !group_expert || !group_first || !group_count ||
        !ngroups || !ticket)
        return QPAL_E_NULL;
    const int mg = moe_max_groups(n, E, top_k);
    if (!mg || H < 8 || H % 8 || H > kMoeMaxH || ld_h < H || max_groups < mg) return QPAL_E_SHAPE;
    if (!(rms_eps > 0.f)) return QPAL_E_PARAM;
    if ((reinterpret_cast<uintptr_t>(router_w_f16) & 15) || (reinterpret_cast<uintptr_t>(rms_w_f16) & 1)) return QPAL_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(h_f32) | reinterpret_cast<uintptr_t>(router_bias) | reinterpret_cast<uintptr_t>(sel) |
         reinterpret_cast<uintptr_t>(gate) | reinterpret_cast<uintptr_t>(order) | reinterpret_cast<uintptr_t>(inv) |
         reinterpret_cast<uintptr_t>(x_index) | reinterpret_cast<uintptr_t>(group_expert) | reinterpret_cast<uintptr_t>(group_first) |
         reinterpret_cast<uintptr_t>(group_count) | reinterpret_cast<uintptr_t>(ngroups) | reinterpret_cast<uintptr_t>(ticket)) & 3)
        return QPAL_E_ALIGN;
    if (reinterpret_cast<uintptr_t>(active) & 7) return QPAL_E_ALIGN;
    qpal_moe_router rt{};
    if (router) {
        rt = *router;
        if (rt.scoring != QPAL_MOE_SOFTMAX && rt.scoring != QPAL_MOE_SIGMOID) return QPAL_E_PARAM;
        if (rt.group_score != QPAL_MOE_GROUP_MAX && rt.group_score != QPAL_MOE_GROUP_TOP2) return QPAL_E_PARAM;
        if (!(rt.routed_scale > 0.f) || !(rt.routed_scale < __builtin_inff())) return QPAL_E_PARAM;
        if (rt.n_group < 1 || E % rt.n_group || rt.topk_group < 1 || rt.topk_group > rt.n_group) return QPAL_E_SHAPE;
        const int S = E / rt.n_group;
        if ((long)rt.topk_group * S < top_k || (rt.group_score == QPAL_MOE_GROUP_TOP2 && S < 2)) return QPAL_E_SHAPE;
        if (rt.shared_gate_f16 && !rt.shared_gate_out) return QPAL_E_NULL;
        if ((reinterpret_cast<uintptr_t>(rt.shared_gate_f16) & 15) ||
            ((reinterpret_cast<uintptr_t>(rt.select_bias) | reinterpret_cast<uintptr_t>(rt.shared_gate_out)) & 3))
            return QPAL_E_ALIGN;
    }
    MoeRouteParams p{h_f32, ld_h, static_cast<const uint16_t *>(rms_w_f16), rms_eps, static_cast<const uint16_t *>(router_w_f16),
                     router_bias, active, n, H, E, top_k, renorm ? 1 : 0, max_groups, sel, gate, order, inv, x_index, group_expert,
                     group_first, group_count, ngroups, ticket, rt};
    if (router)
        hipLaunchKernelGGL(moe_route_kernel<true>, dim3(n), dim3(kRouteThreads), 0, static_cast<hipStream_t>(stream), p);
    else
        hipLaunchKernelGGL(moe_route_kernel<false>, dim3(n), dim3(kRouteThreads), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

extern "C" int qpal_moe_route(const float *h_f32, long ld_h, const void *rms_w_f16, float rms_eps, const void *router_w_f16,
                              const float *router_bias, const long long *active, int n, int H, int E, int top_k, int renorm,
                              int *sel, float *gate, int *order, int *inv, int *x_index, int *group_expert, int *group_first,
                              int *group_count, int *ngroups, int max_groups, unsigned *ticket, void *stream) {
    return moe_route_launch(h_f32, ld_h, rms_w_f16, rms_eps, router_w_f16, router_bias, active, n, H, E, top_k, renorm, sel, gate, order,
                            inv, x_index, group_expert, group_first, group_count, ngroups, max_groups, ticket, nullptr, stream);
}

extern "C" int qpal_moe_route_ex(const float *h_f32, long ld_h, const void *rms_w_f16, float rms_eps, const void *router_w_f16,
                                 const float *router_bias, const long long *active, int n, int H, int E, int top_k, int *sel, float *gate,
                                 int *order, int *inv, int *x_index, int *group_expert, int *group_first, int *group_count, int *ngroups,
                                 int max_groups, unsigned *ticket, const qpal_moe_router *router, void *stream) {
    if (!router) return QPAL_E_NULL;
    return moe_route_launch(h_f32, ld_h, rms_w_f16, rms_eps, router_w_f16, router_bias, active, n, H, E, top_k, router->renorm, sel, gate,
                            order, inv, x_index, group_expert, group_first, group_count, ngroups, max_groups, ticket, router, stream);
}

static int moe_combine_launch(float *out_f32, long ld_out, const float *y_f32, long ld_y, const float *gate, const int *inv, int n,
                              int top_k, int H, int P, int accumulate, bool shared, const float *ys_f32, long ld_ys, const float *sgate,
                              void *stream) {
    if (!out_f32 || !y_f32 || !gate || !inv) return QPAL_E_NULL;
    if (shared) {
        if (!ys_f32 || !sgate) return QPAL_E_NULL;
        if (ld_ys < H) return QPAL_E_SHAPE;
        if ((reinterpret_cast<uintptr_t>(ys_f32) | reinterpret_cast<uintptr_t>(sgate)) & 3) return QPAL_E_ALIGN;
    }
    if (n < 1 || n > kMoeMaxRows || top_k < 1 || top_k > kMoeMaxTopK || H < 1 || P < 1 || ld_out < H || ld_y < H) return QPAL_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(out_f32) | reinterpret_cast<uintptr_t>(y_f32) | reinterpret_cast<uintptr_t>(gate) |
         reinterpret_cast<uintptr_t>(inv)) & 3)
        return QPAL_E_ALIGN;
    MoeCombineParams p{out_f32, ld_out, y_f32, ld_y, gate, inv, n, top_k, H, P, accumulate ? 1 : 0, ys_f32, ld_ys, sgate};
    const int gx = (H + 255) / 256;
    const dim3 grid(gx < 32 ? gx : 32, n);
    if (shared)
        hipLaunchKernelGGL(moe_combine_kernel<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
    else
        hipLaunchKernelGGL(moe_combine_kernel<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

extern "C" int qpal_moe_combine(float *out_f32, long ld_out, const float *y_f32, long ld_y, const float *gate, const int *inv, int n,
                                int top_k, int H, int P, int accumulate, void *stream) {
    return moe_combine_launch(out_f32, ld_out, y_f32, ld_y, gate, inv, n, top_k, H, P, accumulate, false, nullptr, 0, nullptr, stream);
}

extern "C" int qpal_moe_combine_shared(float *out_f32, long ld_out, const float *y_f32, long ld_y, const float *gate, const int *inv,
                                       const float *ys_f32, long ld_ys, const float *sgate, int n, int top_k, int H, int P,
                                       int accumulate, void *stream) {
    return moe_combine_launch(out_f32, ld_out, y_f32, ld_y, gate, inv, n, top_k, H, P, accumulate, true, ys_f32, ld_ys, sgate, stream);
}
