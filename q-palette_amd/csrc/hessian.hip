// Proxy-Hessian accumulation (include/qpal.h: qpal_hessian_accum):  H += X^T X,  colsum += 1^T X  for fp16
// activations X [rows, n] and an fp64 H [n, n] of which only the lower-triangle tiles are formed.
//
// One workgroup of 4 waves owns one 128 x 128 tile (bi >= bj) of H for the whole call; wave (wr, wc) owns its 64 x 64 quarter as
// 4 x 4 blocks of v_mfma_f32_16x16x32_f16.  Both operands of the product are COLUMNS of X (k = the row of X), so the 128 rows of a
// stage (4 k steps) go to LDS as they lie in memory ([row][128 columns], 256 B + 32 B pad per row) and every fragment is two
// ds_read_b64_tr_b16: lane (q = lane >> 4, r = lane & 15) receives column 16 c + r at rows 4 q .. 4 q + 3 and 16 + 4 q .. + 3.
// The A and the B side use the same read, hence the same k order; with the pad the 8 rows x 32 B that a 32-lane half touches fall
// on 64 different banks.  The reads sit outside every lane-dependent branch (EXEC all ones).
//
// fp16 x fp16 products are exact in fp32.  The fp32 accumulators take kFold = 256 rows (2 stages), then they are added to the
// wave's fp64 copy of its quarter (registers) and cleared; H is read, added to and written once, after the last row.  The rows
// past `rows` and the columns past n (n % 128 == 64: a half tile at the edge) are zeros in LDS; their addresses are clamped into
// X, never predicated, so that no load sits behind a branch.  colsum comes from the diagonal tiles: one more MFMA per column
// block with an all-ones A operand.  One owner per element, a fixed order of sums: equal calls give equal bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "launch.h"
#include "qpal.h"

namespace qpal {
namespace hess {

typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef __fp16 fp16x4_t __attribute__((vector_size(8)));
typedef __attribute__((address_space(3))) fp16x4_t *lds_half4_ptr;

constexpr int kTile = QPAL_HESSIAN_TILE;  // columns of X per operand image = rows / columns of H per workgroup
#ifndef QPAL_HESSIAN_KB
#define QPAL_HESSIAN_KB 128
#endif
constexpr int kKB = QPAL_HESSIAN_KB;      // rows of X per stage: kKB / 32 MFMA k steps between two barriers
constexpr int kNP = kKB / 16;             // staging passes: 256 threads move 16 rows x 16 chunks of both images per pass
constexpr int kRS = 2 * kTile + 32;       // LDS row stride in bytes: 72 dwords, rows r .. r + 7 start 8 banks apart
constexpr int kOp = kKB * kRS;            // one operand image
constexpr int kBuf = 2 * kOp;             // A image + B image
constexpr int kFold = 256;                // rows per fp32 accumulation
constexpr int kLdsBytes = 2 * kBuf;       // two stages: one is read while the next is written
static_assert(kTile == 128 && kKB % 32 == 0 && kFold % kKB == 0, "the wave / thread maps below are written for 128-column tiles");
static_assert(kLdsBytes <= 160 * 1024, "LDS of one CU");

__device__ __forceinline__ half8_t tr_frag(const unsigned char *p) {
    const half4_t lo = __builtin_bit_cast(half4_t, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_half4_ptr)(p)));
    const half4_t hi = __builtin_bit_cast(half4_t, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_half4_ptr)(p + 16 * kRS)));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

__global__ __launch_bounds__(256) void hessian_kernel(double *__restrict__ H, double *__restrict__ colsum,
                                                      const uint16_t *__restrict__ X, long ld_x, int rows, int n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    // tile (bi, bj), bi >= bj, of linear id t = bi (bi + 1) / 2 + bj: the float root is a first guess, the integers decide
    const int t = (int)blockIdx.x;
    int bi = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (bi * (bi + 1) / 2 > t) bi--;
    while ((bi + 1) * (bi + 2) / 2 <= t) bi++;
    const int bj = t - bi * (bi + 1) / 2;
    const bool diag = bi == bj;

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, q = lane >> 4, r = lane & 15;
    const bool cs = diag && wr == 0 && colsum != nullptr;  // (wave-uniform) this wave also sums its 64 columns

    // staging: thread = (16-byte chunk sc of a row, rows sr, sr + 16, ... of the stage), for the A and the B image.  A diagonal
    // tile stages its columns twice: a branch around the second copy would put a full memory wait behind every single load
    const int sc = tid & 15, sr = tid >> 4;
    const int colA = bi * kTile + 8 * sc, colB = bj * kTile + 8 * sc;
    const bool okA = colA < n, okB = colB < n;
    const uint16_t *xa = X + (okA ? colA : 0), *xb = X + (okB ? colB : 0);
    u32x4_t ra[kNP], rb[kNP];
    // (the zeros are selected when a stage is committed, not when it is loaded: a select next to its load would wait for it there)
    auto load = [&](int s) {
#pragma unroll
        for (int h = 0; h < kNP; h++) {
            const int row = s * kKB + sr + 16 * h;
            const size_t off = (size_t)(row < rows ? row : rows - 1) * (size_t)ld_x;
            ra[h] = *reinterpret_cast<const u32x4_t *>(xa + off);
            rb[h] = *reinterpret_cast<const u32x4_t *>(xb + off);
        }
    };
    auto commit = [&](int s) {
        unsigned char *d = sm + (s & 1) * kBuf + sr * kRS + sc * 16;
#pragma unroll
        for (int h = 0; h < kNP; h++) {
            const bool in = s * kKB + sr + 16 * h < rows;
            *reinterpret_cast<u32x4_t *>(d + 16 * h * kRS) = (okA && in) ? ra[h] : u32x4_t{0, 0, 0, 0};
            *reinterpret_cast<u32x4_t *>(d + kOp + 16 * h * kRS) = (okB && in) ? rb[h] : u32x4_t{0, 0, 0, 0};
        }
    };

    f32x4_t acc[4][4] = {}, cacc[4] = {};
    double acc64[4][4][4] = {}, c64[4] = {};
    const half8_t ones = {1, 1, 1, 1, 1, 1, 1, 1};
    const int lbase = (4 * q + (r >> 2)) * kRS + 8 * (r & 3);
    auto fold = [&]() {
#pragma unroll
        for (int m = 0; m < 4; m++)
#pragma unroll
            for (int nn = 0; nn < 4; nn++) {
#pragma unroll
                for (int e = 0; e < 4; e++) acc64[m][nn][e] += (double)acc[m][nn][e];
                acc[m][nn] = f32x4_t{0, 0, 0, 0};
            }
        if (cs) {
#pragma unroll
            for (int nn = 0; nn < 4; nn++) {
                c64[nn] += (double)cacc[nn][0];
                cacc[nn] = f32x4_t{0, 0, 0, 0};
            }
        }
    };

    const int nst = (rows + kKB - 1) / kKB;
    load(0);
    commit(0);
    __syncthreads();
    // The stage loop, once with and once without the column sums: a branch inside it would cut the k steps into separate blocks
    // and keep the next step's LDS reads from being issued under this step's MFMAs.
    auto run = [&](auto with_colsum) {
        for (int s = 0; s < nst; s++) {
            const bool more = s + 1 < nst;
            if (more) load(s + 1);
            const unsigned char *As = sm + (s & 1) * kBuf + lbase, *Bs = As + kOp;
            half8_t a[2][4], b[2][4];
            auto frags = [&](int ks) {
#pragma unroll
                for (int m = 0; m < 4; m++) a[ks & 1][m] = tr_frag(As + 32 * ks * kRS + (64 * wr + 16 * m) * 2);
#pragma unroll
                for (int nn = 0; nn < 4; nn++) b[ks & 1][nn] = tr_frag(Bs + 32 * ks * kRS + (64 * wc + 16 * nn) * 2);
            };
            frags(0);
#pragma unroll
            for (int ks = 0; ks < kKB / 32; ks++) {
                if (ks + 1 < kKB / 32) frags(ks + 1);
#pragma unroll
                for (int m = 0; m < 4; m++)
#pragma unroll
                    for (int nn = 0; nn < 4; nn++)
                        acc[m][nn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[ks & 1][m], b[ks & 1][nn], acc[m][nn], 0, 0, 0);
                if constexpr (decltype(with_colsum)::value) {
#pragma unroll
                    for (int nn = 0; nn < 4; nn++) cacc[nn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, b[ks & 1][nn], cacc[nn], 0, 0, 0);
                }
            }
            if ((s + 1) % (kFold / kKB) == 0) fold();
            // the other buffer was last read in stage s - 1, which every wave left through the barrier below
            if (more) commit(s + 1);
            __syncthreads();
        }
    };
    if (cs) run(std::true_type{});
    else run(std::false_type{});
    fold();

    // D of the MFMA: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
        for (int nn = 0; nn < 4; nn++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int i = bi * kTile + 64 * wr + 16 * m + 4 * q + e, j = bj * kTile + 64 * wc + 16 * nn + r;
                if (i < n && j < n) H[(size_t)i * (size_t)n + (size_t)j] += acc64[m][nn][e];
            }
    if (cs && q == 0) {
#pragma unroll
        for (int nn = 0; nn < 4; nn++) {
            const int j = bj * kTile + 64 * wc + 16 * nn + r;
            if (j < n) colsum[j] += c64[nn];
        }
    }
}

}  // namespace hess
}  // namespace qpal

using namespace qpal::hess;

extern "C" int qpal_hessian_accum(double *H, double *colsum, const void *X, long ld_x, int rows, int n, void *stream) {
    if (!H || !X) return QPAL_E_NULL;
    if (n < 64 || n > 32768 || n % 64 || rows < 0 || ld_x < n) return QPAL_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(X) & 15) || (ld_x & 7)) return QPAL_E_ALIGN;  // 16-byte loads of every row
    if ((reinterpret_cast<uintptr_t>(H) | reinterpret_cast<uintptr_t>(colsum)) & 7) return QPAL_E_ALIGN;
    if (rows == 0) return 0;
    const int T = (n + kTile - 1) / kTile;
    return qpal::launch_lds<hessian_kernel>(dim3(T * (T + 1) / 2), dim3(256), kLdsBytes, kLdsBytes, static_cast<hipStream_t>(stream), H, colsum,
                                            static_cast<const uint16_t *>(X), ld_x, rows, n);
}
