/*
 * qpal.h — C-ABI of the MI355X (gfx950) dequant-matmul hot path of Q-Palette.
 *
 * One runtime-shaped entry point per kernel family replaces the reference's ~8k generated,
 * shape-templated pybind functions.  All pointers are DEVICE pointers owned by the caller (the
 * Python op layer allocates them with the torch caching allocator); the library never allocates,
 * frees or synchronises, launches on the stream it is given (graph-capturable) and reports errors
 * by return code instead of exit() (reference: gpuErrchk -> exit, kernels/tcq-kernels/src/inference.h:10-18).
 *
 * Return value: 0 = ok; < 0 = argument error (QPAL_E_*); > 0 = hipError_t of the failed launch.
 *
 * Data formats (bit for bit the reference's; see DESIGN.md §2 and SURVEY.md §8a):
 *   TCQ trellis   int16  [(m/16)*(k/16)][8*KV]      lib/linear/tcq_linear.py:31-35
 *   TCQ codebook  fp16   [2^S][2]                   lib/linear/tcq_linear.py:37-40
 *   LUT-TC        int32  [m][bits*k/32/vec], fp16 lut [2^bits][vec]   lib/linear/vq_linear.py:15-23
 *   LUT-SIMT      uint32 [m][bits*k/32/vec]         lib/quantizer/pack_op.py:288-335, quant_op.py:69-78
 *   x             fp16   [n][k] row-major, 1 <= n <= 128 (tensor-core-order families), 1 <= n <= 8 (SIMT)
 */
#ifndef QPAL_H
#define QPAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QPAL_VERSION 300

#define QPAL_OK 0
#define QPAL_E_SHAPE (-1)   /* m, k, n outside the supported set (m%32, k%32, 1<=n<=128 ...) */
#define QPAL_E_PARAM (-2)   /* S / KV / bits / vec / split combination not supported        */
#define QPAL_E_NULL (-3)    /* required pointer is NULL                                      */
#define QPAL_E_ALIGN (-4)   /* pointer not aligned to the format's natural alignment         */

/* split modes of the TCQ family (lib/linear/comb_linear.py) */
#define QPAL_SPLIT_NONE 0   /* QTIPLinearTCQ:  one stream c1 @ KV1                                   */
#define QPAL_SPLIT_ROWS 1   /* CombLinearTCQ:  rows [0,m/2) from c1 @ KV1, rows [m/2,m) from c2 @ KV2 */
#define QPAL_SPLIT_COLS 2   /* CombtLinearTCQ: cols [0,k/2) from c1 @ KV1, cols [k/2,k) from c2 @ KV2 */

/* Fused trellis decode + GEMV:  out[n][m] (fp32) = sum_k W[m][k] * x[n][k].
 * Replaces decompress_gemm_ptr / _comb_ptr / _combt_ptr, kernels/tcq-kernels/src/inference.cu:1826-1968
 * (bindings kernels/tcq-kernels/src/qtip_torch.cu:14-279).  `out` needs no initialisation.
 * S in {9,10,11}; KV in 2..10 per the reference's S/KV table (lib/linear/__init__.py:166-172).   */
int qpal_tcq_gemv(float *out, const void *c1, const void *c2, const void *x, const void *tlut,
                  int m, int n, int k, int S, int KV1, int KV2, int split, void *stream);

/* Several independent TCQ GEMVs of ONE codec (same S, KV1, KV2, split in {NONE, COLS}, same batch n) in a
 * single launch: out/c1/c2/x/tlut/m/k per job.  No counterpart in the reference (it launches one kernel
 * per linear); exists because on MI355X a launch costs ~5 us of fixed time, more than the q/k/v/o GEMVs
 * themselves.  Intended for projections of one input (q|k|v, gate|up); njobs <= 8.                  */
typedef struct qpal_tcq_job {
    float *out;        /* fp32 [n][m] */
    const void *c1;    /* stream 1 */
    const void *c2;    /* stream 2 (split COLS) or NULL */
    const void *x;     /* fp16 [n][k] */
    const void *tlut;  /* fp16 [2^S][2] */
    int m, k;
    int out_zeroed;    /* 1: the caller guarantees out is all zeros (e.g. pre-zeroed by an earlier launch, below):
                          a split-K job then needs no memset node of its own, and the launch planner may let two workgroups share
                          a row (csrc/qpal_capi.hip plan_launch, DESIGN.md §4.2: +3 % tokens/s on a Llama-8B token) — both use
                          float atomics into the zeroed buffer; with at most two adders per element of a ZEROED output the
                          result is order-independent (0 + a + b).  A job that accumulates (`accumulate`: out += ...) may be
                          split or paired as well: its adders land on the live value h, and (h + a) + b != (h + b) + a in
                          fp32 — such an output is reproducible to rounding, not to the bit */
    const void *wscale; /* fp16 [m] or NULL: fused epilogue out[b][r] = acc * wscale[r] * oscale — the
                          `* Wscale * scale` that follows every quantized linear in the reference's incoherent
                          wrappers (lib/linear/incoherent_linear.py:83-99, 107, 327-337, 496-503) */
    float oscale;      /* 0 is read as 1 */
    long ldo;          /* row stride of out in floats, >= m; 0 is read as m.  Lets q|k|v or up|gate write the
                          column blocks of one [n][sum m] buffer */
    int x_had;         /* 1: x is the UN-rotated input; the kernel stages fp16(fp16(H_k (x * x_su) / sqrt(k)) * x_post)
                          instead — the left rotation of the incoherent wrappers (qpal_hadamard with K = 1, hd = k)
                          without a launch of its own.  Needs qpal_can_fuse_rotation(n, k); all jobs of a launch
                          that share x must share x_su / x_post */
    float x_post;      /* e.g. 1 / scale */
    const void *x_su;  /* fp16 [k] or NULL */
    int kv;            /* 0: the call's KV1.  Otherwise this job's own KV (split NONE only): jobs of one S but different
                          bit widths — q, k, v of a mixed-scheme model — then share ONE launch and one codebook image
                          (KV 2..8 for S = 9, 8..10 for S = 10, 9..10 for S = 11; batch <= 8; no x_had) */
    const void *x_f32; /* fp32 [k] or NULL (see below: only together with x_had) */
    /* decoder-block fusion (x_had jobs): the rotation reads the fp32 residual stream and applies
     * the RMSNorm in front of it (lib/linear/incoherent_linear.py:76-108 is called on `input_layernorm(h)` by the model,
     * model/llama.py), and o_proj / down_proj add their result to it.  With x_had = 1: x_f32 (fp32 [k], 16-byte aligned) may
     * replace x; x_rms_eps > 0 normalises x <- x * rsqrt(mean(x^2) + eps) * x_rms_w (fp16 [k] or NULL) in fp32 before the
     * fp16 rounding and the sign flip.  accumulate = 1 (any job): out += result (out is the residual stream).  The launch
     * may split K on its own: the split-K atomics add onto the live contents of out, no memset is ever issued for an
     * accumulating job, and out_zeroed is ignored for it (leave it 0: the buffer is NOT zero).                           */
    float x_rms_eps;
    const void *x_rms_w;
    int accumulate;
    int kv2;           /* with kv != 0 and c2 != NULL: a COLUMN-SPLIT (combt) layer inside an any-KV launch — stream 1 (columns
                          [0, k/2)) at kv, stream 2 at kv2 bits, both of the call's S; the call's split stays NONE.  tcomb and
                          tcq projections of a mixed-scheme model then share one launch.  0: single stream */
    void *act_out;     /* fp16 [m / 2] or NULL.  Non-NULL (needs x_had, batch 1): the layer is an up | gate pair whose supertile
                          rows (32 output rows) ALTERNATE up, gate, up, gate ... (qpalette_amd.linear.interleave_up_gate builds
                          it from the two layers); the epilogue then writes fp16(silu(fp16 gate)) * fp16 up — the
                          `act_fn(gate) * up` of lib/linear/incoherent_linear.py:333 — here and `out` is not written
                          (may be NULL).  The following rotation reads 2 bytes per element instead of 8 and evaluates no SwiGLU */
    /* x_had with a NON-power-of-two width (round 3): x_K = 28 and k = 14336 = 28 * 512 (the down_proj input of Llama-3.1-8B):
     * the staging applies (hadK (x) H_512) / sqrt(k) with the reference's fp16 rounding between the two factors
     * (lib/utils/matmul_had.py:137-148); x_hadk: fp16 [28][28], y[j] = sum_i x_hadk[j][i] t[i] (what qpal_hadamard takes).
     * Batch 1, fp16 x, no RMSNorm; qpal_can_fuse_rotation_k(n, k, K) says where.  x_K = 0 / 1: power-of-two widths as before. */
    const void *x_hadk;
    int x_K;
    const void *act_su; /* with act_out: fp16 [m / 2] of +-1, multiplied into the activation written — the `* SU` in front of the NEXT
                           projection's rotation (exact: a sign flip), so that rotation reads one vector instead of two; or NULL */
} qpal_tcq_job;
/* prezero/prezero_bytes (may be NULL/0): a buffer this launch also fills with zeros, for a LATER launch on the
 * same stream that accumulates into it with atomics (split-K of a few-rows x long-K layer such as down_proj).
 * Saves that launch's memset node and the two extra graph boundaries around it.  bytes % 16 == 0.           */
int qpal_tcq_gemv_multi(const qpal_tcq_job *jobs, int njobs, int n, int S, int KV1, int KV2, int split,
                        void *prezero, long prezero_bytes, void *stream);

/* Trellis decode to fp16 W[m][k] row-major (bit-exact).  Replaces decompress_ptr / _comb_ptr /
 * _combt_ptr, kernels/tcq-kernels/src/inference.cu:1862-1891, 1970-2035.                         */
int qpal_tcq_dequant(void *out_f16, const void *c1, const void *c2, const void *tlut,
                     int m, int k, int S, int KV1, int KV2, int split, void *stream);

/* VQ/SQ "tensor-core" packed format: fused decode + GEMV, fp32 out[n][m].  vec in {1,2};
 * vec=1: bits 2..8 (sq_dup / sq), vec=2: bits 2..12 (vq2).
 * Replaces decompress_gemm_ptr, kernels/vq-tensor-kernels/src/inference.cu:1112-1180.            */
int qpal_lut_tc_gemv(float *out, const void *qweight, const void *x, const void *lut,
                     int m, int n, int k, int bits, int vec, void *stream);

typedef struct qpal_lut_job {
    float *out;           /* fp32 [n][m] */
    const void *qweight;  /* int32 [m][bits*k/32/vec] */
    const void *x;        /* fp16 [n][k] */
    const void *lut;      /* fp16 [2^bits][vec] */
    int m, k;
    int out_zeroed;       /* as in qpal_tcq_job */
    const void *wscale;   /* as in qpal_tcq_job */
    float oscale;
    long ldo;
    int x_had;            /* as in qpal_tcq_job */
    float x_post;
    const void *x_su;
    const void *x_f32;    /* as in qpal_tcq_job */
    float x_rms_eps;      /* as in qpal_tcq_job */
    const void *x_rms_w;
    int accumulate;
    void *act_out;     /* as in qpal_tcq_job */
    const void *x_hadk; /* as in qpal_tcq_job */
    int x_K;
    const void *act_su;
} qpal_lut_job;
int qpal_lut_tc_gemv_multi(const qpal_lut_job *jobs, int njobs, int n, int bits, int vec, void *prezero,
                           long prezero_bytes, void *stream);

/* Same format decoded to fp16 W[m][k].  Replaces decompress_ptr, vq-tensor inference.cu:1182-1226. */
int qpal_lut_tc_dequant(void *out_f16, const void *qweight, const void *lut,
                        int m, int k, int bits, int vec, void *stream);

/* SIMT packed formats (vec=1: sq_pack_gemm.pack_gemm, kernels/sq-cuda-kernels/gemm.cu:40-85;
 * vec in {2,4}: vq_pack_gemm_*, kernels/vq-cuda-kernels/src/gemm.cu:25-100).  fp16 out[n][m].
 * Accumulates in fp32 (the reference accumulates in fp16) and rounds once at the end.           */
int qpal_lut_simt_gemv(void *out_f16, const void *qweight, const void *x, const void *lut,
                       int m, int n, int k, int bits, int vec, void *stream);

int qpal_lut_simt_dequant(void *out_f16, const void *qweight, const void *lut,
                          int m, int k, int bits, int vec, void *stream);

/* Re-pack a tensor-core-format qweight into the SIMT format on the device (load-time step of
 * VQLinearPackSIMT.gen_layer_from_info, lib/linear/vq_linear.py:175-188 ->
 * lib/quantizer/quant_op.py:246-257).  vec in {1,2}.  dst: uint32 [m][bits*k/32/vec], zeroed by the call. */
int qpal_tc_to_simt(void *dst_simt, const void *src_tc, int m, int k, int bits, int vec, void *stream);

/* Incoherence rotation either side of a quantized linear, one launch:
 *   out[r][blk] = fp16( hadK (x) H_P applied to (f(in)[r][blk] * su) / sqrt(hd) * post_scale [* sv] )
 * for every block of hd = K * 2^p consecutive elements of every row (hd == n: whole-vector transform).
 * Replaces matmul_hadU_cuda (lib/utils/matmul_had.py:137-148: third-party fast_hadamard_transform + hadK
 * matmul) and matmul_hadU_head_cuda (:95-110) plus the elementwise ops around them in
 * lib/linear/incoherent_linear.py:81, 106, 325-337 (incl. act_fn(gate) * up), 488-503.
 *   in_mode   QPAL_IN_F16: fp16 [rows][n];  QPAL_IN_F32: fp32 [rows][n] (rounded to fp16 first, the reference's
 *             .half());  QPAL_IN_SWIGLU_F32: fp32 [rows][2n] = up | gate, f = silu(gate) * up
 *   su, sv    fp16 [n] element-wise pre / post multipliers or NULL (SU sign vector; SV * scale)
 *   hadk      fp16 [K][K] row-major, entries +-1, applied as given (pass the transpose for had_left_T); NULL if K == 1
 *   round_mid 1: fp16 between the butterflies and the hadK product (matmul_hadU_cuda's fp16 pipeline);
 *             0: fp32-grade throughout (matmul_hadU_head_cuda's float path)
 * hd * 4 bytes (+ 1/32 padding) must fit the 160 KiB LDS (hd <= 39 k); K > 1 needs hd / K >= 16; `in` and `su`
 * 16-byte aligned; `out` must not be `in`.                          */
#define QPAL_IN_F16 0
#define QPAL_IN_F32 1
#define QPAL_IN_SWIGLU_F32 2
int qpal_hadamard(void *out_f16, const void *in, const void *su, const void *sv, const void *hadk,
                  int rows, int n, int hd, int K, int in_mode, int round_mid, float post_scale, void *stream);

/* RMSNorm + rotation of a whole row in one launch: out = fp16( fp16( H_n (su * w * x / rms(x)) ) * post_scale ), x fp32 [rows][n]
 * (the residual stream), rms(x) = sqrt(mean(x^2) + rms_eps), w = rms_w (fp16 [n]) or 1 — input_layernorm /
 * post_attention_layernorm (model/llama.py:119) followed by the left rotation of the incoherent wrappers, for the widths the
 * GEMV staging cannot rotate itself (qpal_can_fuse_rotation == 0: k = 8192, 5120, ...).  n = K * 2^p as for qpal_hadamard
 * (hd = n); the norm's scalar is applied after the transform (linear), one fp16 rounding of x * w * 2^-6 on the way in.  Held to
 * the bound of DESIGN.md §25.3 for rows with rms(x) >= 2^-8 (as the x_rms staging of the GEMV launches is); smaller rows put
 * x * w * 2^-6 into fp16 subnormals, which the matrix pipe keeps (measured down to rms 2^-12: same bound).                  */
int qpal_hadamard_rms(void *out_f16, const float *in_f32, const void *rms_w, float rms_eps, const void *su, const void *hadk,
                      int rows, int n, int K, float post_scale, void *stream);

/* fp32 Hadamard rotation for the quantiser's incoherence preprocessing (no fp16 rounding anywhere):
 *   out[r][blk] = (hadK (x) H_P) (in[r][blk] * su[blk]) / sqrt(hd) * post_scale
 * for every block of hd = K * P consecutive elements of every row, P = 2^p >= 16, the block viewed as [K][P] (as
 * qpal_hadamard).  Replaces matmul_hadUt_head / matmul_hadU_head (lib/utils/matmul_had.py:95-120) on W * SU and on the
 * proxy Hessian (lib/quantizer/tcq_quant.py:105-131, vq_quant.py:97-125), which need fp32 precision.  DEVICE pointers:
 *   in, out   fp32 [rows][n], 16-byte aligned; out == in is allowed (every block is read completely before any of it is written)
 *   su        fp32 [n] element-wise pre-multiplier, 16-byte aligned, or NULL
 *   hadk      fp16 [K][K] row-major, entries +-1 (only the sign is read), applied as given (pass the transpose for the Ut
 *             direction); NULL if K == 1
 * K = 1 or a multiple of 4 up to 256 (every factor of get_hadK); the block (hd * 4 bytes, rounded up to 256) and the sign
 * masks of hadK (K * ceil(K / 32) * 4 bytes) must fit the 160 KiB LDS: hd <= 40 960.  Butterflies and the K x K product in
 * fp32.  Argument errors return before any stream work; one launch on `stream`, no synchronisation, no workspace.      */
int qpal_hadamard_f32(float *out, const float *in, const float *su, const void *hadk, int rows, int n, int hd, int K,
                      float post_scale, void *stream);

/* Host-side encoders of the packed formats (plain CPU code; HOST pointers; no GPU involved): what a quantiser or a
 * checkpoint converter calls once per layer.  Bit for bit the reference's packers:
 *   qpal_pack_tcq         Qidxs int32 [m][k/2] (state t of tile (tr, tc) at [16 tr + t/8][8 tc + t%8]) -> int16
 *                         [(m/16)(k/16)][8 KV]: pack_trellis + nibble permutation, lib/codebook/bitshift.py:296-329,
 *                         lib/quantizer/tcq_quant.py:47-60.  QPAL_E_PARAM if the states are not a tail-biting walk.
 *   qpal_pack_tcq_states  the same from uint16 [tiles][128] tile-major states
 *   qpal_pack_lut_tc      indices int32 [m][k/vec] -> int32 [m][bits k/32/vec]: pack_qweight, lib/quantizer/quant_op.py:89-162
 *   qpal_pack_lut_simt    indices -> uint32 [m][bits k/32/vec]: pack_qweight_sq_simt / pack_qweight_vq_simt,
 *                         lib/quantizer/quant_op.py:69-87 (numba loops of lib/quantizer/pack_op.py:288-335)            */
int qpal_pack_tcq(void *dst, const int32_t *qidxs, int m, int k, int KV);
int qpal_pack_tcq_states(void *dst, const uint16_t *states, int m, int k, int KV);
int qpal_pack_lut_tc(void *dst, const int32_t *idx, int m, int k, int bits, int vec);
int qpal_pack_lut_simt(void *dst, const int32_t *idx, int m, int k, int bits, int vec);

/* TCQ encoder (the quantiser's inner loop): tail-biting Viterbi search of the bitshift trellis, L = 16, V = 2, on B independent
 * sequences of 256 values; bit for bit bitshift_codebook(L=16, KV, V=2, tlut_bits=S, decode_mode="quantlut_sym",
 * tlut=tlut16.float()).quantize(X), lib/codebook/bitshift.py:202-294.  DEVICE pointers:
 *   x_f16    fp16 [B][256]: the input ROUNDED TO FP16 (the reference's quantize() does X.to(float16) first), widened to fp32
 *   tlut_f16 fp16 [2^S][2]: the codebook QTIPLinearTCQ.tlut stores
 *   states   int32 [B][128]: the trellis states of the chosen tail-biting walk (the reference's state.T)
 *   hat      fp16 [B][256] or NULL: the reconstruction of states, element 2t + v = pair v of state t (exact in fp16)
 *   ws       qpal_tcq_viterbi_ws_bytes(KV) bytes of device memory, 8-byte aligned, no initialisation; independent of B
 * S in 9..11, KV in 2..10.  Per-state error (r0 - x0)^2 + (r1 - x1)^2 in fp32, each square rounded, no fused multiply-add; cost
 * = error + best predecessor cost in fp32.  Ties: the predecessor with the lowest d (p = g + (d << (16 - KV))) and, at the end, the
 * lowest state — what CPU torch.min / torch.argmin return.  Argument errors return before any stream work; one launch on `stream`,
 * no synchronisation (graph-capturable).                                                                                   */
long qpal_tcq_viterbi_ws_bytes(int KV);
int qpal_tcq_viterbi(int32_t *states, void *hat_or_null, const void *x_f16, const void *tlut_f16, int B, int S, int KV, void *ws,
                     void *stream);

/* VQ / SQ encoder (the fixed-codebook LDLQ quantiser's inner loop): the nearest codeword of every vec-group of m rows of `cols`
 * values, vq_codebook(vec, bits).quantize (lib/codebook/vq_codebook.py), optionally with the in-block error feedback of LDLQ_VQ
 * (lib/algo/ldlq.py).  DEVICE pointers; every fp64 matrix has row stride `ld` (elements):
 *   idx      int32 [m][ld / vec]: the chosen codeword of group g of row r at idx[r * (ld / vec) + g], g < cols / vec
 *   hat      fp64 [m][ld] or NULL: the chosen codewords (fp32 widened)
 *   w        fp64 [m][ld]: the weights of the column block
 *   prod     fp64 [m][ld] or NULL: LDLQ's feedback from the blocks to the right (needs lt)
 *   lt       fp64 or NULL: the cols x cols diagonal block of the unit block-lower LDL factor (diagonal zeroed), COLUMN-major:
 *            L[e][c] at lt[c * ld_l + e]
 *   lut      fp32 [2^bits][vec]: the codebook
 * Without lt every group takes its nearest codeword on its own (target = w).  With lt the groups of a row run from the last to
 * the first and group i's target is (w_i + sum_{e in later groups} L[e][i] (w_e - hat_e)) + prod_i — LDLQ_VQ's WXWX; the
 * feedback uses w - hat, not the target, so prod is a separate input.  Distance sum_v fl((t_v - c_v)^2) in fp64 without fused
 * multiply-add; ties go to the lowest index (CPU torch.argmin).  vec in {1, 2, 4}, bits 1..12, cols % vec == 0, ld >= cols,
 * ld % vec == 0, with lt cols <= 128 and ld_l >= cols.  Argument errors return before any stream work; one launch on `stream`,
 * no synchronisation, no workspace.                                                                                         */
int qpal_vq_encode(int32_t *idx, double *hat_or_null, const double *w, const double *prod_or_null, const double *lt_or_null, int ld,
                   int ld_l, const float *lut, int m, int cols, int bits, int vec, void *stream);

/* One-shot all-gather of a small activation slice across the GPUs of a node by direct peer writes over xGMI (SURVEY.md §8e;
 * no counterpart in the reference, which has no multi-GPU code): rank `rank` stores `bytes` bytes from src into
 * peer_bufs[p] + rank * bytes for every p and raises a flag in peer_ws[p]; the call returns (in stream order) when all
 * `world` slices have arrived in THIS rank's buffer peer_bufs[rank].  peer_bufs / peer_ws: HOST arrays of `world` device
 * pointers — each rank's gather buffer of this call site (world * bytes bytes, 16-byte aligned) and flag block
 * (QPAL_PEER_WS_BYTES_PER_SLOT * number of slots, zero-filled once), opened in every process through IPC handles.
 * slot: index of the call site inside a token (buffers and flags are per call site).  world <= 16; bytes % 16 == 0.
 * Graph-capturable (one kernel, epochs kept in the flag blocks).                                                         */
#define QPAL_PEER_WS_BYTES_PER_SLOT 256
int qpal_peer_gather(const void *src, long bytes, int slot, void *const *peer_bufs, void *const *peer_ws, int rank,
                     int world, void *stream);
/* Set-up helpers of the peer gather (the ONLY entry points of this library that allocate; not on the data path).  The flag
 * blocks are written by a remote GPU while a kernel of this GPU spins on them, so they must not live in ordinary (coarse-
 * grained) device memory, which is only guaranteed coherent at kernel boundaries: qpal_peer_alloc returns `bytes` bytes of
 * zero-filled device memory on the current device — kind 1: fine-grained (hipDeviceMallocFinegrained), 2: uncached
 * (hipDeviceMallocUncached), 0: plain hipMalloc (the gather buffers themselves: their contents are consumed after the
 * kernel boundary).  qpal_ipc_export writes the 64-byte IPC handle of an allocation; qpal_ipc_open maps another process's
 * allocation into this one (peer access enabled lazily); qpal_ipc_close / qpal_peer_free undo them.                      */
#define QPAL_IPC_HANDLE_BYTES 64
int qpal_peer_alloc(void **ptr, long bytes, int kind);
int qpal_peer_free(void *ptr);
int qpal_ipc_export(void *ptr, void *handle64);
int qpal_ipc_open(const void *handle64, void **ptr);
int qpal_ipc_close(void *ptr);

/* Decoder-block glue of a batch-1 decode step, one launch: rotary embedding of the new token's q and k (HF rotate_half
 * convention, cos / sin of pos * inv_freq rounded to fp16, fp16 arithmetic: model/llama.py apply_rotary_pos_emb), q as fp16,
 * k and v written into a static KV cache fp16 [nkv][max_len][hd] at position *pos (device int64).  q / k / v: fp32 (the GEMV
 * epilogue's output) [nq * hd] / [nkv * hd]; inv_freq: fp32 [hd / 2].                                                    */
int qpal_rope_kv(const float *q, const float *k, const float *v, void *q_out_f16, void *kcache_f16, void *vcache_f16,
                 const long *pos, const float *inv_freq, int nq, int nkv, int hd, long max_len, void *stream);

/* Attention of ONE new token over a static KV cache (batch 1, grouped-query heads: nq % nkv == 0), one launch: softmax(q k^T *
 * scale) v over positions 0 .. *pos, fp32 accumulation, fp16 out [nq][hd].  Caches fp16 [nkv][max_len][hd], 16-byte aligned.
 * (torch SDPA runs this shape as ~10 launches.)  max_len up to ~40 k positions (scores live in LDS).                      */
int qpal_attn_decode(const void *q_f16, const void *kcache_f16, const void *vcache_f16, void *out_f16, const long *pos,
                     int nq, int nkv, int hd, long max_len, float scale, void *stream);

/* The tail of a greedy decode step as one launch: x = fp16(fp16(h * rsqrt(mean(h^2) + rms_eps)) * rms_w), two fp16 roundings like
 * the reference's LlamaRMSNorm (rms_w_f16 == NULL: w = 1; rms_eps <= 0: no norm, x = fp16(h), rms_w_f16 ignored), logits = W x with
 * W the fp16 lm_head [vocab][k] (k in {2048, 4096, 8192}, 16-byte aligned), *token = argmax (lowest index on ties); logits
 * (fp32 [vocab]) are also written when the pointer is not NULL.  ws: qpal_lm_head_ws_bytes(vocab) bytes of device memory,
 * zero-filled once, kept across launches.  Replaces model.norm + lm_head + argmax of the reference's decode loop
 * (eval/measure_latency.py: logits[:, -1].argmax).                                                                          */
long qpal_lm_head_ws_bytes(int vocab);
int qpal_lm_head_argmax(const float *h_f32, const void *rms_w_f16, float rms_eps, const void *w_f16, float *logits_f32, long *token,
                        void *ws, long ws_bytes, int vocab, int k, void *stream);

/* The two launches above as one (what a decode step runs): rotary embedding of the new token's q / k, k and v appended to the
 * cache at *pos, attention over positions 0 .. *pos, fp16 out [nq][hd].  q / k / v fp32 as for qpal_rope_kv.  hd in {64, 128,
 * 256}; max_len % 4 == 0.  The new row is read from on-chip memory by every head of its group: nothing this launch reads was
 * written by it.  ws == NULL: one workgroup per query head (scores of the whole context in LDS: max_len up to ~38 k).
 * ws != NULL (qpal_attn_ws_bytes(...) > 0 bytes of device memory, 4-byte aligned, zero-filled ONCE, kept across launches):
 * split-context form for long caches — workgroup (kv head, chunk of the context) serves all nq / nkv query heads of its group,
 * the last workgroup of a kv head to arrive merges the partial softmaxes.  qpal_attn_ws_bytes returns 0 where the split form
 * does not apply (max_len < 2048, nq / nkv not in {1, 2, 4, 8}, (nq / nkv) * hd > 1024): pass ws = NULL then.
 * *pos outside [0, max_len) (it lives on the device: the host cannot check it): the launch does nothing — no cache row is
 * written, out is left as it was; the same holds for qpal_rope_kv / qpal_attn_decode.                                   */
long qpal_attn_ws_bytes(int nq, int nkv, int hd, long max_len);
int qpal_attn_rope_decode(const float *q, const float *k, const float *v, void *kcache_f16, void *vcache_f16, void *out_f16,
                          const long *pos, const float *inv_freq, int nq, int nkv, int hd, long max_len, float scale,
                          void *ws, long ws_bytes, void *stream);

/* Decode attention of B concurrent sequences, one launch (csrc/attn_batch.hip): for every sequence b < B with 0 <= pos[b] < max_len,
 * rotary embedding of its new q and k (qpal_rope_kv's convention), k and v appended as fp16 to ITS cache at row pos[b], and
 * softmax(q k^T * scale) v over its positions 0 .. pos[b] (fp32 accumulation, fp16 out).  q / k / v: fp32 rows [B][ld_qkv] (ld_qkv
 * in elements, >= nq * hd: column slices of the q|k|v GEMV output [B][nq*hd + 2*nkv*hd]), inside a row q [nq * hd], k / v
 * [nkv * hd]; caches fp16 [B][nkv][max_len][hd], 16-byte aligned; out fp16 [B][ld_out], out[b][h * hd + d]; pos int64 [B] on
 * the device (never read by the host: graph-capturable with positions that change between replays); inv_freq fp32 [hd / 2].
 * hd in {64, 128, 256}; nq / nkv in {1, 2, 4, 8} with (nq / nkv) * hd <= 1024; 1 <= B <= 128; max_len % 4 == 0, up to 64 k.
 * A sequence whose pos[b] lies outside [0, max_len) is inactive: its cache and its out row are left as they were.
 * Workgroup = (sequence, kv head, chunk of that sequence's existing context): only rows <= pos[b] are read.
 * ws: qpal_attn_batch_ws_bytes(B, ...) bytes of device memory, 4-byte aligned, zero-filled ONCE, kept across launches; 0: no
 * workspace needed, pass ws = NULL (max_len < 512).  The size is monotone in B and max_len: a workspace sized for (B, max_len)
 * serves every launch of the same nq, nkv, hd with fewer sequences or a shorter cache (launches on one stream may share it). */
long qpal_attn_batch_ws_bytes(int B, int nq, int nkv, int hd, long max_len);
int qpal_attn_rope_decode_batch(const float *q, const float *k, const float *v, long ld_qkv,
                                void *kcache_f16, void *vcache_f16, void *out_f16, long ld_out,
                                const long *pos, const float *inv_freq, int B, int nq, int nkv, int hd,
                                long max_len, float scale, void *ws, long ws_bytes, void *stream);

/* Prompt prefill attention of ONE sequence, one launch (csrc/attn_prefill.hip): T new tokens at positions *pos0 .. *pos0 + T - 1.
 * Rotary embedding of their q and k (qpal_rope_kv's convention), k and v appended as fp16 to the cache at rows *pos0 + t (bit for
 * bit what qpal_rope_kv writes there; no other cache byte changes), and causal attention: row t over positions 0 .. *pos0 + t
 * (the existing context plus new rows 0 .. t), both products on the matrix pipe, online softmax, fp32 accumulation, fp16 out.
 * q / k / v: fp32 rows [T][ld_qkv] as for qpal_attn_rope_decode_batch (row t = the token at *pos0 + t); caches fp16
 * [nkv][max_len][hd] of one sequence, 16-byte aligned (kcache[b] of the batched layout is one); out fp16 [T][ld_out],
 * out[t][h * hd + d]; pos0 int64 on the device (never read by the host: graph-capturable with a position that changes between
 * replays); inv_freq fp32 [hd / 2].  hd in {64, 128, 256}; nq / nkv in {1, 2, 4, 8} with (nq / nkv) * hd <= 1024; 1 <= T <= 128;
 * max_len % 4 == 0, up to 64 k.  *pos0 < 0 or *pos0 + T > max_len: the launch does nothing (no cache byte, no out byte).
 * New rows reach the products from the fp32 inputs, never from the cache: nothing the launch reads from the cache was written by
 * it.  ws: qpal_attn_prefill_ws_bytes(T, ...) bytes of device memory, 4-byte aligned, zero-filled ONCE, kept across launches
 * (split-context partials and tickets, merged in a fixed order: two launches are bitwise equal); 0: no workspace needed, pass
 * ws = NULL (max_len < 512).  The size is monotone in T and max_len: one workspace serves every layer and every shorter chunk. */
long qpal_attn_prefill_ws_bytes(int T, int nq, int nkv, int hd, long max_len);
int qpal_attn_rope_prefill(const float *q, const float *k, const float *v, long ld_qkv,
                           void *kcache_f16, void *vcache_f16, void *out_f16, long ld_out,
                           const long *pos0, const float *inv_freq, int T, int nq, int nkv, int hd,
                           long max_len, float scale, void *ws, long ws_bytes, void *stream);

/* The same two launches on an 8-bit KV cache: OCP e4m3fn (torch.float8_e4m3fn, not the MI300 fnuz encoding), one byte per element,
 * no scales, the layouts above ([B][nkv][max_len][hd] / [nkv][max_len][hd], 16-byte aligned).  With h the fp16 value the fp16
 * entry point writes for a new row (bit for bit qpal_rope_kv's), the stored byte is h -> fp32, clamped to [-448, 448], rounded to
 * nearest even, subnormals kept (torch: h.float().clamp(-448, 448).to(torch.float8_e4m3fn); NaN inputs unspecified).  A byte is
 * converted exactly to fp16 and then used as an fp16 cache row is used: same products, same accumulation order.  The new rows of a
 * launch take part in that launch at their stored value, so a position has ONE value whichever launch reads it, and a cache filled
 * by prefill equals, byte for byte, a cache filled token by token from the same q|k|v.  Arguments, checks, error codes, inactive
 * sequences, the *pos0 fit rule, graph capture and bitwise reproducibility are those of the fp16 siblings.  LDS layout, grid and
 * workspace do not depend on the element type: qpal_attn_batch_ws_bytes / qpal_attn_prefill_ws_bytes size the workspace of both
 * formats, and one workspace may serve launches of both. */
int qpal_attn_rope_decode_batch_kv8(const float *q, const float *k, const float *v, long ld_qkv,
                                    void *kcache_e4m3, void *vcache_e4m3, void *out_f16, long ld_out,
                                    const long *pos, const float *inv_freq, int B, int nq, int nkv, int hd,
                                    long max_len, float scale, void *ws, long ws_bytes, void *stream);
int qpal_attn_rope_prefill_kv8(const float *q, const float *k, const float *v, long ld_qkv,
                               void *kcache_e4m3, void *vcache_e4m3, void *out_f16, long ld_out,
                               const long *pos0, const float *inv_freq, int T, int nq, int nkv, int hd,
                               long max_len, float scale, void *ws, long ws_bytes, void *stream);

/* The same two launches on a PAGED KV cache.  kpool / vpool: [num_pages][nkv][page_size][hd] of one layer, contiguous,
 * 16-byte aligned, elements fp16 (kv_fmt 0) or e4m3fn (kv_fmt 1: the store rule of the _kv8 entry points); page_size in {16, 32,
 * 64, 128, 256}.  block_table: int32 [B][ld_table] on the device, ld_table >= max_pages, 4-byte aligned: entry j of row b is the
 * page that holds positions j * page_size .. (j + 1) * page_size - 1 of sequence b (block_row: the [max_pages] row of the ONE
 * sequence a prefill launch serves).  The table is never read by the host (graph-capturable with entries that change between
 * replays).  max_len = max_pages * page_size takes the place of the contiguous max_len in every rule: the shape rules, the inactive
 * rule (pos[b] outside [0, max_len)), the *pos0 fit rule, the launch geometry and the workspace (qpal_attn_batch_ws_bytes /
 * qpal_attn_prefill_ws_bytes of that max_len; one workspace may serve paged and contiguous launches).
 * Contract: bit for bit the contiguous launch of the same max_len on the gathered cache - out rows and the bytes appended to the
 * pools, in both formats; only where a row lives differs.  Only entries that cover positions 0 .. pos[b] (prefill: 0 .. *pos0 + T
 * - 1) are read; every other entry may hold anything.  A used entry outside [0, num_pages): loads through it read page 0 instead,
 * stores through it are dropped, that sequence's out is unspecified; no byte outside the pools, out and ws is touched.
 * Checks and codes are the contiguous siblings'; in addition page_size outside the set, num_pages < 1, max_pages < 1, ld_table <
 * max_pages, kv_fmt not 0 / 1: QPAL_E_SHAPE; a null table: QPAL_E_NULL; a table that is not 4-byte aligned: QPAL_E_ALIGN. */
int qpal_attn_rope_decode_batch_paged(const float *q, const float *k, const float *v, long ld_qkv,
                                      void *kpool, void *vpool, void *out_f16, long ld_out,
                                      const long *pos, const float *inv_freq, const int *block_table, long ld_table,
                                      int num_pages, int page_size, int max_pages, int kv_fmt /* 0 fp16, 1 e4m3fn */,
                                      int B, int nq, int nkv, int hd, float scale, void *ws, long ws_bytes, void *stream);
int qpal_attn_rope_prefill_paged(const float *q, const float *k, const float *v, long ld_qkv,
                                 void *kpool, void *vpool, void *out_f16, long ld_out,
                                 const long *pos0, const float *inv_freq, const int *block_row /* [max_pages] of ONE sequence */,
                                 int num_pages, int page_size, int max_pages, int kv_fmt,
                                 int T, int nq, int nkv, int hd, float scale, void *ws, long ws_bytes, void *stream);

/* SHARED-PREFIX paged decode attention (csrc/attn_prefix.hip + csrc/attn_batch.hip): qpal_attn_rope_decode_batch_paged
 * for slots that share the pages of a common prefix, which is then read once per group instead of once per slot.  Three DEVICE
 * arrays describe the sharing, never read by the host (a captured launch can be replayed while groups, lengths and positions change):
 *   row_group int32 [B] (the group of slot b, or -1), grp_slot int32 [G] (a member whose table row addresses the group's shared
 *   pages), grp_len int32 [G] (the shared positions), 1 <= G <= 16.
 * Slot b is served as a member of g = row_group[b] iff 0 <= g < G, 0 <= grp_slot[g] < B, grp_len[g] > 0 and a multiple of page_size,
 * grp_len[g] <= pos[b] and 0 <= pos[b] < max_len; every other slot is served bit for bit as the paged launch serves it.  A member
 * reads positions [0, grp_len[g]) through table row grp_slot[g] and [grp_len[g], pos[b]] through its own row; the rotary embedding,
 * the appended k / v rows (both formats), the inactive rule and the page guard are the paged launch's.  Two launches: the prefix
 * phase leaves a partial (max, sum, unnormalised out) per (slot, query head) — softmax weights rounded to fp16 in front of the
 * value product, as in the prefill kernels —, the suffix phase (the paged kernel over [grp_len, pos]) folds it in before the
 * division; stream order is the only synchronisation.  A row's result does not depend on which other slots are in its group; two
 * launches are bitwise equal.  ws: qpal_attn_prefix_ws_bytes(B, G, ...) bytes (max_len = max_pages * page_size; it contains the
 * paged launch's workspace), 4-byte aligned, zero-filled ONCE, kept across launches, always needed.  Checks and codes are the paged
 * sibling's; in addition a null row_group / grp_slot / grp_len: QPAL_E_NULL, G outside [1, 16]: QPAL_E_SHAPE, one of the three not
 * 4-byte aligned: QPAL_E_ALIGN. */
long qpal_attn_prefix_ws_bytes(int B, int G, int nq, int nkv, int hd, long max_len);
int qpal_attn_rope_decode_batch_shared(const float *q, const float *k, const float *v, long ld_qkv,
                                       void *kpool, void *vpool, void *out_f16, long ld_out,
                                       const long *pos, const float *inv_freq, const int *block_table, long ld_table,
                                       int num_pages, int page_size, int max_pages, int kv_fmt /* 0 fp16, 1 e4m3fn */,
                                       const int *row_group, const int *grp_slot, const int *grp_len, int G,
                                       int B, int nq, int nkv, int hd, float scale, void *ws, long ws_bytes, void *stream);

/* RAGGED prefill (csrc/attn_ragged.hip): rows of SEVERAL sequences in one launch.  q / k / v / out have R rows (1 <= R
 * <= 128) cut into S segments (1 <= S <= 128) that three DEVICE arrays describe — never read by the host, so a captured launch can
 * be replayed while segment lengths, sequences and positions change:
 *   seq int32 [S], row0 int32 [S + 1] (cumulative, row0[0] = 0), pos0 int64 [S]
 * Segment s is rows row0[s] .. row0[s + 1] - 1 (T_s rows), the tokens of sequence seq[s] at positions pos0[s] .. pos0[s] + T_s - 1.
 * For each segment the launch does exactly what qpal_attn_rope_prefill does for T = T_s rows on the cache of sequence seq[s]: the
 * rotary embedding, k / v appended (kv_fmt 0: fp16; 1: e4m3fn at the _kv8 store rule), causal attention of row t over positions 0 ..
 * pos0[s] + t of ITS sequence.  A decode token is a segment of one row.  Caches: [B][nkv][max_len][hd], 16-byte aligned; paged:
 * the pools and the block table [B][ld_table] of qpal_attn_rope_decode_batch_paged, max_len = max_pages * page_size.
 * A segment with T_s <= 0, row0[s] < 0, row0[s + 1] > R, seq[s] outside [0, B), pos0[s] < 0 or pos0[s] + T_s > max_len is inactive:
 * no cache byte and no out byte is written for it.  Out rows of no active segment keep what they held.  Two active segments that
 * name one sequence: the caller's error — that sequence's result is unspecified; no byte outside caches / pools, out and ws is
 * touched.  Paged: the guard on table entries outside [0, num_pages) is the paged siblings'.
 * A query tile never straddles two segments (tile j of a segment starts at its row j * TQ, TQ = 16 query rows, 32 / 64 for nq / nkv
 * = 2 / 1): per segment, chunks, partials and merge are those of the one-sequence launch of the same nsplit, so with one chunk
 * (max_len < 512) out is bit for bit that launch's.  The grid is fixed from (R, S, heads, max_len).  ws:
 * qpal_attn_ragged_ws_bytes(R, S, ...) bytes, 4-byte aligned, zero-filled ONCE, kept across launches; monotone in R, S and max_len,
 * 0 (pass NULL) for max_len < 512.  The tickets sit at a fixed offset (128 * nkv words in front of the partials), so a workspace
 * sized for (R, S, max_len) serves every launch of the same nq, nkv, hd with fewer rows, fewer segments or a shorter cache, in
 * either format, in any order (launches on one stream may share it); its layout is the ragged launches' own (a prefill workspace
 * does not stand in).  Two launches on the same input are bitwise equal.  Checks and codes are the siblings' (seq / row0: null QPAL_E_NULL, 4-byte aligned); in
 * addition S outside 1 .. 128, B < 1, kv_fmt not 0 / 1: QPAL_E_SHAPE. */
long qpal_attn_ragged_ws_bytes(int R, int S, int nq, int nkv, int hd, long max_len);
int qpal_attn_rope_prefill_ragged(const float *q, const float *k, const float *v, long ld_qkv,
                                  void *kcache, void *vcache, void *out_f16, long ld_out,
                                  const int *seq, const int *row0, const long *pos0, const float *inv_freq,
                                  int kv_fmt /* 0 fp16, 1 e4m3fn */, int R, int S, int B, int nq, int nkv, int hd,
                                  long max_len, float scale, void *ws, long ws_bytes, void *stream);
int qpal_attn_rope_prefill_ragged_paged(const float *q, const float *k, const float *v, long ld_qkv,
                                        void *kpool, void *vpool, void *out_f16, long ld_out,
                                        const int *seq, const int *row0, const long *pos0, const float *inv_freq,
                                        const int *block_table, long ld_table, int num_pages, int page_size, int max_pages,
                                        int kv_fmt, int R, int S, int B, int nq, int nkv, int hd,
                                        float scale, void *ws, long ws_bytes, void *stream);

/* SLIDING-WINDOW attention: the three launches above — batched decode, one-sequence prefill, ragged prefill — with a
 * lower edge.  window = W >= 1: the row at position p attends to keys lo(p) .. p, lo(p) = max(0, p - W + 1): W keys with its own
 * (Hugging Face's sliding_window).  window = 0: no window, the launch IS the sibling's.  window < 0: QPAL_E_PARAM, behind the null
 * checks and in front of everything else.  One entry point per family serves both element formats (kv_fmt 0 fp16, 1 e4m3fn) and
 * both storages: block_table (block_row) == NULL — contiguous caches of max_len positions, the paged arguments are ignored; else
 * the pools and the table of the paged sibling, max_len = max_pages * page_size, the max_len argument is ignored.
 * The rotary embedding, the append of every new k / v row, the inactive-slot and *pos0 fit rules and the stored bytes are the
 * siblings'.  Nothing outside the window is read: cache rows below lo(pos[b]) (decode) or below lo of the launch's / segment's FIRST
 * row (prefill, ragged) may hold anything, NaN included, and block-table entries of pages that lie wholly below that floor may be
 * -1 (PagedKVCache.trim).  window >= max_len: bit for bit the sibling, output and caches.
 * Decode: the sibling's arithmetic on the keys [lo, pos] — chunks cut on pos - lo; grid and LDS are those of min(max_len, window
 * rounded up to 4) positions, so a short window in a long cache takes one chunk and no merge.  Prefill / ragged: a query tile walks
 * the keys from the multiple of 32 at or below lo(its first row), the mask is per row; the chunks are sized for the longest span a
 * tile can have (window + rows of a tile + 30).  ws: the sibling's qpal_attn_*_ws_bytes of max_len always suffices (a windowed
 * launch never needs more, often none).  Other checks and codes: the siblings'. */
int qpal_attn_rope_decode_batch_window(const float *q, const float *k, const float *v, long ld_qkv,
                                       void *kcache, void *vcache, void *out_f16, long ld_out,
                                       const long *pos, const float *inv_freq, const int *block_table /* NULL: contiguous */,
                                       long ld_table, int num_pages, int page_size, int max_pages, int kv_fmt,
                                       int B, int nq, int nkv, int hd, long max_len, float scale, long window,
                                       void *ws, long ws_bytes, void *stream);
int qpal_attn_rope_prefill_window(const float *q, const float *k, const float *v, long ld_qkv,
                                  void *kcache, void *vcache, void *out_f16, long ld_out,
                                  const long *pos0, const float *inv_freq, const int *block_row /* NULL: contiguous */,
                                  int num_pages, int page_size, int max_pages, int kv_fmt,
                                  int T, int nq, int nkv, int hd, long max_len, float scale, long window,
                                  void *ws, long ws_bytes, void *stream);
int qpal_attn_rope_prefill_ragged_window(const float *q, const float *k, const float *v, long ld_qkv,
                                         void *kcache, void *vcache, void *out_f16, long ld_out,
                                         const int *seq, const int *row0, const long *pos0, const float *inv_freq,
                                         const int *block_table /* NULL: contiguous */, long ld_table, int num_pages, int page_size,
                                         int max_pages, int kv_fmt, int R, int S, int B, int nq, int nkv, int hd,
                                         long max_len, float scale, long window, void *ws, long ws_bytes, void *stream);

/* SCORE MODIFIERS: the three _window launches above with a logit soft cap (Gemma-2's attn_logit_softcapping) and
 * per-head sinks (gpt-oss); the argument lists are the _window ones plus softcap and sinks behind window.  For a row with scaled
 * scores s_j = scale * q.k_j over its admitted keys (causal, and windowed if window > 0):
 *   softcap = c > 0: s_j <- c * tanh(s_j / c), behind scale and in front of the maximum, the mask and everything else, the new
 *     position's own score included.  softcap = 0: no cap.  softcap < 0, NaN or inf: QPAL_E_PARAM (beside window < 0: behind the
 *     null checks, in front of everything else).
 *   sinks: fp32 [nq] on the device, 4-byte aligned (QPAL_E_ALIGN), read at every launch; NULL: none.  Head h's row becomes
 *     out = sum_j e^(s_j - M) v_j / (sum_j e^(s_j - M) + e^(sinks[h] - M)),  M = max(max_j s_j, sinks[h]):
 *     one more logit in the denominator and nowhere else (Hugging Face: concatenate a column, softmax, drop the column).  The sink
 *     is not soft-capped and has no value row; it enters once per row, where the row is finished (behind the chunk merge of a split
 *     launch, behind the last tile of a prefill row).  A sink far above every score drives the row to 0, without inf or NaN;
 *     sinks[h] = -inf is bit for bit the launch without sinks.
 * softcap == 0 && sinks == NULL: the call IS the _window entry point's.  Otherwise one instantiation per (format, storage, hd, rep)
 * built on the windowed kernel body serves every combination; window = 0 runs it with window = max_len.  The rotary embedding,
 * the append and the stored bytes, the inactive-slot and *pos0 fit rules, both formats, paging, the window rules and the
 * workspaces (qpal_attn_*_ws_bytes) are the _window launches'. */
int qpal_attn_rope_decode_batch_score(const float *q, const float *k, const float *v, long ld_qkv,
                                      void *kcache, void *vcache, void *out_f16, long ld_out,
                                      const long *pos, const float *inv_freq, const int *block_table /* NULL: contiguous */,
                                      long ld_table, int num_pages, int page_size, int max_pages, int kv_fmt,
                                      int B, int nq, int nkv, int hd, long max_len, float scale, long window,
                                      float softcap, const float *sinks, void *ws, long ws_bytes, void *stream);
int qpal_attn_rope_prefill_score(const float *q, const float *k, const float *v, long ld_qkv,
                                 void *kcache, void *vcache, void *out_f16, long ld_out,
                                 const long *pos0, const float *inv_freq, const int *block_row /* NULL: contiguous */,
                                 int num_pages, int page_size, int max_pages, int kv_fmt,
                                 int T, int nq, int nkv, int hd, long max_len, float scale, long window,
                                 float softcap, const float *sinks, void *ws, long ws_bytes, void *stream);
int qpal_attn_rope_prefill_ragged_score(const float *q, const float *k, const float *v, long ld_qkv,
                                        void *kcache, void *vcache, void *out_f16, long ld_out,
                                        const int *seq, const int *row0, const long *pos0, const float *inv_freq,
                                        const int *block_table /* NULL: contiguous */, long ld_table, int num_pages, int page_size,
                                        int max_pages, int kv_fmt, int R, int S, int B, int nq, int nkv, int hd,
                                        long max_len, float scale, long window, float softcap, const float *sinks,
                                        void *ws, long ws_bytes, void *stream);

/* Final norm + fp16 lm_head for `rows` rows of the residual stream at once, on the matrix pipe (csrc/lm_head_batch.hip): the
 * logits a sampler needs, and the batch-B tail of a decode step.  h_f32 fp32 [rows][ld_h] (ld_h >= k, in elements), 1 <= rows <=
 * 128; k a multiple of 512, 512 <= k <= 8192; w_f16 the lm_head fp16 [vocab][k]; logits_f32 fp32 [rows][ld_logits], ld_logits >=
 * vocab: logits[b][v] for v < vocab is written, columns vocab .. ld_logits are left as they were.  Per row the arithmetic of
 * qpal_lm_head_argmax: x = fp16(h * rsqrt(mean(h^2) + rms_eps)), then * rms_w in fp16 (rms_w_f16 == NULL: w = 1; rms_eps <= 0: no
 * norm, x = fp16(h), rms_w_f16 ignored); fp32 accumulation.  Every lm_head row is read once for all rows; no workspace, no
 * atomics, one writer per logit: two launches are bitwise equal.  Alignment: w_f16 and h_f32 16 bytes, ld_h % 4 == 0 when rows > 1, rms_w_f16 8 bytes, logits 4. */
int qpal_lm_head_logits(const float *h_f32, long ld_h, const void *rms_w_f16, float rms_eps, const void *w_f16, float *logits_f32,
                        long ld_logits, int rows, int vocab, int k, void *stream);

/* The next token of `rows` sequences (1 .. 128) from their logits fp32 [rows][ld_logits] (ld_logits >= vocab), one launch
 * (csrc/sample.hip).  temperature / top_p fp32 [rows], top_k int32 [rows], seed / ctr int64 [rows], token int64 [rows]: all on the
 * device and never read by the host (a captured launch can be replayed while the caller rewrites them); nothing is allocated.
 * For row b with logits l[0 .. vocab):
 *  1. ctr[b] < 0: the row is inactive; token[b] is not written.
 *  2. temperature[b] <= 0 or top_k[b] == 1: greedy.  token[b] = argmax, lowest index on ties; no row selected (NaN, all -inf): 0.
 *  3. Top-k on the raw fp32 logits: top_k[b] <= 0 or >= vocab keeps all; else keep {i : l[i] >= (k-th largest value)}; ties at the
 *     k-th value are all kept.
 *  4. z[i] = l[i] / T.  Top-p: top_p[b] >= 1 or <= 0 keeps all of step 3's set K.  Else with p[i] = exp(z[i] - zmax) / sum over K
 *     of exp(z[j] - zmax), keep {i in K : p[i] >= tau}, tau the largest value among the p's with sum{p[j] : p[j] >= tau} >= top_p.
 *  5. The race.  Token i: Philox4x32-10 with key (seed_lo, seed_hi) and counter (i >> 2, 0, ctr_lo, ctr_hi) (the 32-bit halves of
 *     seed[b] / ctr[b] as unsigned); x = output word i & 3; u = ((x >> 9) + 0.5) * 2^-23; e = -ln u; s[i] = z[i] - ln e.
 *     token[b] = argmax of s over the kept set, lowest index on ties (nothing selectable: 0).
 * A draw depends on (seed, ctr, token index, the row's logits and parameters) and on nothing else.  A NaN logit is never kept.
 * Integer arithmetic wherever sums could depend on an order: two launches are bitwise equal.                                 */
int qpal_sample(const float *logits_f32, long ld_logits, int rows, int vocab, const float *temperature, const int *top_k,
                const float *top_p, const long *seed, const long *ctr, long *token, void *stream);

/* qpal_sample with three more truncation filters: min-p, top-a and typical-p (csrc/sample.hip), still one launch.
 * min_p / top_a / typical_p fp32 [rows] on the device, never read by the host; each may be NULL, which turns that filter off for
 * every row (all three NULL: the launch of qpal_sample).  Shapes, alignment (4 bytes for the three) and return codes are
 * qpal_sample's, all decided on the host before any stream work.  Steps 1 - 4 of qpal_sample hold word for word: inactive rows,
 * greedy rows, the top-k set K and the nucleus N.  Between step 4 and the race, for row b:
 *  4a. The one distribution: w[i] = exp(z[i] - zmax) for i in N (zmax the maximum over K; it lies in N), S = sum over N of w, q[i] =
 *      w[i] / S — the tempered distribution renormalised over N.  ALL THREE filters are judged on this one q and the kept set is
 *      the intersection R = N ∩ A ∩ B ∩ C: there is no renormalisation between the three and no order among them (libraries that
 *      chain the filters renormalise after each and so depend on their order; this entry does not).
 *      min-p, on iff min_p[b] > 0 (values above 1 read as 1):  A = {i : q[i] >= min_p max q} = {i : w[i] >= min_p}.
 *      top-a, on iff top_a[b] > 0:  B = {i : q[i] >= top_a (max q)^2} = {i : w[i] >= top_a / S}.
 *      typical-p, on iff 0 < typical_p[b] < 1:  c = sum over N of q[i] (zmax - z[i]) (the entropy of q is c + ln S, so -ln q[i] - H =
 *      (zmax - z[i]) - c), d[i] = |(zmax - z[i]) - c|, C = {i in N : d[i] <= delta}, delta the smallest value among the d's with
 *      sum{q[j] : d[j] <= delta} >= typical_p; ties at delta are all kept (step 4's rule mirrored).
 *      R empty (typical-p can exclude the likeliest token, which min-p keeps): R = the one token argmax l over N, lowest id on ties.
 *      +inf logits share the mass equally and have d = 0; no logit above -inf: token 0; a NaN logit is never kept.
 *  5. The race of qpal_sample, over R.
 * A row on which none of the three is on takes steps 1 - 5 of qpal_sample: its token is bitwise the one qpal_sample returns.
 * A draw depends on (seed, ctr, token index, the row's logits and parameters) and on nothing else; two launches are bitwise equal. */
int qpal_sample_trunc(const float *logits_f32, long ld_logits, int rows, int vocab, const float *temperature, const int *top_k,
                      const float *top_p, const float *min_p, const float *top_a, const float *typical_p,
                      const long *seed, const long *ctr, long *token, void *stream);

/* Log-probability of ONE token per row under the plain softmax of the row's raw logits (temperature 1, no top-k / top-p: what
 * "logprobs" means to a sampler's user and what a cross-entropy sums), one launch (csrc/logprob.hip).  logits fp32
 * [rows][ld_logits], 1 <= rows <= 128, 1 <= vocab <= 2^30, ld_logits >= vocab — the shapes and return codes of qpal_sample.  token int64
 * [rows], logprob fp32 [rows]; lse fp32 [rows], rank int32 [rows] and active int64 [rows] may each be NULL.  All on the device and
 * never read by the host (capturable; the caller may rewrite token / active between replays); no workspace, no atomics.
 * For row b with logits l[0 .. vocab) and t = token[b]:
 *  1. t < 0, t >= vocab, or active != NULL and active[b] < 0 (qpal_sample's rule for ctr: a decode step passes its positions):
 *     the row is inactive; nothing is written to any output of it.
 *  2. A NaN logit is read as -inf.  lse[b] = log sum_i exp(l[i]);  logprob[b] = l[t] - lse[b];  rank[b] = #{i : l[i] > l[t]}
 *     on the raw fp32 values (exact; 0: t is a most likely token).
 *  3. l[t] = -inf: logprob = -inf.  No logit above -inf: lse = -inf, logprob = -inf, rank = 0.  +inf logits: lse = +inf and the
 *     +inf entries share the mass, logprob = -log(their number) for each of them, -inf for every other token.
 * Sums run in a fixed order: two launches on the same input are bitwise equal.  lse and logprob are within 2^-15 + 2^-22 max|l|
 * of the fp64 value.                                                                                          */
int qpal_token_logprob(const float *logits_f32, long ld_logits, int rows, int vocab, const long long *token, float *logprob,
                       float *lse, int *rank, const long long *active, void *stream);

/* The n likeliest tokens of every row and their log-probabilities under the plain softmax of the row's raw logits — the
 * "top_logprobs" of a completion API —, one launch (csrc/top_logprob.hip).  logits fp32 [rows][ld_logits],
 * 1 <= rows <= 128, 1 <= vocab <= 2^30, ld_logits >= vocab, 1 <= n <= 64; top_id int32 [rows][n], top_logprob fp32 [rows][n]; lse
 * fp32 [rows] and active int64 [rows] may each be NULL.  Alignment: 4 bytes, 8 for active.  The return codes of qpal_sample
 * (QPAL_E_NULL / QPAL_E_SHAPE / QPAL_E_ALIGN).  All on the device and never read by the host (capturable); one launch, no
 * workspace, no global atomics.  For row b:
 *  1. Inactive rows.  active != NULL and active[b] < 0: nothing of row b is written.
 *  2. Logit values.  l is the row's first vocab fp32 values, with NaN read as -inf.
 *  3. Order and ids.  The tokens are ordered by l descending, comparing fp32 VALUES, so -0 and +0 tie.  Equal values are ordered
 *     by ascending token id; NaN and -inf entries therefore tie with each other and order by id.  top_id[b][j] is the j-th token
 *     of that order for j < min(n, vocab).  The remaining entries are id = -1, logprob = -inf.
 *  4. Log-probabilities.  top_logprob[b][j] is the value qpal_token_logprob defines for token top_id[b][j] on this row, and
 *     lse[b] is that kernel's lse.  Its special cases hold unchanged: no logit above -inf: every log-prob is -inf, lse is -inf,
 *     ids are 0 .. n-1; +inf logits share the mass, -log(count) each, and every other entry is -inf; a token at -inf gets -inf.
 *  5. Bitwise guarantees.  Sums run in a fixed order: two launches are bitwise equal.  top_logprob[b][j] and lse[b] are BITWISE
 *     equal to what qpal_token_logprob returns for token = top_id[b][j] on the same row: the drawn token's entry in the list
 *     carries exactly the sampler's logprob.
 *  6. Greedy consequence.  top_id[b][0] equals qpal_sample's greedy token on every row, degenerate rows included.            */
int qpal_top_logprob(const float *logits_f32, long ld_logits, int rows, int vocab, int n, int *top_id, float *top_logprob,
                     float *lse, const long long *active, void *stream);

/* SPECULATIVE decoding (csrc/spec.hip): the two ends of a step that feeds, per sequence, its pending token and up to
 * K guessed tokens as ONE segment of a ragged step (§18), draws at every row, and keeps the guesses that equal the draws.
 * Everything is on the device and never read by the host (a captured step is replayed while the state moves); no workspace, no
 * global atomics, one writer per word: two launches on one state are bitwise equal.  State of slot b of B (1 .. 128):
 *   hist int32 [B][ld_hist]  the tokens of the sequence          n_tok int64 [B]  how many are known; the last one, at position
 *   limit int64 [B]          the bound n_tok may reach                            n_tok - 1, is PENDING: known, not yet fed
 *   eos   int64 [B]          the stop token, -1: none
 * Slot b is ACTIVE iff 1 <= n_tok[b] < limit[b], n_tok[b] <= max_len and n_tok[b] <= ld_hist.
 *
 * qpal_spec_draft builds the step's inputs.  K 0 .. 15, 1 <= gmin <= gmax <= 8, B <= R <= 128 (the step's rows), max_len >= 1 (cache
 * positions), 1 <= ld_hist < 2^31.  For an active slot with n = n_tok[b]: d_max = max(0, min(K, limit - n - 1, max_len - n)).
 *   ext_draft != NULL (int64 [B][K], ext_n int32 [B]): the drafts are ext_draft[b][0 .. min(ext_n[b], d_max)); an entry outside
 *     [0, 2^30) ends them there.
 *   ext_draft == NULL: prompt lookup.  For g = gmax down to gmin with g < n: the largest j with j + g < n and hist[j .. j + g) ==
 *     hist[n - g .. n); the first g that has one gives the drafts hist[j + g .. min(j + g + d_max, n)); none: no drafts.
 * Packing: segment b is slot b.  row0[0] = 0, row0[b + 1] = row0[b] + (active ? 1 + n_draft[b] : 0); every active slot has its one
 * row (R >= B) and drafts are handed out in slot order until R is full: slot b keeps min(its drafts, R - (active slots) - (drafts
 * kept by slots before it)).  Outputs: tokens int64 [R] (per segment the pending token, then its drafts; 0 in unused rows), seq int32
 * [B] (b, or -1: inactive), row0 int32 [B + 1], pos0 int64 [B] = n_tok - 1 — the descriptors of qpal_attn_rope_prefill_ragged with S
 * = B; row_slot int32 [R] (the slot of each row, -1: unused), row_ctr int64 [R] (the row's position = qpal_sample's ctr, -1: unused),
 * n_draft int32 [B] (0: a plain decode token).  Two stream-ordered launches (search, pack); between them n_draft / pos0 hold the
 * search's interim result.
 *
 * qpal_spec_accept takes drawn int64 [R] (the sampler's token per row) and tokens / seq / row0 as the draft call wrote them.  A
 * segment counts iff seq[b] == b, it has T in 1 .. K + 1 rows inside [0, R] and 1 <= n_tok[b] < limit[b].  With r = row0[b]:
 *   m = the largest value <= T - 1 with tokens[r + i + 1] == drawn[r + i] for all i < m           (the accepted drafts)
 *   emitted = drawn[r .. r + m], cut to limit - n_tok tokens and after the first token equal to eos[b] when eos[b] >= 0
 * The emitted tokens are appended to hist (a token that would land at or past ld_hist is emitted but not recorded; the slot is
 * inactive from then on) and n_tok advances; an emitted eos sets limit[b] = n_tok[b].  out_tok int64 [B][K + 1]: the emitted tokens,
 * entries past n_out keep what they held; n_out int32 [B] (>= 1; 0: the segment did not count, nothing else of it changes); n_acc
 * int32 [B] = m before the cut.
 * Codes are qpal_sample's: a null pointer (ext_draft may be NULL; then ext_n is ignored) QPAL_E_NULL; a range above QPAL_E_SHAPE;
 * int32 arrays 4-byte, int64 arrays 8-byte aligned, else QPAL_E_ALIGN — all decided on the host before any stream work. */
int qpal_spec_draft(const int *hist, long ld_hist, const long *n_tok, const long *limit, const long *ext_draft, const int *ext_n,
                    int B, int K, int gmin, int gmax, int R, long max_len, long *tokens, int *seq, int *row0, long *pos0,
                    int *row_slot, long *row_ctr, int *n_draft, void *stream);
int qpal_spec_accept(const long *tokens, const long *drawn, const int *seq, const int *row0, int *hist, long ld_hist, long *n_tok,
                     long *limit, const long *eos, int B, int K, int R, long *out_tok, int *n_out, int *n_acc, void *stream);

/* LOGIT PROCESSORS (csrc/logit_proc.hip): token masks, a sparse logit bias and repetition / presence / frequency
 * penalties, applied to the logits between qpal_lm_head_logits and qpal_sample.  State of slot b of `slots` (1 .. 128), all on the
 * device and never read by the host (a captured launch is replayed while the caller rewrites the state):
 *   count int32 [slots][ld_count]          how often token i has been counted for the slot (ld_count >= vocab)
 *   repetition, presence, frequency fp32 [slots]      neutral: 1, 0, 0; repetition > 0, all finite
 *   mask uint32 [slots][ld_mask]           bit i & 31 of word i >> 5 set: token i is allowed (ld_mask >= ceil(vocab / 32))
 *   mask_on int32 [slots]                  0: the slot's mask is ignored
 *   bias_id int32 [slots][bias_slots], bias_val fp32 [slots][bias_slots], bias_n int32 [slots]       the first bias_n[b] (clamped
 *                                          to 0 .. bias_slots) entries are the slot's bias; their ids are distinct, values finite
 *
 * qpal_logit_process: logits fp32 [rows][ld_logits] -> out fp32 [rows][ld_out], 1 <= rows <= 128, 1 <= vocab <= 2^30, both strides
 * >= vocab.  out == logits with ld_out == ld_logits is the in-place form; any other overlap is QPAL_E_PARAM.  Row r belongs to slot
 * b = row_slot[r] (int32 [rows]).  It is INACTIVE, and no word of out's row is written, when ctr[r] < 0 (int64 [rows]: qpal_sample's
 * counters), when b is outside [0, slots), or (tokens != NULL) when r - row0[b] is outside 0 .. 15 or row0[b] < 0.  For an active
 * row with logits l[0 .. vocab):
 *  1. c[i] = count[b][i] + #{extra tokens of the row equal to i}.  Extras exist only with tokens != NULL (int64 [rows], row0 int32
 *     [slots + 1]: qpal_spec_draft's): tokens[row0[b] + 1 .. r], the guessed tokens in front of row r in its segment, at most 15;
 *     an extra outside [0, vocab) counts for nothing.
 *  2. Where c[i] > 0 and l is no NaN:  l = l > 0 ? l / repetition : l * repetition;  then  l = l - (presence + frequency * float(c)).
 *     Four fp32 operations, each rounded once to nearest, in exactly this order, no fused multiply-add.  Where c[i] == 0, and under
 *     neutral parameters, l keeps its bits.
 *  3. mask_on[b] != 0 and the bit of i clear: l = -inf (a NaN too).
 *  4. l[bias_id[b][j]] += bias_val[b][j] for j < bias_n[b] (ids outside [0, vocab) are skipped; -inf stays -inf, a NaN stays).
 * A NaN logit passes through 2 and 4 with its bits; qpal_sample reads it as -inf.  Columns vocab .. ld_out are not written.
 * Elementwise over (vocab tiles) x rows workgroups; no workspace, no atomics, one writer per word: two launches are bitwise equal,
 * and equal to logits.reference_process (numpy fp32, the same operations) bit for bit.
 *
 * qpal_logit_observe: count[s][tokens[r]] += 1 for r < n (1 .. 2048), s = slot[r] (int32 [n]) or, with slot == NULL, slot0 for
 * every row.  A row is skipped when s is outside [0, slots), when active != NULL and active[r] < 0 (int64 [n]), or when tokens[r]
 * (int64 [n]) is outside [0, vocab).  Integer atomic adds: the result does not depend on their order.
 *
 * Codes, all decided on the host before any stream work: a null pointer QPAL_E_NULL (tokens and row0 are NULL together; the three
 * bias arrays may be NULL when bias_slots == 0; slot and active may be NULL); rows, n, slots, vocab, a stride below its width or
 * bias_slots outside 0 .. 1024, slot0 outside [0, slots) when slot == NULL: QPAL_E_SHAPE; fp32 / int32 arrays 4-byte, int64 arrays
 * 8-byte aligned, else QPAL_E_ALIGN. */
int qpal_logit_process(const float *logits_f32, long ld_logits, float *out_f32, long ld_out, int rows, int vocab, const int *row_slot,
                       const long *ctr, int slots, const int *count, long ld_count, const float *repetition, const float *presence,
                       const float *frequency, const unsigned *mask, long ld_mask, const int *mask_on, const int *bias_id,
                       const float *bias_val, const int *bias_n, int bias_slots, const long *tokens, const int *row0, void *stream);
int qpal_logit_observe(int *count, long ld_count, int slots, int vocab, const int *slot, int slot0, const long *tokens,
                       const long *active, int n, void *stream);

/* GRAMMAR-CONSTRAINED DECODING (csrc/grammar.hip): a byte-level deterministic automaton per slot, followed on the
 * device.  An automaton of S states (1 .. 65534; state 0 is the start):
 *   trans uint16 [S][256]      the state byte c leads to from state s, 0xFFFF: none (any value >= S is read as none)
 *   accept uint8 [S]           != 0: the text may end here
 * The vocabulary: tok_off int32 [vocab + 1] and tok_bytes uint8 [total_bytes] — token t is the bytes tok_off[t] .. tok_off[t + 1];
 * a token without bytes (or whose offsets do not lie in 0 <= tok_off[t] < tok_off[t + 1] <= total_bytes) is never allowed; eos in
 * [0, vocab) ends a text, whatever bytes it has.  A slot's state is an int32: 0 .. S - 1 a state of its automaton, S FINISHED (eos
 * has been emitted), -1 DEAD; any other value is read as dead.
 *   step(s, t):  s dead: dead.  s == S: t == eos ? S : dead.  t == eos: accept[s] ? S : dead.  t outside [0, vocab): dead.
 *                Else follow t's bytes through trans; a byte without a transition, or an empty token: dead.
 *
 * qpal_grammar_compile: allow uint32 [S + 1][ld_allow] (ld_allow >= ceil(vocab / 32); bit t & 31 of word t >> 5 — the layout of
 * qpal_logit_process's mask).  Row s < S: bit t set iff step(s, t) is not dead; row S: the eos bit only.  Words ceil(vocab / 32) ..
 * ld_allow of a row are not written; the bits past vocab in a row's last word are written as 0.  One thread per (state, token),
 * a wave's 64 verdicts are one ballot = two words; runs once when an automaton is loaded, never in a step.
 *
 * A bank: trans uint16 [grammars][max_states][256], accept uint8 [grammars][max_states], n_states int32 [grammars], allow uint32
 * [grammars][max_states + 1][ld_allow], and per slot gram int32 [slots] (-1: no grammar) and state int32 [slots].  A slot HAS a
 * grammar when gram[b] lies in [0, grammars) and n_states[gram[b]] in [1, max_states]; 1 <= slots <= 128, grammars <= 1024.
 *
 * qpal_grammar_rows: a speculative step's segments (tokens int64 [rows], row0 int32 [slots + 1]: qpal_spec_draft's) ->
 * row_state int32 [rows], 1 <= rows <= 128.  EVERY row is written: -1, except that for a slot b with a grammar, a segment
 * (0 <= row0[b] < row0[b + 1] <= rows, at most 16 rows) and state[b] in [0, S], row row0[b] + j gets
 * step(.. step(state[b], tokens[row0[b] + 1]) .., tokens[row0[b] + j]) — the pending token at row0[b] is already in state[b].
 *
 * qpal_grammar_mask: in place on logits fp32 [rows][ld_logits] (ld_logits >= vocab, 1 <= rows <= 128).  Row r with b = row_slot[r]
 * is SKIPPED, no word of it written, when ctr[r] < 0, b is outside [0, slots), slot b has no grammar, or row_state[r] is outside
 * [0, S].  Else l[t] = -inf for every t < vocab whose bit in allow[gram[b]][row_state[r]] is clear (a NaN too), and nothing else is
 * written; the logits are not read.  A decode step passes state as row_state (row = slot).
 *
 * qpal_grammar_advance: state[b] = step(.. step(state[b], tokens[b][0]) .., tokens[b][m - 1]) over tokens int64 [slots][width]
 * (1 <= width <= 16), m = n[b] clamped to 0 .. width, or width with n == NULL.  Slot b is skipped — state[b] is not written — when
 * it has no grammar, when active != NULL and active[b] < 0 (int64 [slots]), or when m == 0.
 *
 * rows, mask and advance read their state on the device, never synchronise and write each word by one thread: capturable, and
 * equal launches leave equal bits.  Codes, all decided on the host before any stream work: a null pointer (n and active may be
 * NULL) QPAL_E_NULL; n_states, max_states, grammars, slots, rows, width, vocab, total_bytes < 0, eos outside [0, vocab) or a stride
 * below its width QPAL_E_SHAPE; uint16 arrays 2-byte, fp32 / int32 / uint32 arrays 4-byte, int64 arrays 8-byte aligned, else
 * QPAL_E_ALIGN. */
int qpal_grammar_compile(const unsigned short *trans, const unsigned char *accept, int n_states, const int *tok_off,
                         const unsigned char *tok_bytes, int vocab, int total_bytes, int eos, unsigned *allow, long ld_allow,
                         void *stream);
int qpal_grammar_rows(const unsigned short *trans, const unsigned char *accept, const int *n_states, int grammars, int max_states,
                      const int *tok_off, const unsigned char *tok_bytes, int vocab, int total_bytes, int eos, const int *gram,
                      const int *state, int slots, const long *tokens, const int *row0, int rows, int *row_state, void *stream);
int qpal_grammar_mask(float *logits_f32, long ld_logits, int rows, int vocab, const int *row_slot, const long *ctr,
                      const int *row_state, const int *gram, int slots, const int *n_states, int grammars, int max_states,
                      const unsigned *allow, long ld_allow, void *stream);
int qpal_grammar_advance(const unsigned short *trans, const unsigned char *accept, const int *n_states, int grammars, int max_states,
                         const int *tok_off, const unsigned char *tok_bytes, int vocab, int total_bytes, int eos, const int *gram,
                         int *state, int slots, const long *tokens, int width, const int *n, const long *active, void *stream);

/* STOP CONDITIONS (csrc/stop.hip): stop strings, stop token ids, token budgets and the context limit of every slot,
 * judged on the device by one launch at the end of a step.  A STOP SET of S states (1 .. 65535; state 0 is the start) is the
 * byte-level Aho-Corasick automaton of 1 .. 64 byte strings in dense form, failure links resolved:
 *   trans uint16 [S][256]      the state byte c leads to from state s; a value >= S is read as 0
 *   out_len uint16 [S]         the length of the LONGEST string that ends at state s (suffix links closed), 0: none
 * The vocabulary is the grammar block's: tok_off int32 [vocab + 1], tok_bytes uint8 [total_bytes]; a token outside [0, vocab), or
 * whose offsets do not lie in 0 <= tok_off[t] <= tok_off[t + 1] <= total_bytes, has no bytes.
 * A bank (qpal_stop_bank, a HOST struct read before the call returns; every pointer is device memory the host never reads):
 *   trans uint16 [sets][max_states][256], out_len uint16 [sets][max_states], n_states int32 [sets]       sets 1 .. 256
 *   set_id int32 [slots]       the slot's stop set; it HAS one when set_id lies in [0, sets) and n_states[set_id] in [1, max_states]
 *   ac_state int32 [slots]     the automaton state; a value outside [0, S) is read as 0
 *   stop_ids int32 [slots][id_slots], n_ids int32 [slots]     the first n_ids (clamped to 0 .. id_slots; id_slots 1 .. 16) are the ids
 *   max_tokens int32 [slots]   0: no bound          min_tokens int32 [slots]
 *   n_gen int32 [slots]        tokens generated     gen_bytes int64 [slots]      bytes generated
 *   out int64 [slots][cap]     the generated tokens (cap >= 1); a token past cap is counted, not recorded
 *   reason int32 [slots]       0 running, 1 stop id, 2 stop string, 3 max_tokens, 4 context
 *   text_len int64 [slots]     the bytes of the generated text that belong to the answer
 *   hit int32 [slots]          the automaton state at the match (reason 2)
 *   end_pos int64 [slots]      the position the slot had reached when it finished
 *
 * JUDGING one generated token t of slot b whose next position (the one t would be fed at) is q:
 *  1. n_gen += 1; out[b][n_gen - 1] = t if n_gen <= cap.
 *  2. exempt = n_gen < min_tokens.
 *  3. Not exempt and t equals one of the slot's stop ids: reason 1, text_len = gen_bytes; t's bytes are not walked.
 *  4. Else t's bytes are walked through trans from ac_state, gen_bytes += 1 per byte (a slot without a set: gen_bytes += the number
 *     of bytes, no walk, ac_state untouched).  At the FIRST byte whose new state s has out_len[s] > 0, in a token that is not exempt:
 *     reason 2, text_len = gen_bytes - out_len[s], hit = s, the rest of the token is not walked.  ac_state = the last state reached.
 *  5. Still running, max_tokens > 0 and n_gen >= max_tokens: reason 3, text_len = gen_bytes.
 *  6. Still running and q >= max_len: reason 4, text_len = gen_bytes.
 * A slot that finishes gets reason[b] and end_pos[b] = q; reason, text_len, hit and end_pos are written then and only then.
 *
 * qpal_stop_advance, 1 <= slots <= 128, max_len >= 1 (cache positions), tokens int64 [slots][width]:
 *   DECODE mode (n_out == NULL, width == 1, tok / pos int64 [slots]): slot b is judged iff 0 <= pos[b] < max_len, with q = pos[b] + 1.
 *     Finished: pos[b] = -1 (tok[b] keeps its value).  Goes on: tok[b] = tokens[b], pos[b] += 1.  A skipped slot keeps every word.
 *   SPECULATIVE mode (n_out int32 [slots] read and written; n_tok / limit int64 [slots]: qpal_spec_accept's, as the accept left
 *     them; 1 <= width <= 16): with m = n_out[b] clamped to 0 .. width, tokens[b][0 .. m) are judged in order, token j with q =
 *     n_tok[b] - m + j.  At the first j that finishes the slot: n_out[b] = j + 1, n_tok[b] = n_tok[b] - m + j + 1, limit[b] =
 *     n_tok[b] (the slot is inactive from then on).  m == 0: the slot is skipped.  tok / pos are ignored.
 * One wave per slot: the wave fetches the tokens, their offsets and bytes and the stop ids, one lane walks.  No workspace, no
 * atomics, one writer per word: two launches on equal state leave equal bits, equal to stop.reference_stop_advance.
 *
 * qpal_stop_mask: in place on logits fp32 [rows][ld_logits] (1 <= rows <= 128, ld_logits >= vocab), the min_tokens mask in front of
 * the draw.  Row r with b = row_slot[r] is the j-th row of its slot's segment, j = r - row0[b] (row0 int32 [slots + 1]:
 * qpal_spec_draft's) or j = 0 with row0 == NULL (a decode step).  It is SKIPPED when ctr[r] < 0 (int64 [rows]), b is outside
 * [0, slots), or (row0 != NULL) row0[b] < 0 or j outside 0 .. 15.  Else, while n_gen[b] + j < min_tokens[b], l[id] = -inf for each of
 * the slot's stop ids in [0, vocab); nothing else is written and the logits are not read.  One workgroup.
 *
 * Both read their state on the device, never synchronise: capturable.  Codes, all decided on the host before any stream work: a
 * null pointer (the bank's fields included; row0 may be NULL; of n_out / n_tok / limit and tok / pos the mode's own must be there)
 * QPAL_E_NULL; slots, rows, width, sets, max_states, id_slots, cap, vocab, total_bytes, max_len or a stride outside the ranges above
 * QPAL_E_SHAPE; decode mode with width != 1 QPAL_E_PARAM; uint16 arrays 2-byte, fp32 / int32 arrays 4-byte, int64 arrays 8-byte
 * aligned, else QPAL_E_ALIGN. */
typedef struct qpal_stop_bank {
    const unsigned short *trans;
    const unsigned short *out_len;
    const int *n_states;
    const int *set_id;
    int *ac_state;
    const int *stop_ids;
    const int *n_ids;
    const int *max_tokens;
    const int *min_tokens;
    int *n_gen;
    long *gen_bytes;
    long *out;
    int *reason;
    long *text_len;
    int *hit;
    long *end_pos;
    int sets, max_states, id_slots, cap;
} qpal_stop_bank;
int qpal_stop_advance(const qpal_stop_bank *bank, const int *tok_off, const unsigned char *tok_bytes, int vocab, int total_bytes,
                      int slots, const long *tokens, int width, int *n_out, long *n_tok, long *limit, long *tok, long *pos,
                      long max_len, void *stream);
int qpal_stop_mask(float *logits_f32, long ld_logits, int rows, int vocab, const int *row_slot, const long *ctr, const int *row0,
                   const int *stop_ids, int id_slots, const int *n_ids, const int *min_tokens, const int *n_gen, int slots,
                   void *stream);

/* PROXY HESSIAN of a linear layer's inputs (csrc/hessian.hip):  H += X^T X  and  colsum += 1^T X  in one launch.
 *   X       fp16 [rows, n] row-major, row stride ld_x >= n elements (a column slice of a wider buffer is passed as it lies);
 *           base 16-byte aligned, ld_x a multiple of 8
 *   H       fp64 [n, n] row-major.  H is cut into tiles of QPAL_HESSIAN_TILE rows and columns (the last one is half as wide when
 *           n % 128 == 64); the call touches the tiles on and below the diagonal only, diagonal tiles in full.  Tiles above the
 *           diagonal are neither read nor written: the caller mirrors the lower triangle when it needs the whole matrix
 *   colsum  fp64 [n], may be NULL
 *   n       a multiple of 64, 64 .. 32768;  rows >= 0 (0: success, nothing is launched)
 * For every element it owns  H[i][j] += sum_r X[r][i] X[r][j],  colsum[j] += sum_r X[r][j].  The fp16 products are exact in the
 * fp32 accumulator of v_mfma_f32_16x16x32_f16; at most 256 consecutive rows are summed in fp32 before the partial sum is added to
 * an fp64 copy of the tile that stays in registers, and H is read and written once per call:
 *   |error of H[i][j]| <= 256 * 2^-23 * sum_r |X[r][i]| |X[r][j]|   (colsum: sum_r |X[r][j]|), plus fp64 rounding.
 * One workgroup owns a tile for the whole call — no atomics, no split over rows — so equal sequences of calls give equal bits.
 * Never synchronises, capturable.  Codes: H or X null QPAL_E_NULL; n, rows out of range or ld_x < n QPAL_E_SHAPE; X not 16-byte
 * aligned, ld_x % 8, H or colsum not 8-byte aligned QPAL_E_ALIGN — all decided before any stream work. */
#define QPAL_HESSIAN_TILE 128
int qpal_hessian_accum(double *H, double *colsum, const void *X_f16, long ld_x, int rows, int n, void *stream);

/* MULTI-ADAPTER LoRA on one projection group (csrc/lora.hip):  out[i] += B[a] (A[a] xin[i])  with a = row_adapter[i],
 * shrink and expand in ONE launch, no workspace, no atomics.  For every row i < rows whose a lies in [0, N):
 *   xin     the row's input under in_mode, NOT rounded to fp16:
 *             QPAL_IN_F16         `in` fp16 [rows][k], as is
 *             QPAL_IN_F32         `in` fp32 [rows][k], as is; with rms_eps >= 0:  x * rsqrt(mean(x^2) + rms_eps) * w,  w = rms_weight
 *                                 fp16 [k] or NULL (no weight).  rms_eps < 0: no norm (rms_weight must then be NULL)
 *             QPAL_IN_SWIGLU_F32  `in` fp32 [rows][2k] = up | gate:  silu(gate) * up  (qpal_hadamard's convention)
 *           the norm exists for QPAL_IN_F32 only: rms_eps >= 0 or a weight with another mode is QPAL_E_PARAM
 *   shrink  t = A[a] xin.  A fp16 [N][P * R][k] row-major, block p owning rows p R .. p R + R - 1; fp32 sums
 *   expand  for p < P, j < blk_m[p]:  out[i][blk_off[p] + j] += sum_r B[a][boff_p + j][r] t[p R + r].  B fp16 [N][sum blk_m][R]
 *           row-major, the blocks in order (boff_p = blk_m[0] + .. + blk_m[p - 1]); the adapter's scale alpha / r is folded into B
 *           by the caller.  out fp32, row stride ld_out elements; the add is one fp32 read-modify-write by the element's one owner
 * A row whose row_adapter[i] is outside [0, N) (-1: no adapter) has none of its out bytes read or written; a launch of such rows
 * reads row_adapter and leaves.  Columns outside the blocks are never touched.
 *   blk_off, blk_m  HOST arrays of P ints (read before the call returns); row_adapter int32 [rows] on the device
 * Limits: rows 1 .. 128;  R a multiple of 8, 8 .. 64;  P 1 .. 3;  k a multiple of 64, 64 .. 32768;  N >= 1;  blk_m multiples of 16;
 * blk_off >= 0, blk_off + blk_m <= ld_out, the blocks' column ranges disjoint;  in, A, B, rms_weight 16-byte aligned, out and
 * row_adapter 4-byte aligned;  out must not overlap in.
 * Error against exact arithmetic on the stored values:  <= 2e-5 * sum_r |B_jr| * sum_l |A_rl xin_l|  +  2^-23 |out|  per element.
 * Equal launches give equal bits, and a row's out bits depend on its input, its adapter and its out value only — not on its row
 * index, the other rows or their adapters.  Never reads device memory on the host, never synchronises: capturable.
 * Codes, all decided before any stream work (out untouched): a null pointer QPAL_E_NULL; rows, k, R, P, N, blk_m, blk_off or
 * ld_out outside the limits QPAL_E_SHAPE; an unknown in_mode, a norm outside QPAL_IN_F32, out overlapping in QPAL_E_PARAM; a
 * misaligned pointer QPAL_E_ALIGN. */
int qpal_lora_apply(float *out_f32, long ld_out, const void *in, int in_mode, float rms_eps, const void *rms_weight, const void *A,
                    const void *B, const int *blk_off, const int *blk_m, int P, const int *row_adapter, int rows, int k, int R, int N,
                    void *stream);

/* BLOCK GLUE of Qwen- and Gemma-shaped layers (csrc/block_glue.hip; blocks.py restates each rule in numpy float64).
 * Four launches on fp32 rows that lie in memory between the existing launches of a step.  Each is ONE launch on `stream`, reads
 * nothing on the host and never synchronises (capturable); rows == 0 is success with nothing launched; rows up to 65535.  Codes are
 * decided before any stream work: a null pointer QPAL_E_NULL, a size outside the limits QPAL_E_SHAPE, a bad eps / cap / pairing or
 * an overlap QPAL_E_PARAM, a misaligned pointer or stride QPAL_E_ALIGN.
 *
 * qpal_qkv_prep: in place on q [rows][nq * hd], k and v [rows][nkv * hd], fp32 views with ONE row stride ld (elements, >= nq * hd) —
 *   the views every attention entry point takes, in whatever order they lie in the caller's buffer; 4-byte aligned, disjoint.
 *   bias   fp32 [(nq + 2 nkv) hd] in q | k | v order, or NULL:  x += b  on q, k and v (one fp32 add: equal to the host's fp32 x + b)
 *   q_norm_w, k_norm_w  fp32 [hd] each, both or neither (one alone: QPAL_E_PARAM).  BEHIND the bias every head of q and of k becomes
 *          x * rsqrt(mean_hd(x^2) + eps) * w  in fp32 ((x * inv) * w, the sum of squares over the head's hd elements); v is not
 *          normed; a head of zeros stays zero.  w is the EFFECTIVE weight (Gemma's 1 + w is the caller's).  eps <= 0, NaN or inf
 *          with weights given: QPAL_E_PARAM
 *   hd in {64, 128, 256}, nq and nkv 1 .. 1024, else QPAL_E_SHAPE.  Neither bias nor weights: success, nothing is launched.
 *   Columns of the caller's buffer outside the three views are never read or written.
 * qpal_norm_add:  h[r] += y[r] * rsqrt(mean_n(y[r]^2) + eps) * w  in fp32 ((y * inv) * w, then one add), the sandwich post-norm and
 *   the residual add.  n a multiple of 4, 4 .. 16384; w fp32 [n], the effective weight; h, y, w 16-byte aligned, ld_h and ld_y
 *   multiples of 4 and >= n; h must not overlap y (QPAL_E_PARAM); eps as above.
 * qpal_glu_gelu_tanh:  act[r][j] = gelu_tanh(ug[r][inter + j]) * ug[r][j]  for j < inter — ug is the up | gate row pair —,
 *   gelu_tanh(g) = 0.5 g (1 + tanh(0.7978845608 (g + 0.044715 g^3))), the tanh in the clamped exp / rcp form of the attention
 *   soft cap (absolute error <= 4 * 2^-24).  inter a multiple of 4 up to 2^24, ld_act >= inter, ld_ug >= 2 inter; act and ug 16-byte
 *   aligned, strides multiples of 4; act must not overlap ug.
 * qpal_logit_cap:  l <- cap * tanh(l / cap)  in place on logits [rows][ld >= vocab] (columns past vocab are left alone), the same
 *   tanh form: absolute error <= 5 * 2^-24 * cap + 2^-24 |result|.  cap <= 0, NaN or inf: QPAL_E_PARAM.  4-byte aligned. */
int qpal_qkv_prep(float *q, float *k, float *v, long ld, int rows, int nq, int nkv, int hd, const float *bias, const float *q_norm_w,
                  const float *k_norm_w, float eps, void *stream);
int qpal_norm_add(float *h, long ld_h, const float *y, long ld_y, const float *w, float eps, int rows, int n, void *stream);
int qpal_glu_gelu_tanh(float *act, long ld_act, const float *ug, long ld_ug, int rows, int inter, void *stream);
int qpal_logit_cap(float *logits, long ld, int rows, int vocab, float cap, void *stream);

/* MIXTURE-OF-EXPERTS layers (csrc/moe_route.hip, csrc/moe_gemv.hip; moe.py restates each rule in numpy float64).
 * n <= 128 rows, E <= 256 experts, 1 <= top_k <= min(8, E): P = n * top_k routed pairs (r, j), pair id r * top_k + j.  Every entry
 * point is ONE launch on `stream`, reads nothing on the host, uses no memory beyond its arguments and never synchronises
 * (capturable).  Codes are decided before any stream work.
 *
 * qpal_moe_max_groups: the largest number of groups (below) any routing of the shape can give, exactly; 0 for a shape outside the
 *   limits.  It sizes the group table and the grid of qpal_moe_gemv.  qpal_moe_route_ws_bytes: bytes of one buffer that holds the
 *   ticket (first, 16 bytes) and every output of qpal_moe_route, as moe.moe_workspace lays them out.
 * qpal_moe_route: per row  x = h * rsqrt(mean(h^2) + eps) * rms_w  (fp32; rms_w fp16 [H] or NULL),  logits = router_w x + bias
 *   (router_w fp16 [E][H], 16-byte aligned; fp32 accumulation in ONE order for every expert: equal router rows give equal logits;
 *   bias fp32 [E] or NULL),  p = softmax over all E.  The top_k largest logits are chosen, ties to the lower expert id;
 *   sel [n][top_k] lists them in ascending expert id; gate [n][top_k] = p[sel], divided by their sum when renorm.  Rows with
 *   active[r] < 0 (int64 [n]; NULL: all active) choose nothing: sel -1, gate 0.  The layout: the pairs with sel >= 0 sorted by
 *   (expert, pair id) — order [P] the pair at each sorted position, inv [P] the position of each pair or -1, x_index [P] =
 *   order / top_k, the source row (order and x_index: -1 behind the routed pairs) — and every expert's run cut into GROUPS of at
 *   most 8 consecutive positions: group_expert, group_first, group_count [max_groups] in sorted order (-1, 0, 0 behind the last),
 *   ngroups [1].  H a multiple of 8 up to 8192, ld_h >= H, max_groups >= qpal_moe_max_groups.  ticket: one zeroed 32-bit word
 *   of device memory the launch leaves zero again (the last workgroup to arrive builds the layout).
 * qpal_moe_gemv: for every group g < min(*ngroups, max_groups) with 0 <= group_expert[g] < E (others do no work), projection j < nproj
 *   (1 or 2, one k) and row < proj[j].m:
 *     out[group_first[g] + b][proj[j].out_col + row] = (W x[xi(g, b)])[row] * wscale[row] * oscale,   b < group_count[g] <= 8
 *   with W the TCQ matrix of expert e = group_expert[g] — its stream(s) at ((const void *const *)proj[j].c1)[e] (and .c2 for a
 *   column-split matrix: kv2 = kv + 1, columns [k / 2, k)), its fp16 Wscale [m] at .wscale[e] (table NULL: none) — and
 *   xi(g, b) = x_index[group_first[g] + b], or the position itself when x_index is NULL; an index outside [0, x_rows) reads zeros.
 *   x fp16 [x_rows][ldx], 8-byte aligned, ldx % 4 == 0; out fp32 [out_rows][ldo]; a group that reaches past out_rows does no work;
 *   rows of `out` no group names are not written.  The tables are uint64 [E] in device memory.  S = 9 with kv (kv2) in 2 .. 8,
 *   one codebook tlut [512][2] fp16 for the launch; any other codec: QPAL_E_PARAM.  m % 32, k % 32 (k % 64 when split), as
 *   qpal_tcq_gemv.  fp32 accumulation whose order depends on the shapes alone: a row's result is bitwise independent of the rows
 *   that share its group.
 * qpal_moe_combine:  out[r][c] (+)= sum_j gate[r][j] * y[inv[r][j]][c],  j ascending, every product rounded to fp32, the sum built
 *   in j order and then added (accumulate = 1) or stored (0: rows without pairs become zeros).  y fp32 [P][ld_y].                */
typedef struct qpal_moe_proj {
    const void *c1;      /* device table uint64 [E]: stream 1 of every expert                 */
    const void *c2;      /* ... stream 2 (column-split matrices), or NULL                     */
    const void *wscale;  /* ... fp16 [m] output-row scales, or NULL                           */
    int m;               /* output rows of the projection                                     */
    int kv, kv2;         /* trellis dwords per lane of stream 1 / stream 2 (0: single stream) */
    int out_col;         /* first column of this projection inside a row of `out`             */
} qpal_moe_proj;
int qpal_moe_max_groups(int n, int E, int top_k);
long qpal_moe_route_ws_bytes(int n, int E, int top_k);
int qpal_moe_route(const float *h_f32, long ld_h, const void *rms_w_f16, float rms_eps, const void *router_w_f16,
                   const float *router_bias, const long long *active, int n, int H, int E, int top_k, int renorm, int *sel,
                   float *gate, int *order, int *inv, int *x_index, int *group_expert, int *group_first, int *group_count,
                   int *ngroups, int max_groups, unsigned *ticket, void *stream);
int qpal_moe_gemv(float *out, long ldo, int out_rows, const qpal_moe_proj *proj, int nproj, const void *x_f16, long ldx, int x_rows,
                  const int *x_index, const int *group_expert, const int *group_first, const int *group_count, const int *ngroups,
                  int max_groups, int E, int k, const void *tlut, int S, float oscale, void *stream);
int qpal_moe_combine(float *out_f32, long ld_out, const float *y_f32, long ld_y, const float *gate, const int *inv, int n, int top_k,
                     int H, int P, int accumulate, void *stream);

/* THE SECOND ROUTER AND SHARED EXPERTS (csrc/moe_route.hip; moe.reference_route_ex restates each step in float64).
 * qpal_moe_route_ex is qpal_moe_route's argument list (renorm moves into the struct) plus a qpal_moe_router.  Per row:
 *   1. x̂ and logits are exactly as in qpal_moe_route.  The existing router_bias still adds to the logits.
 *   2. score = softmax(logits) over all E (QPAL_MOE_SOFTMAX), or 1 / (1 + exp(-logits)) (QPAL_MOE_SIGMOID).
 *   3. key = score + select_bias (fp32 [E] or NULL).  The bias decides who is chosen and never enters a gate.  (An expert whose
 *      logit is -inf — the kernel's image of a NaN logit too — has key -inf whatever its bias: chosen only when nothing else is left.)
 *   4. With n_group > 1: experts g S .. g S + S - 1, S = E / n_group, form group g.  Its score is the largest key in it
 *      (QPAL_MOE_GROUP_MAX) or the sum of its two largest (QPAL_MOE_GROUP_TOP2).  The topk_group groups with the largest score
 *      are allowed, ties to the lower group id.  An expert outside them is never chosen.  (The Hugging Face code fills masked
 *      keys with 0.0, which differs only when an allowed key is negative.)
 *   5. The chosen set is the top_k largest keys among the allowed experts, ties to the lower expert id.  sel lists it in
 *      ascending expert id.
 *   6. gate = score[sel], not key.  It is divided by its sum over the chosen in ascending-id order when renorm, then multiplied
 *      by routed_scale.
 *   7. shared_gate_out[r] = sigmoid(x̂[r] . shared_gate) (fp16 [H], 16-byte aligned), or exactly 1.0 without shared_gate.  The
 *      dot product runs through the logits' own chain and tree.  shared_gate_out NULL (allowed without shared_gate): not written.
 *   8. Rows with active[r] < 0 get sel -1, gate 0 and shared_gate_out 0.
 *   The layout arrays, the ticket and every limit are qpal_moe_route's.  Equal router rows (and equal biases) give bitwise equal
 *   keys.  QPAL_E_SHAPE unless E % n_group == 0, 1 <= topk_group <= n_group, topk_group * S >= top_k and (TOP2) S >= 2;
 *   QPAL_E_PARAM for an unknown scoring / group_score or a routed_scale that is not finite and > 0; QPAL_E_NULL for a NULL
 *   router, or a shared_gate without shared_gate_out.
 * qpal_moe_combine_shared is qpal_moe_combine plus the shared expert's rows ys fp32 [n][ld_ys] and their gates sgate fp32 [n]:
 *   the routed sum is built as qpal_moe_combine builds it; then t = fp32(sgate[r] * ys[r][c]), one rounding; the row's term is
 *   acc + t, or t alone where the row has no routed pair; the term is added to out or stored.  A row with sgate[r] == 0 exactly
 *   gets no shared term at all, not even 0 * ys: what ys holds for an inactive row never reaches the stream.                    */
#define QPAL_MOE_SOFTMAX 0
#define QPAL_MOE_SIGMOID 1
#define QPAL_MOE_GROUP_MAX 0
#define QPAL_MOE_GROUP_TOP2 1
typedef struct qpal_moe_router {
    int scoring;                 /* QPAL_MOE_SOFTMAX / QPAL_MOE_SIGMOID                             */
    int n_group, topk_group;     /* 1, 1: no group limit                                            */
    int group_score;             /* QPAL_MOE_GROUP_MAX / QPAL_MOE_GROUP_TOP2                        */
    int renorm;                  /* gates divided by their sum over the chosen                      */
    float routed_scale;          /* finite, > 0                                                     */
    const float *select_bias;    /* fp32 [E] added to the scores for the selection only, or NULL    */
    const void *shared_gate_f16; /* fp16 [H] weight of the shared expert's per-row gate, or NULL    */
    float *shared_gate_out;      /* fp32 [n], or NULL (nothing written)                             */
} qpal_moe_router;
int qpal_moe_route_ex(const float *h_f32, long ld_h, const void *rms_w_f16, float rms_eps, const void *router_w_f16,
                      const float *router_bias, const long long *active, int n, int H, int E, int top_k, int *sel, float *gate,
                      int *order, int *inv, int *x_index, int *group_expert, int *group_first, int *group_count, int *ngroups,
                      int max_groups, unsigned *ticket, const qpal_moe_router *router, void *stream);
int qpal_moe_combine_shared(float *out_f32, long ld_out, const float *y_f32, long ld_y, const float *gate, const int *inv,
                            const float *ys_f32, long ld_ys, const float *sgate, int n, int top_k, int H, int P, int accumulate,
                            void *stream);

/* The launch planner of the fused GEMV entry points, on its own (host code, no GPU call; what tests and tools inspect).
 * A launch of njobs jobs — rows[j] supertile rows (m / 32) of steps1[j] + steps2[j] steps (a step = 128 columns; steps2 = 0: one
 * stream) — is cut into workgroup-sized pieces: a GROUP of G = 1 << lg_g workgroups (`waves` = 16 or 8 waves each) owns rg
 * consecutive rows; its work, laid out as a tape (row 0 stream 1, row 0 stream 2, row 1 ...), is cut into G equal ranges and every
 * range into one piece per wave.  flags[j]: bit 0 the output is zeroed, bit 1 the job accumulates, bit 2 SwiGLU epilogue;
 * shared_staging: the jobs read one x / codebook (groups may then run across job boundaries).  out (ints):
 *   [0] grid  [1] items  [2] geometry classes  [3] items of class 0  [4] groups span jobs  [5] class-1 job mask  [6] M  [7] W
 *   then per class c < 2: lg_g, rg, M * W entries (a, b) — a: bits 0..7 row inside the group, 8 stream 2, 9 lead of its row's run,
 *   10 row shared with another workgroup, 11..15 waves in the run, 16 has steps, 17 SwiGLU lead; b: first step | steps << 16 —
 *   then per job: class, first virtual row, end of its virtual rows, 2 if its output must start at zero (shared rows) else 1.
 * out_len >= 8 + 2 * (2 + 2 * M * W) + 4 * njobs (M = 4, W = 16).                                                              */
int qpal_plan_gemv(const int *rows, const int *steps1, const int *steps2, const int *flags, int njobs, int waves, int shared_staging,
                   int *out, int out_len);

/* 1 if the GEMV entry points can apply the rotation themselves (x_had): k in {2048, 4096} at batch 1 (the
 * decode case); 0 otherwise (then call qpal_hadamard first). */
int qpal_can_fuse_rotation(int n, int k);
/* the same for x_K > 1 (K = 28, k = 14336, batch 1; codecs whose codebook image is >= 40 KiB: every TCQ codec) */
int qpal_can_fuse_rotation_k(int n, int k, int K);

/* Calibration of the measurement contract (bench.py `roofline` block; SURVEY.md §8d: "report a measured stream-read ceiling").
 * NOT on the data path — no module calls them; csrc/calib.hip.
 *   qpal_calib_stream_read  one launch (`grid` workgroups of 1024 threads) that does nothing but read srcs[i] (bytes[i] bytes each,
 *                           16-byte aligned, bytes % 16 == 0, nseg <= 16) with 16-byte non-temporal loads; sink: >= 4 KiB of
 *                           device memory (never written in practice).  Over > 1 GB: the stream ceiling; over the packed buffers
 *                           of one GEMV launch: what that launch would take if the decode were free.
 *   qpal_calib_decode_rate  `grid` workgroups of 16 waves run `iters` decode + MFMA steps of the TCQ codec (S, KV) — the step
 *                           function of the fused GEMV kernel itself — on register-resident packed words: no HBM traffic.
 *                           wave-steps executed = grid * 16 * iters (one step = 32 rows x 128 columns of W).            */
int qpal_calib_stream_read(const void *const *srcs, const long *bytes, int nseg, void *sink, int grid, void *stream);
int qpal_calib_decode_rate(const void *tlut, void *sink, int iters, int S, int KV, int grid, void *stream);

const char *qpal_error_string(int code);
int qpal_version(void);

#ifdef __cplusplus
}
#endif
#endif /* QPAL_H */
