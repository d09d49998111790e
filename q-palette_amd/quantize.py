"""Quantisers on the GPU: fp weights -> a QTIPLinearTCQ trellis (reference: lib/codebook/bitshift.py:202-294,
lib/algo/ldlq.py:63-121, lib/quantizer/tcq_quant.py:15-60) or fixed-codebook VQ / SQ codes (reference:
lib/codebook/vq_codebook.py, lib/algo/ldlq.py LDLQ_VQ, lib/quantizer/vq_quant_ldlq.py).

  tcq_viterbi(X, tlut, KV)                  bitshift_codebook(..., "quantlut_sym").quantize(X): the tail-biting Viterbi
                                            search, one HIP kernel (csrc/tcq_viterbi.hip, qpal_tcq_viterbi)
  quantize_tcq_weight(W, tlut, KV, H=None)  qtip_quantize_mat on an already scaled W: 16x16 tiles in the mma element
                                            order, block LDLQ feedback (fp64 torch) when H is given, packed trellis
  make_tcq_linear(W, tlut, KV, H=None)      the QTIPLinearTCQ module of that trellis
  vq_nearest(X, lut)                        vq_codebook.quantize: nearest codeword, one HIP kernel (csrc/vq_encode.hip,
                                            qpal_vq_encode)
  quantize_vq_weight(W, lut, H=None)        vq_quantize_mat_ldlq on an already scaled W: one launch without H; with H block
                                            LDL (b = vec) and one launch per column block (in-block feedback in the kernel,
                                            the feedback between blocks in fp64 torch), packed like the reference
  make_vq_linear(W, lut, H=None)            the VQLinearPackTensorCore (vec 1, 2) / VQLinearPackSIMT (vec 4, simt=True) module

Scaling (Wscale), the incoherence rotation, group Hessians and Hessian collection stay with the caller, as upstream.
"""
import torch

from . import _native, packers
from .linear import QTIPLinearTCQ, VQLinearPackSIMT, VQLinearPackTensorCore

T = 256           # values per sequence (one 16x16 tile)
STEPS = T // 2    # trellis states per sequence (V = 2)
MAX_LAUNCH = 65536  # sequences per kernel launch (the workspace is fixed by the kernel's grid, not by B)

# mma element order of a 16x16 tile (ldlq.py:10-13; oracle/qpal_oracle.c restates it too)
PERMUTE = torch.arange(256).reshape(2, 8, 2, 4, 2).permute(1, 3, 2, 0, 4).flatten()
INV_PERMUTE = torch.empty_like(PERMUTE)
INV_PERMUTE[PERMUTE] = torch.arange(256)


def _bits(tlut):
    S = int(tlut.shape[0]).bit_length() - 1
    if tlut.dim() != 2 or tlut.shape[1] != 2 or tlut.shape[0] != 1 << S:
        raise _native.QpalError("tlut must be a [2^S, 2] codebook")
    return S


def tcq_viterbi(X, tlut, KV, ws=None):
    """X: [B, 256] float CUDA tensor; tlut: fp16 [2^S, 2] codebook -> (hat fp32 [B, 256], states int32 [B, 128]).
    ws: optional workspace of qpal_tcq_viterbi_ws_bytes(KV) bytes on X's device (allocated per call when None).

    X is rounded to fp16 first (through fp32, as torch's CPU conversion does from fp64) like the reference's quantize().
    Ties: lowest predecessor, then lowest final state (CPU torch.min / argmin)."""
    if X.dim() != 2 or X.shape[1] != T or not X.is_cuda:
        raise _native.QpalError("X must be a [B, 256] CUDA tensor")
    S = _bits(tlut)
    dev = X.device
    x16 = X.to(torch.float32).to(torch.float16).contiguous()
    tl = tlut.to(device=dev, dtype=torch.float16).contiguous()
    B = x16.shape[0]
    states = torch.empty(B, STEPS, dtype=torch.int32, device=dev)
    hat = torch.empty(B, T, dtype=torch.float16, device=dev)
    if B == 0:
        return hat.float(), states
    lib = _native.lib()
    if ws is None:
        ws = torch.empty(lib.qpal_tcq_viterbi_ws_bytes(KV), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for b0 in range(0, B, MAX_LAUNCH):
        n = min(MAX_LAUNCH, B - b0)
        _native.check(lib.qpal_tcq_viterbi(states[b0].data_ptr(), hat[b0].data_ptr(), x16[b0].data_ptr(), tl.data_ptr(), n, S,
                                           KV, ws.data_ptr(), stream), "qpal_tcq_viterbi")
    return hat.float(), states


def _quantize_rows(Wb, tlut, KV, ws=None):
    """Wb: [m, 16] column block -> (hat [m, 16] fp64, Qidxs block [m, 8]): ldlq.py:96-110 (for_kernel=True)."""
    m = Wb.shape[0]
    X = Wb.reshape(m // 16, 256)[:, PERMUTE.to(Wb.device)]
    hat, st = tcq_viterbi(X, tlut, KV, ws)
    hat = hat[:, INV_PERMUTE.to(Wb.device)].reshape(m, 16).to(Wb.dtype)
    return hat, st.reshape(m, 8)


def block_ldl(H, b=16):
    """Unit block-lower-triangular L of H = L D L^T (D block diagonal, b x b blocks): the Cholesky factor with every
    column block multiplied by the inverse of its diagonal block (the reference's block_LDL, lib/utils/math_utils.py)."""
    n = H.shape[0]
    nb = n // b
    C = torch.linalg.cholesky(H)
    Dc = torch.diagonal(C.reshape(nb, b, nb, b), dim1=0, dim2=2).permute(2, 0, 1)  # [j] = C[jb:(j+1)b, jb:(j+1)b]
    return torch.einsum("rjb,jbc->rjc", C.reshape(n, nb, b), torch.linalg.inv(Dc)).reshape(n, n)


def _ldlq(W, L, tlut, KV, buf_cols, kv_at=None):
    """Column-block LDLQ with error feedback (ldlq.py:63-121) in fp64; W: [m, n] fp64, L: unit block-lower, zero diagonal.
    kv_at(r0): the KV of the column block starting at r0 (LDLQ_combt, ldlq.py:124-193), KV for every block when None.
    One Viterbi workspace per KV for the whole loop."""
    m, n = W.shape
    nb = buf_cols // 16
    ws = {}
    WT = W.T.contiguous()
    hatT = torch.zeros(n, m, dtype=W.dtype, device=W.device)
    QT = torch.zeros(n // 2, m, dtype=torch.int32, device=W.device)
    prod = torch.zeros(n, m, dtype=W.dtype, device=W.device)
    for cur in range(n // 16, 0, -nb):
        r0, r1 = 16 * (cur - nb), 16 * cur
        bW, bhat, bL, bprod = WT[r0:r1], hatT[r0:r1], L[r0:r1], prod[r0:r1]
        kv = KV if kv_at is None else kv_at(r0)
        if kv not in ws:
            ws[kv] = torch.empty(_native.lib().qpal_tcq_viterbi_ws_bytes(kv), dtype=torch.uint8, device=W.device)
        for i in reversed(range(nb)):
            fb = bL[16 * (i + 1):, r0 + 16 * i:r0 + 16 * (i + 1)].T @ (bW[16 * (i + 1):] - bhat[16 * (i + 1):])
            target = bW[16 * i:16 * (i + 1)] + fb + bprod[16 * i:16 * (i + 1)]
            hat, q = _quantize_rows(target.T, tlut, kv, ws[kv])
            bhat[16 * i:16 * (i + 1)] = hat.T
            QT[(r0 + 16 * i) // 2:(r0 + 16 * (i + 1)) // 2] = q.T
        prod += bL.T @ (bW - bhat)
    return hatT.T.contiguous(), QT.T.contiguous()


def quantize_tcq_weight(W, tlut, KV, H=None, buf_cols=128):
    """W: [m, k] (already scaled) -> (trellis int16 [(m/16)(k/16), 8 KV] (CPU), hatW fp32 [m, k], info).

    H None: every 16x16 tile on its own (the reference's use_hess=False), one launch for the whole matrix.
    H: fp64 [k, k] SPD proxy Hessian: block LDL + LDLQ feedback over column blocks of buf_cols columns.
    info: err = mean((W - hatW)^2) / mean(W^2), orig_err = mean((W - hatW)^2), and with H proxy_err = tr(dW H dW^T) / tr(W H W^T)."""
    if W.dim() != 2 or not W.is_cuda:
        raise _native.QpalError("W must be a 2-D CUDA tensor")
    m, k = W.shape
    if m % 16 or k % 16:
        raise _native.QpalError("W needs m % 16 == 0 and k % 16 == 0 (16x16 trellis tiles)")
    W64 = W.to(torch.float64)
    ntr, ntc = m // 16, k // 16
    if H is None:
        tiles = W64.reshape(ntr, 16, ntc, 16).permute(0, 2, 1, 3).reshape(ntr * ntc, 256)
        hat, st = tcq_viterbi(tiles[:, PERMUTE.to(W.device)], tlut, KV)
        hatW = hat[:, INV_PERMUTE.to(W.device)].reshape(ntr, ntc, 16, 16).permute(0, 2, 1, 3).reshape(m, k).to(torch.float64)
        Qidxs = st.reshape(ntr, ntc, 16, 8).permute(0, 2, 1, 3).reshape(m, k // 2)
    else:
        if tuple(H.shape) != (k, k):
            raise _native.QpalError(f"H must be [{k}, {k}]")
        if k % buf_cols or buf_cols % 16:
            raise _native.QpalError("buf_cols must be a multiple of 16 that divides k")
        H64 = H.to(device=W.device, dtype=torch.float64)
        L = block_ldl(H64, 16)
        L.fill_diagonal_(0)
        hatW, Qidxs = _ldlq(W64, L, tlut, KV, buf_cols)
    trellis = packers.pack_trellis(Qidxs.cpu(), m, k, KV)
    dW = W64 - hatW
    orig_err = dW.pow(2).mean()
    info = {"err": (orig_err / W64.pow(2).mean()).item(), "orig_err": orig_err.item(), "Qidxs": Qidxs}
    if H is not None:
        info["proxy_err"] = (torch.trace(dW @ H64 @ dW.T) / torch.trace(W64 @ H64 @ W64.T)).item()
    return trellis, hatW.to(torch.float32), info


def make_tcq_linear(W, tlut, KV, H=None, bias=None):
    """QTIPLinearTCQ (16x16 tiles, L = 16, V = 2, S = log2 of tlut's rows) whose weight is the TCQ quantisation of W."""
    m, k = W.shape
    S = _bits(tlut)
    trellis, _, _ = quantize_tcq_weight(W, tlut, KV, H)
    layer = QTIPLinearTCQ(k, m, 16, 16, 16, KV, 2, S, bias=bias is not None)
    layer.trellis.data.copy_(trellis)
    layer.tlut.data.copy_(tlut.detach().to("cpu", torch.float16))
    if bias is not None:
        layer.bias.data.copy_(bias.detach().cpu())
    return layer.to(W.device)


# ---------------------------------------------------------------------------------------------------- VQ / SQ (ldlq_<vec>_<bits>)

VQ_MAX_BLOCK = 128  # columns per LDLQ block the kernel takes (qpal_vq_encode)
# (vec, bits) the packers hold: tensor-core order (pack_qweight), SIMT order (pack_qweight_{sq,vq}_simt)
TC_BITS = {1: range(2, 9), 2: range(2, 13)}
SIMT_BITS = {1: range(2, 9), 2: range(3, 13), 4: range(6, 13)}


def _lut_geom(lut):
    if lut.dim() != 2 or lut.shape[1] not in (1, 2, 4):
        raise _native.QpalError("lut must be a [2^bits, vec] codebook with vec in {1, 2, 4}")
    bits = int(lut.shape[0]).bit_length() - 1
    if lut.shape[0] != 1 << bits or not 1 <= bits <= 12:
        raise _native.QpalError("lut must have 2^bits rows, bits in 1..12")
    return int(lut.shape[1]), bits


def _vq_encode(idx, hat, w, lut32, m, cols, bits, vec, ld, prod=None, lt=None, ld_l=0):
    """One qpal_vq_encode launch on pointers into row-major fp64 matrices of row stride ld (see include/qpal.h)."""
    stream = torch.cuda.current_stream(w.device).cuda_stream
    ptr = (lambda t: t.data_ptr() if t is not None else None)
    _native.check(_native.lib().qpal_vq_encode(idx.data_ptr(), ptr(hat), w.data_ptr(), ptr(prod), ptr(lt), ld, ld_l,
                                               lut32.data_ptr(), m, cols, bits, vec, stream), "qpal_vq_encode")


def vq_nearest(X, lut):
    """X: [B, vec] float CUDA tensor; lut: [2^bits, vec] codebook -> (hat fp64 [B, vec], idx int32 [B]).

    vq_codebook.quantize: the codeword nearest to every row in fp64 (the codebook rounded to fp32, as the reference's cached
    codebooks are), direct-form squared distance; ties go to the lowest index (CPU torch.argmin)."""
    vec, bits = _lut_geom(lut)
    if X.dim() != 2 or X.shape[1] != vec or not X.is_cuda:
        raise _native.QpalError(f"X must be a [B, {vec}] CUDA tensor")
    dev = X.device
    x = X.to(torch.float64).contiguous()
    B = x.shape[0]
    hat = torch.empty(B, vec, dtype=torch.float64, device=dev)
    idx = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return hat, idx
    lut32 = lut.to(device=dev, dtype=torch.float32).contiguous()
    _vq_encode(idx, hat, x, lut32, B, vec, bits, vec, vec)
    return hat, idx


def _ldlq_vq(W, LT, lut32, bits, vec, buf_cols):
    """LDLQ_VQ (ldlq.py:16-58) in fp64: W [m, n]; LT = L^T of the unit block-lower L with zero diagonal.  The kernel runs a whole
    column block (the in-block feedback); prod, the feedback of the blocks to the right, is an fp64 torch matmul per block."""
    m, n = W.shape
    hat = torch.empty(m, n, dtype=torch.float64, device=W.device)
    Q = torch.empty(m, n // vec, dtype=torch.int32, device=W.device)
    prod = torch.zeros(m, n, dtype=torch.float64, device=W.device)
    for r1 in range(n, 0, -buf_cols):
        r0 = r1 - buf_cols
        off = r0 * n + r0  # element (r0, r0) of LT: column r0 of the L block, column-major
        _vq_encode(Q[:, r0 // vec:], hat[:, r0:], W[:, r0:], lut32, m, buf_cols, bits, vec, n,
                   prod=prod[:, r0:], lt=LT.view(-1)[off:], ld_l=n)
        if r0:
            prod[:, :r0] += (W[:, r0:r1] - hat[:, r0:r1]) @ LT[:r0, r0:r1].T
    return hat, Q


def quantize_vq_weight(W, lut, H=None, buf_cols=128, simt=False):
    """W: [m, k] (already scaled) -> (qweight int32 (CPU), hatW fp32 [m, k], info).

    H None: every vec-group on its own (the reference's use_hess=False: its L is all zeros), one launch for the whole matrix.
    H: fp64 [k, k] SPD proxy Hessian: block LDL (b = vec) + LDLQ feedback over column blocks of buf_cols columns.
    Packing as vq_quantize_mat_ldlq: tensor-core order (pack_qweight), SIMT order when simt or vec == 4.
    info: err = mean((W - hatW)^2) / mean(W^2), orig_err = mean((W - hatW)^2), Qidxs, and with H
    proxy_err = tr(dW H dW^T) / tr(W H W^T)."""
    vec, bits = _lut_geom(lut)
    if W.dim() != 2 or not W.is_cuda:
        raise _native.QpalError("W must be a 2-D CUDA tensor")
    m, k = W.shape
    if m < 1 or k < vec or k % vec:
        raise _native.QpalError(f"W needs k % {vec} == 0")
    W64 = W.to(torch.float64).contiguous()
    lut32 = lut.to(device=W.device, dtype=torch.float32).contiguous()
    if H is None:
        hatW = torch.empty(m, k, dtype=torch.float64, device=W.device)
        Qidxs = torch.empty(m, k // vec, dtype=torch.int32, device=W.device)
        _vq_encode(Qidxs, hatW, W64, lut32, m, k, bits, vec, k)
    else:
        if tuple(H.shape) != (k, k):
            raise _native.QpalError(f"H must be [{k}, {k}]")
        if not 0 < buf_cols <= VQ_MAX_BLOCK or buf_cols % vec or k % buf_cols:
            raise _native.QpalError(f"buf_cols must be a multiple of {vec}, at most {VQ_MAX_BLOCK}, that divides k")
        H64 = H.to(device=W.device, dtype=torch.float64)
        L = block_ldl(H64, vec)
        L.fill_diagonal_(0)
        hatW, Qidxs = _ldlq_vq(W64, L.T.contiguous(), lut32, bits, vec, buf_cols)
    q = Qidxs.cpu()
    if simt or vec == 4:
        qweight = packers.pack_qweight_sq_simt(q, bits) if vec == 1 else packers.pack_qweight_vq_simt(q, bits, vec)
    else:
        qweight = packers.pack_qweight(q, vec, bits)
    dW = W64 - hatW
    orig_err = dW.pow(2).mean()
    info = {"err": (orig_err / W64.pow(2).mean()).item(), "orig_err": orig_err.item(), "Qidxs": Qidxs}
    if H is not None:
        info["proxy_err"] = (torch.trace(dW @ H64 @ dW.T) / torch.trace(W64 @ H64 @ W64.T)).item()
    return qweight, hatW.to(torch.float32), info


def make_vq_linear(W, lut, H=None, bias=None, simt=None):
    """VQLinearPackTensorCore (vec 1, 2) or VQLinearPackSIMT (vec 4, or simt=True) whose codes are the LDLQ quantisation of W;
    the module's codebook is lut.half(), as the reference's copy_ into the fp16 buffer."""
    vec, bits = _lut_geom(lut)
    simt = bool(simt) or vec == 4
    ok = SIMT_BITS if simt else TC_BITS
    if bits not in ok.get(vec, ()):
        raise _native.QpalError(f"no {'SIMT' if simt else 'tensor-core'} packing for vec {vec}, {bits} bits")
    m, k = W.shape
    qweight, _, _ = quantize_vq_weight(W, lut, H, simt=simt)
    cls = VQLinearPackSIMT if simt else VQLinearPackTensorCore
    layer = cls(k, m, bits, vec, bias=bias is not None, device="cpu")
    layer.qweight.data.copy_(qweight)
    layer.lut.data.copy_(lut.detach().to("cpu", torch.float16))
    if bias is not None:
        layer.bias.data.copy_(bias.detach().cpu())
    return layer.to(W.device)
