"""Whole-layer quantisation on the GPU: an nn.Linear (fp weights, optional proxy Hessian) -> the IncoherentLinear and the layer
file that IncoherentLinear / IncoherentMLP / IncoherentSdpaAttention.gen_layer_from_quantizer_str_and_key load.

  incoherent_preprocess(W, H, SU, SV, ...)   linear_to_incoherent_for_tcq / _for_vq (reference lib/quantizer/tcq_quant.py:105-131,
                                             vq_quant.py:97-125): Wr = Had_U^T (W * SU) / Wscale and HRr = Had^T S H S Had,
                                             rotated in fp32 on qpal_hadamard_f32 (hadamard.rotate_f32)
  quantize_combt_weight(W, tlut, KV, in_part, H)  combt_quantize_mat / LDLQ_combt (lib/quantizer/comb_quant.py, lib/algo/ldlq.py)
  quantize_comb_weight(W, tlut, KV, out_part, H)  inc_linear_to_inc_comb_linear: two TCQ quantisations of the row halves
  make_combt_linear / make_comb_linear       the CombtLinearTCQ / CombLinearTCQ modules of those
  load_hessian(path)                         lib/quantizer/quant_op.py:164-174 (the reference's Hessian file format)
  quantize_linear(linear, quantizer_str, ...)  the front end of the reference's quantize_layer.quantize_linear for
                                             tcq_*, tcomb_*, comb_* and ldlq_* strings
  layer_file_path(quant_dir, qstr, idx, key) where the loaders look for a layer file

Codebooks come from the caller (the library ships none).  sq_* / vq2_* need k-means fitting and are refused.
"""
import os
import time

import torch

from . import _native, packers
from . import hadamard as had
from .linear import CombLinearTCQ, CombtLinearTCQ, IncoherentLinear, QTIPLinearTCQ, VQLinearPackTensorCore
from .quantize import _bits, _ldlq, _lut_geom, block_ldl, quantize_tcq_weight, quantize_vq_weight

QpalError = _native.QpalError


# ------------------------------------------------------------------------------------------------ incoherence preprocessing


def quantlut_sym(tlut, L=16):
    """The codebook of every trellis state, [2^L, 2] (lib/codebook/bitshift.py:71-79), in tlut's dtype."""
    S = _bits(tlut)
    s = torch.arange(1 << L, device=tlut.device)
    h = (s + 1) * s
    sflp = 1 - ((h >> 15) & 1) * 2
    lut = tlut[(h >> (16 - S - 1)) & ((1 << S) - 1)].clone()
    lut[:, 0] = lut[:, 0] * sflp
    return lut


def tcq_lut_rms(tlut):
    """rms over all 2^16 decoded states, as an fp32 value: the `cb.lut` normaliser of linear_to_incoherent_for_tcq."""
    return float(quantlut_sym(tlut.detach().float().cpu()).to(torch.float64).square().mean().sqrt().float())


def random_signs(n, generator=None, device="cpu"):
    """(randn > 0) * 2 - 1 in fp32, the reference's SU / SV."""
    return ((torch.randn(n, generator=generator) > 0.0) * 2.0 - 1.0).to(device=device, dtype=torch.float32)


def _rot(x, hd, su=None, out=None):
    """matmul_hadUt_head(x * su, hd) in fp32 (the Ut direction: hadK transposed)."""
    hadK, K = had.get_hadK(hd, transpose=True)
    return had.rotate_f32(x, hd=hd, hadK=hadK, K=K, su=su, out=out)


def _transpose_square_(A, block=2048):
    """In-place transpose of a square matrix, block by block (no second full-size copy)."""
    n = A.shape[0]
    for i in range(0, n, block):
        i1 = min(i + block, n)
        A[i:i1, i:i1] = A[i:i1, i:i1].T.clone()
        for j in range(i1, n, block):
            j1 = min(j + block, n)
            t = A[i:i1, j:j1].clone()
            A[i:i1, j:j1] = A[j:j1, i:i1].T
            A[j:j1, i:i1] = t.T
    return A


def rotate_hessian(H, SU, chunk=2048):
    """HRr = matmul_hadUt_head(matmul_hadUt_head(H * (1 / SU), n).T * (1 / SU), n) (tcq_quant.py:123-125): fp64 H, each rotation
    in fp32 as the reference's (`.float()` inside matmul_hadU_head_cuda), back to fp64.  One fp32 copy of H on the GPU: the first
    product is formed in fp64 and rounded chunk by chunk, both rotations run in place, the transpose is done block by block."""
    k = H.shape[0]
    dev = SU.device
    inv = 1.0 / SU.to(torch.float32)
    inv64 = inv.to(torch.float64)
    A = torch.empty(k, k, dtype=torch.float32, device=dev)
    for r0 in range(0, k, chunk):
        A[r0:r0 + chunk] = (H[r0:r0 + chunk].to(device=dev, dtype=torch.float64) * inv64).float()
    _rot(A, k, out=A)
    _transpose_square_(A)
    # (fp32 value * fp32 1/SU rounded once: what the reference's fp64 product followed by .float() gives)
    _rot(A, k, su=inv.contiguous(), out=A)
    return A.to(torch.float64)


def incoherent_preprocess(W, H=None, SU=None, SV=None, scale_override=0.9, left_only=True, lut_rms=None):
    """(Wr fp32 [m, k], Wscale fp32 [m], HRr fp64 [k, k] or None, SU fp32 [k], SV fp32 [m]) of an fp weight W [m, k] on the GPU.

    lut_rms given (tcq_lut_rms of the trellis codebook): linear_to_incoherent_for_tcq — Wscale = rms / (lut_rms * scale_override),
    per row when left_only, ONE global rms repeated over the rows when both sides are rotated.
    lut_rms None: linear_to_incoherent_for_vq — Wscale = per-row rms / scale_override, always.
    Wr = Had_U^T (W * SU) / Wscale (left_only), or Had_U^T ((Had_V^T (W^T * SV))^T * SU) / Wscale; SU / SV default to random
    signs, SV is all ones when left_only.  HRr: rotate_hessian(H, SU)."""
    if W.dim() != 2 or not W.is_cuda:
        raise QpalError("W must be a 2-D CUDA tensor")
    m, k = W.shape
    dev = W.device
    SU = random_signs(k, device=dev) if SU is None else SU.to(device=dev, dtype=torch.float32).contiguous()
    SV = random_signs(m, device=dev) if SV is None else SV.to(device=dev, dtype=torch.float32).contiguous()
    if left_only:
        SV = torch.ones_like(SV)
    if SU.numel() != k or SV.numel() != m:
        raise QpalError(f"SU must have {k} and SV {m} elements")
    W32 = W.detach().to(torch.float32).contiguous()
    if left_only:
        Wr = _rot(W32, k, su=SU)
    else:
        Wr = _rot(_rot(W32.T.contiguous(), m, su=SV).T.contiguous(), k, su=SU)
    Wr64 = Wr.to(torch.float64)
    if lut_rms is None:
        Wscale = Wr64.square().mean(-1).sqrt().view(-1, 1).to(torch.float32) / scale_override
    else:
        den = torch.tensor(lut_rms, dtype=torch.float32, device=dev) * scale_override
        if left_only:
            Wscale = Wr64.square().mean(-1).sqrt().view(-1, 1).to(torch.float32) / den
        else:
            Wscale = (Wr64.square().mean().sqrt().view(-1, 1).to(torch.float32) / den).repeat(m, 1)
    del Wr64
    Wr = Wr / Wscale
    HRr = None
    if H is not None:
        if tuple(H.shape) != (k, k):
            raise QpalError(f"H must be [{k}, {k}]")
        HRr = rotate_hessian(H, SU)
    return Wr, Wscale.view(-1), HRr, SU, SV


# ------------------------------------------------------------------------------------------------------- comb / combt


def quantize_combt_weight(W, tlut, KV, in_part, H=None, buf_cols=128):
    """W: [m, k] (already scaled) -> (trellis1, trellis2 int16 (CPU), hatW fp32 [m, k], info): LDLQ_combt.

    Columns [0, in_part[0]) take KV[0], the rest KV[1]; in_part[0] must be a multiple of buf_cols so that every column block
    lies on one side (the reference switches at k // 2 by block start and packs at k // 2: identical for ratio 0.5).
    H None: every tile on its own (use_hess=False).  info as quantize_tcq_weight's (err, orig_err, Qidxs [, proxy_err])."""
    if W.dim() != 2 or not W.is_cuda:
        raise QpalError("W must be a 2-D CUDA tensor")
    m, k = W.shape
    kv1, kv2 = (int(v) for v in KV)
    p0, p1 = (int(v) for v in in_part)
    if p0 + p1 != k or p0 <= 0 or p1 <= 0:
        raise QpalError(f"in_part {tuple(in_part)} does not split {k} columns")
    if m % 16 or k % buf_cols or buf_cols % 16 or p0 % buf_cols:
        raise QpalError(f"combt needs m % 16 == 0, k and in_part[0] multiples of buf_cols ({buf_cols}, a multiple of 16)")
    W64 = W.to(torch.float64)
    if H is None:
        t1, h1, i1 = quantize_tcq_weight(W64[:, :p0].contiguous(), tlut, kv1)
        t2, h2, i2 = quantize_tcq_weight(W64[:, p0:].contiguous(), tlut, kv2)
        hatW = torch.cat([h1, h2], 1).to(torch.float64)
        Qidxs = torch.cat([i1["Qidxs"], i2["Qidxs"]], 1)
    else:
        if tuple(H.shape) != (k, k):
            raise QpalError(f"H must be [{k}, {k}]")
        H64 = H.to(device=W.device, dtype=torch.float64)
        L = block_ldl(H64, 16)
        L.fill_diagonal_(0)
        hatW, Qidxs = _ldlq(W64, L, tlut, kv1, buf_cols, kv_at=lambda r0: kv1 if r0 < p0 else kv2)
        q = Qidxs.cpu()
        t1 = packers.pack_trellis(q[:, :p0 // 2].contiguous(), m, p0, kv1)
        t2 = packers.pack_trellis(q[:, p0 // 2:].contiguous(), m, p1, kv2)
    dW = W64 - hatW
    orig_err = dW.pow(2).mean()
    info = {"err": (orig_err / W64.pow(2).mean()).item(), "orig_err": orig_err.item(), "Qidxs": Qidxs}
    if H is not None:
        info["proxy_err"] = (torch.trace(dW @ H64 @ dW.T) / torch.trace(W64 @ H64 @ W64.T)).item()
    return t1, t2, hatW.to(torch.float32), info


def quantize_comb_weight(W, tlut, KV, out_part, H=None, buf_cols=128):
    """W: [m, k] (already scaled) -> (trellis1, trellis2, hatW fp32, info): rows [0, out_part[0]) at KV[0], the rest at KV[1],
    two quantize_tcq_weight calls with the same H (inc_linear_to_inc_comb_linear)."""
    if W.dim() != 2 or not W.is_cuda:
        raise QpalError("W must be a 2-D CUDA tensor")
    m, k = W.shape
    o0, o1 = (int(v) for v in out_part)
    if o0 + o1 != m or o0 <= 0 or o1 <= 0 or o0 % 16:
        raise QpalError(f"out_part {tuple(out_part)} does not split {m} rows into multiples of 16")
    t1, h1, i1 = quantize_tcq_weight(W[:o0], tlut, int(KV[0]), H, buf_cols)
    t2, h2, i2 = quantize_tcq_weight(W[o0:], tlut, int(KV[1]), H, buf_cols)
    W64 = W.to(torch.float64)
    hatW = torch.cat([h1, h2], 0)
    dW = W64 - hatW.to(torch.float64)
    orig_err = dW.pow(2).mean()
    info = {"err": (orig_err / W64.pow(2).mean()).item(), "orig_err": orig_err.item(),
            "Qidxs": torch.cat([i1["Qidxs"], i2["Qidxs"]], 0), "quant_info1": i1, "quant_info2": i2}
    return t1, t2, hatW, info


def _comb_module(cls, W, tlut, KV, part, t1, t2, bias):
    m, k = W.shape
    layer = cls(k, m, 16, 16, tuple(int(v) for v in part), 16, tuple(int(v) for v in KV), 2, _bits(tlut), bias=bias is not None)
    layer.trellis1.data.copy_(t1)
    layer.trellis2.data.copy_(t2)
    layer.tlut.data.copy_(tlut.detach().to("cpu", torch.float16))
    if bias is not None:
        layer.bias.data.copy_(bias.detach().cpu())
    return layer.to(W.device)


def make_combt_linear(W, tlut, KV, in_part, H=None, bias=None):
    """CombtLinearTCQ whose two trellises are the LDLQ_combt quantisation of W."""
    t1, t2, _, _ = quantize_combt_weight(W, tlut, KV, in_part, H)
    return _comb_module(CombtLinearTCQ, W, tlut, KV, in_part, t1, t2, bias)


def make_comb_linear(W, tlut, KV, out_part, H=None, bias=None):
    """CombLinearTCQ whose two trellises are the TCQ quantisations of W's row halves."""
    t1, t2, _, _ = quantize_comb_weight(W, tlut, KV, out_part, H)
    return _comb_module(CombLinearTCQ, W, tlut, KV, out_part, t1, t2, bias)


# -------------------------------------------------------------------------------------------------------- front end


def load_hessian(path, sigma_reg=0.01):
    """The reference's Hessian file (quant_op.py:164-174): {"flatH": lower triangle row by row, "n", optional "mu"}.
    H = sym(flatH) [+ mu mu^T], regularised (regularize_H: diagonal += sigma_reg * mean diagonal).  Returns fp64 [n, n] (CPU),
    without the reference's trailing group axis."""
    d = torch.load(path, map_location="cpu")
    n, flat = int(d["n"]), d["flatH"]
    H = torch.zeros(n, n, dtype=flat.dtype)
    idx = torch.tril_indices(n, n)
    H[idx.unbind()] = flat
    H[idx[1, :], idx[0, :]] = flat
    if "mu" in d:
        mu = d["mu"]
        H += mu[None, :] * mu[:, None]
    diagmean = torch.diag(H).mean()
    H /= diagmean
    i = torch.arange(n)
    H[i, i] += sigma_reg
    return (H * diagmean).to(torch.float64)


def _tlut_bits(kv):
    if kv <= 8:
        return 9
    if kv in (9, 10):
        return kv + 1
    raise QpalError(f"KV {kv} has no codebook (KV 2..10)")


def parse_quantizer_str(qstr):
    """{"kind": tcq | tcomb | comb | ldlq, "use_hess", "scale_override", and KV + tlut_bits (+ ratio) or vec_sz + lut_bits}
    of a quantizer string, in the reference's order of prefixes; sq_* / vq2_* (k-means fitting) are refused."""
    parts = qstr.split("_")
    try:
        if qstr.startswith("tcq"):
            _, kv, hess, so = parts
            kv = int(kv)
            out = {"kind": "tcq", "KV": kv, "tlut_bits": _tlut_bits(kv)}
        elif qstr.startswith("comb") or qstr.startswith("tcomb"):
            name, kv1, kv2, ratio, hess, so = parts
            kv = (int(kv1), int(kv2))
            out = {"kind": name, "KV": kv, "tlut_bits": _tlut_bits(max(kv)), "ratio": float(ratio)}
        elif qstr.startswith("ldlq"):
            _, vec, bits, hess, so = parts
            out = {"kind": "ldlq", "vec_sz": int(vec), "lut_bits": int(bits)}
        elif qstr.startswith("sq") or qstr.startswith("vq2"):
            raise QpalError(f"{qstr}: sq_* / vq2_* need k-means codebook fitting, which this library does not implement")
        else:
            raise QpalError(f"quantizer {qstr} not supported")
    except ValueError as e:
        raise QpalError(f"malformed quantizer string {qstr}: {e}") from None
    if hess not in ("hess", "none"):
        raise QpalError(f"malformed quantizer string {qstr}: {hess!r} is neither hess nor none")
    out.update(use_hess=hess == "hess", scale_override=float(so))
    return out


def layer_file_path(quant_dir, quantizer_str, layer_idx, layer_key):
    """{quant_dir}/{quantizer_str}/{layer_idx}_{layer_key}.pt: what gen_layer_from_quantizer_str_and_key reads for key
    f"{layer_idx}_{layer_key}"."""
    return os.path.join(quant_dir, quantizer_str, f"{layer_idx}_{layer_key}.pt")


def _codebook(key, codebooks, lut_cache, fname):
    if codebooks is not None and key in codebooks:
        return torch.as_tensor(codebooks[key])
    if lut_cache is not None:
        path = os.path.join(lut_cache, fname)
        if os.path.exists(path):
            return torch.load(path, map_location="cpu")
    raise QpalError(f"no codebook {key!r}: pass codebooks={{{key!r}: ...}} or a lut_cache directory holding {fname}")


def quantize_linear(linear_or_W, quantizer_str, H=None, SU=None, SV=None, left_only=True, codebooks=None, lut_cache=None, bias=None,
                    save_path=None):
    """Quantise one linear layer -> (IncoherentLinear (fp16 buffers, on W's GPU), quant_info).

    linear_or_W: an nn.Linear (its bias is used unless `bias` is given) or a weight [out, in] on a GPU.
    quantizer_str: tcq_{KV}_{hess|none}_{scale}, tcomb_{KV1}_{KV2}_{ratio}_{hess|none}_{scale}, comb_..., ldlq_{vec}_{bits}_...
    H: proxy Hessian [in, in] (or the path of a reference Hessian file, load_hessian); used with `hess`, identity when None.
    SU / SV: sign vectors (random when None) — pass the same SU to q/k/v and to up/gate: the merged modules require it.
    codebooks: {tlut_bits: tlut [2^S, 2]} for the trellis families, {(vec, bits): lut [2^bits, vec]} for ldlq; or lut_cache,
    a directory with the reference's kmeans_{S}_2.pt / vq_kmeans_{bits}_{vec}.pt.
    save_path: write the layer file there (IncoherentLinear.save_info; see layer_file_path)."""
    t0 = time.time()
    q = parse_quantizer_str(quantizer_str)
    if isinstance(linear_or_W, torch.nn.Linear):
        W = linear_or_W.weight.detach()
        if bias is None and linear_or_W.bias is not None:
            bias = linear_or_W.bias.detach()
    else:
        W = linear_or_W.detach()
    if W.dim() != 2 or not W.is_cuda:
        raise QpalError("the weight must be a 2-D CUDA tensor")
    m, k = W.shape
    if isinstance(H, (str, os.PathLike)):
        H = load_hessian(H)
    use_hess = q["use_hess"]
    if q["kind"] == "ldlq":
        vec, bits = q["vec_sz"], q["lut_bits"]
        if vec not in (1, 2):
            raise QpalError(f"{quantizer_str}: ldlq layers are written in the tensor-core packing (vec 1, 2)")
        lut = _codebook((vec, bits), codebooks, lut_cache, f"vq_kmeans_{bits}_{vec}.pt")
        if _lut_geom(lut) != (vec, bits):
            raise QpalError(f"the codebook for {quantizer_str} must be [{2 ** bits}, {vec}]")
        lut_rms = None
    else:
        S = q["tlut_bits"]
        tlut = _codebook(S, codebooks, lut_cache, f"kmeans_{S}_2.pt")
        if _bits(tlut) != S:
            raise QpalError(f"the codebook for {quantizer_str} must be [{2 ** S}, 2]")
        lut_rms = tcq_lut_rms(tlut)
    Wr, Wscale, HRr, SU, SV = incoherent_preprocess(W, H if use_hess else None, SU, SV, q["scale_override"], left_only, lut_rms)
    Hq = HRr if use_hess else None
    kind = q["kind"]
    if kind == "tcq":
        trellis, hat, _ = quantize_tcq_weight(Wr, tlut, q["KV"], Hq)
        inner = QTIPLinearTCQ(k, m, 16, 16, 16, q["KV"], 2, q["tlut_bits"])
        inner.trellis.data.copy_(trellis)
        inner.tlut.data.copy_(tlut.detach().to("cpu", torch.float16))
        info = {"quantizer": "tcq_ldlq", "td_x": 16, "td_y": 16, "KV": q["KV"], "V": 2}
    elif kind == "tcomb":
        part = (int(k * q["ratio"]), int(k * (1 - q["ratio"])))
        t1, t2, hat, _ = quantize_combt_weight(Wr, tlut, q["KV"], part, Hq)
        inner = _comb_module(CombtLinearTCQ, Wr, tlut, q["KV"], part, t1, t2, None).cpu()
        info = {"quantizer": "combt_ldlq", "td_x": 16, "td_y": 16, "KV": q["KV"], "V": 2, "tlut_bits": q["tlut_bits"]}
    elif kind == "comb":
        part = (int(m * q["ratio"]), int(m * (1 - q["ratio"])))
        t1, t2, hat, _ = quantize_comb_weight(Wr, tlut, q["KV"], part, Hq)
        inner = _comb_module(CombLinearTCQ, Wr, tlut, q["KV"], part, t1, t2, None).cpu()
        info = {"quantizer": "comb_ldlq", "td_x": 16, "td_y": 16, "KV": q["KV"], "V": 2}
    else:
        qweight, hat, _ = quantize_vq_weight(Wr, lut, Hq)
        inner = VQLinearPackTensorCore(k, m, bits, vec, device="cpu")
        inner.qweight.data.copy_(qweight)
        inner.lut.data.copy_(lut.detach().to("cpu", torch.float16))
        info = {"quantizer": "vq_ldlq", "vec_sz": vec, "lut_bits": bits}
    ws64 = Wscale.to(torch.float64).view(-1, 1)
    Ws, hatWs = Wr.to(torch.float64) * ws64, hat.to(torch.float64) * ws64  # errors in W's own scale, as the reference reports
    orig_err = (Ws - hatWs).pow(2).mean()
    info.update(use_hess=use_hess, orig_err=orig_err.item(), err=(orig_err / Ws.pow(2).mean()).item(),
                scale_override=q["scale_override"], rot_info="skip_r" if left_only else "all", quantizer_str=quantizer_str)
    del Ws, hatWs
    layer = IncoherentLinear(k, m, k, m, bias=bias is not None, dtype=torch.float16, use_linear=False)
    layer.linear = inner  # (the bias is the wrapper's: the inner module has none)
    layer.SU.data.copy_(1.0 / SU)
    layer.SV.data.copy_(1.0 / SV)
    layer.Wscale.data.copy_(Wscale)
    if bias is not None:
        layer.bias.data.copy_(bias.detach())
    layer.rot_info = info["rot_info"]
    layer.apply_rot_info()
    layer = layer.to(W.device)
    info["time"] = time.time() - t0
    if save_path is not None:
        os.makedirs(os.path.dirname(os.path.abspath(save_path)), exist_ok=True)
        info["save_path"] = save_path
        layer.save_info(save_path, info)
    return layer, info
