"""The glue of Qwen- and Gemma-shaped blocks between the launches of a step (csrc/block_glue.hip): the q | k | v bias
and the per-head QK-norm in front of every attention launch (`qkv_prep`), the sandwich post-norm folded into the residual add
(`norm_add`), GeGLU (`glu_gelu_tanh`) and the final-logit soft cap (`logit_cap`).  Each wrapper is one launch on the current stream
on fp32 rows that lie in memory already; the decoder's step classes call them for `qkv_bias=`, `qk_norm=`, `post_norms=`,
`mlp_act="gelu_tanh"` and `logit_cap=`.

    qkv_prep(q, k, v, nq, nkv, hd, bias=b, q_norm_w=wq, k_norm_w=wk, eps=1e-6)   # in place, q / k / v views of one fp32 buffer
    norm_add(h32, y32, w, eps)                                                   # h32 += RMSNorm(y32) * w
    act = glu_gelu_tanh(ug32)                                                    # gelu_tanh(gate) * up of the up | gate rows
    logit_cap(logits, 30.0)                                                      # l <- 30 tanh(l / 30) in place

The `reference_*` functions are the contracts in numpy float64, in the style of sampling.reference_draw / logits.reference_process:
the kernels are held to them within bounds derived from the formats (tests/block_reference.py)."""
import math

import numpy as np

GELU_C0, GELU_C1 = 0.7978845608, 0.044715   # sqrt(2 / pi) as the kernel's fp32 literal, and the cubic's coefficient
HEAD_DIMS = (64, 128, 256)
MAX_ROWS, NORM_ADD_MAX_N = 65535, 16384


# ------------------------------------------------------------------------------------------------------------------ the contracts
def reference_qkv_prep(q, k, v, nq, nkv, hd, bias=None, q_norm_w=None, k_norm_w=None, eps=0.0):
    """-> (q, k, v) float64 [rows, nq hd], [rows, nkv hd], [rows, nkv hd]: x + b on all three (bias [(nq + 2 nkv) hd] in q | k | v
    order), then every head of q and of k times rsqrt(mean_hd(x^2) + eps) * w.  v is not normed."""
    q, k, v = (np.array(t, dtype=np.float64) for t in (q, k, v))
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)
        q, k, v = q + b[:nq * hd], k + b[nq * hd:(nq + nkv) * hd], v + b[(nq + nkv) * hd:]
    if (q_norm_w is None) != (k_norm_w is None):
        raise ValueError("q_norm_w and k_norm_w: both or neither")
    if q_norm_w is not None:
        def norm(x, heads, w):
            x = x.reshape(x.shape[0], heads, hd)
            return (x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * np.asarray(w, dtype=np.float64)).reshape(x.shape[0], heads * hd)
        q, k = norm(q, nq, q_norm_w), norm(k, nkv, k_norm_w)
    return q, k, v


def reference_norm_add(h, y, w, eps):
    """h + y * rsqrt(mean_n(y^2) + eps) * w per row, float64"""
    h, y = np.asarray(h, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return h + y / np.sqrt((y * y).mean(-1, keepdims=True) + eps) * np.asarray(w, dtype=np.float64)


def reference_gelu_tanh(g):
    g = np.asarray(g, dtype=np.float64)
    return 0.5 * g * (1.0 + np.tanh(GELU_C0 * (g + GELU_C1 * g ** 3)))


def reference_glu_gelu_tanh(ug):
    """gelu_tanh(gate) * up of up | gate rows [rows, 2 inter] -> float64 [rows, inter]"""
    ug = np.asarray(ug, dtype=np.float64)
    inter = ug.shape[-1] // 2
    return reference_gelu_tanh(ug[..., inter:]) * ug[..., :inter]


def reference_logit_cap(logits, cap):
    """cap * tanh(l / cap), float64"""
    return cap * np.tanh(np.asarray(logits, dtype=np.float64) / cap)


# ------------------------------------------------------------------------------------------------------------------- the launches
def _env():
    import torch
    from . import _native
    return torch, _native


def _rows_f32(torch, QpalError, who, name, t, width=None):
    """an fp32 device tensor [rows, width] with contiguous rows -> its row stride in elements"""
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1
            or (width is not None and t.shape[1] != width)):
        raise QpalError(f"{who}: {name} must be an fp32 device tensor [rows, {'n' if width is None else width}] with contiguous rows")
    if t.shape[0] > MAX_ROWS:
        raise QpalError(f"{who}: at most {MAX_ROWS} rows, got {t.shape[0]}")
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))


def _vec_f32(torch, QpalError, who, name, t, n, dev):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.shape != (n,) or not t.is_contiguous() or t.device != dev:
        raise QpalError(f"{who}: {name} must be a contiguous fp32 [{n}] tensor on {dev}")
    return t.data_ptr()


def _eps(QpalError, who, eps):
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not math.isfinite(eps) or eps <= 0:
        raise QpalError(f"{who}: eps must be a finite float > 0, got {eps!r}")
    return float(eps)


def qkv_prep(q, k, v, nq, nkv, hd, bias=None, q_norm_w=None, k_norm_w=None, eps=0.0):
    """In place on q [rows, nq hd], k and v [rows, nkv hd]: fp32 views of one buffer with ONE row stride, the views an attention launch
    takes.  bias: fp32 [(nq + 2 nkv) hd] in q | k | v order or None; q_norm_w / k_norm_w: fp32 [hd] each, both or neither — behind the
    bias every head of q and k becomes x * rsqrt(mean(x^2) + eps) * w (the EFFECTIVE weight: Gemma's 1 + w is the caller's).  With
    neither a bias nor weights nothing is launched."""
    torch, nat = _env()
    who, E = "qkv_prep", nat.QpalError
    if hd not in HEAD_DIMS or nq < 1 or nkv < 1:
        raise E(f"{who}: head_dim must be one of {HEAD_DIMS} and nq, nkv >= 1, got {hd}, {nq}, {nkv}")
    lds = [_rows_f32(torch, E, who, n, t, w) for n, t, w in (("q", q, nq * hd), ("k", k, nkv * hd), ("v", v, nkv * hd))]
    rows, dev = q.shape[0], q.device
    if k.shape[0] != rows or v.shape[0] != rows or k.device != dev or v.device != dev or (rows > 1 and len(set(lds)) != 1):
        raise E(f"{who}: q, k and v must have the same rows, device and row stride")
    if (q_norm_w is None) != (k_norm_w is None):
        raise E(f"{who}: q_norm_w and k_norm_w come together or not at all")
    pb = None if bias is None else _vec_f32(torch, E, who, "bias", bias, (nq + 2 * nkv) * hd, dev)
    pq = pk = None
    if q_norm_w is not None:
        pq, pk = _vec_f32(torch, E, who, "q_norm_w", q_norm_w, hd, dev), _vec_f32(torch, E, who, "k_norm_w", k_norm_w, hd, dev)
        eps = _eps(E, who, eps)
    if rows == 0 or (pb is None and pq is None):
        return
    with torch.cuda.device(dev):
        rc = nat.lib().qpal_qkv_prep(q.data_ptr(), k.data_ptr(), v.data_ptr(), max(lds), rows, nq, nkv, hd, pb, pq, pk, float(eps),
                                     torch.cuda.current_stream(dev).cuda_stream)
    nat.check(rc, "qpal_qkv_prep")


def norm_add(h, y, w, eps):
    """h[r] += y[r] * rsqrt(mean(y[r]^2) + eps) * w: the sandwich post-norm of a sublayer's output y and the residual add, fp32.  h, y
    fp32 [rows, n] with contiguous rows (strides multiples of 4, 16-byte aligned), n a multiple of 4 up to 16384; w fp32 [n], the
    effective weight."""
    torch, nat = _env()
    who, E = "norm_add", nat.QpalError
    ld_h = _rows_f32(torch, E, who, "h", h)
    rows, n = h.shape
    ld_y = _rows_f32(torch, E, who, "y", y, n)
    if y.shape[0] != rows or y.device != h.device:
        raise E(f"{who}: y must have h's rows and device")
    if n < 4 or n % 4 or n > NORM_ADD_MAX_N:
        raise E(f"{who}: n must be a multiple of 4 up to {NORM_ADD_MAX_N}, got {n}")
    pw, eps = _vec_f32(torch, E, who, "w", w, n, h.device), _eps(E, who, eps)
    if h.data_ptr() % 16 or y.data_ptr() % 16 or pw % 16 or ld_h % 4 or ld_y % 4:
        raise E(f"{who}: h, y and w must be 16-byte aligned, the row strides multiples of 4")
    if rows == 0:
        return
    with torch.cuda.device(h.device):
        rc = nat.lib().qpal_norm_add(h.data_ptr(), ld_h, y.data_ptr(), ld_y, pw, eps, rows, n, torch.cuda.current_stream(h.device).cuda_stream)
    nat.check(rc, "qpal_norm_add")


def glu_gelu_tanh(ug, out=None):
    """act = gelu_tanh(gate) * up of fp32 up | gate rows ug [rows, 2 inter] -> fp32 [rows, inter] (out, or a new tensor).  inter a
    multiple of 4; 16-byte aligned rows."""
    torch, nat = _env()
    who, E = "glu_gelu_tanh", nat.QpalError
    ld_ug = _rows_f32(torch, E, who, "ug", ug)
    rows, inter = ug.shape[0], ug.shape[1] // 2
    if ug.shape[1] != 2 * inter or inter < 4 or inter % 4:
        raise E(f"{who}: ug must be [rows, 2 inter] with inter a multiple of 4, got {list(ug.shape)}")
    if out is None:
        out = torch.empty(rows, inter, dtype=torch.float32, device=ug.device)
    ld_out = _rows_f32(torch, E, who, "out", out, inter)
    if out.shape[0] != rows or out.device != ug.device:
        raise E(f"{who}: out must have ug's rows and device")
    if ug.data_ptr() % 16 or out.data_ptr() % 16 or ld_ug % 4 or ld_out % 4:
        raise E(f"{who}: ug and out must be 16-byte aligned, the row strides multiples of 4")
    if rows:
        with torch.cuda.device(ug.device):
            rc = nat.lib().qpal_glu_gelu_tanh(out.data_ptr(), ld_out, ug.data_ptr(), ld_ug, rows, inter,
                                              torch.cuda.current_stream(ug.device).cuda_stream)
        nat.check(rc, "qpal_glu_gelu_tanh")
    return out


def logit_cap(logits, cap, vocab=None):
    """l <- cap * tanh(l / cap) in place on fp32 logits [rows, >= vocab] with contiguous rows (vocab None: every column)."""
    torch, nat = _env()
    who, E = "logit_cap", nat.QpalError
    ld = _rows_f32(torch, E, who, "logits", logits)
    vocab = logits.shape[1] if vocab is None else int(vocab)
    if not 1 <= vocab <= logits.shape[1]:
        raise E(f"{who}: vocab must be in 1 .. {logits.shape[1]}, got {vocab}")
    if isinstance(cap, bool) or not isinstance(cap, (int, float)) or not math.isfinite(cap) or cap <= 0:
        raise E(f"{who}: cap must be a finite float > 0, got {cap!r}")
    if logits.shape[0] == 0:
        return
    with torch.cuda.device(logits.device):
        rc = nat.lib().qpal_logit_cap(logits.data_ptr(), ld, logits.shape[0], vocab, float(cap),
                                      torch.cuda.current_stream(logits.device).cuda_stream)
    nat.check(rc, "qpal_logit_cap")
