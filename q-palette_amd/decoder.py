"""Whole-model decode step of a Llama-shaped model on this library's kernels: B >= 1 sequences, one token each per step.

The residual stream stays fp32 ([B, H]).  Per layer: q|k|v -> rotary embedding + KV append + attention (one launch) -> o_proj
(ADDS into the stream) -> up|gate -> SwiGLU -> down_proj (adds into the stream); then final norm, lm_head and argmax.  Every
projection group reads rotate(RMSNorm(x) * su) / scale: inside the GEMV launch where its staging can rotate the hidden width
(batch 1, k in {2048, 4096}), as one `hadamard.rotate` launch in front of the plain GEMV launch otherwise.

At batch 1 the step also takes what only exists there: up|gate as one interleaved layer whose epilogue writes
fp16 silu(gate) * up, down_proj's 28 x 512 rotation inside its own staging, `qpal_attn_rope_decode` with its split-context
workspace, and `qpal_lm_head_argmax`: 5 or 6 launches per layer, 9 where the hidden width has to be rotated by a launch of its
own (70B: 8192).  `generic=True` runs a batch of one the way every larger batch runs.

    step = DecodeStep(layers, embed, norm, lm_head, kcache, vcache, inv_freq, tok, pos, out_tok)
    step()                      # capturable: reads tok / pos, updates the caches at pos, writes out_tok

With `sampler=sampling.Sampler(B, vocab, device, ...)` the step ends in `qpal_lm_head_logits` + `qpal_sample` at every B instead of
an argmax: out_tok[b] is drawn with slot b's temperature / top-k / top-p / seed and the counter pos[b];
sampler.logits holds the step's logits.  A sampler built with min_p / top_a / typical_p draws with `qpal_sample_trunc` in the same
place, in every step class below (the same launch count; the speculative step stays lossless, a draw depends on
(seed, ctr, logits, parameters) only).  A sampler built with logprobs=True adds `qpal_token_logprob` on the drawn tokens
(sampler.logprob), one built with top_logprobs=n `qpal_top_logprob` behind it (sampler.top_id / sampler.top_logprob
[B, n]: the n likeliest tokens of every row that drew): one more launch each, in every step class below, and `Score(...,
top_logprobs=n)` has the lists at every scored position.

`Prefill` takes a prompt into ONE slot of the same caches: the batch-B layer with rows = consecutive positions of one sequence,
in chunks of at most 128 rows, with `prefill_attention` (causal, rows appended to the slot's cache) in the attention's place.

    pf = Prefill(layers, embed, norm, lm_head, kcache, vcache, inv_freq, chunk=128)
    next_tok = pf(tokens, slot=0, pos0=0)   # then DecodeStep with tok[slot] = next_tok, pos[slot] = len(tokens)

`Score` is `Prefill` with a tail on EVERY row instead of the last one: the log-probability of each next token of a sequence
(`qpal_lm_head_logits` on the chunk's rows + `qpal_token_logprob`), `Score.nll` and `perplexity` over windows.

    sc = Score(layers, embed, norm, lm_head, kcache, vcache, inv_freq, chunk=128)
    lp = sc(tokens, slot=0, pos0=0)         # fp32 [N - 1]: lp[t] = log p(tokens[t + 1] | tokens[0 .. t])
    ppl, loss = perplexity(sc, windows)     # windows int64 [W, N]

`RaggedStep` puts rows of SEVERAL slots into one step of up to 128 rows — prompt chunks of some, one decode token of others — with
`ragged_prefill_attention` in the attention's place and one next token per segment.

    rs = RaggedStep(layers, embed, norm, lm_head, kcache, vcache, inv_freq, rows=128, segments=16)
    next_toks = rs(*rs.pack([(slot, tokens_1d, pos0), ...]))    # int64 [segments]; capturable with the four tensors rewritten

`SpeculativeStep` is a RaggedStep whose segments are built on the device: per slot the pending token and up to `draft` guessed
tokens (prompt lookup, or the caller's), a draw at every row, and the guesses that equal the draws kept — several tokens per slot
and step, the same stream as one-token sampling.

    ss = SpeculativeStep(layers, embed, norm, lm_head, kcache, vcache, inv_freq, draft=4, gram=(2, 4))
    ss.begin(slot, tokens)                  # tokens[:-1] are in the cache, the last one is pending
    out_tok, n_out = ss()                   # int64 [B, draft + 1], int32 [B]; capturable

All of them take `block_table=` for a paged cache (paging.PagedKVCache): kcache / vcache are then the per-layer page
pools [num_pages, nkv, page_size, hd], the table is int32 [B, max_pages], and context = max_pages * page_size.  The caller reserves
pages for every position a call, or a run of graph replays, will reach before it starts: nothing in here allocates or synchronises.

All of them take `adapters=` too, a lora.LoraBank of the caches' slots: every row then runs with the low-rank
adapter of its slot, bank.slot_adapter[slot] (-1: none) — one `lora_apply` launch behind the GEMV of each projection group, four
per layer.  The rows' adapters are looked up on the device in every call, so bank.set(slot, adapter) between replays of a captured
step takes effect without a new capture.

`DecodeStep`, `Prefill` and `SpeculativeStep` take `processor=`, a logits.LogitProcessor of the caches' slots: token
masks, a sparse logit bias and repetition / presence / frequency penalties between the lm_head and the draw.  A step counts the
tokens it feeds (`qpal_logit_observe`), then processes the logits in place (`qpal_logit_process`), then draws: two more launches,
everything on the device, and the processor's setters between replays of a captured step change the next draw.

The same three take `grammar=`, a grammar.GrammarBank of the caches' slots: every slot with a grammar draws only
tokens that keep its text a prefix of a match of its regular expression, and eos only where the text is a whole match.  The mask
comes from the slot's automaton state on the device (`qpal_grammar_mask`, behind the processor and in front of the draw) and the
drawn tokens advance that state (`qpal_grammar_advance`): two more launches, three in a SpeculativeStep, whose rows each carry the
state their guessed tokens lead to (`qpal_grammar_rows`).  No host read in a step; bank.set / reset between replays of a captured
step change the next draw.

`DecodeStep` and `SpeculativeStep` take `stop=`, a stop.StopBank of the caches' slots: stop strings, stop token ids,
max_tokens / min_tokens and the context limit are judged on the device by the step itself (`qpal_stop_advance`, one more launch).  A
DecodeStep then moves tok / pos itself — `for _ in range(n): graph.replay()` generates with no host work — and a slot that is done
gets pos = -1 and falls out of the replays that follow; a SpeculativeStep cuts its emitted run at the token that finishes the slot.
With a bank built with min_tokens=True (needs a sampler) one more launch in front of the draw keeps the stop ids from being drawn
before a slot's min_tokens (`qpal_stop_mask`).  bank.result(slot) reads the record after the run.

All five take `window=`: None, an int W >= 1, or one entry (None or an int) per layer — sliding-window attention,
the row at position p attends to positions max(0, p - W + 1) .. p in the layers that have a window (Mistral: every layer; Gemma-2,
gpt-oss: every other one).  Each layer's attention launch passes its own value; nothing else in a step changes, the launch count
included.  A batch-1 DecodeStep with a window launches the batched attention at B = 1 (the fused single-sequence kernel has no
window), and `shared_prefix=` together with a window raises QpalError.  The steps never give pages back: on a paged cache the
caller calls `cache.trim(slot, window_floor(pos, W))` with the LARGEST window of any layer between steps (not at all if one layer
has none).

All five also take `softcap=`, `sinks=` and `attn_scale=`.  softcap: None, a finite float > 0 or one entry per layer —
every attention score s of that layer becomes softcap * tanh(s / softcap) (Gemma-2's attn_logit_softcapping).  sinks: None or an
fp32 [n_layers, nq] tensor on the device — layer i's launch reads row i, one logit per query head that joins the softmax
denominator only (gpt-oss); the launches read it on the device, so a captured step follows values changed in place between replays.
attn_scale: None (1 / sqrt(head_dim)) or the factor on q.k (Gemma-2 27B's query_pre_attn_scalar).  Nothing else in a step changes, the
launch count included; a batch-1 DecodeStep with a cap or sinks launches the batched attention at B = 1, and `shared_prefix=`
together with either raises QpalError.

All five take the block variants of Qwen2 / 2.5 / 3 and Gemma-2 / 3 shaped layers (blocks.py, csrc/block_glue.hip).  Every
tensor is contiguous fp32 on the step's device, checked in the constructor, and layer i's launch gets the VIEW of row i: values
written in place between replays of a captured step are followed.
  qkv_bias: None or [n_layers, (nq + 2 nkv) hd], q | k | v order — added to the projections (Qwen2).
  qk_norm: None or (eps, [n_layers, 2, hd]) — per-head RMSNorm of q (row 0) and k (row 1) behind the bias, in front of the rotary
    embedding (Qwen3, Gemma-3).  The EFFECTIVE weight: a Gemma caller passes 1 + w.  One `qpal_qkv_prep` launch per layer serves both,
    between the q|k|v launch (and its adapter's) and the attention launch, which itself is untouched.
  mlp_act: "silu" or "gelu_tanh" (GeGLU) — `qpal_glu_gelu_tanh` writes gelu_tanh(gate) * up as fp32 rows, which the rotation in front
    of down_proj and the adapter's "down" update read: one more launch per layer.
  post_norms: None or (eps, [n_layers, 2, H]) — Gemma's sandwich norms: row 0 norms the attention sublayer's output, row 1 the MLP's
    (effective weights again).  o_proj and down_proj (and their adapter updates) then write a scratch row instead of adding into the
    stream, and `qpal_norm_add` folds RMSNorm(scratch) * w into it: two more launches per layer.  The modules'
    `post_attention_layernorm` keeps its Llama meaning throughout, the norm in FRONT of the MLP — Gemma calls that one
    `pre_feedforward_layernorm`; Gemma's own `post_attention_layernorm` is post_norms row 0, its `post_feedforward_layernorm` row 1.
  logit_cap: None or a float > 0 — the final logits become cap * tanh(l / cap) (`qpal_logit_cap`), one launch directly behind the
    lm_head of a sampler's tail, of Score and of SpeculativeStep, in front of the processor, grammar and stop masks; an argmax tail
    needs none (the cap is monotone).
  inv_freq may be fp32 [n_layers, hd / 2]: layer i rotates with row i (Gemma-3's local and global layers have different bases).
With every one of them at its default a step launches exactly what it launched without them.
"""
import math

import torch

from . import _native as nat
from . import hadamard as had
from . import grammar as gram_mod
from . import blocks, linear, logits, lora, ops, sampling
from . import stop as stop_mod
from .attention import _score_mods as _check_score_mods
from .attention import _window as _check_one_window
from .attention import (attention_workspace, decode_attention, paged_decode_attention, paged_prefill_attention,
                        paged_ragged_prefill_attention, prefill_attention, prefill_workspace, ragged_prefill_attention, ragged_workspace,
                        shared_prefix_decode_attention, shared_prefix_workspace)
from .linear import multi_gemv
from .moe import MoEMLP


def ug_layout(mlp):
    """(layers, their Wscale slices) of an IncoherentMLP's up|gate group"""
    inter = mlp.intermediate_size
    if mlp.merge_ug:
        return [mlp.ug_proj], [mlp.Wscale_ug]
    return [mlp.up_proj, mlp.gate_proj], [mlp.Wscale_ug[:inter], mlp.Wscale_ug[inter:]]


def _tc(l):
    return isinstance(l, linear._base.PackedLinearBase) and not isinstance(l, linear.VQLinearPackSIMT)


def fusable(layers):
    """True if the batch-1 step can run on `layers`: tensor-core-order projections, and codecs with a multi-job launch where the
    GEMV staging is to rotate the hidden width."""
    rot_in_gemv = ops.can_fuse_rotation(1, layers[0].self_attn.hidden_size)
    def mlp_proj(m):  # (a sparse layer's experts run the routed launches of moe.py at every batch)
        return [] if isinstance(m, MoEMLP) else ug_layout(m)[0] + [m.down_proj]
    return all(all(_tc(p) for p in l.self_attn._qkv_layout()[0] + mlp_proj(l.mlp) + [l.self_attn.o_proj])
               and (not rot_in_gemv or (linear.rotation_fusable(l.self_attn._qkv_layout()[0], 1)
                                        and linear.rotation_fusable([l.self_attn.o_proj], 1)))
               for l in layers)


def k28_in_gemv(mlp):
    """down_proj's rotation inside its own launch: k = 14336 = 28 x 512, a tensor-core-order layer whose codebook image can lend
    the rotation its scratch (every TCQ codec)."""
    if mlp.inter_K <= 1 or not ops.can_fuse_rotation(1, mlp.intermediate_size, mlp.inter_K):
        return False
    d = mlp.down_proj
    if isinstance(d, linear.VQLinearPackTensorCore):
        idx = d.lut_bits if d.vec_sz == 2 else (2 * d.lut_bits if d.lut_bits <= 6 else d.lut_bits)
        return (4 << (idx + min(15 - idx, 5))) >= 40 * 1024
    return isinstance(d, (linear.QTIPLinearTCQ, linear.CombtLinearTCQ)) and linear._codec_key(d)[0] != "single"


class _Rows:
    """What the step classes share: the model and its caches, the rotation of the hidden width, the fp32 / fp16 row buffers of one
    layer on up to `rows` rows of the residual stream, the layer as every batch runs it, and the tails.  A class adds its attention
    launch (`_attention(i, q, k, v, out)`), that launch's workspace `attn_ws`, and its call."""

    _launches_per = None  # "<class>: launches are per <what>" where a step has no launches per token

    def __init__(self, who, layers, embed, norm, lm_head, kcache, vcache, inv_freq, rows, sampler, block_table, slots=None,
                 logits_tail=False, native_argmax=False, adapters=None, processor=None, grammar=None, window=None, softcap=None,
                 sinks=None, attn_scale=None, stop=None,
                 qkv_bias=None, qk_norm=None, mlp_act="silu", post_norms=None, logit_cap=None):
        """qkv_bias, qk_norm, mlp_act, post_norms, logit_cap: the block variants (the module's last paragraph; `_check_block`);
        window: None, an int or one entry per layer — the sliding window of every layer's attention launch (self.window[i]);
        softcap: None, a float or one entry per layer (self.softcap[i]); sinks: None or fp32 [n_layers, nq] (layer i: row i);
        attn_scale: None (1 / sqrt(head_dim)) or the scale of every layer's scores;
        slots: the sequences of the caches where the caller fixes them (DecodeStep's B), else read off the caches or the table;
        logits_tail: the tail is qpal_lm_head_logits without a sampler too; native_argmax: `_argmax_tail` is the one-launch kernel;
        adapters: a lora.LoraBank of these layers and slots, or None; processor: a logits.LogitProcessor of these slots, or None;
        grammar: a grammar.GrammarBank of these slots, or None; stop: a stop.StopBank of these slots, or None"""
        self.block_table = block_table
        self.moe = [isinstance(l.mlp, MoEMLP) for l in layers]
        if any(self.moe) and adapters is not None:
            raise nat.QpalError(f"{who}: adapters= on a model with MoE layers is not built (no adapters on experts)")
        self.window = self._check_window(who, window, len(layers))
        self.softcap, self.sinks = self._check_score(who, softcap, sinks, layers, embed.device)
        self.slots = self._check_table(who, kcache, block_table, slots)
        self.adapters = self._check_adapters(who, adapters, self.slots, layers, embed)
        # the adapter of every row, looked up on the device before the layers run (DecodeStep: the bank's own vector, row = slot)
        self.row_adapter = None if adapters is None else torch.full((rows,), -1, dtype=torch.int32, device=embed.device)
        self.sampler = self._check_sampler(sampler, self.slots, embed, lm_head)
        if logits_tail:
            self._check_lm_head(who, embed, lm_head)
        self.processor = self._check_processor(who, processor, self.slots, embed, lm_head, sampler is not None or logits_tail)
        self.grammar = self._check_grammar(who, grammar, self.slots, embed, lm_head, sampler is not None)
        self.stop = self._check_stop(who, stop, self.slots, embed, lm_head, sampler is not None)
        self._check_block(who, layers, embed.device, inv_freq, qkv_bias, qk_norm, mlp_act, post_norms, logit_cap)
        att = layers[0].self_attn
        H, dev = att.hidden_size, embed.device
        # an MoE layer is one whose .mlp is a MoEMLP (self.moe; dense and sparse layers may mix): its buffers are its own, sized here
        if any(self.moe) and self.gelu:
            raise nat.QpalError(f"{who}: mlp_act=\"gelu_tanh\" on MoE layers is not built (the routed SwiGLU rotation is silu only)")
        # the step's OWN workspaces, one per shape of sparse layer (launches are stream-ordered): they live as long as the step
        self.moe_ws = {}
        for l, sparse in zip(layers, self.moe):
            if sparse and l.mlp.shape_key() not in self.moe_ws:
                self.moe_ws[l.mlp.shape_key()] = l.mlp.new_workspace(rows)
        dense_inter = max([l.mlp.intermediate_size for l, sparse in zip(layers, self.moe) if not sparse], default=0)
        self.layers, self.embed, self.norm, self.lm_head, self.inv_freq = layers, embed, norm, lm_head, inv_freq
        self.kcache, self.vcache = kcache, vcache
        self.nq, self.nkv, self.head_dim = att.num_heads, att.num_key_value_heads, att.head_dim
        # paged: the pools' third dimension is the page size
        self.context = kcache[0].shape[2] * (1 if block_table is None else block_table.shape[1])
        self.eps, self.attn_scale = layers[0].input_layernorm.eps, 1.0 / math.sqrt(att.head_dim)
        if attn_scale is not None:
            if isinstance(attn_scale, bool) or not isinstance(attn_scale, (int, float)) or not math.isfinite(attn_scale):
                raise nat.QpalError(f"{who}: attn_scale must be None or a finite float, got {attn_scale!r}")
            self.attn_scale = float(attn_scale)
        hk, self.hidden_K = had.get_hadK(H)
        self.hidden_hadT = None if hk is None else hk.T.contiguous().half().to(dev)
        self.h32 = torch.zeros(rows, H, dtype=torch.float32, device=dev)
        self.a16 = torch.zeros(rows, H, dtype=torch.float16, device=dev)
        self.qkv32 = torch.zeros(rows, H + 2 * att.kv_out, dtype=torch.float32, device=dev)
        self.ug32 = torch.zeros(rows, 2 * dense_inter, dtype=torch.float32, device=dev)
        # a sublayer's output in front of its post-norm, and GeGLU's activation: only where a step has them
        self.y32 = None if post_norms is None else torch.zeros(rows, H, dtype=torch.float32, device=dev)
        self.act32 = None if not self.gelu else torch.zeros(rows, dense_inter, dtype=torch.float32, device=dev)
        self.lm_ws = None
        if native_argmax:
            self.lm_ws_bytes = nat.lib().qpal_lm_head_ws_bytes(lm_head.shape[0])
            self.lm_ws = torch.zeros(self.lm_ws_bytes // 4, dtype=torch.float32, device=dev)

    @staticmethod
    def _check_window(who, window, n_layers):
        """window= of a step class as one entry per layer: None (no window) or an int >= 1"""
        if window is None or isinstance(window, int):
            return [_check_one_window(window, who)] * n_layers
        if not isinstance(window, (list, tuple)) or len(window) != n_layers:
            raise nat.QpalError(f"{who}: window must be None, an int >= 1 or one entry per layer ({n_layers}), got {window!r}")
        return [_check_one_window(w, who) for w in window]

    @staticmethod
    def _check_score(who, softcap, sinks, layers, dev):
        """softcap= and sinks= of a step class: one cap (None or a float > 0) per layer, and sinks (None or fp32 [n_layers, nq])"""
        n_layers, nq = len(layers), layers[0].self_attn.num_heads
        if softcap is None or isinstance(softcap, (int, float)):
            caps = [_check_score_mods(softcap, None, who)[0]] * n_layers
        elif isinstance(softcap, (list, tuple)) and len(softcap) == n_layers:
            caps = [_check_score_mods(c, None, who)[0] for c in softcap]
        else:
            raise nat.QpalError(f"{who}: softcap must be None, a float > 0 or one entry per layer ({n_layers}), got {softcap!r}")
        if sinks is not None:
            if (not isinstance(sinks, torch.Tensor) or sinks.dtype != torch.float32 or sinks.shape != (n_layers, nq)
                    or sinks.device != dev or not sinks.is_contiguous()):
                raise nat.QpalError(f"{who}: sinks must be None or a contiguous float32 [{n_layers}, {nq}] tensor on {dev}")
        return caps, sinks

    def _score(self, i):
        """the window= / softcap= / sinks= of layer i's attention launch"""
        return {"window": self.window[i], "softcap": self.softcap[i], "sinks": None if self.sinks is None else self.sinks[i]}

    def _check_block(self, who, layers, dev, inv_freq, qkv_bias, qk_norm, mlp_act, post_norms, logit_cap):
        """the block variants of a step class: sets self.qkv_bias (None or fp32 [n_layers, (nq + 2 nkv) hd]),
        self.qk_norm / self.post_norms (None or (eps, fp32 [n_layers, 2, hd | H])), self.gelu, self.logit_cap (None or a float) and
        self.rope_per_layer (inv_freq is fp32 [n_layers, hd / 2]: layer i rotates with row i)"""
        att = layers[0].self_attn
        L, nq, nkv, hd, H = len(layers), att.num_heads, att.num_key_value_heads, att.head_dim, att.hidden_size

        def rows(name, t, shape):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape or t.device != dev
                    or not t.is_contiguous()):
                raise nat.QpalError(f"{who}: {name} must be a contiguous float32 {list(shape)} tensor on {dev}")
            return t

        def normed(name, arg, width):
            if arg is None:
                return None
            if not isinstance(arg, (tuple, list)) or len(arg) != 2:
                raise nat.QpalError(f"{who}: {name} must be None or (eps, float32 [{L}, 2, {width}])")
            eps, w = arg
            if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not math.isfinite(eps) or eps <= 0:
                raise nat.QpalError(f"{who}: {name}: eps must be a finite float > 0, got {eps!r}")
            return float(eps), rows(name, w, (L, 2, width))

        self.qkv_bias = None if qkv_bias is None else rows("qkv_bias", qkv_bias, (L, (nq + 2 * nkv) * hd))
        self.qk_norm, self.post_norms = normed("qk_norm", qk_norm, hd), normed("post_norms", post_norms, H)
        if (self.qkv_bias is not None or self.qk_norm is not None) and hd not in (64, 128, 256):
            raise nat.QpalError(f"{who}: qkv_bias / qk_norm need a head_dim of 64, 128 or 256, got {hd}")
        if self.post_norms is not None and (H % 4 or H > 16384):
            raise nat.QpalError(f"{who}: post_norms need a hidden width that is a multiple of 4 up to 16384, got {H}")
        if mlp_act not in ("silu", "gelu_tanh"):
            raise nat.QpalError(f"{who}: mlp_act must be 'silu' or 'gelu_tanh', got {mlp_act!r}")
        self.gelu = mlp_act == "gelu_tanh"
        if self.gelu and layers[0].mlp.intermediate_size % 4:
            raise nat.QpalError(f"{who}: mlp_act='gelu_tanh' needs an intermediate size that is a multiple of 4")
        if logit_cap is not None and (isinstance(logit_cap, bool) or not isinstance(logit_cap, (int, float))
                                      or not math.isfinite(logit_cap) or logit_cap <= 0):
            raise nat.QpalError(f"{who}: logit_cap must be None or a finite float > 0, got {logit_cap!r}")
        self.logit_cap = None if logit_cap is None else float(logit_cap)
        self.rope_per_layer = isinstance(inv_freq, torch.Tensor) and inv_freq.dim() == 2
        if self.rope_per_layer:
            rows("a per-layer inv_freq", inv_freq, (L, hd // 2))

    def _inv_freq(self, i):
        """the rotary table of layer i's attention launch: the one table, or row i of a per-layer one (a view)"""
        return self.inv_freq[i] if self.rope_per_layer else self.inv_freq

    def _prep(self, i, q, k, v):
        """bias and per-head QK-norm of layer i on the q | k | v rows, in place, in front of the attention launch (one launch)"""
        if self.qkv_bias is None and self.qk_norm is None:
            return
        eps, w = (0.0, None) if self.qk_norm is None else self.qk_norm
        blocks.qkv_prep(q, k, v, self.nq, self.nkv, self.head_dim, bias=None if self.qkv_bias is None else self.qkv_bias[i],
                        q_norm_w=None if w is None else w[i, 0], k_norm_w=None if w is None else w[i, 1], eps=eps)

    def _cap_logits(self, lg):
        """the final-logit soft cap, directly behind the lm_head (one launch): in front of the processor, grammar and stop masks"""
        if self.logit_cap is not None:
            blocks.logit_cap(lg, self.logit_cap)

    def _block_launches(self):
        """(per layer, tail) launches the block variants add (arithmetic on the configuration: stand-ins may lack the attributes)"""
        per_layer = 1 if getattr(self, "qkv_bias", None) is not None or getattr(self, "qk_norm", None) is not None else 0
        per_layer += 2 if getattr(self, "post_norms", None) is not None else 0
        per_layer += 1 if getattr(self, "gelu", False) else 0
        return per_layer, 1 if getattr(self, "logit_cap", None) is not None and self.sampler is not None else 0

    @staticmethod
    def _check_table(who, kcache, block_table, B=None):
        """the block table's shape against B sequences (None: any number); returns the sequences of the caches"""
        if block_table is None:
            return kcache[0].shape[0] if B is None else B
        if block_table.dim() != 2 or B not in (None, block_table.shape[0]):
            raise nat.QpalError(f"{who}: block_table must be int32 [{'B' if B is None else B}, max_pages], got {list(block_table.shape)}")
        return block_table.shape[0]

    @staticmethod
    def _check_adapters(who, bank, B, layers, embed):
        if bank is None:
            return None
        if not isinstance(bank, lora.LoraBank) or bank.slots != B or len(bank.groups) != len(layers) or bank.device != embed.device:
            raise nat.QpalError(f"{who}: adapters must be a LoraBank of {len(layers)} layers and {B} slots on {embed.device}")
        return bank

    @staticmethod
    def _check_lm_head(who, embed, lm_head):
        H = embed.shape[1]
        if H % 512 or H > 8192 or lm_head.data_ptr() % 16 or not lm_head.is_contiguous():
            raise nat.QpalError(f"{who}: qpal_lm_head_logits needs a hidden width that is a multiple of 512 up to 8192 and a "
                                "contiguous 16-byte aligned lm_head")

    @staticmethod
    def _has_argmax_kernel(embed, lm_head):
        """qpal_lm_head_argmax serves these hidden widths and a 16-byte aligned lm_head; elsewhere `_argmax_tail` runs torch ops"""
        return embed.shape[1] in (2048, 4096, 8192) and lm_head.data_ptr() % 16 == 0

    @staticmethod
    def _check_sampler(sampler, B, embed, lm_head):
        if sampler is None:
            return None
        if sampler.B != B or sampler.vocab != lm_head.shape[0] or sampler.device != embed.device:
            raise nat.QpalError(f"sampler: built for {sampler.B} slots of {sampler.vocab} logits on {sampler.device}, "
                                f"the step has {B} of {lm_head.shape[0]} on {embed.device}")
        _Rows._check_lm_head("sampler", embed, lm_head)
        return sampler

    @staticmethod
    def _check_processor(who, proc, B, embed, lm_head, logits_tail):
        if proc is None:
            return None
        if not logits_tail:
            raise nat.QpalError(f"{who}: a processor works on the logits of a sampler's tail: give the step a sampler")
        if not isinstance(proc, logits.LogitProcessor) or proc.B != B or proc.vocab != lm_head.shape[0] or proc.device != embed.device:
            raise nat.QpalError(f"{who}: processor must be a LogitProcessor of {B} slots of {lm_head.shape[0]} logits on {embed.device}")
        return proc

    @staticmethod
    def _check_grammar(who, bank, B, embed, lm_head, sampled):
        if bank is None:
            return None
        if not sampled:
            raise nat.QpalError(f"{who}: a grammar masks the logits of a sampler's tail: give the step a sampler (greedy: temperature 0)")
        if not isinstance(bank, gram_mod.GrammarBank) or bank.B != B or bank.vocab != lm_head.shape[0] or bank.device != embed.device:
            raise nat.QpalError(f"{who}: grammar must be a GrammarBank of {B} slots of {lm_head.shape[0]} tokens on {embed.device}")
        return bank

    @staticmethod
    def _check_stop(who, bank, B, embed, lm_head, sampled):
        if bank is None:
            return None
        if not isinstance(bank, stop_mod.StopBank) or bank.B != B or bank.vocab != lm_head.shape[0] or bank.device != embed.device:
            raise nat.QpalError(f"{who}: stop must be a StopBank of {B} slots of {lm_head.shape[0]} tokens on {embed.device}")
        if bank.min_tokens_mask and not sampled:
            raise nat.QpalError(f"{who}: the min_tokens mask works on the logits of a sampler's tail: give the step a sampler "
                                "(greedy: temperature 0) or build the bank without min_tokens=True")
        return bank

    @property
    def launches_per_token(self):
        raise nat.QpalError(f"{self._launches_per} (9 per layer), not per token")

    def _gemv(self, proj, x, su, scale, rms=None, **kw):
        """multi_gemv of one projection group on rotate(RMSNorm(x) * su) / scale: RMSNorm + rotation as ONE launch, then the plain GEMV
        launch"""
        xr = had.rotate(x, hadK=self.hidden_hadT, K=self.hidden_K, su=su, post_scale=1.0 / scale, rms=rms,
                        in_mode=had.IN_F32 if x.dtype == torch.float32 else had.IN_F16)
        return multi_gemv(proj, xr, oscale=scale, **kw)

    def _lora(self, i, group, x, out, in_mode, rms=None):
        """with a bank: the low-rank update of one projection group of layer i on the rows of x, added to out (one launch)"""
        if self.adapters is not None:
            g = self.adapters.group(i, group)
            lora.lora_apply(out, x, in_mode, rms, g.A, g.B, g.blk_off, g.blk_m, self.row_adapter[:x.shape[0]])

    def _layer(self, i, h32, a16, qkv32, ug32):
        """layer i on the rows of h32: the row buffers, or their first n rows"""
        layer = self.layers[i]
        att = layer.self_attn
        proj, wsc, blocks = att._qkv_layout()
        rms = (self.eps, layer.input_layernorm.weight)
        self._gemv(proj, h32, att.SU_qkv, att.scale, rms=rms, wscales=wsc, outs=list(qkv32.split([l.out_features for l in proj], dim=1)))
        self._lora(i, "qkv", h32, qkv32, had.IN_F32, rms)
        parts = dict(zip([b[0] for b in blocks], qkv32.split([b[1] for b in blocks], dim=1)))
        self._prep(i, parts["q"], parts["k"], parts["v"])  # behind the adapter's update, as the modules add their bias and norm
        self._attention(i, parts["q"], parts["k"], parts["v"], a16)
        y32 = self._sub_out(h32)
        self._gemv([att.o_proj], a16, att.SU_o, att.scale, wscales=[att.Wscale_o], outs=[y32], accumulate=y32 is h32)
        self._lora(i, "o", a16, y32, had.IN_F16)  # before up|gate reads the stream
        self._post_norm(i, 0, h32, y32)
        self._mlp(i, h32, ug32)

    def _sub_out(self, h32):
        """where a sublayer's last projection writes: ADDED into the stream, or with post_norms overwritten into the rows of the
        scratch that `_post_norm` then folds into the stream"""
        return h32 if self.post_norms is None else self.y32[:h32.shape[0]]

    def _post_norm(self, i, which, h32, y32):
        """with post_norms: h32 += RMSNorm(y32) * w[i, which] (0: behind the attention sublayer and its adapter, 1: behind the MLP's)"""
        if self.post_norms is not None:
            eps, w = self.post_norms
            blocks.norm_add(h32, y32, w[i, which], eps)

    def _moe_active(self):
        """the row-activity vector of the routed launches (int64, negative: the row chooses no expert) where a class holds one on
        the device, else None"""
        return None

    def _moe(self, i, h32):
        """a sparse layer on the rows of h32: the six launches of moe.MoEMLP.run (rotation with the norm, route, routed up | gate,
        SwiGLU rotation of the sorted rows, routed down, combine into the stream or the post-norm scratch); a layer of the second
        router routes through qpal_moe_route_ex and runs its shared expert in front of the one combine"""
        mlp, rms = self.layers[i].mlp, (self.eps, self.layers[i].post_attention_layernorm.weight)
        y32 = self._sub_out(h32)
        mlp.run(h32, rms, y32, y32 is h32, active=self._moe_active(), ws=self.moe_ws[mlp.shape_key()])
        self._post_norm(i, 1, h32, y32)

    def _mlp(self, i, h32, ug32):
        if self.moe[i]:
            return self._moe(i, h32)
        mlp, rms = self.layers[i].mlp, (self.eps, self.layers[i].post_attention_layernorm.weight)
        ugl, ugw = ug_layout(mlp)
        self._gemv(ugl, h32, mlp.SU_ug, mlp.scale, rms=rms, wscales=ugw, outs=list(ug32.split([l.out_features for l in ugl], dim=1)))
        self._lora(i, "ug", h32, ug32, had.IN_F32, rms)
        if self.gelu:  # GeGLU: the activation in fp32 rows of its own, which the rotation and the adapter read as they are
            act, act_mode = blocks.glu_gelu_tanh(ug32, out=self.act32[:ug32.shape[0]]), had.IN_F32
        else:
            act, act_mode = ug32, had.IN_SWIGLU_F32
        x = had.rotate(act, in_mode=act_mode, hadK=mlp.had_left_dp_T, K=mlp.inter_K, su=mlp.SU_dp, post_scale=1.0 / mlp.scale)
        y32 = self._sub_out(h32)
        multi_gemv([mlp.down_proj], x, outs=[y32], wscales=[mlp.Wscale_dp], oscale=mlp.scale, accumulate=y32 is h32)
        self._lora(i, "down", act, y32, act_mode)  # reads up | gate with their own update in
        self._post_norm(i, 1, h32, y32)

    def _run_layers(self, tokens, n=None):
        """the embedding rows of `tokens` through every layer, in the row buffers or (n: a short chunk) their first n rows; returns
        those rows of the residual stream"""
        bufs = (self.h32, self.a16, self.qkv32, self.ug32)
        if n is not None:
            bufs = tuple(t[:n] for t in bufs)
        bufs[0].copy_(self.embed[tokens])
        for i in range(len(self.layers)):
            self._layer(i, *bufs)
        return bufs[0]

    def _sample_tail(self, h32, smp, ctr, out_tok, row_slot=None, fed=None, gslot=None):
        """final norm + lm_head of every row of h32 into smp.logits, then one draw per row with the counters ctr: two launches; with
        smp.logprob a third, the log-probability of the tokens just drawn (rows with ctr < 0 drew nothing and keep theirs); with
        smp.top_id one more behind it, the likeliest tokens of every row that drew and their log-probabilities.  With a
        processor (row_slot: the rows' slots) two launches in between: the tokens `fed` to the rows are counted where given, and the
        logits are processed in place — the draw and the log-probabilities are those of the processed logits.  With a grammar two
        more: the mask of every row's automaton state behind the processor, and behind the draw the advance of the states by the
        drawn tokens (gslot None: row = slot, all of them; an int: the one row is that slot's).  With a stop bank built with min_tokens
        one more in front of the draw: the stop ids of the slots that are below their min_tokens become -inf"""
        sampling.lm_head_logits(h32, self.norm.weight, self.norm.eps, self.lm_head, out=smp.logits)
        self._cap_logits(smp.logits)
        if self.processor is not None:
            if fed is not None:
                logits.observe(self.processor, fed, row_slot, active=ctr)
            logits.process(smp.logits, self.processor, row_slot, ctr)
        if self.grammar is not None:
            state = self.grammar.state if gslot is None else self.grammar.state[gslot:gslot + 1]
            gram_mod.grammar_mask(smp.logits, self.grammar, row_slot, ctr, row_state=state)
        if self.stop is not None and self.stop.min_tokens_mask:
            stop_mod.stop_mask(smp.logits, self.stop, row_slot, ctr)
        sampling.sample(smp.logits, smp, ctr, out=out_tok)
        if self.grammar is not None:
            gram_mod.grammar_advance(self.grammar, out_tok, active=ctr, slot0=gslot or 0)
        if smp.logprob is not None:
            sampling.token_logprobs(smp.logits, out_tok, out=smp.logprob, active=ctr)
        if smp.top_id is not None:
            sampling.top_logprobs(smp.logits, smp.top_id.shape[1], ids=smp.top_id, logprob=smp.top_logprob, active=ctr)

    def _argmax_tail(self, rows32, out_tok):
        """final norm + lm_head + argmax of the rows: one launch (ONE row) where the class found the kernel available, else torch ops"""
        # (logit_cap needs nothing here: cap * tanh(l / cap) is monotone, the argmax of the capped logits is that of the plain ones)
        if self.lm_ws is None:
            out_tok.copy_((self.norm(rows32.half()) @ self.lm_head.T).argmax(-1))
            return
        dev = rows32.device
        with torch.cuda.device(dev):
            rc = nat.lib().qpal_lm_head_argmax(rows32.data_ptr(), self.norm.weight.data_ptr(), self.norm.eps, self.lm_head.data_ptr(),
                                               None, out_tok.data_ptr(), self.lm_ws.data_ptr(), self.lm_ws_bytes,
                                               self.lm_head.shape[0], rows32.shape[1], torch.cuda.current_stream(dev).cuda_stream)
        nat.check(rc, "qpal_lm_head_argmax")


class DecodeStep(_Rows):
    """layers: modules with self_attn (IncoherentSdpaAttention), mlp (IncoherentMLP), input_layernorm, post_attention_layernorm;
    embed / lm_head fp16 [vocab, H]; norm: the final RMSNorm; kcache / vcache: per-layer fp16 or float8_e4m3fn [B, nkv, context, hd]; inv_freq fp32
    [hd / 2]; tok, pos, out_tok int64 [B] (pos[b] outside the cache: sequence b is inactive).  The caller owns the caches and
    tok / pos / out_tok and may write them between replays of a captured step.  swiglu_epilogue, k28_fusion, native_lm_head,
    split_attention switch single fusions of the batch-1 step off (profiling).  qpal_lm_head_argmax serves the hidden widths
    2048, 4096 and 8192: on any other width the batch-1 step ends in the torch tail every larger batch has, as Prefill does.
    sampler: a sampling.Sampler of B slots — the tail becomes lm_head logits of all B rows + one draw per active row with the
    counter pos[b] (two launches); None: argmax.  A sampler
    built with logprobs=True adds a third launch: sampler.logprob[b] = the log-probability of out_tok[b] under the plain softmax of
    sampler.logits[b], for the rows that drew (pos[b] >= 0 — the positions are the launch's `active` vector; other slots keep theirs).
    A sampler built with top_logprobs=n adds one more behind it: sampler.top_id[b] / sampler.top_logprob[b] = the n likeliest tokens
    of sampler.logits[b] — the logits the draw saw — and their log-probabilities, for the same rows (sampling.top_logprobs).
    block_table: int32 [B, max_pages] on the device — kcache / vcache are then the per-layer page pools [num_pages, nkv, page_size, hd]
    of a paged cache, context = max_pages * page_size, and the attention launch is paged_decode_attention (a batch of one as well:
    the fused single-sequence kernel reads contiguous caches only).  shared_prefix: paging.SharedPrefix (cache.prefix, with block_table=
    cache.table) — the attention launch becomes shared_prefix_decode_attention, which reads a forked prefix once per group: one more
    launch per layer, everything else in the step is untouched; without block_table: QpalError.  The caller has reserved a page for every position the step, or
    a run of replays of the captured step, will write: the step reads the table on the device and never allocates.
    window: None, an int W >= 1 or one entry per layer — sequence b attends to positions max(0, pos[b] - W + 1) .. pos[b] in the
    layers that have one (decode_attention's window=); with one anywhere a batch of one launches the batched attention too, and
    shared_prefix with a window is a QpalError.  The step never trims: PagedKVCache.trim between replays is the caller's.
    softcap / sinks / attn_scale: the module's last paragraph (decode_attention's softcap= and sinks=, layer i reading sinks[i]);
    with either modifier a batch of one launches the batched attention, and shared_prefix with either is a QpalError.
    adapters: a lora.LoraBank of B slots — row b runs with adapter bank.slot_adapter[b], read by the launches themselves: four more
    launches per layer.  At batch 1 the interleaved up|gate epilogue and down_proj's staged rotation are then off (they never put
    up | gate into memory: the swiglu_epilogue=False step); RMSNorm and the rotation stay inside the GEMV staging.
    processor: a logits.LogitProcessor of B slots (needs a sampler).  The tail becomes lm_head logits, observe — every active row's
    fed token tok[b] is counted for slot b —, process in place on sampler.logits, the draw, then the log-probability launch of a
    sampler with logprobs: sampler.logits and sampler.logprob are then the PROCESSED logits and the log-probabilities under them.
    Two more launches.  The step counts every token it feeds, whatever the processor's count_prompt.
    grammar: a grammar.GrammarBank of B slots (needs a sampler; greedy is temperature 0).  Behind the processor every active row of
    a slot with a grammar is masked with the tokens its automaton state allows (bank.state[b], read by the launch), and behind the
    draw out_tok[b] advances that state, with the positions as the active vector: two more launches.  sampler.logits and
    sampler.logprob are then the MASKED logits and the log-probabilities under them.  The grammar sees generated tokens only.
    stop: a stop.StopBank of B slots.  The LAST launch of the step judges out_tok[b] of every slot with pos[b] inside
    the cache against the slot's stop ids, stop strings, max_tokens and the context, records it in the bank, and moves the step's own
    inputs: a slot that goes on gets tok[b] = out_tok[b], pos[b] += 1, a slot that is done pos[b] = -1 — it is inactive in every
    launch of the replays that follow, and its cache rows past bank.end_pos[b] are never written.  It runs behind the draw, the
    log-probability launches and the grammar's advance, which read pos as their active vector.  Works with the argmax tail and with
    a sampler: one more launch.  A bank built with min_tokens=True (needs a sampler) adds the mask launch behind the processor and
    the grammar mask, in front of the draw: two more.
    qkv_bias / qk_norm / mlp_act / post_norms / logit_cap, a per-layer inv_freq: the module's last paragraph.  At batch 1
    mlp_act="gelu_tanh" switches the interleaved up|gate epilogue and down_proj's staged rotation off, the way adapters do (both are
    built on silu(gate) * up in fp16); RMSNorm and the rotation stay inside the GEMV staging of q|k|v and up|gate, and qkv_prep works in
    front of the fused single-sequence attention kernel as in front of every other.  layers[i].post_attention_layernorm is the norm
    in FRONT of the MLP (Gemma: pre_feedforward_layernorm).
    Gemma's embedding scale needs no argument: embed and lm_head are separate.  Gemma multiplies the embedding row by fp16(sqrt(H)) and
    rounds to the activation dtype, so the caller passes embed = fp16(table * fp16(sqrt(H))) and lm_head = the unscaled table."""

    def __init__(self, layers, embed, norm, lm_head, kcache, vcache, inv_freq, tok, pos, out_tok, generic=False,
                 swiglu_epilogue=True, k28_fusion=True, native_lm_head=True, split_attention=True, sampler=None, block_table=None,
                 adapters=None, processor=None, grammar=None, shared_prefix=None, window=None, softcap=None, sinks=None,
                 attn_scale=None, stop=None,
                 qkv_bias=None, qk_norm=None, mlp_act="silu", post_norms=None, logit_cap=None):
        B = tok.shape[0]
        if shared_prefix is not None and block_table is None:
            raise nat.QpalError("DecodeStep: shared_prefix needs a paged cache (block_table=cache.table)")
        if shared_prefix is not None and any(w is not None for w in self._check_window("DecodeStep", window, len(layers))):
            raise nat.QpalError("DecodeStep: no sliding window in the shared-prefix launches (shared_prefix with window)")
        if shared_prefix is not None and (softcap is not None or sinks is not None):
            raise nat.QpalError("DecodeStep: no soft cap and no sinks in the shared-prefix launches (shared_prefix with softcap / sinks)")
        self.batch1 = B == 1 and not generic
        super().__init__("DecodeStep", layers, embed, norm, lm_head, kcache, vcache, inv_freq, B, sampler, block_table, slots=B,
                         native_argmax=self.batch1 and native_lm_head and self._has_argmax_kernel(embed, lm_head), adapters=adapters,
                         processor=processor, grammar=grammar, window=window, softcap=softcap, sinks=sinks, attn_scale=attn_scale,
                         stop=stop,
                         qkv_bias=qkv_bias, qk_norm=qk_norm, mlp_act=mlp_act, post_norms=post_norms, logit_cap=logit_cap)
        masked = processor is not None or grammar is not None or (stop is not None and stop.min_tokens_mask)
        self._row_slot = torch.arange(B, dtype=torch.int32, device=embed.device) if masked else None  # row = slot
        if adapters is not None:
            self.row_adapter, swiglu_epilogue = adapters.slot_adapter, False  # row = slot
        if self.gelu:
            swiglu_epilogue = False  # the interleaved epilogue is silu(gate) * up: GeGLU runs the plain up|gate launch, as adapters do
        if self.batch1 and not fusable(layers):
            raise nat.QpalError("DecodeStep: these layers have no batch-1 step (fusable(layers))")
        self.tok, self.pos, self.out_tok = tok, pos, out_tok
        dev = embed.device
        self.rot_in_gemv = self.batch1 and ops.can_fuse_rotation(1, self.h32.shape[1])  # k in {2048, 4096}: the GEMV staging rotates x
        self.ug_il = None
        if self.rot_in_gemv and swiglu_epilogue:
            # up | gate as ONE layer with interleaved supertile rows: the launch's epilogue writes fp16 silu(gate) * up itself
            self.act16 = torch.zeros(1, self.ug32.shape[1] // 2, dtype=torch.float16, device=dev)
            self.ug_il = []
            for m in (l.mlp for l in layers):
                if isinstance(m, MoEMLP):
                    self.ug_il.append(None)  # (a sparse layer: _moe)
                    continue
                il = linear.interleave_up_gate(m.ug_proj, None) if m.merge_ug else linear.interleave_up_gate(m.up_proj, m.gate_proj)
                linear.share_codebooks([il, m.down_proj] + ug_layout(m)[0])
                inter = m.intermediate_size
                self.ug_il.append((il, linear.interleave_rows(m.Wscale_ug[:inter], m.Wscale_ug[inter:]),
                                   k28_fusion and k28_in_gemv(m)))
        # the fused single-sequence attention kernel reads contiguous fp16 caches only: on float8_e4m3fn or paged caches the batch-1
        # step keeps its GEMV fusions and launches the batched attention at B = 1 (same launch count); it has no
        # window either, no soft cap and no sinks: a step with one of them in any layer does the same
        self.attn_batch = (not self.batch1 or kcache[0].dtype != torch.float16 or block_table is not None
                           or any(w is not None for w in self.window) or any(c is not None for c in self.softcap)
                           or self.sinks is not None)
        self.shared_prefix = shared_prefix
        if shared_prefix is not None:
            self.attn_ws = shared_prefix_workspace(B, shared_prefix.G, self.nq, self.nkv, self.head_dim, self.context, dev)
        elif self.attn_batch:
            self.attn_ws = attention_workspace(B, self.nq, self.nkv, self.head_dim, self.context, dev)
        else:
            # long caches: split-context attention (one workspace serves every layer: launches are stream-ordered)
            self.attn_ws_bytes = nat.lib().qpal_attn_ws_bytes(self.nq, self.nkv, self.head_dim, self.context) if split_attention else 0
            self.attn_ws = torch.zeros(max(self.attn_ws_bytes, 4) // 4, dtype=torch.float32, device=dev)

    @property
    def launches_per_token(self):
        """kernel launches of one step: per layer q|k|v, attention, o, up|gate, SwiGLU rotation, down (+ a rotation in front of
        q|k|v, o and up|gate where the GEMV cannot rotate; - the SwiGLU rotation where down_proj's staging runs it); + the norm /
        lm_head / argmax launch, or the lm_head logits and the draw with a sampler, + the log-probability launch of a sampler with
        logprobs, + the top-N launch of a sampler with top_logprobs (the embedding row copy is a memcpy node); with adapters + 4
        per layer, one per projection group; with a
        processor + 2, observe and process; with a grammar + 2, mask and advance; with shared_prefix + 1 per layer, the prefix
        phase in front of the attention launch; with stop + 1, the stop launch that ends the step, + 2 with a bank built with
        min_tokens=True, whose mask launch sits in front of the draw; with qkv_bias or qk_norm (one launch for both) + 1 per layer,
        with post_norms + 2 per layer, with mlp_act="gelu_tanh" + 1 per layer (the activation; the rotation behind it is the SwiGLU
        rotation's launch), with logit_cap + 1 behind a sampler's lm_head (an argmax tail needs none)"""
        dense_il = [e for e in (self.ug_il or []) if e is not None]
        mlp_dense = (2 if dense_il and dense_il[0][2] else 3) if self.rot_in_gemv else 4
        per_layer = (3 if self.rot_in_gemv else 5) + mlp_dense
        block_layer, block_tail = _Rows._block_launches(self)
        per_layer += block_layer
        per_layer += 1 if getattr(self, "shared_prefix", None) is not None else 0
        per_layer += 4 if getattr(self, "adapters", None) is not None else 0  # (arithmetic on the configuration: stand-ins may lack it)
        tail = 1 if self.sampler is None else (2 if self.sampler.logprob is None else 3)
        tail += 1 if getattr(self.sampler, "top_id", None) is not None else 0
        tail += 2 if getattr(self, "processor", None) is not None else 0
        tail += 2 if getattr(self, "grammar", None) is not None else 0
        stop = getattr(self, "stop", None)
        tail += 0 if stop is None else (2 if stop.min_tokens_mask else 1)
        # a sparse layer: its routed launches (six; more with a shared expert: MoEMLP.launches) in place of the dense MLP's
        sparse = sum(l.mlp.launches(self.h32.shape[0]) - mlp_dense for l, s in zip(self.layers, getattr(self, "moe", ())) if s)
        return per_layer * len(self.layers) + sparse + tail + block_tail

    def _gemv(self, proj, x, su, scale, rms=None, **kw):
        """batch 1, k in {2048, 4096}: RMSNorm + rotation inside the GEMV launch; else (70B: 8192, every batch > 1) the launch pair"""
        if self.rot_in_gemv:
            return multi_gemv(proj, x, oscale=scale, x_rot=(su, 1.0 / scale), x_rms=rms, **kw)
        return super()._gemv(proj, x, su, scale, rms=rms, **kw)

    def _attention(self, i, q, k, v, out):
        kc, vc = self.kcache[i], self.vcache[i]
        if not self.attn_batch:  # one sequence on contiguous fp16 caches: the fused kernel
            dev = out.device
            with torch.cuda.device(dev):
                rc = nat.lib().qpal_attn_rope_decode(q.data_ptr(), k.data_ptr(), v.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(),
                                                     self.pos.data_ptr(), self._inv_freq(i).data_ptr(), self.nq, self.nkv, self.head_dim,
                                                     self.context, self.attn_scale, self.attn_ws.data_ptr() if self.attn_ws_bytes else None,
                                                     self.attn_ws_bytes, torch.cuda.current_stream(dev).cuda_stream)
            return nat.check(rc, "qpal_attn_rope_decode")
        if self.shared_prefix is not None:
            return shared_prefix_decode_attention(q, k, v, kc, vc, self.block_table, self.pos, self._inv_freq(i), self.shared_prefix,
                                                  scale=self.attn_scale, out=out, ws=self.attn_ws)
        if self.block_table is None:
            attend, cache = decode_attention, (kc, vc)
        else:
            attend, cache = paged_decode_attention, (kc, vc, self.block_table)
        attend(q, k, v, *cache, self.pos, self._inv_freq(i), scale=self.attn_scale, out=out, ws=self.attn_ws, **self._score(i))

    def _moe_active(self):
        return self.pos  # an idle slot (pos < 0) routes nothing

    def _mlp(self, i, h32, ug32):
        if not self.ug_il or self.ug_il[i] is None:
            return super()._mlp(i, h32, ug32)
        mlp, rms = self.layers[i].mlp, (self.eps, self.layers[i].post_attention_layernorm.weight)
        il, il_w, fuse28 = self.ug_il[i]
        # with the fused rotation the gate|up epilogue also applies down_proj's sign vector (a sign flip: exact), so the rotation
        # inside every down_proj workgroup reads one 28 KiB vector instead of two
        self._gemv([il], h32, mlp.SU_ug, mlp.scale, rms=rms, wscales=[il_w], act_out=self.act16, act_su=mlp.SU_dp if fuse28 else None)
        if fuse28:  # the 28 x 512 rotation inside down_proj's x staging (csrc/rot_k28.h): no launch of its own
            x, x_rot = self.act16, (None, 1.0 / mlp.scale, mlp.had_left_dp_T, mlp.inter_K)
        else:
            x, x_rot = had.rotate(self.act16, hadK=mlp.had_left_dp_T, K=mlp.inter_K, su=mlp.SU_dp, post_scale=1.0 / mlp.scale), None
        y32 = self._sub_out(h32)
        multi_gemv([mlp.down_proj], x, outs=[y32], wscales=[mlp.Wscale_dp], oscale=mlp.scale, x_rot=x_rot, accumulate=y32 is h32)
        self._post_norm(i, 1, h32, y32)

    def hidden(self):
        """fp16 [B, H]: the final norm of the residual stream the last step left (a torch op: for checks, not part of the step)"""
        return self.norm(self.h32.half())

    def __call__(self):
        self._run_layers(self.tok)
        if self.sampler is not None:
            self._sample_tail(self.h32, self.sampler, self.pos, self.out_tok, row_slot=self._row_slot, fed=self.tok)
        else:
            self._argmax_tail(self.h32, self.out_tok)
        if self.stop is not None:  # the last launch: everything in front of it has read pos as its active vector
            stop_mod.stop_advance(self.stop, self.out_tok, self.context, tok=self.tok, pos=self.pos)


class Prefill(_Rows):
    """A prompt into ONE slot of the caches a DecodeStep is built on (per-layer fp16 or float8_e4m3fn [B, nkv, context, hd]): chunks of at most
    `chunk` <= 128 rows, each through DecodeStep's batch-B layer with rows = consecutive positions and `prefill_attention` on
    kcache[i][slot] / vcache[i][slot] (rotary embedding at pos0 + row, rows appended, causal); final norm, lm_head and argmax for
    the LAST row only.  Other slots are not touched.  The position lives on the device and the chunk loop advances it there: no
    host synchronisation inside the call.

        next_tok = pf(tokens, slot=0, pos0=0)   # tokens int64 [N] on the device, N >= 1; returns int64 [1]

    pos0 as a Python int is checked on the host (N + pos0 > context: QpalError); as a device tensor it is not read by the host,
    and a prompt that does not fit leaves caches untouched from the first chunk that crosses the end (the kernel's rule).

    sampler: the sampling.Sampler of the DecodeStep whose caches this fills (one slot per sequence of the caches).  The token is then
    drawn with slot `slot`'s parameters and the counter of the last prompt row's position, pos0 + N - 1 (computed on the device):
    the counter a DecodeStep would have used had it fed that token.  sampler.logits[slot] holds the logits, and with a sampler
    built with logprobs=True sampler.logprob[slot] the token's log-probability, with top_logprobs=n sampler.top_id[slot] /
    sampler.top_logprob[slot] the n likeliest tokens of those logits (one more launch each).

    block_table: int32 [B, max_pages] — kcache / vcache are the per-layer page pools of a paged cache, the slot's row block_table[slot]
    addresses them (paged_prefill_attention), context = max_pages * page_size.  The caller has reserved pages for positions pos0 ..
    pos0 + N - 1 of the slot (PagedKVCache.reserve(slot, pos0 + N)) before the call.

    adapters: a lora.LoraBank of the caches' slots — every row of the call runs with bank.slot_adapter[slot], copied on the device.

    processor: the logits.LogitProcessor of that DecodeStep (needs a sampler).  With processor.count_prompt the tokens of the call
    are counted for the slot, chunk by chunk (one observe launch each); the last row's logits are processed with the slot's state
    before the draw.  The counts are not reset: a new request calls processor.reset(slot) first.

    grammar: the grammar.GrammarBank of that DecodeStep (needs a sampler).  The prompt is not walked: the last row's logits are
    masked with the slot's state as it stands (bank.set / reset put it at the start) and the drawn token advances it.

    window: as for DecodeStep (prefill_attention's window=): the row at position p attends to positions max(0, p - W + 1) .. p; the
    caches end up byte for byte as without a window.  softcap / sinks / attn_scale: as for DecodeStep (prefill_attention's)."""

    _launches_per = "Prefill: launches are per chunk"

    def __init__(self, layers, embed, norm, lm_head, kcache, vcache, inv_freq, chunk=128, native_lm_head=True, sampler=None,
                 block_table=None, adapters=None, processor=None, grammar=None, window=None, softcap=None, sinks=None,
                 attn_scale=None,
                 qkv_bias=None, qk_norm=None, mlp_act="silu", post_norms=None, logit_cap=None):
        if not 1 <= int(chunk) <= 128:
            raise nat.QpalError(f"Prefill: chunk must be in 1 .. 128, got {chunk}")
        self.chunk = int(chunk)
        dev, H = embed.device, embed.shape[1]
        super().__init__("Prefill", layers, embed, norm, lm_head, kcache, vcache, inv_freq, self.chunk, sampler, block_table,
                         native_argmax=native_lm_head and self._has_argmax_kernel(embed, lm_head), adapters=adapters,
                         processor=processor, grammar=grammar, window=window, softcap=softcap, sinks=sinks, attn_scale=attn_scale,
                         qkv_bias=qkv_bias, qk_norm=qk_norm, mlp_act=mlp_act, post_norms=post_norms, logit_cap=logit_cap)
        self._row_slot = None if processor is None and grammar is None else torch.zeros(1, dtype=torch.int32, device=dev)  # the call's slot
        self.pos = torch.zeros(1, dtype=torch.int64, device=dev)
        self.out_tok = torch.zeros(1, dtype=torch.int64, device=dev)
        self.ctr = torch.zeros(1, dtype=torch.int64, device=dev)  # with a sampler: the last prompt row's position
        self.last32 = torch.zeros(1, H, dtype=torch.float32, device=dev)  # the last prompt row of the residual stream
        self.slot = 0
        self.attn_ws = prefill_workspace(self.chunk, self.nq, self.nkv, self.head_dim, self.context, dev)

    def _attention(self, i, q, k, v, out):
        kc, vc = self.kcache[i], self.vcache[i]
        if self.block_table is None:
            attend, cache = prefill_attention, (kc[self.slot], vc[self.slot])
        else:
            attend, cache = paged_prefill_attention, (kc, vc, self.block_table[self.slot])
        attend(q, k, v, *cache, self.pos, self._inv_freq(i), scale=self.attn_scale, out=out, ws=self.attn_ws, **self._score(i))

    def hidden(self):
        """fp16 [1, H]: the final norm of the last prompt row"""
        return self.norm(self.last32.half())

    def _begin(self, tokens, slot, pos0, least=1):
        """the argument checks of a call; sets self.slot and the device position; returns N"""
        who = type(self).__name__
        if tokens.dim() != 1 or tokens.shape[0] < least or tokens.dtype != torch.int64 or tokens.device != self.embed.device:
            raise nat.QpalError(f"{who}: tokens must be int64 [N >= {least}] on {self.embed.device}")
        N = tokens.shape[0]
        if not 0 <= int(slot) < self.slots:
            raise nat.QpalError(f"{who}: slot {slot} outside the caches' {self.slots} sequences")
        self.slot = int(slot)
        if self._row_slot is not None:
            self._row_slot.fill_(self.slot)
        if self.adapters is not None:
            self.row_adapter.copy_(self.adapters.slot_adapter[self.slot:self.slot + 1].expand(self.chunk))
        if isinstance(pos0, torch.Tensor):
            self.pos.copy_(pos0.reshape(1))
        else:
            if pos0 < 0 or N + pos0 > self.context:
                raise nat.QpalError(f"{who}: {N} tokens from position {pos0} do not fit a cache of {self.context} positions")
            self.pos.fill_(int(pos0))
        return N

    def _chunks(self, tokens, N):
        """runs the layers chunk by chunk; yields (c, h32) after chunk tokens[c : c + n], h32 its n rows of the residual stream"""
        for c in range(0, N, self.chunk):
            n = min(self.chunk, N - c)
            h32 = self._run_layers(tokens[c:c + n], n)
            if self.processor is not None and self.processor.count_prompt:
                logits.observe(self.processor, tokens[c:c + n], self.slot)
            self.pos += n
            yield c, h32
        self.last32.copy_(h32[n - 1:n])

    def __call__(self, tokens, slot=0, pos0=0):
        N = self._begin(tokens, slot, pos0)
        for _ in self._chunks(tokens, N):
            pass
        if self.sampler is not None:
            torch.sub(self.pos, 1, out=self.ctr)
            self._sample_tail(self.last32, self.sampler.slot(self.slot), self.ctr, self.out_tok, row_slot=self._row_slot, gslot=self.slot)
        else:
            self._argmax_tail(self.last32, self.out_tok)
        return self.out_tok


class Score(Prefill):
    """The log-probability of every next token of a sequence: Prefill's chunks (same caches, chunking, slot / pos0 rules and errors),
    each followed by `qpal_lm_head_logits` on ALL rows of the chunk and `qpal_token_logprob` against the tokens that follow them.

        sc = Score(layers, embed, norm, lm_head, kcache, vcache, inv_freq, chunk=128)
        lp = sc(tokens, slot=0, pos0=0)     # tokens int64 [N >= 2] on the device -> fp32 [N - 1]
        # lp[t] = log p(tokens[t + 1] | the cache below pos0, tokens[0 .. t]); sc.rank int32 [N - 1]: tokens more likely than it

    The logits live in ONE fp32 [chunk, vocab] buffer (sc.logits: the last chunk's n rows); lp and sc.rank are views of buffers of
    max_tokens entries (default: the caches' context) that the next call overwrites.  No host synchronisation inside the call.  The
    last row has no next token: its logits are computed, its row of the log-prob launch is inactive.  The slot is left as Prefill
    leaves it: a DecodeStep can continue at position pos0 + N.  The lm_head must suit qpal_lm_head_logits (a sampler's demands).
    block_table: as for Prefill (a paged cache; the caller reserves the slot's pages for pos0 .. pos0 + N - 1).  adapters: as for
    Prefill.  top_logprobs=n (1 .. 64): one `qpal_top_logprob` launch more per chunk; sc.top_id int32 / sc.top_logprob fp32 [N - 1, n]
    are then the n likeliest tokens at every scored position and their log-probabilities (views of max_tokens x n buffers, like lp).
    window, softcap, sinks, attn_scale: as for Prefill — the log-probabilities are those of the model with that attention."""

    def __init__(self, layers, embed, norm, lm_head, kcache, vcache, inv_freq, chunk=128, max_tokens=None, block_table=None,
                 adapters=None, top_logprobs=0, window=None, softcap=None, sinks=None, attn_scale=None,
                 qkv_bias=None, qk_norm=None, mlp_act="silu", post_norms=None, logit_cap=None):
        self._check_lm_head("Score", embed, lm_head)
        super().__init__(layers, embed, norm, lm_head, kcache, vcache, inv_freq, chunk=chunk, native_lm_head=False,
                         block_table=block_table, adapters=adapters, window=window, softcap=softcap, sinks=sinks,
                         attn_scale=attn_scale,
                         qkv_bias=qkv_bias, qk_norm=qk_norm, mlp_act=mlp_act, post_norms=post_norms, logit_cap=logit_cap)
        self.max_tokens = self.context if max_tokens is None else int(max_tokens)
        if self.max_tokens < 2:
            raise nat.QpalError(f"Score: max_tokens must be at least 2, got {max_tokens}")
        dev = embed.device
        self._logits = torch.zeros(self.chunk, lm_head.shape[0], dtype=torch.float32, device=dev)
        self._targets = torch.zeros(self.max_tokens, dtype=torch.int64, device=dev)  # tokens[1:], then -1: the row without a target
        self._lp = torch.zeros(self.max_tokens, dtype=torch.float32, device=dev)
        self._rank = torch.zeros(self.max_tokens, dtype=torch.int32, device=dev)
        self.logits, self.rank = self._logits[:0], self._rank[:0]
        self.top_n = int(top_logprobs or 0)
        if not 0 <= self.top_n <= 64:
            raise nat.QpalError(f"Score: top_logprobs must be in 0 .. 64, got {top_logprobs}")
        self.top_id = self.top_logprob = None
        if self.top_n:
            self._top_id = torch.full((self.max_tokens, self.top_n), -1, dtype=torch.int32, device=dev)
            self._top_logprob = torch.full((self.max_tokens, self.top_n), float("-inf"), dtype=torch.float32, device=dev)
            self.top_id, self.top_logprob = self._top_id[:0], self._top_logprob[:0]

    def __call__(self, tokens, slot=0, pos0=0):
        N = self._begin(tokens, slot, pos0, least=2)
        if N > self.max_tokens:
            raise nat.QpalError(f"Score: {N} tokens, built for max_tokens = {self.max_tokens}")
        self._targets[:N - 1].copy_(tokens[1:])
        self._targets[N - 1:N].fill_(-1)
        for c, h32 in self._chunks(tokens, N):
            n = h32.shape[0]
            self.logits = self._logits[:n]
            sampling.lm_head_logits(h32, self.norm.weight, self.norm.eps, self.lm_head, out=self.logits)
            self._cap_logits(self.logits)
            sampling.token_logprobs(self.logits, self._targets[c:c + n], out=self._lp[c:c + n], rank=self._rank[c:c + n])
            if self.top_n:  # (the row without a target is inactive here as well)
                sampling.top_logprobs(self.logits, self.top_n, ids=self._top_id[c:c + n], logprob=self._top_logprob[c:c + n],
                                      active=self._targets[c:c + n])
        self.rank = self._rank[:N - 1]
        if self.top_n:
            self.top_id, self.top_logprob = self._top_id[:N - 1], self._top_logprob[:N - 1]
        return self._lp[:N - 1]

    def nll(self, tokens, slot=0, pos0=0):
        """device scalar (fp64): the mean of -lp over the N - 1 predicted tokens — the cross-entropy loss of one window"""
        return -self(tokens, slot=slot, pos0=pos0).double().mean()


class RaggedStep(_Rows):
    """ONE step on `rows` <= 128 rows that belong to up to `segments` <= 128 slots of the caches a DecodeStep is built on: segment s
    is rows row0[s] .. row0[s + 1] - 1, the tokens of slot seq[s] at positions pos0[s] .. (a prompt chunk; one row: a decode token).
    DecodeStep's batch-B layer on all rows with `ragged_prefill_attention` in the attention's place, then per segment the final
    norm and lm_head of its LAST row and one draw.

        out_tok = rs(tokens, seq, row0, pos0)   # tokens int64 [rows], seq int32 [segments], row0 int32 [segments + 1], pos0 int64
                                                # [segments], all on the device; returns rs.out_tok int64 [segments]

    Nothing in a call reads the device or synchronises: it can be captured, and the four tensors rewritten between replays.  The
    segment rules are ragged_prefill_attention's; an inactive segment keeps its out_tok.  Rows that belong to no segment are
    computed by the linears and ignored: their tokens must be valid ids.  Two active segments of one slot are the caller's error.

    sampler: the sampling.Sampler of the caches' slots; segment s draws with slot seq[s]'s parameters (gathered on the device into
    rs.draw, a Sampler of `segments` rows the step owns) and the counter of its last row's position, pos0[s] + rows of s - 1 —
    the draw Prefill or DecodeStep would have made.  None: argmax.  rs.draw.logits [segments, vocab] holds the logits, and with a
    sampler built with logprobs=True rs.draw.logprob the drawn tokens' log-probabilities, with top_logprobs=n rs.draw.top_id /
    rs.draw.top_logprob [segments, n] the n likeliest tokens per segment (an inactive segment keeps its list).

    block_table: int32 [B, max_pages] — a paged cache, as for DecodeStep; the caller has reserved the pages of every position the
    step writes.

    adapters: a lora.LoraBank of the caches' slots — a row of segment s runs with bank.slot_adapter[seq[s]], rows of no segment
    with none; the map row -> segment -> slot -> adapter is made on the device in every call.

    processor: not on a RaggedStep (QpalError): a prompt chunk's rows would have to be counted row by row; SpeculativeStep has one.
    grammar: not on a RaggedStep either (QpalError); DecodeStep, Prefill and SpeculativeStep take one.
    stop: not on a RaggedStep (a prompt chunk generates nothing to judge); DecodeStep and SpeculativeStep take one.
    window: as for DecodeStep (ragged_prefill_attention's window=), per segment what Prefill does with it.
    softcap / sinks / attn_scale: as for DecodeStep."""

    _launches_per = "RaggedStep: launches are per step"

    def __init__(self, layers, embed, norm, lm_head, kcache, vcache, inv_freq, rows=128, segments=16, sampler=None, block_table=None,
                 adapters=None, processor=None, grammar=None, window=None, softcap=None, sinks=None, attn_scale=None, stop=None,
                 qkv_bias=None, qk_norm=None, mlp_act="silu", post_norms=None, logit_cap=None):
        who = type(self).__name__
        if stop is not None and not isinstance(self, SpeculativeStep):
            raise nat.QpalError("RaggedStep: no stop bank on a ragged step (DecodeStep and SpeculativeStep take one)")
        if processor is not None and not isinstance(self, SpeculativeStep):
            raise nat.QpalError("RaggedStep: no processor on a ragged step (DecodeStep, Prefill and SpeculativeStep take one)")
        if grammar is not None and not isinstance(self, SpeculativeStep):
            raise nat.QpalError("RaggedStep: no grammar on a ragged step (DecodeStep, Prefill and SpeculativeStep take one)")
        if not 1 <= int(rows) <= 128 or not 1 <= int(segments) <= 128:
            raise nat.QpalError(f"{who}: rows and segments must be in 1 .. 128, got {rows}, {segments}")
        self.rows, self.segments = int(rows), int(segments)
        super().__init__(who, layers, embed, norm, lm_head, kcache, vcache, inv_freq, self.rows, sampler, block_table, logits_tail=True,
                         adapters=adapters, processor=processor, grammar=grammar, window=window, softcap=softcap, sinks=sinks,
                         attn_scale=attn_scale, stop=stop,
                         qkv_bias=qkv_bias, qk_norm=qk_norm, mlp_act=mlp_act, post_norms=post_norms, logit_cap=logit_cap)
        dev = embed.device
        self._row_id = torch.arange(self.rows, dtype=torch.int32, device=dev)
        self._no_adapter = torch.full((self.rows,), -1, dtype=torch.int32, device=dev)
        self.seq = self.row0 = self.pos0 = None  # the descriptors of the call under way
        self.attn_ws = ragged_workspace(self.rows, self.segments, self.nq, self.nkv, self.head_dim, self.context, dev)
        top_n = 0 if sampler is None or sampler.top_id is None else sampler.top_id.shape[1]
        self._setup_tail(lm_head.shape[0], dev, sampler is not None and sampler.logprob is not None, top_n)

    def _setup_tail(self, vocab, dev, logprobs, top_n):
        """what the tail of the step owns: per SEGMENT its last row of the stream, that row's counter, a draw and a token"""
        S = self.segments
        self.out_tok = torch.zeros(S, dtype=torch.int64, device=dev)
        self.ctr = torch.full((S,), -1, dtype=torch.int64, device=dev)  # the last row's position; -1: the segment is inactive
        self._inactive = torch.full((S,), -1, dtype=torch.int64, device=dev)
        self.last32 = torch.zeros(S, self.h32.shape[1], dtype=torch.float32, device=dev)  # each segment's last row of the stream
        # the draw's per-segment parameters: greedy, or gathered from the sampler's slots seq[s] in every call
        self.draw = sampling.Sampler(S, vocab, dev, temperature=0.0, logprobs=logprobs, top_logprobs=top_n, truncation=self._truncating())

    def _attention(self, i, q, k, v, out):
        kc, vc = self.kcache[i], self.vcache[i]
        if self.block_table is None:
            attend, cache = ragged_prefill_attention, (kc, vc)
        else:
            attend, cache = paged_ragged_prefill_attention, (kc, vc, self.block_table)
        attend(q, k, v, *cache, self.seq, self.row0, self.pos0, self._inv_freq(i), scale=self.attn_scale, out=out, ws=self.attn_ws,
               **self._score(i))

    def _map_rows(self, seq, row0):
        """with a bank: self.row_adapter[r] = the adapter of the slot whose segment holds row r, -1 for rows of no segment or of a
        segment without a valid slot; torch ops on the device, no synchronisation"""
        if self.adapters is None:
            return
        S = self.segments
        seg = torch.searchsorted(row0[1:], self._row_id, right=True).clamp(max=S - 1)  # the segments that end at or before r
        slot = seq[seg]
        held = (self._row_id >= row0[seg]) & (self._row_id < row0[seg + 1]) & (slot >= 0) & (slot < self.slots)
        torch.where(held, self.adapters.slot_adapter[slot.clamp(0, self.slots - 1).to(torch.int64)], self._no_adapter, out=self.row_adapter)

    def _truncating(self):
        """the sampler carries min_p / top_a / typical_p: self.draw does too, and the draw is qpal_sample_trunc"""
        return self.sampler is not None and self.sampler.min_p is not None

    def _gather_draw(self, slot):
        """the sampler's parameters of the slots `slot` (int64, one per row of self.draw) into self.draw, on the device"""
        for name in ("temperature", "top_k", "top_p", "seed") + (sampling.TRUNCATION if self._truncating() else ()):
            torch.index_select(getattr(self.sampler, name), 0, slot, out=getattr(self.draw, name))

    def hidden(self):
        """fp16 [segments, H]: the final norm of each segment's last row (rows of inactive segments mean nothing)"""
        return self.norm(self.last32.half())

    @staticmethod
    def pack_host(items, rows, segments, slots, context):
        """pack's checks and layout on the host: (tokens int64 [rows], seq int32 [segments], row0 int32 [segments + 1], pos0 int64
        [segments]) as CPU tensors.  Unused rows hold token 0; unused segments have no rows and seq = -1."""
        if len(items) > segments:
            raise nat.QpalError(f"RaggedStep.pack: {len(items)} items, built for {segments} segments")
        tokens = torch.zeros(rows, dtype=torch.int64)
        seq = torch.full((segments,), -1, dtype=torch.int32)
        row0 = torch.zeros(segments + 1, dtype=torch.int32)
        pos0 = torch.zeros(segments, dtype=torch.int64)
        at, seen = 0, set()
        for s, (slot, toks, p0) in enumerate(items):
            slot, p0 = int(slot), int(p0)
            if toks.dim() != 1 or toks.shape[0] < 1 or toks.dtype != torch.int64:
                raise nat.QpalError(f"RaggedStep.pack: item {s}: tokens must be int64 [n >= 1]")
            n = toks.shape[0]
            if not 0 <= slot < slots or slot in seen:
                raise nat.QpalError(f"RaggedStep.pack: item {s}: slot {slot} is outside the caches' {slots} sequences or named twice")
            if p0 < 0 or p0 + n > context:
                raise nat.QpalError(f"RaggedStep.pack: item {s}: {n} tokens from position {p0} do not fit a cache of {context} positions")
            if at + n > rows:
                raise nat.QpalError(f"RaggedStep.pack: {at + n} rows and more, built for {rows}")
            seen.add(slot)
            tokens[at:at + n] = toks.cpu()
            seq[s], pos0[s] = slot, p0
            at += n
            row0[s + 1] = at
        row0[len(items) + 1:] = at
        return tokens, seq, row0, pos0

    def pack(self, items):
        """[(slot, tokens int64 [n], pos0), ...] -> (tokens, seq, row0, pos0) on the device, padded to rows / segments: the arguments
        of a call.  Checked on the host: distinct slots of the caches, at most `segments` items and `rows` rows, every item inside
        the cache.  A host convenience (it copies to the device): not part of a captured step."""
        return tuple(t.to(self.embed.device) for t in self.pack_host(items, self.rows, self.segments, self.slots, self.context))

    def __call__(self, tokens, seq, row0, pos0):
        dev, S = self.embed.device, self.segments
        for name, t, dtype, n in (("tokens", tokens, torch.int64, self.rows), ("seq", seq, torch.int32, S),
                                  ("row0", row0, torch.int32, S + 1), ("pos0", pos0, torch.int64, S)):
            if t.dtype != dtype or t.shape != (n,) or t.device != dev or not t.is_contiguous():
                raise nat.QpalError(f"RaggedStep: {name} must be a contiguous {dtype} [{n}] tensor on {dev}")
        self.seq, self.row0, self.pos0 = seq, row0, pos0
        self._map_rows(seq, row0)
        self._run_layers(tokens)
        # ---- the tail, on the device: which segments are active (the kernel's rules), their last rows and counters
        first, end = row0[:-1], row0[1:]
        n = (end - first).to(torch.int64)
        active = (first >= 0) & (n > 0) & (end <= self.rows) & (seq >= 0) & (seq < self.slots) & (pos0 >= 0) & (pos0 + n <= self.context)
        torch.where(active, pos0 + n - 1, self._inactive, out=self.ctr)
        torch.index_select(self.h32, 0, (end.to(torch.int64) - 1).clamp(0, self.rows - 1), out=self.last32)
        if self.sampler is not None:
            self._gather_draw(seq.to(torch.int64).clamp(0, self.slots - 1))
        self._sample_tail(self.last32, self.draw, self.ctr, self.out_tok)
        return self.out_tok


class SpeculativeStep(RaggedStep):
    """ONE step that can emit several tokens per slot: slot b feeds its pending token and up to `draft` guessed
    tokens as one segment of a ragged step, every row draws the token the model would have drawn at its position, and the guesses
    that equal the draws are kept — the first draw that differs is the correction, the draw after a fully accepted draft the bonus.
    The stream of a slot is token for token what DecodeStep sampling emits on the same logits, greedy or seeded.

        ss = SpeculativeStep(layers, embed, norm, lm_head, kcache, vcache, inv_freq, draft=4, gram=(2, 4))
        ss.begin(slot, tokens, limit=len(tokens) + 64, eos=2)   # tokens[:-1] are in the cache (Prefill / RaggedStep); the last is pending
        out_tok, n_out = ss()                                    # int64 [B, draft + 1], int32 [B]: out_tok[b, :n_out[b]] are new
        out_tok, n_out = ss(ext_draft, ext_n)                    # the caller's drafts (int64 [B, draft], int32 [B]) instead of lookup

    Without arguments the drafts are prompt lookup: the tokens that followed the most recent earlier occurrence of the last gram[1]
    (down to gram[0]) tokens.  The step owns the state — hist int32 [B, history], n_tok / limit / eos int64 [B] — and ss.n_acc int32
    [B], the accepted drafts of the last call.  A slot with n_tok >= limit (finished, released, never begun) has no rows.  Nothing
    in a call reads the device: it can be captured, and `begin` / `release` (host conveniences, not part of a captured step) may
    run between replays.

    rows: the step's rows, B <= rows <= 128 (default min(128, B * (draft + 1))); drafts are cut where the rows are full.  sampler:
    the sampling.Sampler of the caches' slots — row r draws with its slot's parameters (gathered into ss.draw, a Sampler of `rows`
    rows) and the counter of its position; None: greedy.  A sampler built with logprobs=True: the call returns (out_tok, n_out,
    logprob fp32 [B, draft + 1]), the emitted tokens' log-probabilities, from one token_logprobs launch on the rows.  A sampler
    built with top_logprobs=n: one top_logprobs launch on the rows next to it, gathered the same way into ss.out_top_id int32 /
    ss.out_top_logprob fp32 [B, draft + 1, n] — entry (b, j), j < n_out[b], is the list of the row that emitted out_tok[b, j]; the
    call's return tuple stays as it is.
    No cache rollback: the next step starts at the new pending position and rewrites the K / V rows a rejected draft left before
    anything reads them.  block_table: a paged cache as for DecodeStep; the caller has reserved the pages of min(limit, n_tok +
    draft) positions of every slot before the call.  adapters: as for RaggedStep (the rows of slot b run with slot b's adapter).

    processor: a logits.LogitProcessor of the caches' slots.  A fed draft may be rejected, so nothing is counted
    when feeding: `begin` resets the slot's counts and counts the known tokens, the pending one included (count_prompt=False: it
    only resets); every row's logits are processed with its slot's state and, as extras, the guessed tokens in front of it in its
    segment — what sequential decoding would have counted by then; after the accept the emitted tokens are counted.  So count[b] is
    always the histogram of the counted part of hist[b][0 .. n_tok[b]), and the stream stays the sequential one.  `release` leaves
    the counts alone.  A slot's mask holds for all rows of its segment: a caller's own mask cannot change inside a multi-token
    step — a grammar that must follow the text goes in as `grammar=`.  More launches per step: process, observe, and two small
    torch ops that build observe's active vector from n_out.

    grammar: a grammar.GrammarBank of the caches' slots (needs a sampler, greedy is temperature 0).  Behind the
    draft every row gets the automaton state its guessed tokens lead to from bank.state[b] (`qpal_grammar_rows`; a row behind a
    guess the grammar forbids is dead), every live row is masked with its own state behind the processor, and behind the accept
    out_tok[b, :n_out[b]] advances bank.state[b]: three more launches.  A guess the grammar forbids at its position cannot equal
    the masked draw of the row in front of it, so the draft is cut there, and every row before the cut carries the state sequential
    decoding would have had: the stream is the sequential one.  `begin` puts the slot's state at the start; `release` leaves it
    alone.  Give `begin` the table's eos as `eos`, so that the slot stops where its text ends.

    stop: a stop.StopBank of the caches' slots.  Directly behind the accept the emitted run out_tok[b, :n_out[b]] is
    judged token by token; at the first token that finishes the slot n_out, n_tok and limit are cut there (the slot has no rows from
    then on), so the grammar's advance and the processor's observe see the cut run: one more launch.  The verdict depends on the
    emitted bytes only, so stream, reason and text_len are those of DecodeStep(stop=).  `begin` resets the slot's record; the stop ids
    live in the bank, so `begin`'s own eos can stay -1 (a slot that the accept's eos or limit ends first keeps reason 0).  A bank
    built with min_tokens=True (needs a sampler) adds the mask launch in front of the draw: row j of a segment is masked as the
    j-th token from now — the mask depends on the accepted prefix in front of the row only, the stream stays the sequential one.

    window, softcap, sinks, attn_scale: as for RaggedStep; the stream is then token for token that DecodeStep's."""

    def __init__(self, layers, embed, norm, lm_head, kcache, vcache, inv_freq, draft=4, gram=(2, 4), rows=None, sampler=None,
                 block_table=None, history=None, adapters=None, processor=None, grammar=None, window=None, softcap=None, sinks=None,
                 attn_scale=None, stop=None,
                 qkv_bias=None, qk_norm=None, mlp_act="silu", post_norms=None, logit_cap=None):
        B, K = self._check_table("SpeculativeStep", kcache, block_table), int(draft)
        if not 0 <= K <= 15 or len(gram) != 2 or not 1 <= int(gram[0]) <= int(gram[1]) <= 8:
            raise nat.QpalError(f"SpeculativeStep: draft must be in 0 .. 15 and 1 <= gram[0] <= gram[1] <= 8, got {draft}, {gram}")
        rows = min(128, B * (K + 1)) if rows is None else int(rows)
        if not 1 <= B <= rows <= 128:
            raise nat.QpalError(f"SpeculativeStep: rows must be in B = {B} .. 128, got {rows}")
        self.draft_len, self.gram = K, (int(gram[0]), int(gram[1]))
        super().__init__(layers, embed, norm, lm_head, kcache, vcache, inv_freq, rows=rows, segments=B, sampler=sampler,
                         block_table=block_table, adapters=adapters, processor=processor, grammar=grammar, window=window,
                         softcap=softcap, sinks=sinks, attn_scale=attn_scale, stop=stop,
                         qkv_bias=qkv_bias, qk_norm=qk_norm, mlp_act=mlp_act, post_norms=post_norms, logit_cap=logit_cap)
        dev = embed.device
        self._row_state = None if grammar is None else torch.full((rows,), -1, dtype=torch.int32, device=dev)
        self.history = self.context if history is None else int(history)
        if self.history < 1:
            raise nat.QpalError(f"SpeculativeStep: history must be at least 1, got {history}")
        i32, i64 = torch.int32, torch.int64
        self.hist = torch.zeros(B, self.history, dtype=i32, device=dev)
        self.n_tok, self.limit = torch.zeros(B, dtype=i64, device=dev), torch.zeros(B, dtype=i64, device=dev)
        self.eos = torch.full((B,), -1, dtype=i64, device=dev)
        self.tokens = torch.zeros(rows, dtype=i64, device=dev)
        self.seq, self.row0 = torch.full((B,), -1, dtype=i32, device=dev), torch.zeros(B + 1, dtype=i32, device=dev)
        self.pos0 = torch.zeros(B, dtype=i64, device=dev)
        self.row_slot, self.row_ctr = torch.full((rows,), -1, dtype=i32, device=dev), torch.full((rows,), -1, dtype=i64, device=dev)
        self.n_draft, self.n_out, self.n_acc = (torch.zeros(B, dtype=i32, device=dev) for _ in range(3))
        self._gather = torch.zeros(rows, dtype=i64, device=dev)  # the rows' embedding indices when the caller drafts
        if processor is not None:  # the observe launch behind the accept: entry (b, i) of out_tok counts for slot b iff i < n_out[b]
            self._obs_slot = torch.arange(B, dtype=i32, device=dev).repeat_interleave(K + 1).contiguous()
            self._obs_active = torch.zeros(B * (K + 1), dtype=i64, device=dev)
            self._lane1 = torch.arange(1, K + 2, dtype=i64, device=dev)

    def _moe_active(self):
        return self.row_ctr  # rows no slot holds (-1) route nothing

    def _setup_tail(self, vocab, dev, logprobs, top_n):
        """a draw at every ROW and up to draft + 1 tokens per slot: no last rows, no per-segment counters"""
        B, K = self.segments, self.draft_len
        self.drawn = torch.zeros(self.rows, dtype=torch.int64, device=dev)
        self.out_tok = torch.zeros(B, K + 1, dtype=torch.int64, device=dev)
        self.draw = sampling.Sampler(self.rows, vocab, dev, temperature=0.0, logprobs=logprobs, top_logprobs=top_n,
                                     truncation=self._truncating())  # greedy unless gathered
        self.out_logprob = torch.zeros(B, K + 1, dtype=torch.float32, device=dev) if logprobs else None
        self.out_top_id = torch.full((B, K + 1, top_n), -1, dtype=torch.int32, device=dev) if top_n else None
        self.out_top_logprob = torch.full((B, K + 1, top_n), float("-inf"), dtype=torch.float32, device=dev) if top_n else None
        self._lane = torch.arange(K + 1, dtype=torch.int64, device=dev)

    def hidden(self):
        """fp16 [rows, H]: the final norm of every row of the last step (rows of no segment mean nothing)"""
        return self.norm(self.h32.half())

    def begin(self, slot, tokens, limit=None, eos=-1):
        """a new sequence in `slot`: tokens (ints, at least one) are its known tokens, the last one pending — the caller has put the
        others into the slot's cache at positions 0 .. len - 2.  limit: the length generation stops at (default: all the history and
        the cache hold), eos: the stop token or -1.  Copies to the device: not part of a captured step."""
        toks = torch.as_tensor(tokens, dtype=torch.int64).reshape(-1).cpu()
        n, top = toks.shape[0], min(self.history, self.context)
        limit = top if limit is None else int(limit)
        if not 0 <= int(slot) < self.slots:
            raise nat.QpalError(f"SpeculativeStep.begin: slot {slot} outside the caches' {self.slots} sequences")
        if not 1 <= n <= limit <= top:
            raise nat.QpalError(f"SpeculativeStep.begin: {n} tokens and limit {limit} must satisfy 1 <= tokens <= limit <= {top}")
        if int(toks.min()) < 0 or int(toks.max()) >= self.lm_head.shape[0]:
            raise nat.QpalError(f"SpeculativeStep.begin: token ids must be in 0 .. {self.lm_head.shape[0] - 1}")
        self.hist[int(slot), :n] = toks.to(torch.int32).to(self.hist.device)
        if not -1 <= int(eos) < self.lm_head.shape[0]:
            raise nat.QpalError(f"SpeculativeStep.begin: eos must be -1 or a token id below {self.lm_head.shape[0]}, got {eos}")
        self.n_tok[int(slot)], self.limit[int(slot)], self.eos[int(slot)] = n, limit, int(eos)
        if self.processor is not None:
            self.processor.reset(slot)
            if self.processor.count_prompt:
                self.processor.count_tokens(slot, toks)
        if self.grammar is not None:
            self.grammar.reset(slot)
        if self.stop is not None:
            self.stop.reset(slot)

    def release(self, slot):
        """the slot has no sequence: no rows in the steps that follow"""
        if not 0 <= int(slot) < self.slots:
            raise nat.QpalError(f"SpeculativeStep.release: slot {slot} outside the caches' {self.slots} sequences")
        self.n_tok[int(slot)], self.limit[int(slot)], self.eos[int(slot)] = 0, 0, -1

    def __call__(self, ext_draft=None, ext_n=None):
        from . import speculative as spec
        if ext_draft is None and ext_n is not None:
            raise nat.QpalError("SpeculativeStep: ext_n without ext_draft")
        spec.spec_draft(self.hist, self.n_tok, self.limit, self.draft_len, self.gram, self.context, self.tokens, self.seq, self.row0,
                        self.pos0, self.row_slot, self.row_ctr, self.n_draft, ext_draft=ext_draft, ext_n=ext_n)
        if self.grammar is not None:
            gram_mod.grammar_rows(self.grammar, self.tokens, self.row0, self._row_state)
        # a caller's draft may be no token of the model: it can equal no draw, so any valid row of the embedding stands in for it
        tokens = self.tokens if ext_draft is None else torch.clamp(self.tokens, max=self.embed.shape[0] - 1, out=self._gather)
        self._map_rows(self.seq, self.row0)
        self._run_layers(tokens)
        sampling.lm_head_logits(self.h32, self.norm.weight, self.norm.eps, self.lm_head, out=self.draw.logits)
        self._cap_logits(self.draw.logits)
        if self.processor is not None:
            logits.process(self.draw.logits, self.processor, self.row_slot, self.row_ctr, tokens=self.tokens, row0=self.row0)
        if self.grammar is not None:
            gram_mod.grammar_mask(self.draw.logits, self.grammar, self.row_slot, self.row_ctr, row_state=self._row_state)
        if self.stop is not None and self.stop.min_tokens_mask:
            stop_mod.stop_mask(self.draw.logits, self.stop, self.row_slot, self.row_ctr, row0=self.row0)
        if self.sampler is not None:
            self._gather_draw(self.row_slot.to(torch.int64).clamp(min=0))
        sampling.sample(self.draw.logits, self.draw, self.row_ctr, out=self.drawn)
        if self.out_logprob is not None or self.out_top_id is not None:  # the rows that may emit slot b's tokens: row0[b] + 0 .. draft
            rows = (self.row0[:-1].to(torch.int64)[:, None] + self._lane[None, :]).clamp(max=self.rows - 1).reshape(-1)
        if self.out_logprob is not None:
            sampling.token_logprobs(self.draw.logits, self.drawn, out=self.draw.logprob, active=self.row_ctr)
            torch.index_select(self.draw.logprob, 0, rows, out=self.out_logprob.view(-1))
        if self.out_top_id is not None:
            n = self.draw.top_id.shape[1]
            sampling.top_logprobs(self.draw.logits, n, ids=self.draw.top_id, logprob=self.draw.top_logprob, active=self.row_ctr)
            torch.index_select(self.draw.top_id, 0, rows, out=self.out_top_id.view(-1, n))
            torch.index_select(self.draw.top_logprob, 0, rows, out=self.out_top_logprob.view(-1, n))
        spec.spec_accept(self.tokens, self.drawn, self.seq, self.row0, self.hist, self.n_tok, self.limit, self.eos, self.out_tok,
                         self.n_out, self.n_acc)
        if self.stop is not None:  # cuts n_out / n_tok / limit where a slot finishes inside its run: what follows sees the cut
            stop_mod.stop_advance(self.stop, self.out_tok, self.context, n_out=self.n_out, n_tok=self.n_tok, limit=self.limit)
        if self.grammar is not None:
            gram_mod.grammar_advance(self.grammar, self.out_tok, n=self.n_out)
        if self.processor is not None:
            torch.sub(self.n_out.to(torch.int64)[:, None], self._lane1[None, :], out=self._obs_active.view(-1, self.draft_len + 1))
            logits.observe(self.processor, self.out_tok.view(-1), self._obs_slot, active=self._obs_active)
        if self.out_logprob is not None:
            return self.out_tok, self.n_out, self.out_logprob
        return self.out_tok, self.n_out


def perplexity(score, windows, slot=0, out=None):
    """(ppl, avg_loss) of int64 windows [W, N] on the device: every window scored from an empty context (pos0 = 0) in `slot`;
    avg_loss = the mean over windows of each window's mean loss, summed on the device in fp64 and read once; ppl = exp(avg_loss).
    out: an optional fp32 [W, N - 1] device tensor that receives the log-probabilities the figure was computed from."""
    if windows.dim() != 2 or windows.shape[0] < 1 or windows.shape[1] < 2 or windows.dtype != torch.int64:
        raise nat.QpalError("perplexity: windows must be int64 [W >= 1, N >= 2]")
    W, N = windows.shape
    if out is not None and (out.shape != (W, N - 1) or out.dtype != torch.float32 or out.device != windows.device):
        raise nat.QpalError(f"perplexity: out must be fp32 [{W}, {N - 1}] on {windows.device}")
    total = torch.zeros((), dtype=torch.float64, device=windows.device)
    for w in range(W):
        lp = score(windows[w], slot=slot, pos0=0)
        if out is not None:
            out[w].copy_(lp)
        total -= lp.double().mean()
    avg = float(total) / W
    return math.exp(avg), avg
