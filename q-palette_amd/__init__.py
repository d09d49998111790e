"""qpalette_amd — MI355X (gfx950) native implementation of Q-Palette's dequant-matmul hot path.

Layout:
  csrc/            hand-written HIP kernels + the C-ABI (include/qpal.h) -> libqpal_hip.so
  _native.py       ctypes binding of the C-ABI (fails loudly when the library is missing)
  ops.py           ``torch.ops.ours_lib.*`` operator surface of the reference (lib/linear/__init__.py)
  linear/          nn.Module mirror of lib/linear/{tcq,comb,vq}_linear.py
  mem_op.py        quantizer-string grammar, Llama layer shapes, synthetic packed weights
                   (lib/utils/mem_op.py:2-307)
  hadamard.py      get_hadK (generated Paley factors), matmul_hadU*_cuda, the one-launch `rotate` (lib/utils/matmul_had.py)
  linear/incoherent_linear.py  IncoherentLinear / IncoherentMLP / IncoherentSdpaAttention (lib/linear/incoherent_linear.py)
  attention.py     decode_attention / attention_workspace: rope + KV append + GQA attention of B sequences, one launch;
                   prefill_attention / prefill_workspace: the same for up to 128 new tokens of one sequence, causal;
                   paged_decode_attention / paged_prefill_attention: both on page pools behind a block table;
                   shared_prefix_decode_attention / shared_prefix_workspace: paged decode that reads a forked prefix once per group;
                   ragged_prefill_attention / paged_ragged_prefill_attention / ragged_workspace: up to 128 rows of SEVERAL
                   sequences in one launch (segments described on the device);
                   window= on all of these but the shared-prefix launch: sliding-window attention; window_floor: its lower edge
                   softcap= / sinks= on the same launches: the logit soft cap and per-head sinks
  paging.py        PagedKVCache: per-layer page pools, the block table and the host-side page allocator (reserve / release / fork /
                   trim: the pages a sliding window has passed go back to the pool);
                   SharedPrefix (cache.prefix): the groups of slots that share a forked prefix, as the shared-prefix launch reads them
  decoder.py       DecodeStep: the whole-model decode step at batch B >= 1 on the kernels above (per-layer launch sequence,
                   scratch buffers, final norm + lm_head + argmax, launches per token); Prefill: a prompt into one cache slot;
                   Score: the log-probability of every next token of a sequence, nll and perplexity;
                   RaggedStep: prompt chunks and decode tokens of several slots in ONE 128-row step;
                   SpeculativeStep: the pending token + guessed tokens of every slot in one step, several tokens out per slot
  speculative.py   spec_draft / spec_accept (csrc/spec.hip): prompt-lookup drafts and the packing of a verify step, exact-match
                   acceptance and the state update, all on the device; reference_spec_draft / reference_spec_accept: the contracts
  sampling.py      lm_head_logits (final norm + lm_head for up to 128 rows), sample / Sampler (temperature, top-k, top-p, seeded
                   draw; per-slot parameters on the device; with min_p / top_a / typical_p the truncating draw of csrc/sample.hip),
                   reference_draw (the draw's contract in numpy fp64) and truncation_mask (the set the three filters keep);
                   token_logprobs (log softmax of a row at one token, csrc/logprob.hip) and its contract reference_logprob;
                   top_logprobs (the n likeliest tokens of a row and their log-probabilities, csrc/top_logprob.hip) and its
                   contract reference_top_logprobs
  logits.py        logit processors between the lm_head and the draw: LogitProcessor (per-slot token mask, sparse bias, repetition /
                   presence / frequency penalties and token counts on the device), process / observe (csrc/logit_proc.hip) and the
                   contract reference_process (numpy fp32, bit for bit)
  grammar.py       grammar-constrained decoding: compile_regex (a regular expression -> a minimal, trimmed byte-level DFA), TokenTable,
                   GrammarBank (the automata, their per-state token bitmasks and the slots' states on the device), grammar_rows /
                   grammar_mask / grammar_advance (csrc/grammar.hip) and the contracts reference_allow / _step / _rows / _mask /
                   _advance (numpy, bit for bit)
  stop.py          stop conditions on the device: compile_stops (byte strings -> a dense byte-level Aho-Corasick automaton), StopBank
                   (the stop sets and per slot the stop ids, budgets, automaton state and generation record), stop_advance /
                   stop_mask (csrc/stop.hip: the launch that ends a step and the min_tokens mask) and the contracts
                   reference_stop_advance / reference_stop_mask (numpy, bit for bit)
  blocks.py        the glue of Qwen- and Gemma-shaped blocks (csrc/block_glue.hip): qkv_prep (q | k | v bias and per-head QK-norm in
                   front of every attention launch), norm_add (sandwich post-norm + residual add), glu_gelu_tanh (GeGLU), logit_cap
                   (final-logit soft cap) and their float64 contracts reference_*; the step classes take them as qkv_bias= /
                   qk_norm= / post_norms= / mlp_act= / logit_cap=
  moe.py           mixture-of-experts MLPs (csrc/moe_route.hip, csrc/moe_gemv.hip): route (RMSNorm, router, softmax, top-k and the
                   expert-sorted layout in one launch), moe_gemv (the routed fused decode + GEMV: experts through device pointer
                   tables), combine, MoEMLP / quantize_experts and the contracts reference_route / _layout / _moe_mlp (numpy float64)
  packers.py       pack_trellis / pack_qweight / pack_qweight_{sq,vq}_simt on the C-ABI's host-side encoders
  quantize.py      TCQ quantiser: tail-biting Viterbi encoder (csrc/tcq_viterbi.hip) + LDLQ -> QTIPLinearTCQ
                   VQ / SQ quantiser: nearest-codeword LDLQ encoder (csrc/vq_encode.hip) -> VQLinearPack{TensorCore,SIMT}
  quantize_layer.py  whole layers: incoherence preprocessing (fp32 rotation, csrc/hadamard_f32.hip), comb / combt LDLQ,
                   quantize_linear (tcq_* / tcomb_* / comb_* / ldlq_* strings) -> IncoherentLinear + layer file
  calibrate.py     HessianAccumulator (csrc/hessian.hip: H += X^T X of fp16 rows, fp64 sums), collect_hessians over token windows of a
                   DenseModel, quantize_model: the seven quantize_linear calls per layer -> the layers the step classes take
  lora.py          low-rank adapters on the quantised base: lora_apply (csrc/lora.hip: out += B[a] (A[a] xin) with the adapter a
                   per row, shrink and expand in one launch), its contract reference_lora, LoraBank (the packed adapters and
                   the slot -> adapter vector the step classes take as `adapters=`), load_peft_adapter
  shard.py         row-sharding of packed layers across GPUs (torch.distributed / RCCL)

There is deliberately no CPU implementation here: the CPU restatement lives in /oracle and is test
infrastructure only.
"""
from . import _native  # noqa: F401
from . import ops  # noqa: F401
from . import mem_op  # noqa: F401
from . import shard  # noqa: F401
from . import hadamard  # noqa: F401
from . import packers  # noqa: F401
from .linear import (  # noqa: F401
    IncoherentLinear,
    IncoherentMLP,
    IncoherentSdpaAttention,
    make_linear,
    CombLinearTCQ,
    CombtLinearTCQ,
    QTIPLinearTCQ,
    VQLinearPackSIMT,
    VQLinearPackTensorCore,
    make_linear_from_info,
    multi_gemv,
    share_codebooks,
)
from . import quantize  # noqa: F401
from . import quantize_layer  # noqa: F401
from . import attention  # noqa: F401
from .attention import attention_workspace, decode_attention, prefill_attention, prefill_workspace  # noqa: F401
from .attention import paged_decode_attention, paged_prefill_attention  # noqa: F401
from .attention import reference_shared_rows, shared_prefix_decode_attention, shared_prefix_workspace  # noqa: F401
from .attention import paged_ragged_prefill_attention, ragged_prefill_attention, ragged_workspace  # noqa: F401
from .attention import window_floor  # noqa: F401
from . import paging  # noqa: F401
from .paging import PagedKVCache, SharedPrefix  # noqa: F401
from . import sampling  # noqa: F401
from .sampling import Sampler, lm_head_logits, reference_draw, reference_logprob, sample, token_logprobs, truncation_mask  # noqa: F401
from .sampling import reference_top_logprobs, top_logprobs  # noqa: F401
from . import logits  # noqa: F401
from .logits import LogitProcessor, reference_process  # noqa: F401
from . import grammar  # noqa: F401
from .grammar import ByteDFA, GrammarBank, TokenTable, compile_regex, grammar_advance, grammar_mask, grammar_rows  # noqa: F401
from . import stop  # noqa: F401
from .stop import StopBank, StopSet, compile_stops, reference_stop_advance, reference_stop_mask, stop_advance, stop_mask  # noqa: F401
from . import blocks  # noqa: F401
from . import moe  # noqa: F401
from .moe import MoEMLP, quantize_experts, reference_layout, reference_moe_mlp, reference_route  # noqa: F401
from .moe import Router, reference_combine_shared, reference_moe_mlp_ex, reference_route_ex  # noqa: F401
from . import decoder  # noqa: F401
from .decoder import DecodeStep, Prefill, RaggedStep, Score, SpeculativeStep, perplexity  # noqa: F401
from . import speculative  # noqa: F401
from .speculative import reference_spec_accept, reference_spec_draft, spec_accept, spec_draft  # noqa: F401
from .quantize_layer import incoherent_preprocess, layer_file_path, load_hessian, quantize_linear  # noqa: F401
from . import calibrate  # noqa: F401
from .calibrate import (  # noqa: F401
    DenseModel,
    HessianAccumulator,
    collect_hessians,
    quantize_model,
    random_dense_model,
    reference_hessian,
)
from . import lora  # noqa: F401
from .lora import LoraBank, load_peft_adapter, lora_apply, reference_lora  # noqa: F401

__version__ = "0.1.0"
