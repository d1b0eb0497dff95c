"""Batched generation: static KV cache, prefill, and a hipGraph-captured decode step.

Replaces HF ``generate`` as used by the reference (rollouts rl.py:38-44, evaluation rl.py:411-417):
prompts are left-padded into one batch, prefilled with the flash kernel (K/V appended to a static
cache by the fused RoPE kernel), then every decode step — embedding, 32 x (norm, LoRA-fused
projections, RoPE+append, split-K decode attention, SwiGLU), final norm, LM head, on-device
sampler (which also emits the behaviour log-prob), value head, and the bookkeeping kernel — is one
graph replay with zero host synchronisation. Finished rows are masked on device; the host polls
completion only every ``sync_every`` steps.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import ops
from ..models.decoder import pack_enabled, packed_index
from ..runtime import GraphRunner


@dataclass
class SamplingParams:
    max_new_tokens: int = 128
    temperature: float = 0.7            # reference rl.py:41
    top_k: int = 50                     # HF 4.x generate default the reference ran with
    top_p: float = 1.0
    do_sample: bool = True              # reference rl.py:42
    max_length: Optional[int] = None    # reference semantics: prompt + new tokens (rl.py:40)
    # stop strings / stop token ids: the defaults of a ``ContinuousBatcher(stops=True)``; empty = off.
    # stop: one string or at most 4 strings of 1..32 UTF-8 bytes; stop_token_ids: at most 8 ids
    stop: Optional[object] = None
    stop_token_ids: Sequence[int] = ()
    seed: int = 0
    # prompt-lookup speculative decoding (batch-1..8 RAG answers): K draft tokens per step, proposed
    # from the sequence's own history (the tokens after the latest earlier occurrence of its last
    # n-gram, n = lookup_ngram .. 1) and verified in one forward over K + 1 positions. 0: off
    lookup_tokens: int = 0
    lookup_ngram: int = 2
    # logit penalties: the defaults of a ``ContinuousBatcher(penalties=True)``; neutral = off.
    # repetition_penalty rho > 0 (HF semantics, prompt and generated tokens), presence / frequency
    # penalty in [-2, 2] (OpenAI semantics, generated tokens), logit_bias {token: bias in [-100, 100]}
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    logit_bias: Optional[object] = None

    @property
    def greedy(self) -> bool:
        return (not self.do_sample) or self.temperature <= 0

    @property
    def inv_temp(self) -> float:
        return 1.0 if self.greedy else 1.0 / self.temperature


MAX_LOGIT_BIAS = 16  # (token, bias) pairs per request


def _bias_pairs(logit_bias):
    """``logit_bias`` (None, a dict or a list of pairs) as a tuple of (token, bias) pairs; ValueError
    for more than 16 pairs, a token that is no integer >= 0, a duplicate token, or a bias outside
    [-100, 100]. Keys that are strings of digits (the OpenAI API's JSON object) are accepted."""
    if logit_bias is None:
        return ()
    items = list(logit_bias.items()) if isinstance(logit_bias, dict) else [tuple(x) for x in logit_bias]
    if len(items) > MAX_LOGIT_BIAS:
        raise ValueError(f"logit_bias: {len(items)} entries, at most {MAX_LOGIT_BIAS} per request")
    out, seen = [], set()
    for it in items:
        if len(it) != 2:
            raise ValueError(f"logit_bias: entries are (token, bias) pairs, got {it!r}")
        t, v = it
        if isinstance(t, str) and t.strip().lstrip("+").isdigit():
            t = int(t)
        if isinstance(t, bool) or not isinstance(t, int) or t < 0:
            raise ValueError(f"logit_bias: token {t!r} must be an integer >= 0")
        if t in seen:
            raise ValueError(f"logit_bias: token {t} given twice")
        seen.add(t)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not -100 <= v <= 100:
            raise ValueError(f"logit_bias[{t}] = {v!r}: must be in [-100, 100]")
        out.append((t, float(v)))
    return tuple(out)


def _check_penalties(rho, pi, phi, logit_bias, vocab=None):
    """Range checks of the four penalty settings (None: not set); returns the bias pairs."""
    if rho is not None and not (rho > 0 and rho != float("inf")):
        raise ValueError(f"repetition_penalty = {rho}: must be a finite number > 0 (1 = off)")
    if pi is not None and not -2 <= pi <= 2:
        raise ValueError(f"presence_penalty = {pi}: must be in [-2, 2] (0 = off)")
    if phi is not None and not -2 <= phi <= 2:
        raise ValueError(f"frequency_penalty = {phi}: must be in [-2, 2] (0 = off)")
    pairs = _bias_pairs(logit_bias)
    if vocab is not None:
        for t, _ in pairs:
            if t >= vocab:
                raise ValueError(f"logit_bias: token {t} is outside the vocabulary [0, {vocab})")
    return pairs


def _check_stops(stop, stop_token_ids, vocab=None):
    """``stop`` (None, a string or a sequence of strings) and ``stop_token_ids`` (None or a sequence
    of ids) as (tuple of UTF-8 byte strings, tuple of ids); ValueError for more than 4 strings, a
    string that is empty or longer than 32 bytes, a duplicate string, more than 8 ids, or an id that is
    no integer in [0, vocab)."""
    strings = () if stop is None else (stop,) if isinstance(stop, (str, bytes)) else tuple(stop)
    if len(strings) > ops.STOP_MAX_STR:
        raise ValueError(f"stop: {len(strings)} strings, at most {ops.STOP_MAX_STR} per request")
    out = []
    for st in strings:
        if not isinstance(st, (str, bytes)):
            raise ValueError(f"stop: entries are strings, got {st!r}")
        raw = st.encode("utf-8") if isinstance(st, str) else bytes(st)
        if not 1 <= len(raw) <= ops.STOP_MAX_LEN:
            raise ValueError(f"stop: {st!r} is {len(raw)} bytes of UTF-8, must be 1..{ops.STOP_MAX_LEN}")
        if raw in out:
            raise ValueError(f"stop: {st!r} given twice")
        out.append(raw)
    ids = () if stop_token_ids is None else tuple(stop_token_ids)
    if len(ids) > ops.STOP_MAX_TOK:
        raise ValueError(f"stop_token_ids: {len(ids)} ids, at most {ops.STOP_MAX_TOK} per request")
    uniq = []
    for t in ids:
        if isinstance(t, bool) or not isinstance(t, int) or t < 0 or (vocab is not None and t >= vocab):
            raise ValueError(f"stop_token_ids: {t!r} must be an integer in [0, "
                             f"{vocab if vocab is not None else 'the vocabulary size'})")
        if t not in uniq:
            uniq.append(t)
    return tuple(out), tuple(uniq)


def _neutral_stops(params) -> bool:
    return not params.stop and not tuple(params.stop_token_ids or ())


_STOPS_NEED = ("stop strings and stop token ids (stop, stop_token_ids) are served by ContinuousBatcher(per_request=True, "
               "stops=True, token_bytes=...) only")


_MIX = 0x9E3779B97F4A7C15  # 2**64 / golden ratio: spreads consecutive integers over 64 bits


def derive_seed(base_seed: int, count: int) -> int:
    """The seed of the ``count``-th request that brought none of its own: a fixed function of the
    batcher's ``SamplingParams.seed`` and the admission count (splitmix64's finaliser), < 2**63."""
    z = (int(base_seed) * _MIX + (int(count) + 1) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    return (z ^ (z >> 31)) & (2 ** 63 - 1)


@dataclass
class RequestSampling:
    """One request's sampling settings under ``ContinuousBatcher(per_request=True)``; a field left
    ``None`` takes the batcher's ``SamplingParams`` value (an unseeded request: ``derive_seed``)."""
    temperature: Optional[float] = None   # 0: greedy
    top_k: Optional[int] = None           # 0: off
    top_p: Optional[float] = None
    do_sample: Optional[bool] = None
    seed: Optional[int] = None
    max_new_tokens: Optional[int] = None
    # draft tokens per verify step of this request, 0 .. the batcher's lookup_tokens (None: the
    # batcher's); only for batchers with prompt-lookup decoding on
    lookup_tokens: Optional[int] = None
    # logit penalties, only for batchers built with ``penalties=True`` (None: the batcher's
    # ``SamplingParams`` value): repetition penalty rho > 0 (1 = off), presence / frequency penalty
    # in [-2, 2] (0 = off), logit_bias = {token: bias in [-100, 100]} or a list of such pairs (<= 16)
    repetition_penalty: Optional[float] = None
    presence_penalty: Optional[float] = None
    frequency_penalty: Optional[float] = None
    logit_bias: Optional[object] = None
    # where the answer ends, only for batchers built with ``stops=True`` (None: the batcher's
    # ``SamplingParams`` value): one string or at most 4 strings of 1..32 UTF-8 bytes, searched in the
    # text of the generated tokens, and at most 8 token ids; the matched text is not part of the answer
    stop: Optional[object] = None
    stop_token_ids: Optional[Sequence[int]] = None

    @property
    def has_stops(self) -> bool:
        """True when the request sets a stop field (empty values included)"""
        return self.stop is not None or self.stop_token_ids is not None

    @property
    def has_penalties(self) -> bool:
        """True when the request sets a penalty field (neutral values included)"""
        return any(v is not None for v in (self.repetition_penalty, self.presence_penalty, self.frequency_penalty,
                                           self.logit_bias))

    def validate(self, max_new: Optional[int] = None, lookup: Optional[int] = None, vocab: Optional[int] = None):
        """ValueError for a setting outside its range (``max_new``: the batcher's output width;
        ``lookup``: the batcher's draft length K, 0 = lookup off, None = not checked here; ``vocab``:
        the vocabulary size bias tokens must lie in, None = not checked here)."""
        _check_penalties(self.repetition_penalty, self.presence_penalty, self.frequency_penalty, self.logit_bias, vocab)
        _check_stops(self.stop, self.stop_token_ids, vocab)
        if self.lookup_tokens is not None:
            if not (isinstance(self.lookup_tokens, int) and 0 <= self.lookup_tokens <= 7):
                raise ValueError(f"lookup_tokens = {self.lookup_tokens}: must be an integer in [0, 7]")
            if lookup == 0:
                raise ValueError(f"lookup_tokens = {self.lookup_tokens}: prompt-lookup decoding is off on this batcher "
                                 f"(ContinuousBatcher(lookup_tokens=K))")
            if lookup is not None and self.lookup_tokens > lookup:
                raise ValueError(f"lookup_tokens = {self.lookup_tokens}: must be in [0, {lookup}] (the batcher's "
                                 f"lookup_tokens)")
        if self.temperature is not None and not self.temperature >= 0:
            raise ValueError(f"temperature = {self.temperature}: must be >= 0 (0 = greedy)")
        if self.top_k is not None and not self.top_k >= 0:
            raise ValueError(f"top_k = {self.top_k}: must be >= 0 (0 = off)")
        if self.top_p is not None and not 0 < self.top_p <= 1:
            raise ValueError(f"top_p = {self.top_p}: must be in (0, 1]")
        if self.max_new_tokens is not None and not (self.max_new_tokens >= 1 and
                                                    (max_new is None or self.max_new_tokens <= max_new)):
            raise ValueError(f"max_new_tokens = {self.max_new_tokens}: must be in [1, "
                             f"{max_new if max_new is not None else 'the output width'}]")
        if self.seed is not None and not 0 <= self.seed < 2 ** 63:
            raise ValueError(f"seed = {self.seed}: must be in [0, 2**63)")

    def resolve(self, params: SamplingParams, max_new: int, default_seed: int):
        """(inv_temp, top_k, top_p, greedy, seed, max_new_tokens) with the batcher's defaults filled in"""
        self.validate(max_new)
        pick = lambda v, d: d if v is None else v  # noqa: E731
        temp = float(pick(self.temperature, params.temperature))
        greedy = (not pick(self.do_sample, params.do_sample)) or temp <= 0
        return (1.0 if greedy else 1.0 / temp, int(pick(self.top_k, params.top_k)),
                float(pick(self.top_p, params.top_p)), bool(greedy), int(pick(self.seed, default_seed)),
                int(pick(self.max_new_tokens, max_new)))

    def resolve_penalties(self, params: SamplingParams, vocab: Optional[int] = None):
        """(rho, presence, frequency, ((token, bias), ...)) with the batcher's defaults filled in"""
        pick = lambda v, d: d if v is None else v  # noqa: E731
        rho = float(pick(self.repetition_penalty, params.repetition_penalty))
        pi = float(pick(self.presence_penalty, params.presence_penalty))
        phi = float(pick(self.frequency_penalty, params.frequency_penalty))
        pairs = _check_penalties(rho, pi, phi, pick(self.logit_bias, params.logit_bias), vocab)
        return rho, pi, phi, pairs

    def resolve_stops(self, params: SamplingParams, vocab: Optional[int] = None):
        """((stop string bytes, ...), (stop token id, ...)) with the batcher's defaults filled in"""
        return _check_stops(params.stop if self.stop is None else self.stop,
                            params.stop_token_ids if self.stop_token_ids is None else self.stop_token_ids, vocab)


class _RowParams:
    """Static per-row sampling parameters (device memory the captured decode step reads)."""

    def __init__(self, B: int, device):
        self.inv_temp = torch.ones(B, dtype=torch.float32, device=device)
        self.top_k = torch.zeros(B, dtype=torch.int32, device=device)
        self.top_p = torch.ones(B, dtype=torch.float32, device=device)
        self.greedy = torch.zeros(B, dtype=torch.uint8, device=device)
        self.seed = torch.zeros(B, dtype=torch.long, device=device)
        self.max_new = torch.ones(B, dtype=torch.int32, device=device)
        # the row's own draft length (prompt-lookup decoding in the continuous batch): allocated by
        # the first batcher that turns lookup on, read by the draft kernel only
        self.row_draft = None

    def draft_buffer(self, K: int):
        """row_draft, every row at the batcher's K"""
        if self.row_draft is None:
            self.row_draft = torch.empty_like(self.max_new)
        self.row_draft.fill_(K)
        return self.row_draft

    def tensors(self):
        return [self.inv_temp, self.top_k, self.top_p, self.greedy, self.seed, self.max_new]

    def write(self, b0: int, rows):
        """rows: ``RequestSampling.resolve`` tuples of rows b0.. (host-to-device copies, outside any graph)"""
        for t, col in zip(self.tensors(), zip(*rows)):
            t[b0:b0 + len(rows)].copy_(torch.tensor(col, dtype=t.dtype))


class _RowPenalties:
    """Static per-row logit-penalty parameters (device memory the captured decode step reads);
    every row starts neutral."""

    def __init__(self, B: int, device):
        self.rho = torch.ones(B, dtype=torch.float32, device=device)
        self.inv_rho = torch.ones(B, dtype=torch.float32, device=device)  # 1 / rho, rounded once on the host
        self.pi = torch.zeros(B, dtype=torch.float32, device=device)
        self.phi = torch.zeros(B, dtype=torch.float32, device=device)
        self.nbias = torch.zeros(B, dtype=torch.int32, device=device)
        self.bias_tok = torch.zeros(B, MAX_LOGIT_BIAS, dtype=torch.int32, device=device)
        self.bias_val = torch.zeros(B, MAX_LOGIT_BIAS, dtype=torch.float32, device=device)

    def tensors(self):
        return [self.rho, self.inv_rho, self.pi, self.phi, self.nbias, self.bias_tok, self.bias_val]

    def reset(self):
        for t, v in zip(self.tensors(), (1, 1, 0, 0, 0, 0, 0)):
            t.fill_(v)

    def write(self, b0: int, rows):
        """rows: ``RequestSampling.resolve_penalties`` tuples of rows b0.. (host-to-device copies,
        outside any graph)"""
        n = len(rows)
        rho = torch.tensor([r[0] for r in rows], dtype=torch.float32)
        tok = torch.zeros(n, MAX_LOGIT_BIAS, dtype=torch.int32)
        val = torch.zeros(n, MAX_LOGIT_BIAS, dtype=torch.float32)
        for i, r in enumerate(rows):
            for j, (t, v) in enumerate(r[3]):
                tok[i, j], val[i, j] = t, v
        cols = (rho, 1.0 / rho, torch.tensor([r[1] for r in rows], dtype=torch.float32),
                torch.tensor([r[2] for r in rows], dtype=torch.float32),
                torch.tensor([len(r[3]) for r in rows], dtype=torch.int32), tok, val)
        for t, col in zip(self.tensors(), cols):
            t[b0:b0 + n].copy_(col)


class _RowStops:
    """Static per-row stop strings / stop token ids and the scan state of ``ops.stop_rows`` (device
    memory the captured decode step reads and writes); every row starts without stops."""

    def __init__(self, B: int, device):
        i32 = dict(dtype=torch.int32, device=device)
        self.n_stop = torch.zeros(B, **i32)
        self.stop_len = torch.zeros(B, ops.STOP_MAX_STR, **i32)
        self.stop_bytes = torch.zeros(B, ops.STOP_MAX_STR, ops.STOP_MAX_LEN, dtype=torch.uint8, device=device)
        self.n_stop_tok = torch.zeros(B, **i32)
        self.stop_tok = torch.zeros(B, ops.STOP_MAX_TOK, **i32)
        self.seen = torch.zeros(B, **i32)      # generated tokens already scanned
        self.nbytes = torch.zeros(B, **i32)    # table bytes already scanned (a stripped leading space included)
        self.stop_hit = torch.full((B,), -1, **i32)  # -1 none, 0..3 the string, 4 + j stop id j
        self.stop_at = torch.zeros(B, **i32)   # byte offset in the stream text where the answer ends

    def tensors(self):
        return [self.n_stop, self.stop_len, self.stop_bytes, self.n_stop_tok, self.stop_tok, self.seen, self.nbytes,
                self.stop_hit, self.stop_at]

    def reset(self):
        for t in self.tensors():
            t.fill_(-1 if t is self.stop_hit else 0)

    def write(self, b0: int, rows):
        """rows: ``RequestSampling.resolve_stops`` tuples of rows b0..; the scan state of the rows
        starts over (host-to-device copies, outside any graph)"""
        n = len(rows)
        slen = torch.zeros(n, ops.STOP_MAX_STR, dtype=torch.int32)
        sbytes = torch.zeros(n, ops.STOP_MAX_STR, ops.STOP_MAX_LEN, dtype=torch.uint8)
        stok = torch.zeros(n, ops.STOP_MAX_TOK, dtype=torch.int32)
        for i, (strings, ids) in enumerate(rows):
            for j, raw in enumerate(strings):
                slen[i, j] = len(raw)
                sbytes[i, j, :len(raw)] = torch.tensor(list(raw), dtype=torch.uint8)
            for j, t in enumerate(ids):
                stok[i, j] = t
        zero = torch.zeros(n, dtype=torch.int32)
        cols = (torch.tensor([len(r[0]) for r in rows], dtype=torch.int32), slen, sbytes,
                torch.tensor([len(r[1]) for r in rows], dtype=torch.int32), stok, zero, zero, zero - 1, zero)
        for t, col in zip(self.tensors(), cols):
            t[b0:b0 + n].copy_(col)

    def rows(self, r0: int, r1: int):
        return [t[r0:r1] for t in self.tensors()]


def _neutral_penalties(params: SamplingParams) -> bool:
    return (params.repetition_penalty == 1.0 and params.presence_penalty == 0.0 and params.frequency_penalty == 0.0
            and not params.logit_bias)


@dataclass
class GenerationOutput:
    tokens: torch.Tensor        # [B, T] generated ids (pad after finish)
    lengths: torch.Tensor       # [B] number of generated tokens
    logprobs: torch.Tensor      # [B, T] behaviour log-probs of the drawn tokens (tempered dist.)
    values: Optional[torch.Tensor]  # [B, T] value-head outputs at each generating state
    prompt_ids: torch.Tensor    # [B, S] left-padded prompts
    prompt_start: torch.Tensor  # [B] first real prompt token
    timings: dict = field(default_factory=dict)


class _GraphSet:
    """Captured decode steps by key (sampling parameters, output width, row bucket): replaying a
    generator at another batch bucket switches graphs instead of recapturing. Least recently used
    graphs beyond ``max_graphs`` are dropped; ``reset()`` drops all (e.g. when the output buffers
    they captured are reallocated). Same interface as ``runtime.GraphRunner``."""

    def __init__(self, max_graphs: int = 8):
        from collections import OrderedDict

        self.graphs = OrderedDict()
        self.cur = None
        self.max_graphs = max_graphs

    def needs(self, key) -> bool:
        r = self.graphs.get(key)
        if r is None:
            return True
        self.graphs.move_to_end(key)
        self.cur = r
        return False

    def capture(self, fn, key=None, keep=(), restore=()):
        r = GraphRunner()
        r.capture(fn, key, keep, restore)
        self.graphs[key] = r
        self.cur = r
        while len(self.graphs) > self.max_graphs:
            self.graphs.popitem(last=False)

    def replay(self):
        self.cur.replay()

    def reset(self):
        self.graphs.clear()
        self.cur = None


def _fp4_decode_on(model) -> bool:
    layers = getattr(model, "layers", None)
    return bool(layers) and getattr(layers[0], "fp4_decode", False)


class KVCache:
    """Static K/V cache [L, B, Hkv, Smax, D]. ``fp8``: e4m3fn bytes (K rows k-permuted) plus one
    fp32 scale per (layer, row, kv head, slot) in ``ks`` / ``vs`` [L, B, Hkv, SmaxP] (SmaxP = Smax
    rounded up to 16; zero-initialised so never-written slots scale to 0) — config 5's rollout
    cache, half the bytes the decode attention streams (``ops.kv_store_fp8``)."""

    def __init__(self, num_layers, B, Hkv, Smax, D, device, dtype=torch.bfloat16, fp8: bool = False):
        alloc = torch.empty if torch.device(device).type == "cuda" else torch.zeros
        self.fp8 = fp8
        cdt = torch.uint8 if fp8 else dtype
        self.k = alloc(num_layers, B, Hkv, Smax, D, device=device, dtype=cdt)
        self.v = alloc(num_layers, B, Hkv, Smax, D, device=device, dtype=cdt)
        self.ks = self.vs = None
        if fp8:
            if D != ops.FP8_KV_D:
                raise ValueError(f"fp8 KV cache needs head_dim {ops.FP8_KV_D}, got {D}")
            smaxp = (Smax + 15) // 16 * 16
            self.ks = torch.zeros(num_layers, B, Hkv, smaxp, device=device, dtype=torch.float32)
            self.vs = torch.zeros(num_layers, B, Hkv, smaxp, device=device, dtype=torch.float32)
        self.B, self.Smax = B, Smax

    def scales(self, layer: int):
        """(k_scale, v_scale) of one layer, or (None, None) for a bf16 cache"""
        return (self.ks[layer], self.vs[layer]) if self.fp8 else (None, None)

    @property
    def nbytes(self):
        n = 2 * self.k.numel() * self.k.element_size()
        if self.fp8:
            n += 2 * self.ks.numel() * 4
        return n


class Generator:
    """Owns the cache and captured graph for one (model, max_batch, max_seq) configuration."""

    def __init__(self, model, max_batch: int, max_seq: int, device=None, use_graph: bool = True,
                 value_head=None, sync_every: int = 16, kv_fp8: Optional[bool] = None):
        self.model = model
        cfg = model.cfg
        self.cfg = cfg
        self.device = torch.device(device or model.embed.device)
        self.max_batch, self.max_seq = max_batch, max_seq
        self.use_graph = use_graph and self.device.type == "cuda"
        self.value_head = value_head
        self.sync_every = sync_every
        # generation never differentiates: by default adapters run on merged bf16 weights (one
        # weight stream per projection). False: the unmerged LoRA K-extension, i.e. exactly the
        # weights the training forward scores with (PPO behaviour policy == target policy at
        # theta_old, PPOConfig.merged_lora_rollout = False)
        self.merge_lora = True
        # fp8 K/V cache (config 5): the model's setting unless given; GPU MFMA decode kernels only
        # (head_dim 128), the CPU path runs the quantise / dequantise reference
        kv_fp8 = getattr(model, "kv_fp8", False) if kv_fp8 is None else kv_fp8
        self.cache = KVCache(cfg.num_layers, max_batch, cfg.num_kv_heads, max_seq, cfg.head_dim, self.device,
                             model.dtype, fp8=bool(kv_fp8))
        dev = self.device
        B = max_batch
        self.workspace = ops.decode_workspace(B, cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, max_seq, dev) \
            if dev.type == "cuda" else None
        # device-resident decode state (static addresses for graph replay)
        self.tok_in = torch.zeros(B, dtype=torch.long, device=dev)
        self.kv_len = torch.zeros(B, dtype=torch.int32, device=dev)
        self.kv_start = torch.zeros(B, dtype=torch.int32, device=dev)
        self.pos = torch.zeros(B, dtype=torch.int32, device=dev)
        self.attn_len = torch.zeros(B, dtype=torch.int32, device=dev)
        self.active = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.gen_len = torch.zeros(B, dtype=torch.int32, device=dev)
        self.step = torch.zeros(1, dtype=torch.long, device=dev)
        self.rng_offset = torch.zeros(1, dtype=torch.long, device=dev)
        self.sampled = torch.zeros(B, dtype=torch.long, device=dev)
        self.sampled_lp = torch.zeros(B, dtype=torch.float32, device=dev)
        self.values = torch.zeros(B, dtype=torch.float32, device=dev)
        self.out_tokens = None
        self.runner = _GraphSet()  # captured decode steps (runtime.GraphRunner each, shared graph pool)
        # prompt-lookup decoding: token history (indexed like cache slots) and, per K, the verify
        # step's static buffers — allocated on first use, untouched when lookup_tokens == 0
        self.hist = None
        self._lookup = {}
        self._lk = None
        # True while a ContinuousBatcher with lookup_tokens > 0 owns the generator: the verify step
        # then keeps per-row figures and, with per-request sampling, reads the row buffers
        self._lk_rows = False
        # per-request sampling (ContinuousBatcher(per_request=True)): per-row parameter buffers,
        # allocated on first use; _rows_on selects the per-row sampler and bookkeeping in _emit
        self.rowp = None
        self._rows_on = False
        # per-request adapters (ContinuousBatcher(adapters=bank)): the bank and a static adapter slot
        # per row (-1 = base model), written at admission outside any graph like the row parameters
        self.adapters = None
        self.adapter_ids = None
        # per-request logit penalties (ContinuousBatcher(penalties=True)): per-row parameter buffers,
        # allocated on first use; _pen_on puts ops.logit_rows_penalty in front of the per-row sampler
        self.penp = None
        self._pen_on = False
        # per-request stop strings / stop token ids (ContinuousBatcher(stops=True)): the vocabulary
        # byte table, the per-row stop buffers (allocated on first use); _stop_on puts ops.stop_rows
        # behind the bookkeeping kernel
        self.stopp = None
        self.token_bytes = None
        self._stop_on = False

    # ------------------------------------------------------------------ one decode step (device only)
    def _bucket(self, B: int) -> int:
        """Rows a decode step runs for a batch of B: the next power of two (capped at max_batch).
        A serving generator sized for 16 or 64 users then decodes one answer at the batch-1 cost;
        each bucket has its own captured graph (the rows past B stay inactive)."""
        nb = 1
        while nb < B:
            nb *= 2
        return min(nb, self.max_batch)

    def _step(self, params: SamplingParams, eos_ids: torch.Tensor, pad_id: int):
        # attn_len = kv_len + 1 and pos = kv_len - kv_start were set by the previous bookkeeping
        # (decode_update on the GPU, _update_cpu on the CPU) — no elementwise launches here
        nb = self._nb
        cache = self.cache if nb == self.max_batch else _SubCache(self.cache, nb)
        if self.adapters is not None:
            h = self.model.decode(self.tok_in[:nb], self.pos[:nb], self.kv_len[:nb], self.attn_len[:nb],
                                  self.kv_start[:nb], cache, self.workspace,
                                  adapters=(self.adapters, self.adapter_ids[:nb]))
        else:
            h = self.model.decode(self.tok_in[:nb], self.pos[:nb], self.kv_len[:nb], self.attn_len[:nb],
                                  self.kv_start[:nb], cache, self.workspace)
        self._emit(h, params, eos_ids, pad_id)

    def _lookup_buffers(self, K: int) -> "_LookupState":
        if self.hist is None:
            self.hist = torch.zeros(self.max_batch, self.max_seq, dtype=torch.long, device=self.device)
        st = self._lookup.get(K)
        if st is None:
            st = self._lookup[K] = _LookupState(self.max_batch, K + 1, self.device)
        return st

    def _penalty_buffers(self) -> _RowPenalties:
        """The penalty parameters and the token history the kernel scans (shared with lookup)"""
        if self.penp is None:
            self.penp = _RowPenalties(self.max_batch, self.device)
        if self.hist is None:
            self.hist = torch.zeros(self.max_batch, self.max_seq, dtype=torch.long, device=self.device)
        return self.penp

    def _stop_buffers(self) -> _RowStops:
        if self.stopp is None:
            self.stopp = _RowStops(self.max_batch, self.device)
        return self.stopp

    def _stop_rows(self, r0: int, r1: int):
        """The stop scan of rows [r0, r1) over the tokens the bookkeeping just emitted"""
        ops.stop_rows(self.out_tokens[r0:r1], self.gen_len[r0:r1], self.active[r0:r1], self.token_bytes,
                      *self.stopp.rows(r0, r1))

    def _row_buffers(self) -> _RowParams:
        if self.rowp is None:
            self.rowp = _RowParams(self.max_batch, self.device)
        return self.rowp

    def _check_lookup(self, params: SamplingParams):
        K, n = params.lookup_tokens, params.lookup_ngram
        if not 0 <= K <= 7:
            raise ValueError(f"lookup_tokens = {K}: supported 0..7 draft tokens per step")
        if K == 0:
            return
        if n < 1:
            raise ValueError(f"lookup_ngram = {n}: must be >= 1")
        if self.cache.fp8:
            raise NotImplementedError("prompt-lookup decoding does not support the fp8 K/V cache")
        if self.cfg.arch == "opt":
            raise NotImplementedError("prompt-lookup decoding does not support learned-position (opt) models")
        if self.value_head is not None:
            raise NotImplementedError("prompt-lookup decoding does not support a value head (PPO rollouts)")

    def _check_verify_rows(self, rows: int, K: int, fused: bool = True):
        """A verify step runs rows * (K + 1) rows through the decode layer: ValueError above the fused
        layer's limit (``fused``: checked) or the 16 rows of the MXFP4 decode kernels."""
        if fused:
            layers = getattr(self.model, "layers", None)
            fp8 = bool(layers) and getattr(layers[0], "fp8_enabled", False)
            max_b = getattr(self.model, "fused_decode_max_batch_fp8" if fp8 else "fused_decode_max_batch", None)
            if max_b is not None and rows * (K + 1) > max_b:
                raise ValueError(f"prompt-lookup decoding: {rows} rows x {K + 1} positions exceed the fused "
                                 f"decode layer's limit of {max_b} rows")
        if _fp4_decode_on(self.model) and rows * (K + 1) > 16:
            raise ValueError(f"prompt-lookup decoding: {rows} rows x {K + 1} positions exceed the 16 rows of the "
                             f"MXFP4 decode kernels (model.fp4_decode)")

    def _step_verify(self, params: SamplingParams, eos_ids: torch.Tensor, pad_id: int):
        """One verify step: forward over G = K + 1 positions per row (the last emitted token and the
        draft), the ordinary sampler on every position, then the accept and draft bookkeeping."""
        nb, st = self._nb, self._lk
        G = st.G
        cache = self.cache if nb == self.max_batch else _SubCache(self.cache, nb)
        h = self.model.decode_verify(st.inp[:nb], self.pos[:nb], self.kv_len[:nb], self.attn_len[:nb],
                                     self.kv_start[:nb], cache, self.workspace)
        logits = self.model.logits(h)
        rp = self.rowp if (self._rows_on and self._lk_rows) else None
        if rp is not None:
            # G positions per request: position j draws with the counter of output index gen_len + j,
            # the one the plain per-request step would use for that token
            ops.sample_rows(logits, rp.inv_temp[:nb], rp.top_k[:nb], rp.top_p[:nb], rp.greedy[:nb], rp.seed[:nb],
                            self.gen_len[:nb], st.row_active[:nb * G], st.sampled[:nb * G], st.sampled_lp[:nb * G],
                            group=G)
        else:
            ops.sample(logits, params.inv_temp, params.top_k, params.top_p, params.greedy, params.seed,
                       self.rng_offset, st.row_active[:nb * G], st.sampled[:nb * G], st.sampled_lp[:nb * G])
        if self._lk_rows:
            # continuous batch: per-row figures, and the row's own answer length under per-request sampling
            ops.lookup_accept(st.sampled[:nb * G], st.sampled_lp[:nb * G], st.inp[:nb], st.n_draft[:nb],
                              self.out_tokens[:nb], self.out_logp[:nb], self.hist[:nb], self.active[:nb],
                              self.kv_len[:nb], self.pos[:nb], self.attn_len[:nb], self.kv_start[:nb],
                              self.gen_len[:nb], self.step, self.rng_offset, st.counters, eos_ids,
                              row_max_new=None if rp is None else rp.max_new[:nb], row_stats=st.row_stats[:nb])
        else:
            ops.lookup_accept(st.sampled[:nb * G], st.sampled_lp[:nb * G], st.inp[:nb], st.n_draft[:nb],
                              self.out_tokens[:nb], self.out_logp[:nb], self.hist[:nb], self.active[:nb],
                              self.kv_len[:nb], self.pos[:nb], self.attn_len[:nb], self.kv_start[:nb],
                              self.gen_len[:nb], self.step, self.rng_offset, st.counters, eos_ids)
        if self._stop_on and self._lk_rows:
            # before the draft: a stopped row gets no further inputs
            self._stop_rows(0, nb)
        self._draft(params, pad_id)

    def _draft(self, params: SamplingParams, pad_id: int, r0: int = 0, r1: Optional[int] = None):
        """The next verify step's inputs of rows [r0, r1) (default: the row bucket); every buffer is
        sliced per row, so other rows' inputs, draft counts and row masks are not touched."""
        st = self._lk
        r1 = self._nb if r1 is None else r1
        rd = self.rowp.row_draft[r0:r1] if (self._rows_on and self._lk_rows) else None
        ops.lookup_draft(self.hist[r0:r1], self.kv_len[r0:r1], self.kv_start[r0:r1], self.active[r0:r1],
                         params.lookup_ngram, pad_id, st.inp[r0:r1], st.n_draft[r0:r1],
                         st.row_active[r0 * st.G:r1 * st.G], row_draft=rd)

    def _emit(self, h, params: SamplingParams, eos_ids, pad_id, r0: int = 0, append: bool = True):
        """Sample from the hidden states of rows [r0, r0 + len(h)) and run the bookkeeping for them
        (the decode step's row bucket, or one row admitted by continuous batching). ``append``
        (logit penalties only): the rows' input tokens join their history first — True for a decode
        step, False for an admission's prefill logits (the history is the prompt alone)."""
        r1 = r0 + h.shape[0]
        logits = self.model.logits(h)
        rp = self.rowp if self._rows_on else None
        if rp is not None and self._pen_on:
            # the row's own penalties, in place, before its sampler reads the logits
            pp = self.penp
            ops.logit_rows_penalty(logits, self.hist[r0:r1], self.tok_in[r0:r1] if append else None,
                                   self.kv_len[r0:r1], self.kv_start[r0:r1], self.gen_len[r0:r1], self.active[r0:r1],
                                   pp.rho[r0:r1], pp.inv_rho[r0:r1], pp.pi[r0:r1], pp.phi[r0:r1], pp.nbias[r0:r1],
                                   pp.bias_tok[r0:r1], pp.bias_val[r0:r1])
        if rp is not None:
            # the row's own settings and stream: (seed, tokens generated so far) key the draw
            ops.sample_rows(logits, rp.inv_temp[r0:r1], rp.top_k[r0:r1], rp.top_p[r0:r1], rp.greedy[r0:r1],
                            rp.seed[r0:r1], self.gen_len[r0:r1], self.active[r0:r1], self.sampled[r0:r1],
                            self.sampled_lp[r0:r1])
        else:
            ops.sample(logits, params.inv_temp, params.top_k, params.top_p, params.greedy, params.seed,
                       self.rng_offset, self.active[r0:r1], self.sampled[r0:r1], self.sampled_lp[r0:r1])
        if self.value_head is not None:
            self.values[r0:r1].copy_(self.value_head(h))
        if h.is_cuda and rp is not None:
            vh = self.value_head is not None
            ops.native().decode_update_rows(self.sampled[r0:r1], self.out_tokens[r0:r1], self.out_logp[r0:r1],
                                            self.sampled_lp[r0:r1], self.out_values[r0:r1] if vh else None,
                                            self.values[r0:r1] if vh else None, self.active[r0:r1],
                                            self.kv_len[r0:r1], self.pos[r0:r1], self.tok_in[r0:r1],
                                            self.gen_len[r0:r1], self.step, self.rng_offset, eos_ids, pad_id,
                                            self.attn_len[r0:r1], self.kv_start[r0:r1], rp.max_new[r0:r1])
        elif h.is_cuda:
            vh = self.value_head is not None
            ops.native().decode_update(self.sampled[r0:r1], self.out_tokens[r0:r1], self.out_logp[r0:r1],
                                       self.sampled_lp[r0:r1], self.out_values[r0:r1] if vh else None,
                                       self.values[r0:r1] if vh else None, self.active[r0:r1],
                                       self.kv_len[r0:r1], self.pos[r0:r1], self.tok_in[r0:r1],
                                       self.gen_len[r0:r1], self.step, self.rng_offset, eos_ids, pad_id,
                                       self.attn_len[r0:r1], self.kv_start[r0:r1])
        else:
            self._update_cpu(eos_ids, pad_id, r0, r1)
        if rp is not None and self._stop_on:
            self._stop_rows(r0, r1)

    def _update_cpu(self, eos_ids, pad_id, r0: int = 0, r1: Optional[int] = None):
        """CPU twin of decode_update_kernel over rows [r0, r1): each active row writes at its own
        output position gen_len[b] (the step counter for a static batch)."""
        r1 = self.max_batch if r1 is None else r1
        T = self.out_tokens.shape[1]
        act = self.active[r0:r1].bool()
        gl = self.gen_len[r0:r1]
        act = act & (gl < T)
        # the row's own answer length under per-request sampling
        lim = self.rowp.max_new[r0:r1].clamp(max=T) if self._rows_on else T
        rows = torch.nonzero(act).flatten()
        if rows.numel():
            idx = gl[rows].long()
            samp = self.sampled[r0:r1]
            self.out_tokens[r0 + rows, idx] = samp[rows]
            self.out_logp[r0 + rows, idx] = self.sampled_lp[r0:r1][rows]
            if self.value_head is not None:
                self.out_values[r0 + rows, idx] = self.values[r0:r1][rows]
            fin = torch.isin(samp, eos_ids) | (gl + 1 >= lim)
            gl[act] += 1
            self.kv_len[r0:r1][act] += 1
            self.tok_in[r0:r1].copy_(torch.where(act, samp, torch.full_like(samp, pad_id)))
            self.active[r0:r1][act & fin] = 0
        else:
            self.tok_in[r0:r1].fill_(pad_id)
        self.step += 1
        self.rng_offset += 1
        torch.add(self.kv_len, 1, out=self.attn_len)
        torch.sub(self.kv_len, self.kv_start, out=self.pos)

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def generate(self, prompts: List[List[int]], params: SamplingParams, pad_id: int = 0,
                 eos_ids: Sequence[int] = ()) -> GenerationOutput:
        """Synchronous generation with early exit once every row has finished."""
        return self.generate_async(prompts, params, pad_id, eos_ids, early_stop=True).result()

    @torch.no_grad()
    def generate_async(self, prompts: List[List[int]], params: SamplingParams, pad_id: int = 0,
                       eos_ids: Sequence[int] = (), early_stop=False) -> "_Pending":
        """Enqueue prefill + the decode steps on the current stream and return.

        ``early_stop``:
          * False   — every decode step is enqueued now (the host never waits);
          * True    — stop once every row has finished, polling with a blocking read every
            ``sync_every`` steps (batch-1 answers: the host is idle anyway);
          * "async" — the same early exit without stalling the GPU: steps are enqueued in chunks
            of ``sync_every``; after each chunk the "any row active" flag is copied to pinned host
            memory behind an event, and the host, keeping two chunks queued ahead of the GPU,
            reads a chunk's flag only when the GPU has already started the next one. The first
            two chunks are enqueued here, the rest by ``result()`` (so work the caller does
            between the two calls, e.g. reward scoring, overlaps the decode). Rows are masked
            after EOS, and the sampler's RNG counter is advanced by the skipped steps, so outputs
            and later draws are identical to a run without the exit."""
        import time

        cfg = self.cfg
        dev = self.device
        B = len(prompts)
        assert 0 < B <= self.max_batch, f"batch {B} > max_batch {self.max_batch}"
        S = max(len(p) for p in prompts)
        T = params.max_new_tokens
        if params.max_length is not None:
            T = max(1, min(T, params.max_length - S))
        self._check_lookup(params)
        if not _neutral_penalties(params):
            raise ValueError("logit penalties (repetition_penalty, presence_penalty, frequency_penalty, logit_bias) "
                             "are served by ContinuousBatcher(per_request=True, penalties=True) only, not by "
                             "Generator.generate")
        if not _neutral_stops(params):
            raise ValueError(_STOPS_NEED + ", not by Generator.generate")
        self._rows_on = False  # a batch under one SamplingParams: the scalar sampler and its stream
        self._pen_on = False
        self._stop_on = False
        self._lk_rows = False
        K = params.lookup_tokens
        # the last verify step may append K rows past the last emitted token
        assert S + T + K <= self.max_seq, f"prompt {S} + new {T} (+ {K} draft) exceeds cache {self.max_seq}"
        t0 = time.perf_counter()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if dev.type == "cuda" else None
        if ev:
            ev[0].record()
        ids = torch.full((B, S), pad_id, dtype=torch.long)
        start = torch.zeros(B, dtype=torch.int32)
        for b, p in enumerate(prompts):
            ids[b, S - len(p):] = torch.tensor(p, dtype=torch.long)
            start[b] = S - len(p)
        ids = ids.to(dev, non_blocking=True)
        MB = self.max_batch
        # reset device state (rows >= B stay inactive)
        self.kv_start.zero_()
        self.kv_start[:B].copy_(start.to(dev))
        self.active.zero_()
        self.active[:B] = 1
        self.gen_len.zero_()
        self.step.zero_()
        self.tok_in.fill_(pad_id)
        if self.out_tokens is None or self.out_tokens.shape[1] != T:
            self.out_tokens = torch.full((MB, T), pad_id, dtype=torch.long, device=dev)
            self.out_logp = torch.zeros(MB, T, dtype=torch.float32, device=dev)
            self.out_values = torch.zeros(MB, T, dtype=torch.float32, device=dev)
            self.runner.reset()
        else:
            self.out_tokens.fill_(pad_id)
            self.out_logp.zero_()
            self.out_values.zero_()
        eos_list = list(eos_ids) or [cfg.eos_token_id]
        eos = torch.tensor(eos_list, dtype=torch.long, device=dev)
        # prefill on the first B rows of the cache
        sub = _SubCache(self.cache, B)
        # generation never differentiates: run adapters on merged weights (one weight stream per
        # projection; the merged images are refreshed in place after each adapter update)
        prev_merged = self.model.set_lora_merged(self.merge_lora) if hasattr(self.model, "set_lora_merged") else None
        try:
            return self._enqueue(params, B, S, T, ids, start, eos, eos_list, pad_id, sub, early_stop, t0, ev)
        finally:
            if prev_merged is not None:
                self.model.set_lora_merged(prev_merged)

    def _enqueue(self, params, B, S, T, ids, start, eos, eos_list, pad_id, sub, early_stop, t0, ev):
        cfg, dev, MB = self.cfg, self.device, self.max_batch
        packed = None
        n_real = B * S - int(start.sum())
        if pack_enabled() and n_real < 0.97 * B * S:
            # varlen prefill: the projection GEMMs run on the real prompt tokens only
            packed = packed_index(start.numpy(), np.full(B, S), S, dev)
        h_last = self.model.prefill(ids, self.kv_start[:B], sub, packed=packed) if packed is not None else \
            self.model.prefill(ids, self.kv_start[:B], sub)
        K = params.lookup_tokens
        self._nb = self._bucket(B)
        if K > 0:
            self._check_verify_rows(self._nb, K, fused=dev.type == "cuda")
        if hasattr(self.model, "refresh_decode_weights"):
            # folded / tile-ordered / fp8 images of graph replays; a verify step runs rows * (K + 1) rows
            self.model.refresh_decode_weights(self._nb * (K + 1))
        h = torch.zeros(self._nb, cfg.hidden_size, dtype=h_last.dtype, device=dev)
        h[:B] = h_last
        # the first sampled token is not in the cache yet: the bookkeeping kernel advances kv_len
        # to S, so the first decode step writes it at slot S
        self.kv_len.fill_(S - 1)
        self._emit(h, params, eos, pad_id)
        if ev:
            ev[1].record()
        steps = T - 1
        self._lk = None
        if K > 0:
            st = self._lk = self._lookup_buffers(K)
            st.counters.zero_()  # reported (as zeros) even when no verify step runs (T == 1)
        if K > 0 and steps > 0:
            # history = the left-padded prompt, then the first sampled token at slot S (= kv_len, where
            # the first verify step appends it); the first draft is made outside the captured step
            self.hist[:B, :S] = ids
            self.hist[:self._nb, S] = self.tok_in[:self._nb]
            self._draft(params, pad_id)
        if steps > 0:
            self._ensure_graph(params, eos, eos_list, pad_id, T)
        loop = _DecodeLoop(self, steps, params, eos, pad_id, early_stop)
        loop.run()
        pend = _Pending(self, B, ids, start, t0, ev, loop)
        if loop.finished and ev:
            ev[2].record()
            pend._recorded = True
        return pend

    def _ensure_graph(self, params, eos, eos_list, pad_id, T):
        """The captured decode step for (sampling parameters, output width, row bucket)."""
        key = (T, params.inv_temp, params.top_k, params.top_p, params.greedy, params.seed, tuple(eos_list), pad_id,
               self._nb)
        step = self._step
        if self._rows_on:
            # parameters are read from the row buffers: one graph per bucket whatever the mix
            key = (T, "rows", tuple(eos_list), pad_id, self._nb)
        if _fp4_decode_on(self.model):
            key = key + ("fp4",)  # the captured step of the other setting streams other weight images
        if self.adapters is not None:
            key = key + ("adapters",)  # slots are read from the row buffer: one graph per bucket whatever the mix
        if self._pen_on:
            key = key + ("penalties",)  # the step carries the penalty launch; settings are read from the row buffers
        keep = (eos,)
        if self._stop_on:
            # the step carries the stop scan; stops are read from the row buffers. The byte table's
            # device memory is baked into the step: the key names it and the graph keeps it alive, so a
            # batcher with another table captures its own step instead of replaying this one
            key = key + ("stops", self.token_bytes.key)
            keep = (eos, self.token_bytes.offsets, self.token_bytes.blob)
        if self._lk is not None:
            # a verify step is its own graph per (K, n-gram length); plain keys are unchanged
            key = key + ("lookup", params.lookup_tokens, params.lookup_ngram)
            step = self._step_verify
        if self.use_graph and self.runner.needs(key):
            # the EOS tensor is created per call: the runner keeps the captured one alive
            self.runner.capture(lambda: step(params, eos, pad_id), key, keep=keep, restore=self._state())

    def _replay(self, params, eos, pad_id):
        if self.use_graph:
            self.runner.replay()
        elif self._lk is not None:
            self._step_verify(params, eos, pad_id)
        else:
            self._step(params, eos, pad_id)

    def _state(self):
        st = [self.tok_in, self.kv_len, self.pos, self.attn_len, self.active, self.gen_len, self.step,
              self.rng_offset, self.sampled, self.sampled_lp, self.values, self.out_tokens, self.out_logp,
              self.out_values]
        if self._lk is not None:
            st += [self.hist] + self._lk.tensors()
        if self.rowp is not None:
            st += self.rowp.tensors()
        if self._pen_on:
            st += [self.hist] + self.penp.tensors()
        if self._stop_on:
            st += self.stopp.tensors()
        return st


class _DecodeLoop:
    """Enqueues the decode steps of one generation (see ``Generator.generate_async``)."""

    AHEAD = 2  # chunks kept queued ahead of the GPU in the "async" early-exit mode

    def __init__(self, gen: "Generator", steps: int, params, eos, pad_id, early_stop):
        self.gen, self.steps, self.params, self.eos, self.pad_id = gen, steps, params, eos, pad_id
        self.mode = early_stop
        self.done = 0
        self.pending = []  # (chunk index, event) of flags not read yet
        self.stopped = False
        if early_stop == "async" and steps > 0:
            dev = gen.device
            n = (steps + gen.sync_every - 1) // gen.sync_every
            self.flags_dev = torch.zeros(n, dtype=torch.int32, device=dev)
            self.flags = torch.zeros(n, dtype=torch.int32, pin_memory=dev.type == "cuda")

    @property
    def finished(self) -> bool:
        return self.stopped or self.done >= self.steps

    def _chunk(self, n):
        g = self.gen
        for _ in range(n):
            g._replay(self.params, self.eos, self.pad_id)
        self.done += n

    def run(self, to_end: bool = False):
        g = self.gen
        if self.mode is False:
            self._chunk(self.steps - self.done)
            return
        if self.mode is True:
            while not self.finished:
                self._chunk(min(g.sync_every, self.steps - self.done))
                if self.done < self.steps and int(g.active.sum().item()) == 0:
                    self._stop()
            return
        # "async": keep AHEAD chunks queued; read a chunk's flag once the GPU is past it
        while not self.finished:
            if len(self.pending) >= self.AHEAD:
                c, ev = self.pending.pop(0)
                if not to_end and not ev.query():
                    return  # result() continues from here
                ev.synchronize()
                if int(self.flags[c]) == 0:
                    self._stop()
                    break
            c = self.done // g.sync_every
            self._chunk(min(g.sync_every, self.steps - self.done))
            if self.done < self.steps:
                self.flags_dev[c:c + 1].copy_(g.active.amax().reshape(1))
                self.flags[c:c + 1].copy_(self.flags_dev[c:c + 1], non_blocking=True)
                ev = torch.cuda.Event() if g.device.type == "cuda" else None
                if ev is not None:
                    ev.record()
                    self.pending.append((c, ev))
                elif int(self.flags[c]) == 0:
                    self._stop()
            if not to_end and len(self.pending) >= self.AHEAD:
                return

    def _stop(self):
        """Every row has finished: skip the remaining steps, but advance the sampler's RNG counter
        as if they had run (later generations draw the same numbers either way)."""
        skipped = self.steps - self.done
        if skipped > 0:
            self.gen.rng_offset.add_(skipped)
        self.stopped = True
        self.skipped = skipped


class _Pending:
    """Handle of an enqueued generation; ``result()`` finishes enqueuing (async early exit), waits
    and copies the outputs out."""

    def __init__(self, gen: "Generator", B, ids, start, t0, ev, loop: Optional[_DecodeLoop] = None):
        self.gen, self.B, self.ids, self.start, self.t0, self.ev = gen, B, ids, start, t0, ev
        self.loop = loop
        self.lk = gen._lk  # this generation's lookup buffers (None: plain decoding)
        self._recorded = False

    @torch.no_grad()
    def result(self) -> GenerationOutput:
        import time

        g, B = self.gen, self.B
        if self.loop is not None and not self.loop.finished:
            # the remaining steps run under the same conditions the loop started with: no autograd,
            # adapters merged (generate_async restored the caller's mode on return; the eager
            # non-graph path would otherwise decode with unmerged adapters)
            m = g.model
            prev = m.set_lora_merged(g.merge_lora) if hasattr(m, "set_lora_merged") else None
            try:
                self.loop.run(to_end=True)
            finally:
                if prev is not None:
                    m.set_lora_merged(prev)
        if self.ev and not self._recorded:
            self.ev[2].record()
            self._recorded = True
        if self.ev:
            self.ev[2].synchronize()
        t_total = time.perf_counter() - self.t0
        tim = {"total_s": t_total}
        if self.ev:
            tim["prefill_s"] = self.ev[0].elapsed_time(self.ev[1]) / 1e3
            tim["decode_s"] = self.ev[1].elapsed_time(self.ev[2]) / 1e3
        if self.loop is not None:
            tim["decode_steps"] = self.loop.done
        if self.lk is not None:
            # summed over rows, read once here (no per-step host sync)
            c = self.lk.counters.tolist()
            tim["lookup_steps"], tim["lookup_drafted"], tim["lookup_accepted"] = int(c[0]), int(c[1]), int(c[2])
        return GenerationOutput(g.out_tokens[:B].clone(), g.gen_len[:B].clone().long(), g.out_logp[:B].clone(),
                                g.out_values[:B].clone() if g.value_head is not None else None, self.ids,
                                self.start.to(g.device).long(), tim)


class _LookupState:
    """Static buffers of the verify step for one K (G = K + 1 positions per row)."""

    def __init__(self, B: int, G: int, device):
        self.G = G
        self.inp = torch.zeros(B, G, dtype=torch.long, device=device)          # last emitted token | draft
        self.n_draft = torch.zeros(B, dtype=torch.int32, device=device)
        self.row_active = torch.zeros(B * G, dtype=torch.uint8, device=device)  # the sampler's row mask
        self.sampled = torch.zeros(B * G, dtype=torch.long, device=device)
        self.sampled_lp = torch.zeros(B * G, dtype=torch.float32, device=device)
        self.counters = torch.zeros(3, dtype=torch.long, device=device)         # row-steps, drafted, accepted
        # continuous batch: per row (verify steps it was active in, accepted tokens emitted)
        self.row_stats = torch.zeros(B, 2, dtype=torch.int32, device=device)

    def tensors(self):
        return [self.inp, self.n_draft, self.row_active, self.sampled, self.sampled_lp, self.counters,
                self.row_stats]


class _SubCache:
    """View of the first B batch rows of a KVCache (prefill of a partial batch)."""

    def __init__(self, cache: KVCache, B: int):
        self.k = [cache.k[l, :B] for l in range(cache.k.shape[0])]
        self.v = [cache.v[l, :B] for l in range(cache.v.shape[0])]
        self.fp8 = cache.fp8
        if cache.fp8:
            self.ks = [cache.ks[l, :B] for l in range(cache.ks.shape[0])]
            self.vs = [cache.vs[l, :B] for l in range(cache.vs.shape[0])]

    def scales(self, layer: int):
        return (self.ks[layer], self.vs[layer]) if self.fp8 else (None, None)


def generate_text(model, tokenizer, prompts: List[str], params: SamplingParams, generator: Optional[Generator] = None,
                  max_prompt_tokens: Optional[int] = None) -> List[str]:
    enc = tokenizer.encode_batch(prompts)
    if max_prompt_tokens:
        enc = [e[-max_prompt_tokens:] for e in enc]
    if generator is None:
        S = max(len(e) for e in enc)
        generator = Generator(model, len(enc), S + params.max_new_tokens + 1)
    out = generator.generate(enc, params, pad_id=tokenizer.pad_token_id, eos_ids=[tokenizer.eos_token_id])
    res = []
    for b in range(len(prompts)):
        n = int(out.lengths[b])
        res.append(tokenizer.decode(out.tokens[b, :n].tolist()))
    return res


class _RowCache:
    """View of batch rows [b, b + n) of a KVCache (prefill of admitted requests)."""

    def __init__(self, cache: KVCache, b: int, n: int = 1):
        self.k = [cache.k[l, b:b + n] for l in range(cache.k.shape[0])]
        self.v = [cache.v[l, b:b + n] for l in range(cache.v.shape[0])]
        self.fp8 = cache.fp8
        if cache.fp8:
            self.ks = [cache.ks[l, b:b + n] for l in range(cache.ks.shape[0])]
            self.vs = [cache.vs[l, b:b + n] for l in range(cache.vs.shape[0])]

    def scales(self, layer: int):
        return (self.ks[layer], self.vs[layer]) if self.fp8 else (None, None)


def _check_bank(gen: "Generator", params: SamplingParams, bank):
    """Per-request adapters run decode steps of at most 16 rows on the fused Llama / Mistral layer
    over the unmerged base; everything else is refused with the reason."""
    model = gen.model
    if gen.max_batch > 16:
        raise ValueError(f"per-request adapters: max_batch {gen.max_batch} exceeds the 16 rows of the per-row adapter "
                         f"kernels")
    if params.lookup_tokens > 0:
        raise ValueError("per-request adapters: prompt-lookup decoding (lookup_tokens > 0) is not supported")
    if gen.cfg.arch == "opt":
        raise ValueError("per-request adapters: learned-position (opt) models have no fused decode layer")
    if bank.model is not model:
        raise ValueError("per-request adapters: the bank was built for another model")
    if any(layer.lora and layer.lora_enabled for layer in model.layers):
        raise ValueError("per-request adapters: the model carries LoRA adapters of its own, which decode merged into "
                         "the base weights; save them (save_adapter) and load them into the bank instead")
    if any(getattr(layer, "fp8_enabled", False) for layer in model.layers):
        raise ValueError("per-request adapters: fp8 weights (set_fp8) are not supported yet: the fp8 prefill merges "
                         "adapters into the weights")
    if not getattr(model, "fused_decode", True):
        raise ValueError("per-request adapters need the fused decode layer (model.fused_decode)")


@dataclass
class FinishedRow:
    tag: object
    tokens: List[int]
    logprobs: List[float]
    prompt_len: int
    steps_waited: int
    seed: Optional[int] = None  # per-request sampling: the seed the row drew with (given or derived)
    adapter: Optional[str] = None  # per-request adapters: the adapter the row ran with (None: base model)
    # prompt-lookup decoding (None when off): verify steps the row was active in, and the accepted
    # draft tokens among its output (len(tokens) == 1 + lookup_steps + lookup_accepted)
    lookup_steps: Optional[int] = None
    lookup_accepted: Optional[int] = None
    # why the row left the batch: "stop" (a stop string or stop token id, batchers with stops=True),
    # "eos" or "length"
    finish_reason: Optional[str] = None
    # finish_reason == "stop": the matched stop string or stop token id, and the length in bytes of
    # the stream text to keep (the UTF-8 bytes of decode(tokens) up to where the match begins)
    stop: Optional[object] = None
    text_bytes: Optional[int] = None


class ContinuousBatcher:
    """Iteration-level (continuous) batching over one Generator's static cache and captured decode
    step: a request is admitted into a free batch row between decode steps — its prompt is
    prefilled into that row alone (``_RowCache``), its first token sampled from the prefill — and
    the graph-replayed decode step then advances every active row at once; each row writes at its
    own output position (``decode_update_kernel`` indexes by the row's generated length) and
    leaves the batch when it emits EOS or reaches ``max_new_tokens``, freeing the row for the next
    request. Rows are independent: other rows' K/V, positions and attention lengths are untouched
    by an admission. One sampling configuration per batcher unless ``per_request``; the decode
    step runs the power-of-two bucket of rows that covers the active ones (inactive rows in it are
    masked).

    ``per_request=True``: every admission may bring a ``RequestSampling`` (temperature, top-k, top-p,
    greedy or sampled, seed, answer length). The settings live in per-row device buffers that the
    captured step reads (``ops.sample_rows``, the per-row bookkeeping limit), so one graph per bucket
    serves any mix, and a row's random stream is keyed by (its seed, its generated length): the
    same request draws the same answer in any row, beside any batch mates, at any time. A request
    without a seed gets ``derive_seed(params.seed, admission count)``; ``FinishedRow.seed`` reports
    it. With ``per_request=False`` graph keys and the RNG stream are the scalar sampler's.

    ``lookup_tokens=K`` (1..7; ``lookup_ngram``): prompt-lookup speculative decoding. The replayed
    step is the verify step (``Generator._step_verify``) over K + 1 positions per row, so
    ``max_batch * (K + 1)`` must fit the fused decode layer (16 rows under MXFP4 decode) and a
    prompt needs room for K more cache slots. An admission writes its rows' token history and first
    draft only; a row emits 1 .. K + 1 tokens per step, and ``FinishedRow.lookup_steps`` /
    ``lookup_accepted`` report its verify steps and accepted draft tokens. Greedy answers are the
    plain batcher's. With ``per_request`` the sampler draws position j of a row with the counter of
    output index ``gen_len + j``: a sampled answer is the plain per-request answer for the same
    seed, and ``RequestSampling.lookup_tokens`` (0..K) gives a request its own draft length.
    Not with adapters. ``SamplingParams.lookup_tokens`` stays refused here (it selects lookup for
    ``Generator.generate``); with ``lookup_tokens=0`` nothing differs from a batcher without it.

    ``penalties=True`` (needs ``per_request``): a ``RequestSampling`` may also bring
    ``repetition_penalty``, ``presence_penalty``, ``frequency_penalty`` and ``logit_bias`` (defaults:
    the ``SamplingParams`` fields of the same names). ``ops.logit_rows_penalty`` rewrites the touched
    logits of each row in place between the LM head and the sampler, inside the captured step and on
    an admission's prefill logits, from per-row device buffers and the row's token history
    (``Generator.hist``): one graph per bucket whatever the mix, the reported log-probs are those of
    the penalised distribution, and a neutral row's tokens, log-probs and random stream are those
    of a batcher without the flag. ``max_seq`` at most ``ops.LOGIT_ROWS_MAX_SEQ``; not together with
    ``lookup_tokens``. With the flag off no buffer, graph key or launch differs.

    ``stops=True, token_bytes=ops.TokenBytes`` (needs ``per_request``): a ``RequestSampling`` may also
    bring ``stop`` (one string or at most 4 strings of 1..32 UTF-8 bytes) and ``stop_token_ids`` (at
    most 8; defaults: the ``SamplingParams`` fields of the same names). ``ops.stop_rows`` runs behind
    the bookkeeping kernel of the captured step (between accept and draft of a verify step) and
    eagerly after an admission's first token: it searches the stream text of the row's generated
    tokens (their entries in the vocabulary byte table; the prompt is never searched) and ends the row
    at the first token that completes a stop string or is a stop id. ``FinishedRow.finish_reason`` is
    then ``"stop"``, ``stop`` the matched string or id, and ``text_bytes`` the bytes of
    ``decode(tokens)`` to keep; ``tokens`` run up to and including the token that completed the
    match. One graph per bucket whatever the mix; rows without stops are bit for bit those of a
    batcher without the flag. Works with ``penalties``, ``adapters`` and ``lookup_tokens``; with
    lookup a stop can drop tokens a verify step had already accepted, which a row's
    ``lookup_accepted`` still counts. With the flag off no buffer, graph key or launch differs.

    Usage: ``admit(prompt_ids, tag)`` while ``free_rows()``; ``step(n)``; ``collect()`` returns the
    rows that finished (a host read of the per-row flags once per call)."""

    def __init__(self, gen: Generator, params: SamplingParams, pad_id: int = 0, eos_ids: Sequence[int] = (),
                 per_request: bool = False, adapters=None, lookup_tokens: int = 0, lookup_ngram: int = 2,
                 penalties: bool = False, stops: bool = False, token_bytes=None):
        if adapters is not None:
            _check_bank(gen, params, adapters)
        self.stops = bool(stops)
        if self.stops:
            if not per_request:
                raise ValueError("stop strings are per-request settings: ContinuousBatcher(stops=True) needs "
                                 "per_request=True")
            if not isinstance(token_bytes, ops.TokenBytes):
                raise ValueError("ContinuousBatcher(stops=True) needs token_bytes=ops.TokenBytes.from_tokenizer(...), "
                                 "the vocabulary byte table stop strings are searched through")
            if token_bytes.vocab_size != gen.cfg.vocab_size:
                raise ValueError(f"stop strings: the byte table has {token_bytes.vocab_size} entries, the model's "
                                 f"vocabulary {gen.cfg.vocab_size}")
            if token_bytes.device != gen.device:
                raise ValueError(f"stop strings: the byte table is on {token_bytes.device}, the generator on "
                                 f"{gen.device}")
            _check_stops(params.stop, params.stop_token_ids, gen.cfg.vocab_size)
        elif not _neutral_stops(params):
            raise ValueError("SamplingParams with " + _STOPS_NEED + " (the stops flag is off)")
        self.penalties = bool(penalties)
        if self.penalties:
            if not per_request:
                raise ValueError("logit penalties are per-request settings: ContinuousBatcher(penalties=True) needs "
                                 "per_request=True")
            if int(lookup_tokens) > 0:
                raise ValueError("logit penalties with prompt-lookup decoding (lookup_tokens > 0) are not supported: "
                                 "position j of a verify step would need the draft tokens before it in its history")
            if gen.max_seq > ops.LOGIT_ROWS_MAX_SEQ:
                raise ValueError(f"logit penalties: max_seq {gen.max_seq} exceeds the {ops.LOGIT_ROWS_MAX_SEQ} history "
                                 f"slots the penalty kernel stages per row")
            _check_penalties(params.repetition_penalty, params.presence_penalty, params.frequency_penalty,
                             params.logit_bias, gen.cfg.vocab_size)
        elif not _neutral_penalties(params):
            raise ValueError("SamplingParams with logit penalties (repetition_penalty, presence_penalty, "
                             "frequency_penalty, logit_bias) need ContinuousBatcher(per_request=True, penalties=True)")
        if params.lookup_tokens > 0:
            raise NotImplementedError("prompt-lookup decoding in the continuous batch is selected by the batcher's own "
                                      "keyword, ContinuousBatcher(..., lookup_tokens=K, lookup_ngram=n), not by "
                                      "SamplingParams.lookup_tokens")
        if _fp4_decode_on(gen.model) and gen.max_batch > 16:
            raise ValueError(f"continuous batching with MXFP4 decode (model.fp4_decode): max_batch {gen.max_batch} "
                             f"exceeds the 16 rows of the MXFP4 decode kernels")
        K = int(lookup_tokens)
        # the parameters the generator's step runs under: the caller's, plus the batcher's lookup setting
        self.vparams = params
        if K != 0:
            import dataclasses

            self.vparams = dataclasses.replace(params, lookup_tokens=K, lookup_ngram=int(lookup_ngram))
            gen._check_lookup(self.vparams)
            if adapters is not None:
                raise ValueError("per-request adapters: prompt-lookup decoding (lookup_tokens > 0) is not supported")
            gen._check_verify_rows(gen.max_batch, K)
        self.K = K
        self.gen, self.params, self.pad_id = gen, params, pad_id
        g = gen
        g._lk = None
        g._lk_rows = False
        dev, MB, T = g.device, g.max_batch, params.max_new_tokens
        self.T = T
        self.eos_list = list(eos_ids) or [g.cfg.eos_token_id]
        self.eos = torch.tensor(self.eos_list, dtype=torch.long, device=dev)
        g.active.zero_()
        g.gen_len.zero_()
        g.step.zero_()
        g.kv_start.zero_()
        g.kv_len.zero_()
        g.tok_in.fill_(pad_id)
        if g.out_tokens is None or g.out_tokens.shape[1] != T:
            g.out_tokens = torch.full((MB, T), pad_id, dtype=torch.long, device=dev)
            g.out_logp = torch.zeros(MB, T, dtype=torch.float32, device=dev)
            g.out_values = torch.zeros(MB, T, dtype=torch.float32, device=dev)
            g.runner.reset()
        g._nb = 1
        self.per_request = bool(per_request)
        g._rows_on = self.per_request
        self.admitted = 0   # admission count: numbers the derived seeds
        self.row_seed = {}  # row -> seed (per_request)
        if self.per_request:
            # every row starts at the batcher's defaults (the capture below runs the step on them)
            g._row_buffers().write(0, [RequestSampling().resolve(params, T, 0)] * MB)
        g._pen_on = self.penalties
        if self.penalties:
            # neutral everywhere until an admission writes a row's own (the capture below runs on them)
            g._penalty_buffers().reset()
        g._stop_on = self.stops
        self.row_stops = {}  # row -> (stop string bytes, stop token ids) of its request
        if self.stops:
            # no row has stops until an admission writes its own (the capture below runs on them)
            g.token_bytes = token_bytes
            g._stop_buffers().reset()
        self.lookup_totals = None  # (row-steps, drafted, accepted) of the device counters, read in collect()
        if K > 0:
            # history and the verify step's buffers exist before the capture; no row is active, so the
            # captured step's sampler and bookkeeping are masked everywhere
            st = g._lk = g._lookup_buffers(K)
            g._lk_rows = True
            for t in (st.counters, st.row_stats, st.n_draft, st.row_active):
                t.zero_()
            st.inp.fill_(pad_id)
            # the verify attention's row invariant (slot = keys - 1 >= 0) also for never-admitted rows
            g.attn_len.fill_(1)
            g.pos.zero_()
            if self.per_request:
                g.rowp.draft_buffer(K)
            self.lookup_totals = (0, 0, 0)
        self._prev_merged = g.model.set_lora_merged(g.merge_lora) if hasattr(g.model, "set_lora_merged") else None
        self.adapters = adapters
        self.row_adapter = {}  # row -> adapter name
        g.adapters = adapters
        if adapters is not None:
            if g.adapter_ids is None:
                g.adapter_ids = torch.empty(MB, dtype=torch.int32, device=dev)
            g.adapter_ids.fill_(-1)
            adapters.refresh()
        if hasattr(g.model, "refresh_decode_weights"):
            g.model.refresh_decode_weights(MB * (K + 1))  # a verify step runs K + 1 positions per row
        if T > 1:
            g._ensure_graph(self.vparams, self.eos, self.eos_list, pad_id, T)  # captured while no row is active
        self.rows = {}  # row -> (tag, prompt_len, steps at admission)
        self.free = list(range(MB))
        self.steps = 0

    def close(self):
        self.gen._rows_on = False
        self.gen._pen_on = False
        self.gen._stop_on = False
        self.gen.adapters = None
        if self.K > 0:
            self.gen._lk = None
            self.gen._lk_rows = False
        if self._prev_merged is not None:
            self.gen.model.set_lora_merged(self._prev_merged)
            self._prev_merged = None

    def free_rows(self) -> int:
        return len(self.free)

    def active_rows(self) -> int:
        return len(self.rows)

    @torch.no_grad()
    def admit(self, prompt: List[int], tag=None, sampling: Optional[RequestSampling] = None,
              adapter: Optional[str] = None) -> int:
        return self.admit_many([prompt], [tag], [sampling], [adapter])[0]

    @torch.no_grad()
    def admit_many(self, prompts: List[List[int]], tags=None, sampling=None, adapters=None) -> List[int]:
        """Admit len(prompts) <= free_rows() requests. The lowest free rows are taken and every run
        of consecutive rows is prefilled as ONE left-padded batch into its cache rows.
        ``sampling``: one ``RequestSampling`` or None per prompt (``per_request`` batchers only).
        ``adapters``: one loaded adapter name or None (base model) per prompt (batchers with a bank)."""
        g = self.gen
        tags = list(tags) if tags is not None else [None] * len(prompts)
        sampling = list(sampling) if sampling is not None else [None] * len(prompts)
        adapters = list(adapters) if adapters is not None else [None] * len(prompts)
        if len(sampling) != len(prompts):
            raise ValueError(f"{len(sampling)} sampling entries for {len(prompts)} prompts")
        if len(adapters) != len(prompts):
            raise ValueError(f"{len(adapters)} adapter entries for {len(prompts)} prompts")
        if self.adapters is None and any(a is not None for a in adapters):
            raise ValueError("per-request adapters need ContinuousBatcher(adapters=bank)")
        # unknown names fail here (KeyError), before any row is taken
        slots = [self.adapters.slot(a) for a in adapters] if self.adapters is not None else None
        if not self.per_request and any(s is not None for s in sampling):
            raise ValueError("per-request sampling settings need ContinuousBatcher(per_request=True)")
        if len(prompts) > len(self.free):
            raise ValueError(f"{len(prompts)} requests for {len(self.free)} free rows")
        if not self.penalties and any(s is not None and s.has_penalties for s in sampling):
            raise ValueError("logit penalty settings need ContinuousBatcher(per_request=True, penalties=True)")
        if not self.stops and any(s is not None and s.has_stops for s in sampling):
            raise ValueError("stop / stop_token_ids in the request need ContinuousBatcher(per_request=True, stops=True, "
                             "token_bytes=...): the stops flag is off")
        resolved = drafts = pens = stops = None
        if self.per_request:
            # validated before any row is taken; unseeded requests are numbered by admission
            for s in sampling:
                if s is not None:
                    s.validate(self.T, self.K, g.cfg.vocab_size)
            if self.penalties:
                pens = [(s or RequestSampling()).resolve_penalties(self.params, g.cfg.vocab_size) for s in sampling]
            if self.stops:
                stops = [(s or RequestSampling()).resolve_stops(self.params, g.cfg.vocab_size) for s in sampling]
            resolved = [(s or RequestSampling()).resolve(self.params, self.T, derive_seed(self.params.seed,
                                                                                         self.admitted + i))
                        for i, s in enumerate(sampling)]
            if self.K > 0:
                drafts = [self.K if s is None or s.lookup_tokens is None else s.lookup_tokens for s in sampling]
        for p in prompts:
            # the last verify step may append K rows past the last emitted token
            if len(p) < 1 or len(p) + self.T + self.K > g.max_seq:
                raise ValueError(f"prompt of {len(p)} tokens + {self.T} new" + (f" + {self.K} draft" if self.K else "") +
                                 f" exceeds the cache ({g.max_seq})")
        self.free.sort()
        rows, self.free = self.free[:len(prompts)], self.free[len(prompts):]
        try:
            if slots is None:
                self._admit_runs(rows, prompts, tags, resolved, drafts, pens, stops)
            else:
                self._admit_adapter_runs(rows, prompts, tags, resolved, adapters, slots, pens, stops)
        except BaseException:
            # all-or-nothing: rows of this call that were already prefilled leave the batch again
            # (inactive, back on the free list), so the caller can fail every request it passed
            for b in rows:
                self.rows.pop(b, None)
                self.row_seed.pop(b, None)
                self.row_adapter.pop(b, None)
                self.row_stops.pop(b, None)
            g.active[torch.tensor(rows, device=g.device)] = 0
            self.free = sorted(self.free + rows)
            raise
        self.admitted += len(prompts)
        return rows

    def _admit_adapter_runs(self, rows, prompts, tags, resolved, names, slots, pens=None, stops=None):
        """``_admit_runs`` per piece of consecutive rows with one adapter: each piece is prefilled with
        its slot active, unmerged (``AdapterBank.active``), under ``ops.batch_invariant`` — the
        K-extension GEMMs whatever the piece's token count, i.e. the scoring forward's numerics."""
        g = self.gen
        i = 0
        while i < len(rows):
            j = i + 1
            while j < len(rows) and rows[j] == rows[j - 1] + 1 and slots[j] == slots[i]:
                j += 1
            g.adapter_ids[rows[i]:rows[i] + (j - i)].fill_(slots[i])
            with self.adapters.active(names[i]), ops.batch_invariant():
                self._admit_runs(rows[i:j], prompts[i:j], tags[i:j], None if resolved is None else resolved[i:j],
                                 None, None if pens is None else pens[i:j], None if stops is None else stops[i:j])
            for r in range(i, j):
                self.row_adapter[rows[r]] = names[r]
            i = j

    def _admit_runs(self, rows, prompts, tags, resolved=None, drafts=None, pens=None, stops=None):
        g = self.gen
        i = 0
        while i < len(rows):
            j = i + 1
            while j < len(rows) and rows[j] == rows[j - 1] + 1:
                j += 1
            b0, n = rows[i], j - i
            grp = prompts[i:j]
            S = max(len(p) for p in grp)
            ids = torch.full((n, S), self.pad_id, dtype=torch.long)
            start = torch.zeros(n, dtype=torch.int32)
            for r, p in enumerate(grp):
                ids[r, S - len(p):] = torch.tensor(p, dtype=torch.long)
                start[r] = S - len(p)
            g.kv_start[b0:b0 + n].copy_(start.to(g.device, non_blocking=True))
            ids = ids.to(g.device, non_blocking=True)
            h_last = g.model.prefill(ids, g.kv_start[b0:b0 + n], _RowCache(g.cache, b0, n))
            g.kv_len[b0:b0 + n].fill_(S - 1)  # the first bookkeeping advances them to S
            g.gen_len[b0:b0 + n].zero_()
            g.active[b0:b0 + n].fill_(1)
            if resolved is not None:
                g.rowp.write(b0, resolved[i:j])
            if stops is not None:
                # the row's own stops and a fresh scan state, before _emit scans the first token
                g.stopp.write(b0, stops[i:j])
            if pens is not None:
                # the prefill logits are penalised over the prompt alone (no generated token yet); the
                # first sampled token then sits at slot S, where the first decode step appends it again
                g.penp.write(b0, pens[i:j])
                g.hist[b0:b0 + n, :S] = ids
                g._emit(h_last, self.params, self.eos, self.pad_id, r0=b0, append=False)
                g.hist[b0:b0 + n, S] = g.tok_in[b0:b0 + n]
            else:
                g._emit(h_last, self.params, self.eos, self.pad_id, r0=b0)
            if self.K > 0:
                # what _enqueue does for a static batch, for these rows alone: history = the left-padded
                # prompt, then the first sampled token at slot S (= kv_len, where the first verify step
                # appends it), and the first draft. Slots past S hold the previous occupant's tokens,
                # which the drafter never reads (it searches [kv_start, kv_len]).
                g.hist[b0:b0 + n, :S] = ids
                g.hist[b0:b0 + n, S] = g.tok_in[b0:b0 + n]
                g._lk.row_stats[b0:b0 + n].zero_()
                if drafts is not None:
                    g.rowp.row_draft[b0:b0 + n].copy_(torch.tensor(drafts[i:j], dtype=torch.int32))
                g._draft(self.vparams, self.pad_id, b0, b0 + n)
            for r in range(n):
                self.rows[b0 + r] = (tags[i + r], len(grp[r]), self.steps)
                if resolved is not None:
                    self.row_seed[b0 + r] = resolved[i + r][4]
                if stops is not None:
                    self.row_stops[b0 + r] = stops[i + r]
            i = j

    def step(self, n: int = 1):
        """n decode steps over the power-of-two bucket of rows covering every active row (rows are
        handed out lowest-first, so the active set stays compact); one captured graph per bucket."""
        g = self.gen
        nb = g._bucket(max(self.rows) + 1 if self.rows else 1)
        if nb != g._nb:
            g._nb = nb
            if self.T > 1:
                g._ensure_graph(self.vparams, self.eos, self.eos_list, self.pad_id, self.T)
        for _ in range(n):
            g._replay(self.vparams, self.eos, self.pad_id)
        self.steps += n

    def collect(self) -> List[FinishedRow]:
        """Rows that have finished since the last call (their outputs copied to the host)."""
        if not self.rows:
            return []
        g = self.gen
        act = g.active.cpu()
        done = [b for b in self.rows if not bool(act[b])]
        out = []
        if done:
            idx = torch.tensor(done, device=g.device)
            lens = g.gen_len.index_select(0, idx).cpu().tolist()
            toks = g.out_tokens.index_select(0, idx).cpu()
            lps = g.out_logp.index_select(0, idx).cpu()
            stats = [(None, None)] * len(done)
            if self.K > 0:
                # the stream is already drained by the reads above: two more small copies, no new wait
                stats = g._lk.row_stats.index_select(0, idx).cpu().tolist()
                self.lookup_totals = tuple(int(c) for c in g._lk.counters.tolist())
            hits = [(-1, 0)] * len(done)
            if self.stops:
                hits = list(zip(g.stopp.stop_hit.index_select(0, idx).cpu().tolist(),
                                g.stopp.stop_at.index_select(0, idx).cpu().tolist()))
            for b, n, t, lp, (ls, la), (hit, at) in zip(done, lens, toks, lps, stats, hits):
                tag, S, s0 = self.rows.pop(b)
                toks_b = t[:n].tolist()
                strings, ids = self.row_stops.pop(b, ((), ()))
                reason, what, keep = "length", None, None
                if hit >= 0:
                    reason, keep = "stop", at
                    what = strings[hit].decode("utf-8", "replace") if hit < ops.STOP_MAX_STR else \
                        ids[hit - ops.STOP_MAX_STR]
                elif toks_b and toks_b[-1] in self.eos_list:
                    reason = "eos"
                out.append(FinishedRow(tag, toks_b, lp[:n].tolist(), S, self.steps - s0,
                                       self.row_seed.pop(b, None), self.row_adapter.pop(b, None), ls, la,
                                       reason, what, keep))
                self.free.append(b)
        return out
