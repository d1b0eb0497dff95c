"""Continuous (iteration-level) batching for RAG answering.

Where ``BatchingEngine`` forms a batch and runs it to completion, ``ContinuousEngine`` keeps one
decode batch running: between chunks of ``chunk`` graph-replayed decode steps the worker thread
admits queued requests into free rows (one batched retrieval for the newcomers, then a per-row
prefill, ``generation.ContinuousBatcher``) and hands finished rows back to their callers. A new
request waits for at most one chunk plus its prefill instead of a whole in-flight generation, and
the batch stays full under load.

Same client API as ``BatchingEngine``: ``submit`` -> Future[RagAnswer], ``answer``, ``answer_many``,
``close``. ``timings``: ``queue_s`` (submit -> admission), ``total_s`` (submit -> answer),
``retrieve_s``, ``new_tokens``, ``prompt_tokens``, ``decode_steps`` (steps the row was in flight).

``per_request_sampling=True``: ``submit(..., sampling=RequestSampling(...))`` gives a request its own
temperature, top-k, top-p, greedy flag, seed and answer length inside the shared batch
(``ContinuousBatcher(per_request=True)``); ``timings["seed"]`` is the seed the answer was drawn
with, so a client can ask for the same answer again.

``adapters=bank`` (``models.AdapterBank``): ``submit(..., adapter="name")`` answers with that loaded
LoRA adapter over the shared base weights, beside rows of other adapters or of the base model
(``ContinuousBatcher(adapters=bank)``, at most 16 rows); ``timings["adapter"]`` reports it.

Prompt-lookup decoding: a pipeline whose ``sampling.lookup_tokens`` is K > 0 (``serve
--eval.lookup_tokens=3``) runs the batch on verify steps (``ContinuousBatcher(lookup_tokens=K,
lookup_ngram=n)``; the batcher's ``SamplingParams`` carry ``lookup_tokens=0``). An answer's
``timings`` gain ``lookup_steps`` (verify steps the row was active in) and ``lookup_accepted`` (its
accepted draft tokens); ``stats`` keeps the running totals ``lookup_steps`` / ``lookup_drafted`` /
``lookup_accepted`` over all rows. With ``per_request_sampling`` a request may bring its own
``RequestSampling.lookup_tokens`` in 0..K. Not together with adapters.

``logit_penalties=True`` (needs ``per_request_sampling``; not with prompt-lookup decoding): a request's
``RequestSampling`` may also carry ``repetition_penalty``, ``presence_penalty``, ``frequency_penalty``
and ``logit_bias`` (``ContinuousBatcher(penalties=True)``).

``stop_sequences=True`` (needs ``per_request_sampling``): a request's ``RequestSampling`` may also
carry ``stop`` and ``stop_token_ids`` (``ContinuousBatcher(stops=True)``; the engine builds the
vocabulary byte table from the pipeline's tokenizer). The decoded answer is cut where the match
begins, and every answer's ``timings`` gain ``finish_reason`` (``"stop"``, ``"eos"`` or ``"length"``).
"""
from __future__ import annotations

import concurrent.futures as cf
import queue
import threading
import time
from typing import List, Optional

import torch

import dataclasses

from ..generation import ContinuousBatcher, RequestSampling
from ..rag.pipeline import RagAnswer
from ..rag.prompt import extract_answer


class ContinuousEngine:
    def __init__(self, pipeline, chunk: int = 4, per_request_sampling: bool = False, adapters=None,
                 logit_penalties: bool = False, stop_sequences: bool = False):
        if stop_sequences and not per_request_sampling:
            raise ValueError("stop_sequences needs per_request_sampling=True (stops are per-request settings)")
        self.stop_sequences = bool(stop_sequences)
        self._token_bytes = None  # the vocabulary byte table (stop_sequences), built by the worker
        if logit_penalties and not per_request_sampling:
            raise ValueError("logit_penalties needs per_request_sampling=True (penalties are per-request settings)")
        self.logit_penalties = bool(logit_penalties)
        self.lookup_tokens = int(pipeline.sampling.lookup_tokens)
        self.lookup_ngram = int(getattr(pipeline.sampling, "lookup_ngram", 2))
        layers = getattr(pipeline.gen.model, "layers", None)
        if layers and getattr(layers[0], "fp4_decode", False) and pipeline.max_batch > 16:
            raise ValueError(f"continuous batching with MXFP4 decode (model.fp4_decode): max_batch {pipeline.max_batch} "
                             f"exceeds the 16 rows of the MXFP4 decode kernels")
        self.pipeline = pipeline
        self.chunk = max(1, chunk)
        self.per_request_sampling = bool(per_request_sampling)
        self.adapters = adapters
        self._q: "queue.Queue" = queue.Queue()
        self._closed = False
        self._dead: Optional[BaseException] = None  # the error that ended the worker, if any
        self._lock = threading.Lock()  # submit's closed-check + put vs the worker's final drain
        self.stats = {"admitted": 0, "finished": 0, "steps": 0, "max_active": 0}
        if self.lookup_tokens > 0:
            self.stats.update({"lookup_steps": 0, "lookup_drafted": 0, "lookup_accepted": 0})
        self._row_steps = 0  # sum over decode steps of the active rows (an answer's mean batch)
        self._ready = threading.Event()
        self._init_error = None
        self._worker = threading.Thread(target=self._loop, name="rag-continuous", daemon=True)
        self._worker.start()
        self._ready.wait()
        if self._init_error is not None:
            raise self._init_error

    # ---------------------------------------------------------------- client side
    def submit(self, query: str, top_k: Optional[int] = None,
               sampling: Optional[RequestSampling] = None, adapter: Optional[str] = None) -> cf.Future:
        if adapter is not None:
            if self.adapters is None:
                raise ValueError("an adapter in the request needs ContinuousEngine(adapters=bank)")
            self.adapters.slot(adapter)  # KeyError for a name that is not loaded
        if sampling is not None:
            if not self.per_request_sampling:
                raise ValueError("per-request sampling settings need ContinuousEngine(per_request_sampling=True)")
            if sampling.has_penalties and not self.logit_penalties:
                raise ValueError("logit penalty settings in the request need ContinuousEngine(logit_penalties=True)")
            if sampling.has_stops and not self.stop_sequences:
                raise ValueError("stop / stop_token_ids in the request need ContinuousEngine(stop_sequences=True)")
            sampling.validate(self.pipeline.sampling.max_new_tokens, self.lookup_tokens,
                              self.pipeline.gen.cfg.vocab_size)
        with self._lock:
            if self._closed:
                if self._dead is not None:
                    raise RuntimeError(f"ContinuousEngine worker failed: {self._dead!r}") from self._dead
                raise RuntimeError("ContinuousEngine is closed")
            fut: cf.Future = cf.Future()
            self._q.put((query, top_k, fut, time.perf_counter(), sampling, adapter))
        return fut

    @property
    def alive(self) -> bool:
        return not self._closed and self._worker.is_alive()

    def answer(self, query: str, top_k: Optional[int] = None, timeout: Optional[float] = None,
               sampling: Optional[RequestSampling] = None, adapter: Optional[str] = None) -> RagAnswer:
        return self.submit(query, top_k, sampling, adapter).result(timeout)

    def answer_many(self, queries: List[str], timeout: Optional[float] = None) -> List[RagAnswer]:
        futs = [self.submit(q) for q in queries]
        return [f.result(timeout) for f in futs]

    def close(self, timeout: Optional[float] = 60.0):
        with self._lock:
            was_open, self._closed = not self._closed, True
        if was_open:
            self._q.put(None)
        self._worker.join(timeout)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---------------------------------------------------------------- worker
    def _admit(self, cb: ContinuousBatcher, items):
        p = self.pipeline
        live = [it for it in items if it[2].set_running_or_notify_cancel()]
        if not live:
            return
        t0 = time.perf_counter()
        try:
            ks = [it[1] or p.top_k for it in live]
            scores, ids = p.retrieve([it[0] for it in live], max(ks))
            ids_l = [row[:k] for row, k in zip(ids.tolist(), ks)]
            sc_l = [row[:k] for row, k in zip(scores.tolist(), ks)]
        except BaseException as e:  # noqa: BLE001
            for it in live:
                it[2].set_exception(e)
            return
        t1 = time.perf_counter()
        prompts, metas, samplings, names = [], [], [], []
        for it, row_ids, row_sc in zip(live, ids_l, sc_l):
            docs = [p.docs[i] for i in row_ids if i >= 0]
            prompt = p._prompt_ids(it[0], docs)
            if len(prompt) + cb.T + cb.K > p.gen.max_seq:
                it[2].set_exception(ValueError("prompt does not fit the serving cache"))
                continue
            prompts.append(prompt)
            samplings.append(it[4])
            names.append(it[5])
            metas.append({"query": it[0], "fut": it[2], "t_submit": it[3], "t_admit": time.perf_counter(),
                          "retrieve_s": t1 - t0, "doc_ids": row_ids, "docs": docs, "scores": row_sc,
                          "rows0": (self._row_steps, self.stats["steps"])})
        if not prompts:
            return
        try:
            # consecutive free rows share one prefill
            cb.admit_many(prompts, metas, samplings if self.per_request_sampling else None,
                          names if self.adapters is not None else None)
        except BaseException as e:  # noqa: BLE001
            for m in metas:
                m["fut"].set_exception(e)
            return
        self.stats["admitted"] += len(prompts)

    def _finish(self, rows):
        p = self.pipeline
        now = time.perf_counter()
        for r in rows:
            m = r.tag
            if m["fut"].done():  # failed or cancelled elsewhere: nothing to deliver
                continue
            if r.text_bytes is not None:
                # the stream text from the byte table, cut where the match begins: a cut (or a stop
                # token) inside a multi-byte character decodes with replacement instead of raising
                text = self._token_bytes.stream_text(r.tokens)[:r.text_bytes].decode("utf-8", "replace")
            else:
                text = p.tok.decode(r.tokens)
            text = extract_answer(text)
            rs0, st0 = m["rows0"]
            steps = self.stats["steps"] - st0
            tim = {"queue_s": m["t_admit"] - m["t_submit"], "retrieve_s": m["retrieve_s"],
                   "total_s": now - m["t_submit"], "new_tokens": len(r.tokens), "prompt_tokens": r.prompt_len,
                   "decode_steps": r.steps_waited,
                   "batch_size": (self._row_steps - rs0) / steps if steps > 0 else 0.0}
            if r.seed is not None:
                tim["seed"] = r.seed
            if self.adapters is not None:
                tim["adapter"] = r.adapter
            if self.stop_sequences:
                tim["finish_reason"] = r.finish_reason
            if r.lookup_steps is not None:
                tim["lookup_steps"], tim["lookup_accepted"] = r.lookup_steps, r.lookup_accepted
            m["fut"].set_result(RagAnswer(m["query"], text, m["doc_ids"], m["docs"], m["scores"], tim))
            self.stats["finished"] += 1

    def _loop(self):
        p = self.pipeline
        try:
            if self.stop_sequences:
                from ..ops import TokenBytes

                # one table per generator and tokenizer: engines that follow each other on a pipeline
                # share it, and with it the captured steps that read it
                tb = p.gen.token_bytes
                if not (isinstance(tb, TokenBytes) and tb.source is p.tok and tb.device == p.gen.device):
                    tb = TokenBytes.from_tokenizer(p.tok, p.gen.device, p.gen.cfg.vocab_size)
                self._token_bytes = tb
            # the batcher takes lookup as its own keyword; its SamplingParams carry none
            cb = ContinuousBatcher(p.gen, dataclasses.replace(p.sampling, lookup_tokens=0),
                                   pad_id=p.tok.pad_token_id, eos_ids=[p.tok.eos_token_id],
                                   per_request=self.per_request_sampling, adapters=self.adapters,
                                   lookup_tokens=self.lookup_tokens, lookup_ngram=self.lookup_ngram,
                                   penalties=self.logit_penalties, stops=self.stop_sequences,
                                   token_bytes=self._token_bytes)
        except BaseException as e:  # noqa: BLE001
            self._init_error = e
            self._ready.set()
            return
        self._ready.set()
        stop = False
        try:
            with torch.no_grad():
                while True:
                    # admissions: block only when nothing is in flight
                    new = []
                    while not stop and len(new) < cb.free_rows():
                        try:
                            item = self._q.get(timeout=0.1) if (cb.active_rows() == 0 and not new) else \
                                self._q.get_nowait()
                        except queue.Empty:
                            break
                        if item is None:
                            stop = True
                            break
                        new.append(item)
                    if new:
                        self._admit(cb, new)
                    if cb.active_rows() == 0:
                        if stop:
                            break
                        continue
                    self.stats["max_active"] = max(self.stats["max_active"], cb.active_rows())
                    self._row_steps += cb.active_rows() * self.chunk
                    cb.step(self.chunk)
                    self.stats["steps"] += self.chunk
                    done = cb.collect()
                    if cb.lookup_totals is not None:
                        (self.stats["lookup_steps"], self.stats["lookup_drafted"],
                         self.stats["lookup_accepted"]) = cb.lookup_totals
                    self._finish(done)
        except BaseException as e:  # noqa: BLE001 - in-flight callers get the error
            self._dead = e
            for b, (meta, _, _) in list(cb.rows.items()):
                if not meta["fut"].done():
                    meta["fut"].set_exception(e)
            cb.rows.clear()
        finally:
            # the worker is gone for good: later submits raise instead of queueing futures nothing
            # would resolve, and whatever is queued now fails
            with self._lock:
                self._closed = True
                pending = []
                while True:
                    try:
                        pending.append(self._q.get_nowait())
                    except queue.Empty:
                        break
            cb.close()
            err = RuntimeError(f"ContinuousEngine worker failed: {self._dead!r}" if self._dead is not None
                               else "ContinuousEngine closed")
            for item in pending:
                if item is not None and item[2].set_running_or_notify_cancel():
                    item[2].set_exception(err)
