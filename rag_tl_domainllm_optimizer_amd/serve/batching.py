"""Dynamic request batching for RAG answering (the serving half of SURVEY §2 D8 / N2).

Concurrent callers (HTTP handlers, threads) ``submit`` queries and get futures; ONE worker thread
owns the GPU: it takes the first waiting request, keeps collecting for at most ``max_wait_s`` or
until ``pipeline.max_batch`` requests are queued, and answers the group with one batched retrieve
(query encoder + IVF scan), one prefill and one graph-replayed decode (``RagPipeline.answer``). A
decode step at batch 16 costs 3.25 ms against 2.92 ms at batch 1 on Mistral-7B (README), so under
load the engine serves ~an order of magnitude more answers per second than one-at-a-time
generation, at the price of up to ``max_wait_s`` of queueing for the first request of a group.

Each answer's ``timings`` gains ``queue_s`` (submit -> its batch starts) and ``batch_size``.
"""
from __future__ import annotations

import concurrent.futures as cf
import queue
import threading
import time
from typing import List, Optional


class BatchingEngine:
    def __init__(self, pipeline, max_wait_s: float = 0.004, max_batch: Optional[int] = None):
        self.pipeline = pipeline
        self.max_batch = max(1, min(max_batch or pipeline.max_batch, pipeline.max_batch))
        self.max_wait_s = max_wait_s
        self._q: "queue.Queue" = queue.Queue()
        self._closed = False
        self.stats = {"batches": 0, "requests": 0, "max_batch_seen": 0}
        self._worker = threading.Thread(target=self._loop, name="rag-batching", daemon=True)
        self._worker.start()

    # ---------------------------------------------------------------- client side
    def submit(self, query: str, top_k: Optional[int] = None, sampling=None) -> cf.Future:
        if sampling is not None:
            # a request group runs to completion under the pipeline's one SamplingParams
            raise ValueError("BatchingEngine does not support per-request sampling settings; use "
                             "ContinuousEngine(per_request_sampling=True) (and logit_penalties=True for "
                             "repetition_penalty, presence_penalty, frequency_penalty and logit_bias, stop_sequences=True "
                             "for stop and stop_token_ids)")
        if self._closed:
            raise RuntimeError("BatchingEngine is closed")
        fut: cf.Future = cf.Future()
        self._q.put((query, top_k, fut, time.perf_counter()))
        return fut

    def answer(self, query: str, top_k: Optional[int] = None, timeout: Optional[float] = None):
        return self.submit(query, top_k).result(timeout)

    def answer_many(self, queries: List[str], timeout: Optional[float] = None):
        futs = [self.submit(q) for q in queries]
        return [f.result(timeout) for f in futs]

    def close(self, timeout: Optional[float] = 30.0):
        if not self._closed:
            self._closed = True
            self._q.put(None)
            self._worker.join(timeout)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---------------------------------------------------------------- worker
    def _collect(self, first) -> tuple:
        batch, stop = [first], False
        deadline = time.perf_counter() + self.max_wait_s
        while len(batch) < self.max_batch:
            rem = deadline - time.perf_counter()
            try:
                item = self._q.get(timeout=rem) if rem > 0 else self._q.get_nowait()
            except queue.Empty:
                break
            if item is None:
                stop = True
                break
            batch.append(item)
        return batch, stop

    def _loop(self):
        stop = False
        while not stop:
            try:
                first = self._q.get(timeout=0.1)
            except queue.Empty:
                continue
            if first is None:
                break
            batch, stop = self._collect(first)
            live = [it for it in batch if it[2].set_running_or_notify_cancel()]
            if not live:
                continue
            t_start = time.perf_counter()
            try:
                res = self.pipeline.answer([it[0] for it in live], top_ks=[it[1] for it in live])
            except BaseException as e:  # noqa: BLE001 - every waiting caller gets the error
                for it in live:
                    it[2].set_exception(e)
                continue
            for it, r in zip(live, res):
                r.timings["queue_s"] = t_start - it[3]
                r.timings["batch_size"] = len(live)
                r.timings["total_s"] = r.timings.get("total_s", 0.0) + r.timings["queue_s"]
                it[2].set_result(r)
            self.stats["batches"] += 1
            self.stats["requests"] += len(live)
            self.stats["max_batch_seen"] = max(self.stats["max_batch_seen"], len(live))
        # drain: anything still queued after close() fails fast instead of hanging its caller
        while True:
            try:
                item = self._q.get_nowait()
            except queue.Empty:
                break
            if item is not None and item[2].set_running_or_notify_cancel():
                item[2].set_exception(RuntimeError("BatchingEngine closed"))
