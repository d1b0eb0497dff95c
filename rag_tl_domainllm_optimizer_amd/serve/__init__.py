"""HTTP answer service (the README's optional frontend, README.md:9,31: Streamlit / Gradio are not
installed; FastAPI + uvicorn are). POST /answer {"query": "...", "top_k": 3} ->
{"answer", "doc_ids", "docs", "scores", "timings"}; GET /health; GET /stats.
With ``per_request_sampling`` (config ``serve.per_request_sampling``, continuous batching only) the
body may also carry ``temperature``, ``top_k_tokens``, ``top_p``, ``do_sample``, ``seed`` and
``max_new_tokens``; ``timings["seed"]`` returns the seed the answer was drawn with. On a server
with prompt-lookup decoding (``serve --eval.lookup_tokens=3``; GET /health reports ``lookup_tokens``)
the body may also carry ``lookup_tokens`` in 0..K, the request's own draft length. With
``logit_penalties`` (config ``serve.logit_penalties``, needs ``per_request_sampling``) the body may
also carry ``repetition_penalty``, ``presence_penalty``, ``frequency_penalty`` and ``logit_bias``, a
JSON object of token id (as a string) -> bias, as in the OpenAI API. With ``stop_sequences`` (config
``serve.stop_sequences``, needs ``per_request_sampling``) the body may also carry ``stop`` (a string or
a list of at most 4 strings of 1..32 UTF-8 bytes) and ``stop_token_ids`` (at most 8); the answer ends
where the first of them begins, and ``timings["finish_reason"]`` says why the answer ended
(``"stop"``, ``"eos"`` or ``"length"``).

Concurrent requests are batched: the async handler awaits a future while one worker thread owns the
GPU — by default ``serve.continuous.ContinuousEngine`` (requests join the running decode batch
between steps), or ``serve.batching.BatchingEngine`` (batches formed per request group and run to
completion)."""

from typing import Optional

from .batching import BatchingEngine  # noqa: F401
from .continuous import ContinuousEngine  # noqa: F401


SAMPLING_FIELDS = ("temperature", "top_k_tokens", "top_p", "do_sample", "seed", "max_new_tokens", "lookup_tokens")
PENALTY_FIELDS = ("repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias")
STOP_FIELDS = ("stop", "stop_token_ids")


def request_sampling(q, max_new_tokens: Optional[int] = None, lookup_tokens: Optional[int] = None,
                     vocab: Optional[int] = None):
    """The ``RequestSampling`` of an /answer body (None when it sets no sampling field); ValueError
    for a value outside its range. ``top_k`` stays the document count: the token top-k is
    ``top_k_tokens``. ``lookup_tokens``: the engine's draft length K (0: lookup off; None: the
    body's value is only checked against 0..7). ``vocab``: the vocabulary ``logit_bias`` tokens must
    lie in (None: not checked here)."""
    from ..generation import RequestSampling

    vals = {f: getattr(q, f, None) for f in SAMPLING_FIELDS + PENALTY_FIELDS + STOP_FIELDS}
    if all(v is None for v in vals.values()):
        return None
    rs = RequestSampling(temperature=vals["temperature"], top_k=vals["top_k_tokens"], top_p=vals["top_p"],
                         do_sample=vals["do_sample"], seed=vals["seed"], max_new_tokens=vals["max_new_tokens"],
                         lookup_tokens=vals["lookup_tokens"], **{f: vals[f] for f in PENALTY_FIELDS + STOP_FIELDS})
    rs.validate(max_new_tokens, lookup_tokens, vocab)
    return rs


def create_app(pipeline, max_wait_s: float = 0.004, continuous: bool = False, per_request_sampling: bool = False,
               adapters=None, logit_penalties: bool = False, stop_sequences: bool = False):
    import asyncio
    from typing import Dict, List, Union

    from fastapi import FastAPI, HTTPException
    from pydantic import BaseModel

    if per_request_sampling and not continuous:
        raise ValueError("per_request_sampling needs continuous batching (continuous=True)")
    if adapters is not None and not continuous:
        raise ValueError("per-request adapters need continuous batching (continuous=True)")
    if logit_penalties and not per_request_sampling:
        raise ValueError("logit_penalties needs per_request_sampling (penalties are per-request settings)")
    if stop_sequences and not per_request_sampling:
        raise ValueError("stop_sequences needs per_request_sampling (stops are per-request settings)")
    if continuous:
        engine = ContinuousEngine(pipeline, per_request_sampling=per_request_sampling, adapters=adapters,
                                  logit_penalties=bool(logit_penalties), stop_sequences=bool(stop_sequences))
    else:
        engine = BatchingEngine(pipeline, max_wait_s=max_wait_s)
    vocab = getattr(getattr(getattr(pipeline, "gen", None), "cfg", None), "vocab_size", None)
    app = FastAPI(title="rag-tl-domainllm-optimizer-amd")
    app.state.engine = engine
    engine_k = getattr(engine, "lookup_tokens", 0) if continuous else 0  # the verify steps' draft length

    class Query(BaseModel):
        query: str
        top_k: Optional[int] = None  # retrieved documents
        temperature: Optional[float] = None
        top_k_tokens: Optional[int] = None
        top_p: Optional[float] = None
        do_sample: Optional[bool] = None
        seed: Optional[int] = None
        max_new_tokens: Optional[int] = None
        lookup_tokens: Optional[int] = None  # draft tokens per step, 0 .. the server's eval.lookup_tokens
        adapter: Optional[str] = None  # a loaded LoRA adapter (servers with serve.adapters); None: the base model
        # servers with serve.logit_penalties
        repetition_penalty: Optional[float] = None
        presence_penalty: Optional[float] = None
        frequency_penalty: Optional[float] = None
        logit_bias: Optional[Dict[str, float]] = None  # token id (as a string) -> bias in [-100, 100]
        # servers with serve.stop_sequences
        stop: Optional[Union[str, List[str]]] = None
        stop_token_ids: Optional[List[int]] = None

    @app.get("/health")
    def health():
        return {"status": "ok", "docs": len(pipeline.docs), "max_batch": pipeline.max_batch,
                "batching": "continuous" if continuous else "dynamic", "per_request_sampling": per_request_sampling,
                "adapters": adapters.loaded() if adapters is not None else [], "lookup_tokens": engine_k,
                "logit_penalties": bool(logit_penalties), "stop_sequences": bool(stop_sequences)}

    @app.get("/stats")
    def stats():
        return dict(engine.stats)

    @app.post("/answer")
    async def answer(q: Query):
        try:
            rs = request_sampling(q, getattr(getattr(pipeline, "sampling", None), "max_new_tokens", None),
                                  engine_k if per_request_sampling else None, vocab)
        except ValueError as e:
            raise HTTPException(status_code=422, detail=str(e))
        if rs is not None and rs.has_penalties and per_request_sampling and not logit_penalties:
            raise HTTPException(status_code=400, detail="logit penalties in the request need the server flag "
                                                        "serve.logit_penalties (off on this server)")
        if rs is not None and rs.has_stops and per_request_sampling and not stop_sequences:
            raise HTTPException(status_code=400, detail="stop / stop_token_ids in the request need the server flag "
                                                        "serve.stop_sequences (off on this server)")
        if rs is not None and not per_request_sampling:
            raise HTTPException(status_code=400, detail="sampling settings in the request need the server flag "
                                                        "serve.per_request_sampling (off on this server)")
        if q.adapter is not None:
            if adapters is None:
                raise HTTPException(status_code=400, detail="an adapter in the request needs a server started with "
                                                            "serve.adapters (none on this server)")
            if q.adapter not in adapters.loaded():
                raise HTTPException(status_code=422, detail=f"unknown adapter {q.adapter!r}; loaded: {adapters.loaded()}")
            a = await asyncio.wrap_future(engine.submit(q.query, q.top_k, rs, q.adapter))
            return {"answer": a.answer, "doc_ids": a.doc_ids, "docs": a.docs, "scores": a.scores, "timings": a.timings}
        a = await asyncio.wrap_future(engine.submit(q.query, q.top_k, rs) if rs is not None else
                                      engine.submit(q.query, q.top_k))
        return {"answer": a.answer, "doc_ids": a.doc_ids, "docs": a.docs, "scores": a.scores, "timings": a.timings}

    @app.on_event("shutdown")
    def _shutdown():
        engine.close()

    return app


def serve(cfg, host: str = "127.0.0.1", port: int = 8000, max_batch: int = 16, max_wait_s: float = 0.004,
          continuous: bool = True, per_request_sampling: Optional[bool] = None, adapters=None,
          logit_penalties: Optional[bool] = None, stop_sequences: Optional[bool] = None):
    import uvicorn

    from ..cli import apply_fp4, build_stack
    from ..generation import SamplingParams
    from ..parallel import init
    from ..rag import RagPipeline

    di = init()
    st = build_stack(cfg, di.device)
    apply_fp4(cfg, st["policy"])
    sp = SamplingParams(max_new_tokens=cfg.ppo.max_new_tokens, temperature=cfg.eval.temperature,
                        do_sample=cfg.eval.do_sample, top_k=cfg.eval.top_k, lookup_tokens=cfg.eval.lookup_tokens,
                        lookup_ngram=cfg.eval.lookup_ngram)
    rag = RagPipeline(st["encoder"], st["index"], st["docs"], st["policy"], st["tokenizer"], cfg.retrieval.top_k, sp,
                      cfg.ppo.max_prompt_tokens, max_batch=max_batch)
    if per_request_sampling is None:
        per_request_sampling = cfg.serve.per_request_sampling
    if logit_penalties is None:
        logit_penalties = cfg.serve.logit_penalties
    if stop_sequences is None:
        stop_sequences = cfg.serve.stop_sequences
    # per-request adapters: serve.adapters {name: PEFT directory}, plus / overridden by ``adapters``
    named = dict(getattr(cfg.serve, "adapters", None) or {})
    named.update(adapters or {})
    bank = None
    if named:
        from ..models import AdapterBank
        from ..models.lora import LoraConfig
        import json
        import os

        ranks = []
        for path in named.values():
            with open(os.path.join(path, "adapter_config.json")) as f:
                ranks.append(int(json.load(f).get("r", LoraConfig.r)))
        bank = AdapterBank(st["policy"], slots=max(8, len(named)), r_max=next(r for r in (8, 16, 32, 64) if r >= max(ranks)))
        for name, path in named.items():
            bank.load(name, path)
    uvicorn.run(create_app(rag, max_wait_s, continuous, per_request_sampling, bank, logit_penalties, stop_sequences),
                host=host, port=port)
