"""Per-request sampling on the CPU paths: ``ops.reference.sample_rows``, the per_request
ContinuousBatcher, ContinuousEngine(per_request_sampling=True) and the HTTP request fields."""
import pytest
import torch

from rag_tl_domainllm_optimizer_amd import models, ops
from rag_tl_domainllm_optimizer_amd.generation import (ContinuousBatcher, Generator, RequestSampling, SamplingParams,
                                                       derive_seed)
from rag_tl_domainllm_optimizer_amd.ops import reference as ref


def _rowp(rows):
    """rows: (inv_temp, top_k, top_p, greedy, seed, counter)"""
    dt = (torch.float32, torch.int32, torch.float32, torch.uint8, torch.long, torch.int32)
    return [torch.tensor(c, dtype=d) for c, d in zip(zip(*rows), dt)]


def test_ref_sample_rows_filters_and_keying():
    torch.manual_seed(0)
    V = 97
    logits = torch.randn(6, V) * 2
    rows = [(1.0, 1, 1.0, 0, 3, 0), (1 / 0.7, 5, 1.0, 0, 4, 1), (1.0, 0, 0.5, 0, 5, 2), (2.0, 20, 0.8, 0, 6, 3),
            (1.0, 0, 1.0, 1, 7, 4), (1 / 1.3, 0, 1.0, 0, 8, 5)]
    p = _rowp(rows)
    tok, lp = ops.sample_rows(logits, *p)  # the CPU dispatch of the public op
    assert int(tok[0]) == int(logits[0].argmax()) and int(tok[4]) == int(logits[4].argmax())  # top_k = 1, greedy
    for b, (it, k, tp, g, _, _) in enumerate(rows):
        keep = ref.filter_logits(logits[b:b + 1], it, k, tp)[0]
        assert bool(keep[tok[b]]), b
        want = torch.log_softmax(logits[b] * it, -1)[tok[b]]
        assert abs(float(lp[b]) - float(want)) < 1e-5
    # an inactive row returns the argmax
    active = torch.tensor([1, 1, 1, 1, 1, 0], dtype=torch.uint8)
    tok_i, _ = ref.sample_rows(logits, *p, active)
    assert int(tok_i[5]) == int(logits[5].argmax()) and torch.equal(tok_i[:5], tok[:5])
    # the draw is a function of (seed, counter) and the row's own logits: any place, any batch mates
    perm = torch.tensor([3, 5, 0, 2, 4, 1])
    tok_p, lp_p = ref.sample_rows(logits[perm], *[t[perm] for t in p])
    assert torch.equal(tok_p, tok[perm]) and torch.equal(lp_p, lp[perm])
    one, _ = ref.sample_rows(logits[3:4], *[t[3:4] for t in p])
    assert int(one) == int(tok[3])
    # many rows of one distribution: the counter (and the seed) change the draw
    flat = torch.zeros(64, V)
    base = [(1.0, 0, 1.0, 0, 9, 0)] * 64
    t0, _ = ref.sample_rows(flat, *_rowp(base))
    assert bool((t0 == t0[0]).all())  # same (seed, counter) everywhere: one draw
    t1, _ = ref.sample_rows(flat, *_rowp([(1.0, 0, 1.0, 0, 9, c) for c in range(64)]))
    t2, _ = ref.sample_rows(flat, *_rowp([(1.0, 0, 1.0, 0, s, 0) for s in range(64)]))
    assert len(set(t1.tolist())) > 16 and len(set(t2.tolist())) > 16


def test_request_sampling_validation():
    for bad in (dict(temperature=-0.1), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(max_new_tokens=0),
                dict(max_new_tokens=9), dict(seed=-1), dict(seed=2 ** 63), dict(temperature=float("nan"))):
        with pytest.raises(ValueError):
            RequestSampling(**bad).validate(8)
    RequestSampling(temperature=0.0, top_k=0, top_p=1.0, max_new_tokens=8, seed=2 ** 63 - 1).validate(8)
    sp = SamplingParams(max_new_tokens=8, temperature=0.7, top_k=50, top_p=0.95, seed=3)
    assert RequestSampling().resolve(sp, 8, 42) == (1 / 0.7, 50, 0.95, False, 42, 8)
    assert RequestSampling(temperature=0.0, seed=5, max_new_tokens=2).resolve(sp, 8, 42) == (1.0, 50, 0.95, True, 5, 2)
    assert RequestSampling(do_sample=False).resolve(sp, 8, 42)[3] is True
    assert derive_seed(3, 0) != derive_seed(3, 1) and derive_seed(3, 0) == derive_seed(3, 0)
    assert 0 <= derive_seed(2 ** 62, 10 ** 9) < 2 ** 63


def _run(cb):
    got = {}
    while cb.active_rows():
        cb.step(1)
        for f in cb.collect():
            got[f.tag] = f
    return got


def test_batcher_per_request_lengths_greedy_row_and_seed():
    m = models.CausalLM(models.resolve_preset("tiny-llama"), device="cpu", dtype=torch.float32, seed=3)
    sp = SamplingParams(max_new_tokens=6, temperature=0.9, top_k=0, seed=7)
    prompts = [[5, 9, 33, 41, 7], [12, 300, 4, 8, 9, 10, 11], [20, 21, 22], [100, 200, 300, 400]]
    greedy = Generator(m, 1, 64, "cpu", use_graph=False).generate(
        [prompts[2]], SamplingParams(max_new_tokens=6, do_sample=False), pad_id=0, eos_ids=[-1]).tokens[0].tolist()
    settings = [RequestSampling(seed=11, max_new_tokens=3), RequestSampling(temperature=1.3, top_p=0.9, seed=12),
                RequestSampling(do_sample=False, max_new_tokens=5), None]

    def serve(order):
        gen = Generator(m, 4, 64, "cpu", use_graph=False)
        cb = ContinuousBatcher(gen, sp, pad_id=0, eos_ids=[-1], per_request=True)
        cb.admit_many([prompts[i] for i in order], list(order), [settings[i] for i in order])
        got = _run(cb)
        cb.close()
        return got

    got = serve([0, 1, 2, 3])
    assert [len(got[i].tokens) for i in range(4)] == [3, 6, 5, 6]           # each row stops at its own length
    assert got[2].tokens == greedy[:5]                                      # a greedy row among sampled rows
    assert [got[i].seed for i in range(3)] == [11, 12, derive_seed(7, 2)]   # given or derived, reported back
    assert got[3].seed == derive_seed(7, 3)
    # seeded requests draw the same answer in other rows, beside other batch mates
    again = serve([1, 0])
    assert again[0].tokens == got[0].tokens and again[1].tokens == got[1].tokens
    assert again[0].logprobs == pytest.approx(got[0].logprobs, abs=1e-5)


def test_batcher_rejects_bad_settings_and_flag_off():
    m = models.CausalLM(models.resolve_preset("tiny-llama"), device="cpu", dtype=torch.float32, seed=3)
    sp = SamplingParams(max_new_tokens=4, do_sample=False)
    cb = ContinuousBatcher(Generator(m, 2, 64, "cpu", use_graph=False), sp, pad_id=0, eos_ids=[-1], per_request=True)
    for bad in (dict(temperature=-1.0), dict(top_k=-2), dict(top_p=0.0), dict(max_new_tokens=5), dict(seed=-3)):
        with pytest.raises(ValueError):
            cb.admit([5, 6, 7], "x", RequestSampling(**bad))
    assert cb.free_rows() == 2 and cb.active_rows() == 0  # nothing was admitted
    cb.close()
    off = ContinuousBatcher(Generator(m, 2, 64, "cpu", use_graph=False), sp, pad_id=0, eos_ids=[-1])
    with pytest.raises(ValueError):
        off.admit([5, 6, 7], "x", RequestSampling(temperature=0.5))
    off.admit([5, 6, 7], "y")
    assert _run(off)["y"].seed is None
    off.close()
    with pytest.raises(NotImplementedError):
        ContinuousBatcher(Generator(m, 2, 64, "cpu", use_graph=False), SamplingParams(max_new_tokens=4, lookup_tokens=2),
                          per_request=True)


def _tiny_pipe(max_batch=2, new=5, **sampling):
    from rag_tl_domainllm_optimizer_amd.rag import RagPipeline
    from rag_tl_domainllm_optimizer_amd.retrieval import Encoder, FlatIndex
    from rag_tl_domainllm_optimizer_amd.tokenizer import Tokenizer

    pol = models.CausalLM(models.resolve_preset("tiny-llama"), device="cpu", dtype=torch.float32, seed=1)
    enc_m = models.build_model("tiny-bert", device="cpu", dtype=torch.float32, seed=2).eval()
    tok = Tokenizer.synthetic(pol.cfg.vocab_size, pol.cfg.arch)
    enc = Encoder(enc_m, Tokenizer.synthetic(enc_m.cfg.vocab_size, enc_m.cfg.arch), max_length=32)
    words = tok.words()
    docs = [" ".join(words[(7 * i + j) % len(words)] for j in range(12)) for i in range(30)]
    index = FlatIndex(enc.dim, "ip", "cpu")
    index.add(enc.encode(docs))
    pipe = RagPipeline(enc, index, docs, pol, tok, top_k=2, sampling=SamplingParams(max_new_tokens=new, **sampling),
                       max_prompt_tokens=96, max_batch=max_batch, use_graph=False)
    return pipe, words


@pytest.fixture(scope="module")
def sampled_pipe():
    return _tiny_pipe(max_batch=2, new=5, temperature=1.0, top_k=0, seed=1)


def test_engine_per_request_sampling(sampled_pipe):
    from rag_tl_domainllm_optimizer_amd.serve import BatchingEngine, ContinuousEngine

    pipe, words = sampled_pipe
    q = f"{words[1]} {words[4]}"
    greedy_pipe, _ = _tiny_pipe(max_batch=2, new=5, do_sample=False)
    direct = greedy_pipe.answer([q])[0]
    with ContinuousEngine(pipe, chunk=2, per_request_sampling=True) as eng:
        futs = [eng.submit(q, sampling=RequestSampling(do_sample=False)),
                eng.submit(f"{words[2]} {words[5]}", sampling=RequestSampling(temperature=1.5, max_new_tokens=2)),
                eng.submit(q, sampling=RequestSampling(seed=77))]
        a, b, c = [f.result(120) for f in futs]
        with pytest.raises(ValueError):
            eng.submit(q, sampling=RequestSampling(top_p=0.0))
        with pytest.raises(ValueError):
            eng.submit(q, sampling=RequestSampling(max_new_tokens=6))
    assert a.answer == direct.answer and a.doc_ids == direct.doc_ids
    assert b.timings["new_tokens"] == 2 and c.timings["seed"] == 77
    assert isinstance(b.timings["seed"], int) and b.timings["seed"] == derive_seed(1, 1)
    # the same seed and query, each alone on a fresh engine: the same answer text
    texts = []
    for _ in range(2):
        with ContinuousEngine(pipe, chunk=3, per_request_sampling=True) as eng:
            texts.append(eng.answer(q, sampling=RequestSampling(seed=77), timeout=120).answer)
    assert texts[0] == texts[1] == c.answer
    with ContinuousEngine(pipe, chunk=2) as eng:  # the flag is off by default
        with pytest.raises(ValueError, match="per_request_sampling"):
            eng.submit(q, sampling=RequestSampling(seed=1))
        assert "seed" not in eng.answer(q, timeout=120).timings
    with BatchingEngine(pipe, max_wait_s=0.0) as eng:
        with pytest.raises(ValueError):
            eng.submit(q, sampling=RequestSampling(seed=1))


def test_http_sampling_fields(sampled_pipe):
    from fastapi.testclient import TestClient

    from rag_tl_domainllm_optimizer_amd.serve import create_app

    pipe, words = sampled_pipe
    q = f"{words[1]} {words[4]}"
    with TestClient(create_app(pipe, continuous=True, per_request_sampling=True)) as c:
        assert c.get("/health").json()["per_request_sampling"] is True
        assert c.post("/answer", json={"query": q, "top_p": 0}).status_code == 422
        assert c.post("/answer", json={"query": q, "max_new_tokens": 6}).status_code == 422
        assert c.post("/answer", json={"query": q, "seed": "x"}).status_code == 422
        r = c.post("/answer", json={"query": q, "top_k": 1, "seed": 5, "temperature": 0.8, "top_k_tokens": 20,
                                    "max_new_tokens": 3})
        assert r.status_code == 200
        body = r.json()
        assert body["timings"]["seed"] == 5 and body["timings"]["new_tokens"] == 3 and len(body["doc_ids"]) == 1
        r2 = c.post("/answer", json={"query": q, "top_k": 1, "seed": 5, "temperature": 0.8, "top_k_tokens": 20,
                                     "max_new_tokens": 3}).json()
        assert r2["answer"] == body["answer"]
        assert isinstance(c.post("/answer", json={"query": q}).json()["timings"]["seed"], int)
    with TestClient(create_app(pipe, continuous=True)) as c:
        r = c.post("/answer", json={"query": q, "temperature": 0.5})
        assert r.status_code == 400 and "per_request_sampling" in r.json()["detail"]
        assert c.post("/answer", json={"query": q, "top_p": 0}).status_code == 422
        assert c.post("/answer", json={"query": q}).status_code == 200
    with pytest.raises(ValueError):
        create_app(pipe, continuous=False, per_request_sampling=True)


def test_config_and_cli_flag():
    from rag_tl_domainllm_optimizer_amd import config as C

    assert C.RunConfig().serve.per_request_sampling is False
    assert C.load(overrides=["--serve.per_request_sampling=true"]).serve.per_request_sampling is True
