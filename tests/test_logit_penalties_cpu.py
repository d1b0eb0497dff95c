"""Per-request logit penalties on the CPU paths: ``ops.reference.logit_rows_penalty`` against an
independent fp64 loop, ``ContinuousBatcher(per_request=True, penalties=True)``, validation, the
engine, the HTTP fields and the config / CLI flag."""
import math

import pytest
import torch

from rag_tl_domainllm_optimizer_amd import models, ops
from rag_tl_domainllm_optimizer_amd.generation import (ContinuousBatcher, Generator, RequestSampling, SamplingParams)

S_MAX = 48


def spec_row(row, prompt, generated, rho, pi, phi, bias):
    """The specification, token by token in fp64 with one rounding to the row's dtype: returns
    {token: expected value} for the touched elements. ``1 / rho`` is the stored fp32 reciprocal."""
    V = row.numel()
    inv = float(1.0 / torch.tensor(rho, dtype=torch.float32))
    rho32 = float(torch.tensor(rho, dtype=torch.float32))
    pi32, phi32 = float(torch.tensor(pi, dtype=torch.float32)), float(torch.tensor(phi, dtype=torch.float32))
    out = {}
    for v in range(V):
        in_p, c = v in prompt, generated.count(v)
        b = [float(torch.tensor(x, dtype=torch.float32)) for t, x in bias if t == v]
        if not in_p and c == 0 and not b:
            continue
        l = float(row[v].double())
        if in_p or c > 0:
            l = l * inv if l > 0 else l * rho32
        l -= pi32 * (1.0 if c > 0 else 0.0) + phi32 * c
        for x in b:
            l += x
        out[v] = torch.tensor(l, dtype=torch.float64).to(row.dtype)
    return out


def ulp_steps(a, b):
    """distance of two values of one dtype in units in the last place"""
    if a.dtype == torch.bfloat16:
        ia, ib = a.view(torch.int16).to(torch.int64), b.view(torch.int16).to(torch.int64)
    else:
        ia, ib = a.view(torch.int32).to(torch.int64), b.view(torch.int32).to(torch.int64)
    # sign-magnitude -> a monotone integer line
    key = lambda i: torch.where(i < 0, -(i & (0x7FFF if a.dtype == torch.bfloat16 else 0x7FFFFFFF)), i)  # noqa: E731
    return (key(ia) - key(ib)).abs()


def make_rows(V):
    """(kv_start, prompt, generated, rho, pi, phi, bias, active) per row: duplicates, tokens 0 and
    V - 1, an empty generated part, left padding, bias tokens in and outside the history, a neutral
    row and an inactive row."""
    last = V - 1
    return [
        (0, [5, 9, 5, 0, last], [9, 9, 33, last], 1.3, 0.0, 0.0, [], 1),
        (3, [7, 8, 7, 7], [], 1.7, 0.5, 0.25, [], 1),                                # left padding, nothing generated
        (0, [1, 2, 3], [2, 2, 2, 40, 0], 1.0, 0.7, 1.1, [(2, 4.5), (50, -3.25)], 1),  # bias in / not in the history
        (2, [last, 11], [last, last, 12], 0.8, -0.5, -0.3, [(t, 0.5 * t - 3) for t in range(20, 36)], 1),  # 16 biases
        (0, [4, 4, 4], [6], 1.0, 0.0, 0.0, [(0, 100.0)], 1),                          # bias alone
        (1, [13, 14], [15, 16], 1.0, 0.0, 0.0, [], 1),                                # neutral
        (0, [17, 18], [19], 1.5, 1.0, 1.0, [(17, -100.0)], 0),                        # inactive
    ]


def pack(rows, V, device="cpu", append=True, S=S_MAX):
    """the op's arguments for ``rows``; with ``append`` the newest generated token is held back in
    ``tok_in`` (slot kv_len holds a marker the op must overwrite)"""
    B = len(rows)
    hist = torch.full((B, S), 3, dtype=torch.long)
    tok_in = torch.zeros(B, dtype=torch.long)
    kv_len = torch.zeros(B, dtype=torch.int32)
    kv_start = torch.zeros(B, dtype=torch.int32)
    gen_len = torch.zeros(B, dtype=torch.int32)
    active = torch.zeros(B, dtype=torch.uint8)
    rho, pi, phi = torch.ones(B), torch.zeros(B), torch.zeros(B)
    nbias = torch.zeros(B, dtype=torch.int32)
    btok, bval = torch.zeros(B, 16, dtype=torch.int32), torch.zeros(B, 16)
    for b, (ks, prompt, gen, r, p, f, bias, act) in enumerate(rows):
        seq = prompt + gen
        use_append = append and len(gen) > 0
        hist[b, ks:ks + len(seq)] = torch.tensor(seq)
        kv_len[b] = ks + len(seq) - 1
        if use_append:
            hist[b, ks + len(seq) - 1] = seq[-1] ^ 1  # a wrong token: the op writes the right one
            tok_in[b] = seq[-1]
        else:
            tok_in[b] = seq[-1]  # appending the token that is already there changes nothing
        kv_start[b], gen_len[b], active[b] = ks, len(gen), act
        rho[b], pi[b], phi[b], nbias[b] = r, p, f, len(bias)
        for j, (t, x) in enumerate(bias):
            btok[b, j], bval[b, j] = t, x
    t = dict(hist=hist, tok_in=tok_in, kv_len=kv_len, kv_start=kv_start, gen_len=gen_len, active=active, rho=rho,
             inv_rho=1.0 / rho, pi=pi, phi=phi, nbias=nbias, bias_tok=btok, bias_val=bval)
    return {k: v.to(device) for k, v in t.items()}


def call(logits, a, append=True):
    return ops.logit_rows_penalty(logits, a["hist"], a["tok_in"] if append else None, a["kv_len"], a["kv_start"], a["gen_len"], a["active"],
                                  a["rho"], a["inv_rho"], a["pi"], a["phi"], a["nbias"], a["bias_tok"], a["bias_val"])


def check_against_spec(x0, got, rows):
    """touched elements within one ulp of the spec, everything else bitwise the input"""
    for b, (ks, prompt, gen, r, p, f, bias, act) in enumerate(rows):
        neutral = r == 1.0 and p == 0.0 and f == 0.0 and not bias
        want = {} if (not act or neutral) else spec_row(x0[b], prompt, gen, r, p, f, bias)
        mask = torch.ones(x0.shape[1], dtype=torch.bool)
        if want:
            idx = torch.tensor(sorted(want))
            exp = torch.stack([want[int(v)] for v in idx])
            steps = ulp_steps(got[b, idx], exp)
            print(f"row {b}: {len(idx)} touched, max ulp distance {int(steps.max())}")
            assert int(steps.max()) <= 1, (b, idx[steps > 1].tolist())
            mask[idx] = False
        assert torch.equal(got[b][mask], x0[b][mask]), b  # untouched: bitwise


@pytest.mark.parametrize("V", [97, 1000])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_twin_against_independent_loop(V, dtype):
    g = torch.Generator().manual_seed(V)  # a generator of its own: the global streams stay as they are
    rows = make_rows(V)
    x0 = (torch.randn(len(rows), V, generator=g) * 3).to(dtype)
    for append in (True, False):
        a = pack(rows, V, append=append)
        h0 = a["hist"].clone()
        got = call(x0.clone(), a, append)
        check_against_spec(x0, got, rows)
        # the newest token joined the history of the rows that are served, nothing else moved
        want_h = h0.clone()
        for b, (ks, prompt, gen, r, p, f, bias, act) in enumerate(rows):
            if act and not (r == 1.0 and p == 0.0 and f == 0.0 and not bias):
                want_h[b, int(a["kv_len"][b])] = int(a["tok_in"][b])
        assert torch.equal(a["hist"], want_h)


# ----------------------------------------------------------------------------- through the batcher
PROMPTS = [[5, 9, 33, 41, 7], [12, 300, 4, 8, 9, 10, 11], [20, 21, 22], [100, 200, 300, 400]]


@pytest.fixture(scope="module")
def model():
    return models.CausalLM(models.resolve_preset("tiny-llama"), device="cpu", dtype=torch.float32, seed=3)


def _run(cb):
    got = {}
    while cb.active_rows():
        cb.step(1)
        for f in cb.collect():
            got[f.tag] = f
    return got


def _serve(model, sp, settings, prompts=PROMPTS, penalties=True, rows=4):
    gen = Generator(model, rows, 96, "cpu", use_graph=False)
    cb = ContinuousBatcher(gen, sp, pad_id=0, eos_ids=[-1], per_request=True, penalties=penalties)
    cb.admit_many(prompts, list(range(len(prompts))), settings)
    got = _run(cb)
    cb.close()
    return got


def test_batcher_neutral_rows_forced_and_banned_tokens(model):
    sp = SamplingParams(max_new_tokens=8, temperature=0.9, top_k=0, seed=7)
    base = [RequestSampling(seed=11), RequestSampling(seed=12, temperature=1.2), RequestSampling(do_sample=False),
            RequestSampling(seed=14)]
    plain = _serve(model, sp, base, penalties=False)
    first = plain[2].tokens[0]
    mixed = [RequestSampling(seed=11),                                               # neutral
             RequestSampling(seed=12, temperature=1.2, logit_bias={77: 100}),        # forced token
             RequestSampling(do_sample=False, logit_bias=[(first, -100)]),           # banned token
             RequestSampling(seed=14, repetition_penalty=1.0, presence_penalty=0.0)]  # neutral, spelled out
    got = _serve(model, sp, mixed)
    for i in (0, 3):
        assert got[i].tokens == plain[i].tokens and got[i].logprobs == plain[i].logprobs  # bitwise
        assert got[i].seed == plain[i].seed
    assert got[1].tokens == [77] * 8
    assert first not in got[2].tokens and plain[2].tokens[0] == first


def test_frequency_penalty_caps_a_biased_token(model):
    """Greedy, bias +30 on token t, frequency_penalty 2, T = 32 tokens. With c earlier emissions, t is
    emitted again only if l_t + 30 - 2 c >= l_v for every token v that was never emitted (such a v
    carries no penalty and no bias). Fewer than 32 distinct tokens were emitted before any step, t
    among them once c >= 1, so at least one of the 33 largest logits belongs to a never-emitted
    v != t: 2 c <= 30 + l_t - l_v <= 30 + D, D = the largest minus the 33rd largest logit of the step.
    The random-init tiny model keeps D < 2 (asserted below on the run's own states, from the plain
    model's logits), hence c <= 15 at every emission and at most ceil(30 / 2) + 1 = 16 emissions."""
    t, T = 9, 32
    sp = SamplingParams(max_new_tokens=T, do_sample=False)
    got = _serve(model, sp, [RequestSampling(frequency_penalty=2.0, logit_bias={t: 30.0})], prompts=[PROMPTS[0]], rows=1)
    toks = got[0].tokens
    assert len(toks) == T
    n = toks.count(t)
    print("emissions of the biased token:", n)
    assert 1 <= n <= math.ceil(30 / 2) + 1
    with torch.no_grad():
        ids = torch.tensor([PROMPTS[0] + toks])
        logits = model.logits(model.forward(ids)).float()[len(PROMPTS[0]) - 1:]
    top = logits.topk(33, -1).values
    D = float((top[:, 0] - top[:, 32]).max())
    print("largest minus 33rd largest logit of the plain model over the run:", D)
    assert D < 2.0


def test_validation():
    bad = [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")),
           dict(repetition_penalty=float("inf")), dict(presence_penalty=2.5), dict(presence_penalty=-2.1),
           dict(frequency_penalty=2.01), dict(frequency_penalty=float("nan")), dict(logit_bias={3: 100.5}),
           dict(logit_bias={3: -101}), dict(logit_bias={-1: 1.0}), dict(logit_bias=[(3, 1.0), (3, 2.0)]),
           dict(logit_bias={i: 1.0 for i in range(17)}), dict(logit_bias={"x": 1.0}), dict(logit_bias=[(1, 2, 3)])]
    for kw in bad:
        with pytest.raises(ValueError):
            RequestSampling(**kw).validate(8)
    with pytest.raises(ValueError):
        RequestSampling(logit_bias={512: 1.0}).validate(8, None, 512)  # token >= V
    ok = RequestSampling(repetition_penalty=1.2, presence_penalty=-2, frequency_penalty=2,
                         logit_bias={"5": 100, 511: -100})
    ok.validate(8, None, 512)
    sp = SamplingParams(max_new_tokens=8, repetition_penalty=1.1, frequency_penalty=0.5, logit_bias={4: 1.0})
    assert ok.resolve_penalties(sp, 512) == (1.2, -2.0, 2.0, ((5, 100.0), (511, -100.0)))
    assert RequestSampling().resolve_penalties(sp, 512) == (1.1, 0.0, 0.5, ((4, 1.0),))
    assert RequestSampling().resolve_penalties(SamplingParams()) == (1.0, 0.0, 0.0, ())
    # the sampling 6-tuple is what it was
    assert ok.resolve(SamplingParams(max_new_tokens=8, temperature=0.7, top_k=50, top_p=0.95), 8, 42) == \
        (1 / 0.7, 50, 0.95, False, 42, 8)


def test_batcher_refusals(model):
    sp = SamplingParams(max_new_tokens=4, do_sample=False)
    mk = lambda **kw: Generator(model, 2, kw.pop("max_seq", 64), "cpu", use_graph=False)  # noqa: E731
    with pytest.raises(ValueError, match="per_request"):
        ContinuousBatcher(mk(), sp, pad_id=0, eos_ids=[-1], penalties=True)
    with pytest.raises(ValueError, match="lookup"):
        ContinuousBatcher(mk(), sp, pad_id=0, eos_ids=[-1], per_request=True, penalties=True, lookup_tokens=2)
    with pytest.raises(ValueError, match="max_seq"):
        ContinuousBatcher(mk(max_seq=ops.LOGIT_ROWS_MAX_SEQ + 1), sp, pad_id=0, eos_ids=[-1], per_request=True,
                          penalties=True)
    with pytest.raises(ValueError, match="penalties"):  # batcher-wide defaults need the flag too
        ContinuousBatcher(mk(), SamplingParams(max_new_tokens=4, repetition_penalty=1.2), pad_id=0, eos_ids=[-1],
                          per_request=True)
    with pytest.raises(ValueError, match="penalties"):
        Generator(model, 1, 64, "cpu", use_graph=False).generate([[5, 6]], SamplingParams(max_new_tokens=2,
                                                                                           presence_penalty=1.0))
    off = ContinuousBatcher(mk(), sp, pad_id=0, eos_ids=[-1], per_request=True)
    with pytest.raises(ValueError, match="penalties=True"):
        off.admit([5, 6, 7], "x", RequestSampling(repetition_penalty=1.1))
    assert off.free_rows() == 2 and off.gen.penp is None and off.gen.hist is None  # nothing allocated
    off.close()
    on = ContinuousBatcher(mk(), sp, pad_id=0, eos_ids=[-1], per_request=True, penalties=True)
    for kw in (dict(repetition_penalty=0.0), dict(logit_bias={512: 1.0}), dict(logit_bias={1: 101})):
        with pytest.raises(ValueError):
            on.admit([5, 6, 7], "x", RequestSampling(**kw))
    assert on.free_rows() == 2 and on.active_rows() == 0
    on.close()


# ----------------------------------------------------------------------------------------- serving
@pytest.fixture(scope="module")
def pipe():
    from test_per_request_sampling_cpu import _tiny_pipe

    return _tiny_pipe(max_batch=2, new=5, temperature=1.0, top_k=0, seed=1)


def test_engine_fields_reach_the_row(pipe):
    from rag_tl_domainllm_optimizer_amd.serve import BatchingEngine, ContinuousEngine

    p, words = pipe
    q = f"{words[1]} {words[4]}"
    forced = p.tok.decode([41] * 5)
    with ContinuousEngine(p, chunk=2, per_request_sampling=True, logit_penalties=True) as eng:
        a = eng.submit(q, sampling=RequestSampling(logit_bias={41: 100}))
        b = eng.submit(q, sampling=RequestSampling(seed=77))
        a, b = a.result(120), b.result(120)
        with pytest.raises(ValueError):
            eng.submit(q, sampling=RequestSampling(repetition_penalty=0))
        with pytest.raises(ValueError):
            eng.submit(q, sampling=RequestSampling(logit_bias={p.gen.cfg.vocab_size: 1.0}))
    from rag_tl_domainllm_optimizer_amd.rag.prompt import extract_answer

    assert a.answer == extract_answer(forced) and a.timings["new_tokens"] == 5
    with ContinuousEngine(p, chunk=2, per_request_sampling=True) as eng:  # the flag is off by default
        assert eng.answer(q, sampling=RequestSampling(seed=77), timeout=120).answer == b.answer  # neutral = plain
        with pytest.raises(ValueError, match="logit_penalties"):
            eng.submit(q, sampling=RequestSampling(presence_penalty=0.5))
    with pytest.raises(ValueError, match="per_request_sampling"):
        ContinuousEngine(p, logit_penalties=True)
    with BatchingEngine(p, max_wait_s=0.0) as eng:
        with pytest.raises(ValueError):
            eng.submit(q, sampling=RequestSampling(frequency_penalty=1.0))


def test_http_penalty_fields(pipe):
    from fastapi.testclient import TestClient

    from rag_tl_domainllm_optimizer_amd.rag.prompt import extract_answer
    from rag_tl_domainllm_optimizer_amd.serve import PENALTY_FIELDS, SAMPLING_FIELDS, create_app

    assert SAMPLING_FIELDS == ("temperature", "top_k_tokens", "top_p", "do_sample", "seed", "max_new_tokens",
                               "lookup_tokens")
    assert PENALTY_FIELDS == ("repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias")
    p, words = pipe
    q = f"{words[1]} {words[4]}"
    with TestClient(create_app(p, continuous=True, per_request_sampling=True, logit_penalties=True)) as c:
        assert c.get("/health").json()["logit_penalties"] is True
        r = c.post("/answer", json={"query": q, "logit_bias": {"41": 100}, "max_new_tokens": 3})
        assert r.status_code == 200 and r.json()["answer"] == extract_answer(p.tok.decode([41] * 3))
        r = c.post("/answer", json={"query": q, "repetition_penalty": 1.2, "presence_penalty": 0.5,
                                    "frequency_penalty": 0.5, "seed": 3})
        assert r.status_code == 200 and r.json()["timings"]["seed"] == 3
        assert c.post("/answer", json={"query": q, "repetition_penalty": 0}).status_code == 422
        assert c.post("/answer", json={"query": q, "presence_penalty": 3}).status_code == 422
        assert c.post("/answer", json={"query": q, "logit_bias": {"41": 101}}).status_code == 422
        assert c.post("/answer", json={"query": q, "logit_bias": {"99999": 1}}).status_code == 422
        assert c.post("/answer", json={"query": q, "logit_bias": {"x": 1}}).status_code == 422
    with TestClient(create_app(p, continuous=True, per_request_sampling=True)) as c:
        assert c.get("/health").json()["logit_penalties"] is False
        r = c.post("/answer", json={"query": q, "repetition_penalty": 1.2})
        assert r.status_code == 400 and "logit_penalties" in r.json()["detail"]
        assert c.post("/answer", json={"query": q, "frequency_penalty": 9}).status_code == 422
        assert c.post("/answer", json={"query": q, "seed": 3}).status_code == 200
    with TestClient(create_app(p, continuous=True)) as c:
        r = c.post("/answer", json={"query": q, "logit_bias": {"41": 1}})
        assert r.status_code == 400 and "per_request_sampling" in r.json()["detail"]
    with pytest.raises(ValueError):
        create_app(p, continuous=True, logit_penalties=True)


def test_config_and_cli_flag(monkeypatch):
    from rag_tl_domainllm_optimizer_amd import cli
    from rag_tl_domainllm_optimizer_amd import config as C
    from rag_tl_domainllm_optimizer_amd import serve as serve_pkg

    assert C.RunConfig().serve.logit_penalties is False
    assert C.load(overrides=["--serve.logit_penalties=true"]).serve.logit_penalties is True
    seen = {}
    monkeypatch.setattr(serve_pkg, "serve", lambda cfg, **kw: seen.update(kw, cfg=cfg))
    cli.main(["serve", "--per-request-sampling", "--logit-penalties"])
    assert seen["logit_penalties"] is True and seen["per_request_sampling"] is True
    assert seen["cfg"].serve.logit_penalties is True
    seen.clear()
    cli.main(["serve", "--per-request-sampling"])
    assert seen["logit_penalties"] is False
    with pytest.raises(SystemExit, match="per-request-sampling"):
        cli.main(["serve", "--logit-penalties"])
