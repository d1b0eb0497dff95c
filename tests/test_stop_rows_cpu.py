"""Per-request stop strings and stop token ids on the CPU: the vocabulary byte table against
``Tokenizer.decode``, ``ops.reference.stop_rows`` against a brute force over ``decode``,
``ContinuousBatcher(per_request=True, stops=True)``, validation, refusals and the serving layers."""
import random

import pytest
import torch

from rag_tl_domainllm_optimizer_amd import models, ops
from rag_tl_domainllm_optimizer_amd.generation import (ContinuousBatcher, Generator, RequestSampling, SamplingParams,
                                                        _RowStops)
from rag_tl_domainllm_optimizer_amd.ops import reference as ref
from rag_tl_domainllm_optimizer_amd.tokenizer import Tokenizer

LLAMA_SP = {"unk": ("<unk>", 0), "bos": ("<s>", 1), "eos": ("</s>", 2)}


def tok_wordlevel():
    return Tokenizer.synthetic(96, "llama")


def tok_wordpiece():
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "ab", "cd", "query", ":", "##x", "##yz", "##ab", "a", "context", "."]
    sp = {"pad": ("[PAD]", 0), "unk": ("[UNK]", 1), "bos": ("[CLS]", 2), "eos": ("[SEP]", 3)}
    return Tokenizer("wordpiece", {w: i for i, w in enumerate(words)}, [], sp, True, "##", template="cls_sep")


def tok_bpe():
    # byte-level pieces in the GPT-2 alphabet: G-dot = space, C-dot = newline
    words = ["<|end|>", "a", "b", "ab", "Ġa", "Ġ", "Ċ", "ĊĊ", "Query", ":", "ĠQuery",
             "Ã©", "ba"]
    return Tokenizer("bpe", {w: i for i, w in enumerate(words)}, [], {"eos": ("<|end|>", 0)})


def tok_sp():
    words = ["<unk>", "<s>", "</s>", "▁a", "b", "ab", "▁", "<0x0A>", "<0x20>", "<0x41>", "a", "▁ab",
             "ba", "▁Query", ":", "▁▁"]
    return Tokenizer("sp_bpe", {w: i for i, w in enumerate(words)}, [], LLAMA_SP, add_prefix_space=True,
                     byte_fallback=True)


TOKENIZERS = {"wordlevel": tok_wordlevel, "wordpiece": tok_wordpiece, "bpe": tok_bpe, "sp_bpe": tok_sp}


def stream_text(table, ids):
    """The stream text of an id list from the byte table and the start rule"""
    offsets, blob, strip = table
    raw = b"".join(bytes(blob[int(offsets[t]):int(offsets[t + 1])].tolist()) for t in ids)
    return raw[1:] if (strip and raw[:1] == b" ") else raw


@pytest.mark.parametrize("kind", list(TOKENIZERS))
def test_table_invariant(kind):
    tok = TOKENIZERS[kind]()
    table = tok.token_bytes()
    offsets, blob, strip = table
    V = tok.vocab_size
    assert offsets.dtype == torch.int32 and offsets.shape == (V + 1,) and blob.dtype == torch.uint8
    assert int(offsets[0]) == 0 and int(offsets[-1]) == blob.numel()
    assert strip == (kind != "bpe")
    for t in range(V):
        assert bytes(blob[int(offsets[t]):int(offsets[t + 1])].tolist()) == tok._impl.token_bytes(t)
    specials = [tok.token_to_id(s) for s in tok.special_tokens]
    assert specials and all(int(offsets[s + 1]) == int(offsets[s]) for s in specials)
    rng = random.Random(kind)
    used = set()
    held = ops.TokenBytes(*table)
    for i in range(200):
        ids = [rng.randrange(V) for _ in range(rng.randrange(0, 13))]
        if i % 3 == 0 and ids:
            ids[rng.randrange(len(ids))] = rng.choice(specials)  # also at the front
        used.update(ids)
        assert stream_text(table, ids) == tok.decode(ids, skip_special_tokens=True).encode("utf-8"), ids
        assert held.stream_text(ids) == stream_text(table, ids)
    assert used >= set(specials)
    if kind == "sp_bpe":
        assert used >= {tok.token_to_id("<0x0A>"), tok.token_to_id("<0x20>"), tok.token_to_id("<0x41>")}


def test_stream_text_of_a_broken_character():
    """A token list that ends inside a multi-byte character (byte fallback) has a stream text, which
    the engine decodes with replacement after cutting it at ``text_bytes``"""
    words = ["<unk>", "<s>", "</s>", "▁a", "<0xC3>", "<0xA9>"]
    tok = Tokenizer("sp_bpe", {w: i for i, w in enumerate(words)}, [], LLAMA_SP, add_prefix_space=True,
                    byte_fallback=True)
    tb = ops.TokenBytes.from_tokenizer(tok, vocab_size=8)  # two ids the tokenizer does not know
    assert tb.source is tok and tb.vocab_size == 8
    assert tb.stream_text([3, 4, 5, 7, 2]) == "a\u00e9".encode() == tok.decode([3, 4, 5]).encode()
    assert tb.stream_text([3, 3, 4]) == b"a a\xc3"
    assert tb.stream_text([3, 3, 4])[:4].decode("utf-8", "replace") == "a a\ufffd"


# ------------------------------------------------------------------------ oracle against brute force
def brute(tok, tokens, strings, ids):
    """(n, kind, offset): the first n for which decode(tokens[:n]) contains a stop string or
    tokens[n - 1] is a stop id, with the earliest offset at that n; None without one"""
    for n in range(1, len(tokens) + 1):
        text = tok.decode(tokens[:n]).encode("utf-8")
        cands = []
        if tokens[n - 1] in ids:
            cands.append((len(tok.decode(tokens[:n - 1]).encode("utf-8")), 0, 4 + ids.index(tokens[n - 1])))
        for i, s in enumerate(strings):
            p = text.find(s)
            if p >= 0:
                cands.append((p, 1, i))
        if cands:
            at, _, kind = min(cands)
            return n, kind, at
    return None


def pack_rows(rows, T, device="cpu"):
    """rows: (tokens, strings, ids) -> out_tokens [B, T] and a _RowStops with the rows' stops"""
    st = _RowStops(len(rows), device)
    st.write(0, [(tuple(s), tuple(i)) for _, s, i in rows])
    out = torch.zeros(len(rows), T, dtype=torch.long)
    for b, (toks, _, _) in enumerate(rows):
        out[b, :len(toks)] = torch.tensor(toks)
    return out.to(device), st


def run_oracle(table, rows, T, G):
    """The oracle stepped G tokens at a time over every row; returns the final state"""
    out, st = pack_rows(rows, T)
    tb = ops.TokenBytes(*table)
    gen_len = torch.zeros(len(rows), dtype=torch.int32)
    active = torch.ones(len(rows), dtype=torch.uint8)
    lens = torch.tensor([len(r[0]) for r in rows], dtype=torch.int32)
    for _ in range(0, T, G):
        gen_len = torch.where(active.bool(), torch.minimum(gen_len + G, lens), gen_len)
        active = active * (gen_len < lens).to(torch.uint8)  # a row that reached its length finishes, and is scanned
        ops.stop_rows(out, gen_len, active, tb, *st.tensors())
    return gen_len, active, st


def classify(tok, table, tokens, strings, ids, res):
    """The cases of the issue's list that this row shows"""
    seen = set()
    if res is None:
        offsets, blob, strip = table
        raw = b"".join(bytes(blob[int(offsets[t]):int(offsets[t + 1])].tolist()) for t in tokens)
        if strip and raw[:1] == b" " and any(raw.startswith(s) for s in strings):
            seen.add("needs the stripped space")
        return seen
    n, kind, at = res
    text = tok.decode(tokens[:n]).encode("utf-8")
    bounds = [len(tok.decode(tokens[:k]).encode("utf-8")) for k in range(n + 1)]
    hits = [(text.find(s), i) for i, s in enumerate(strings) if text.find(s) >= 0]
    if kind < 4:
        first_tok = max(k for k in range(n) if bounds[k] <= at)  # the token the match begins in
        seen.add({1: "inside one token", 2: "straddles two", 3: "straddles three"}.get(n - first_tok, "more"))
    if len({p for p, _ in hits}) >= 2:
        seen.add("two stops at one token")
    if tokens[n - 1] in ids and hits:
        seen.add("token and string at one step")
    if n == 1:
        seen.add("first token")
    if n % 4 == 2:
        seen.add("second token of a G=4 step")
    return seen


def test_oracle_against_brute_force():
    tok = tok_sp()
    table = tok.token_bytes()
    V, T = tok.vocab_size, 12
    rng = random.Random(5)
    alphabet = [b"ab", b" a", b"a", b"b a", b"aba", b"ab a", b"\n", b"a\nb", b" ab a", b"bb", b" Query:", b"b  a", b"A a"]
    a, b_, ab, sp_a = tok.token_to_id("a"), tok.token_to_id("b"), tok.token_to_id("ab"), tok.token_to_id("▁a")
    # constructed rows: the stripped space (" a" would match only with it), a stop over three tokens,
    # a stop id where a string completes, two strings completing at one token
    rows = [([sp_a, b_, b_, b_], [b" a"], []),
            ([b_, b_, a, b_, a, b_], [b"aba"], []),
            ([b_, a, ab, b_], [b"ab"], [ab]),
            ([b_, b_, a, ab, b_], [b"ab", b"bba"], []),
            ([ab, b_], [b"ab"], []),
            ([b_, b_, b_, b_, a, ab], [b"bab"], [])]
    for _ in range(400):
        toks = [rng.choice([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 2]) for _ in range(rng.randrange(1, T + 1))]
        strings = rng.sample(alphabet, rng.randrange(0, 5))
        ids = rng.sample(range(V), rng.randrange(0, 3)) if rng.random() < 0.4 else []
        rows.append((toks, strings, ids))
    expect = [brute(tok, *r) for r in rows]
    cases = set()
    for r, e in zip(rows, expect):
        cases |= classify(tok, table, *r, e)
    assert cases >= {"inside one token", "straddles two", "straddles three", "two stops at one token",
                     "token and string at one step", "first token", "needs the stripped space",
                     "second token of a G=4 step"}, cases
    assert any(e is None for e in expect) and sum(e is not None for e in expect) > 100
    for G in (1, 4):
        gen_len, active, st = run_oracle(table, rows, T, G)
        for b, (r, e) in enumerate(zip(rows, expect)):
            got = (int(gen_len[b]), int(st.stop_hit[b]), int(st.stop_at[b]))
            if e is None:
                # a row without stops is never scanned: its cursors stay where the admission put them
                scanned = bool(r[1] or r[2])
                raw_len = sum(len(tok._impl.token_bytes(t)) for t in r[0]) if scanned else 0
                assert got == (len(r[0]), -1, 0) and int(st.nbytes[b]) == raw_len, (G, b, r, got)
                assert int(st.seen[b]) == (len(r[0]) if scanned else 0), (G, b, r)
            else:
                assert got == e and int(active[b]) == 0, (G, b, r, e, got)


# ----------------------------------------------------------------------------- validation, refusals
def test_validation():
    bad = [dict(stop=["a", "b", "c", "d", "e"]), dict(stop=""), dict(stop=["ok", ""]), dict(stop="x" * 33),
           dict(stop="é" * 17), dict(stop=["a", "a"]), dict(stop=[1]), dict(stop_token_ids=list(range(9))),
           dict(stop_token_ids=[-1]), dict(stop_token_ids=[512]), dict(stop_token_ids=[1.5])]
    for kw in bad:
        with pytest.raises(ValueError):
            RequestSampling(**kw).validate(8, None, 512)
    ok = RequestSampling(stop="\n\nQuery:", stop_token_ids=[511, 0])
    ok.validate(8, None, 512)
    assert ok.has_stops and not RequestSampling(seed=1).has_stops
    sp = SamplingParams(max_new_tokens=8, stop=["x" * 32, "é" * 16], stop_token_ids=[7])
    assert ok.resolve_stops(sp, 512) == ((b"\n\nQuery:",), (511, 0))
    assert RequestSampling().resolve_stops(sp, 512) == ((b"x" * 32, ("é" * 16).encode()), (7,))
    assert RequestSampling().resolve_stops(SamplingParams()) == ((), ())


def test_long_vocabulary_entry_is_refused():
    vocab = {"<unk>": 0, "<s>": 1, "</s>": 2, "w" * 255: 3, "ok": 4}
    ops.TokenBytes.from_tokenizer(Tokenizer("wordlevel", vocab, [], LLAMA_SP))  # a space + 255 bytes: the limit
    vocab["w" * 256] = 5
    with pytest.raises(ValueError, match="256"):
        ops.TokenBytes.from_tokenizer(Tokenizer("wordlevel", vocab, [], LLAMA_SP))


@pytest.fixture(scope="module")
def model():
    return models.CausalLM(models.resolve_preset("tiny-llama"), device="cpu", dtype=torch.float32, seed=3)


@pytest.fixture(scope="module")
def tok(model):
    return Tokenizer.synthetic(model.cfg.vocab_size, model.cfg.arch)


def test_batcher_refusals(model, tok):
    sp = SamplingParams(max_new_tokens=4, do_sample=False)
    tb = ops.TokenBytes.from_tokenizer(tok)
    mk = lambda: Generator(model, 2, 64, "cpu", use_graph=False)  # noqa: E731
    with pytest.raises(ValueError, match="per_request"):
        ContinuousBatcher(mk(), sp, pad_id=0, eos_ids=[-1], stops=True, token_bytes=tb)
    with pytest.raises(ValueError, match="token_bytes"):
        ContinuousBatcher(mk(), sp, pad_id=0, eos_ids=[-1], per_request=True, stops=True)
    with pytest.raises(ValueError, match="entries"):
        ContinuousBatcher(mk(), sp, pad_id=0, eos_ids=[-1], per_request=True, stops=True,
                          token_bytes=ops.TokenBytes.from_tokenizer(tok_sp()))
    with pytest.raises(ValueError, match="stops"):  # batcher-wide defaults need the flag too
        ContinuousBatcher(mk(), SamplingParams(max_new_tokens=4, stop="x"), pad_id=0, eos_ids=[-1], per_request=True)
    for kw in (dict(stop=["x"]), dict(stop_token_ids=[5])):
        with pytest.raises(ValueError, match="ContinuousBatcher"):
            Generator(model, 1, 64, "cpu", use_graph=False).generate([[5, 6]], SamplingParams(max_new_tokens=2, **kw))
    off = ContinuousBatcher(mk(), sp, pad_id=0, eos_ids=[-1], per_request=True)
    with pytest.raises(ValueError, match="stops"):
        off.admit([5, 6, 7], "x", RequestSampling(stop="a"))
    with pytest.raises(ValueError, match="stops"):
        off.admit([5, 6, 7], "x", RequestSampling(stop_token_ids=[3]))
    assert off.free_rows() == 2 and off.gen.stopp is None and off.gen.token_bytes is None  # nothing allocated
    off.close()
    on = ContinuousBatcher(mk(), sp, pad_id=0, eos_ids=[-1], per_request=True, stops=True, token_bytes=tb)
    for kw in (dict(stop=""), dict(stop=["a"] * 2), dict(stop_token_ids=[model.cfg.vocab_size]), dict(stop="x" * 33)):
        with pytest.raises(ValueError):
            on.admit([5, 6, 7], "x", RequestSampling(**kw))
    assert on.free_rows() == 2 and on.active_rows() == 0
    on.close()


# --------------------------------------------------------------------------------------- the batcher
PROMPTS = [[5, 9, 33, 41, 7], [12, 300, 4, 8, 9, 10, 11], [20, 21, 22], [100, 200, 300, 400]]


def _run(cb):
    got = {}
    while cb.active_rows():
        cb.step(1)
        for f in cb.collect():
            got[f.tag] = f
    return got


def straddling_stop(tok, tokens, lo, hi):
    """A substring of decode(tokens) that begins and ends inside tokens and whose first occurrence
    completes at token n in [lo, hi]; (stop string, n, text bytes to keep) or None"""
    text = tok.decode(tokens).encode("utf-8")
    bounds = [len(tok.decode(tokens[:k]).encode("utf-8")) for k in range(len(tokens) + 1)]
    for k in range(2, len(tokens) + 1):
        # from the middle of token k - 1's text to the middle of token k's
        a, b = (bounds[k - 2] + bounds[k - 1] + 1) // 2, (bounds[k - 1] + bounds[k]) // 2
        if not (bounds[k - 2] < a < bounds[k - 1] < b < bounds[k]) or b - a > 32:
            continue
        s = text[a:b]
        p = text.find(s)  # the first occurrence may lie earlier than the one the string was cut from
        n = min(j for j in range(len(bounds)) if bounds[j] >= p + len(s))
        if lo <= n <= hi and p not in bounds and p + len(s) not in bounds:
            return s.decode("utf-8"), n, p
    return None


def test_batcher_neutral_rows_and_stop_rows(model, tok):
    T = 10
    sp = SamplingParams(max_new_tokens=T, temperature=1.0, top_k=0, seed=7)
    base = [RequestSampling(seed=11), RequestSampling(seed=12), RequestSampling(seed=13), RequestSampling(seed=14)]
    tb = ops.TokenBytes.from_tokenizer(tok)

    def serve(settings, **kw):
        cb = ContinuousBatcher(Generator(model, 4, 96, "cpu", use_graph=False), sp, pad_id=0, eos_ids=[-1],
                               per_request=True, **kw)
        cb.admit_many(PROMPTS, list(range(4)), settings)
        return cb, _run(cb)

    cb, plain = serve(base)
    cb.close()
    assert all(plain[i].finish_reason == "length" and plain[i].text_bytes is None for i in range(4))
    cb, neutral = serve(base, stops=True, token_bytes=tb)
    cb.close()
    for i in range(4):
        assert neutral[i].tokens == plain[i].tokens and neutral[i].logprobs == plain[i].logprobs  # bitwise
        assert neutral[i].seed == plain[i].seed and neutral[i].finish_reason == "length"
    pick = straddling_stop(tok, plain[1].tokens, 3, T - 3)
    assert pick is not None
    stop, n1, keep1 = pick
    stop_id = plain[2].tokens[4]
    n2 = plain[2].tokens.index(stop_id) + 1
    mixed = [base[0], RequestSampling(seed=12, stop=["zzzz", stop]), RequestSampling(seed=13, stop_token_ids=[stop_id]),
             RequestSampling(seed=14, stop=[], stop_token_ids=[])]
    cb, got = serve(mixed, stops=True, token_bytes=tb)
    for i in (0, 3):
        assert got[i].tokens == plain[i].tokens and got[i].logprobs == plain[i].logprobs
        assert got[i].finish_reason == "length" and got[i].stop is None
    assert got[1].tokens == plain[1].tokens[:n1] and got[1].logprobs == plain[1].logprobs[:n1]
    assert (got[1].finish_reason, got[1].stop, got[1].text_bytes) == ("stop", stop, keep1)
    assert tok.decode(got[1].tokens).encode()[:keep1] == tok.decode(plain[1].tokens).encode()[:keep1]
    assert got[2].tokens == plain[2].tokens[:n2]
    assert (got[2].finish_reason, got[2].stop) == ("stop", stop_id)
    assert got[2].text_bytes == len(tok.decode(plain[2].tokens[:n2 - 1]).encode())
    # every row is free again, and a new occupant of a stopped row scans from its own first token
    assert cb.free_rows() == 4
    cb.admit(PROMPTS[1], "again", RequestSampling(seed=12, stop=stop))
    again = _run(cb)["again"]
    assert again.tokens == got[1].tokens and again.text_bytes == keep1 and again.finish_reason == "stop"
    cb.close()


def test_batcher_stops_with_lookup(model, tok):
    """Greedy rows under prompt-lookup decoding end at the same token and text as the plain stop run"""
    T = 12
    sp = SamplingParams(max_new_tokens=T, do_sample=False)
    tb = ops.TokenBytes.from_tokenizer(tok)
    prompts = [p * 3 for p in PROMPTS[:2]]

    def serve(settings, **kw):
        cb = ContinuousBatcher(Generator(model, 2, 96, "cpu", use_graph=False), sp, pad_id=0, eos_ids=[-1],
                               per_request=True, stops=True, token_bytes=tb, **kw)
        cb.admit_many(prompts, [0, 1], settings)
        got = _run(cb)
        cb.close()
        return got

    plain = serve(None)
    pick = straddling_stop(tok, plain[1].tokens, 3, T - 2)
    assert pick is not None
    settings = [None, RequestSampling(stop=pick[0])]
    want, got = serve(settings), serve(settings, lookup_tokens=3)
    assert want[1].tokens == plain[1].tokens[:pick[1]] and want[1].text_bytes == pick[2]
    assert got[1].lookup_accepted > 0  # drafts were accepted on the way
    for i in (0, 1):
        assert got[i].tokens == want[i].tokens and got[i].text_bytes == want[i].text_bytes
        assert got[i].finish_reason == want[i].finish_reason


# ------------------------------------------------------------------------------------------ serving
@pytest.fixture(scope="module")
def pipe():
    from test_per_request_sampling_cpu import _tiny_pipe

    return _tiny_pipe(max_batch=2, new=8, temperature=1.0, top_k=0, seed=1)


def test_engine_and_http(pipe):
    from fastapi.testclient import TestClient

    from rag_tl_domainllm_optimizer_amd.rag.prompt import extract_answer
    from rag_tl_domainllm_optimizer_amd.serve import STOP_FIELDS, BatchingEngine, ContinuousEngine, create_app

    assert STOP_FIELDS == ("stop", "stop_token_ids")
    p, words = pipe
    q = f"{words[1]} {words[4]}"
    with ContinuousEngine(p, chunk=2, per_request_sampling=True) as eng:  # the flag is off by default
        full = eng.answer(q, sampling=RequestSampling(seed=77), timeout=120)
        assert "finish_reason" not in full.timings
        with pytest.raises(ValueError, match="stop_sequences"):
            eng.submit(q, sampling=RequestSampling(stop="a"))
    text = full.answer.encode()
    cut = len(text) // 2
    stop = text[cut:cut + 3].decode()
    keep = text.find(stop.encode())
    with ContinuousEngine(p, chunk=2, per_request_sampling=True, stop_sequences=True) as eng:
        a = eng.answer(q, sampling=RequestSampling(seed=77, stop=stop), timeout=120)
        b = eng.answer(q, sampling=RequestSampling(seed=77), timeout=120)
        with pytest.raises(ValueError):
            eng.submit(q, sampling=RequestSampling(stop=""))
    assert a.answer == extract_answer(text[:keep].decode()) and a.timings["finish_reason"] == "stop"
    assert a.timings["new_tokens"] < full.timings["new_tokens"]
    assert b.answer == full.answer and b.timings["finish_reason"] == "length"
    with pytest.raises(ValueError, match="per_request_sampling"):
        ContinuousEngine(p, stop_sequences=True)
    with BatchingEngine(p, max_wait_s=0.0) as eng:
        with pytest.raises(ValueError, match="stop_sequences"):
            eng.submit(q, sampling=RequestSampling(stop="a"))
    with TestClient(create_app(p, continuous=True, per_request_sampling=True, stop_sequences=True)) as c:
        assert c.get("/health").json()["stop_sequences"] is True
        r = c.post("/answer", json={"query": q, "seed": 77, "stop": stop})
        assert r.status_code == 200 and r.json()["answer"] == a.answer and r.json()["timings"]["finish_reason"] == "stop"
        r = c.post("/answer", json={"query": q, "seed": 77, "stop": ["zzzz", stop], "stop_token_ids": [5]})
        assert r.status_code == 200
        assert c.post("/answer", json={"query": q, "stop": ""}).status_code == 422
        assert c.post("/answer", json={"query": q, "stop": ["a"] * 5}).status_code == 422
        assert c.post("/answer", json={"query": q, "stop_token_ids": [99999]}).status_code == 422
    with TestClient(create_app(p, continuous=True, per_request_sampling=True)) as c:
        assert c.get("/health").json()["stop_sequences"] is False
        r = c.post("/answer", json={"query": q, "stop": "a"})
        assert r.status_code == 400 and "stop_sequences" in r.json()["detail"]
        r = c.post("/answer", json={"query": q, "seed": 77})
        assert r.status_code == 200 and "finish_reason" not in r.json()["timings"]
    with TestClient(create_app(p, continuous=True)) as c:
        r = c.post("/answer", json={"query": q, "stop_token_ids": [4]})
        assert r.status_code == 400 and "per_request_sampling" in r.json()["detail"]
    with pytest.raises(ValueError):
        create_app(p, continuous=True, stop_sequences=True)


def test_config_and_cli_flag(monkeypatch):
    from rag_tl_domainllm_optimizer_amd import cli
    from rag_tl_domainllm_optimizer_amd import config as C
    from rag_tl_domainllm_optimizer_amd import serve as serve_pkg

    assert C.RunConfig().serve.stop_sequences is False
    assert C.load(overrides=["--serve.stop_sequences=true"]).serve.stop_sequences is True
    seen = {}
    monkeypatch.setattr(serve_pkg, "serve", lambda cfg, **kw: seen.update(kw, cfg=cfg))
    cli.main(["serve", "--per-request-sampling", "--stop-sequences"])
    assert seen["stop_sequences"] is True and seen["cfg"].serve.stop_sequences is True
    seen.clear()
    cli.main(["serve", "--per-request-sampling"])
    assert seen["stop_sequences"] is False
    with pytest.raises(SystemExit, match="per-request-sampling"):
        cli.main(["serve", "--stop-sequences"])
