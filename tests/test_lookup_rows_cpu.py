"""Prompt-lookup decoding in the continuous batch on the CPU path (fp32, eager): staggered
admissions against the plain batcher, the per-request stream property, per-request lengths and draft
lengths, refusals, the engine, and the extended reference twins (grouped ``sample_rows``, accept with
``row_max_new`` / ``row_stats``, draft with ``row_draft``)."""
import dataclasses

import pytest
import torch

from rag_tl_domainllm_optimizer_amd import models, ops
from rag_tl_domainllm_optimizer_amd.generation import (ContinuousBatcher, Generator, RequestSampling, SamplingParams)
from rag_tl_domainllm_optimizer_amd.models.config import PRESETS
from rag_tl_domainllm_optimizer_amd.ops import reference as ref

from test_lookup_decode_cpu import PROMPTS, brute_draft

PAD, T, MB, SMAX = 0, 24, 4, 96
REQS = PROMPTS + [PROMPTS[0][2:]]  # four requests from the prompts that repeat n-grams


def _model(seed=2, preset="tiny-llama"):
    return models.CausalLM(PRESETS[preset], dtype=torch.float32, seed=seed)


@pytest.fixture(scope="module")
def model():
    return _model()


def _batcher(m, sp, K=0, per_request=False, eos=(-1,), max_batch=MB, max_seq=SMAX, **kw):
    g = Generator(m, max_batch, max_seq, "cpu", use_graph=False)
    return ContinuousBatcher(g, sp, PAD, list(eos), per_request=per_request, lookup_tokens=K, **kw)


def _drain(cb, got, n=None, emitted=None):
    """n steps (None: until no row is active), collecting after each; ``emitted``: per-step token counts"""
    while (n is None and cb.active_rows()) or (n is not None and n > 0):
        before = cb.gen.gen_len.clone()
        cb.step(1)
        if emitted is not None:
            emitted.append((cb.gen.gen_len - before).tolist())
        for f in cb.collect():
            got[f.tag] = f
        n = None if n is None else n - 1
    return got


def _staggered(m, sp, K, per_request=False, sampling=None, eos=(-1,), emitted=None):
    """admit 2 rows, step 3, admit 2 more, step to the end"""
    cb = _batcher(m, sp, K, per_request, eos)
    s = sampling or [None] * 4
    got = {}
    cb.admit_many(REQS[:2], [0, 1], s[:2] if per_request else None)
    _drain(cb, got, 3, emitted)
    cb.admit_many(REQS[2:], [2, 3], s[2:] if per_request else None)
    _drain(cb, got, None, emitted)
    totals = cb.lookup_totals
    cb.close()
    assert cb.gen._lk is None and not cb.gen._lk_rows
    return got, totals


GREEDY = SamplingParams(max_new_tokens=T, do_sample=False)


@pytest.fixture(scope="module")
def plain_greedy(model):
    return _staggered(model, GREEDY, 0)[0]


@pytest.mark.parametrize("K", [1, 3, 5])
def test_greedy_staggered_equals_plain(model, plain_greedy, K):
    got, totals = _staggered(model, GREEDY, K)
    for i in range(4):
        assert got[i].tokens == plain_greedy[i].tokens, (K, i)
        assert got[i].logprobs == pytest.approx(plain_greedy[i].logprobs, abs=1e-4)
        # every token after the first comes from a verify step: one per step plus the accepted ones
        assert got[i].lookup_steps + got[i].lookup_accepted == T - 1
        assert plain_greedy[i].lookup_steps is None and plain_greedy[i].lookup_accepted is None
    assert max(got[i].lookup_accepted for i in range(4)) > 0
    steps, drafted, accepted = totals
    assert steps == sum(got[i].lookup_steps for i in range(4))
    assert accepted == sum(got[i].lookup_accepted for i in range(4)) and accepted <= drafted <= K * steps


def _settings():
    return [RequestSampling(seed=100 + i, temperature=0.7, top_k=50) for i in range(4)]


def test_sampled_per_request_equals_plain_and_stream_property(model):
    sp = SamplingParams(max_new_tokens=T, temperature=1.0, top_k=0, seed=9)
    plain, _ = _staggered(model, sp, 0, True, _settings())
    look, _ = _staggered(model, sp, 3, True, _settings())
    for i in range(4):
        assert look[i].tokens == plain[i].tokens, i
        assert look[i].logprobs == pytest.approx(plain[i].logprobs, abs=1e-4)
        assert look[i].seed == 100 + i
    assert len({tuple(look[i].tokens) for i in range(4)}) == 4
    # at temperature 0.7 this random-weight model is near uniform over its top 50 and reproduces no
    # draft; a colder mix of the same requests does, so positions j > 0 of a step are emitted too
    cold = [RequestSampling(seed=200 + i, temperature=0.12, top_k=50) for i in range(4)]
    plain_c, _ = _staggered(model, sp, 0, True, cold)
    look_c, _ = _staggered(model, sp, 3, True, cold)
    for i in range(4):
        assert look_c[i].tokens == plain_c[i].tokens, i
    assert sum(look_c[i].lookup_accepted for i in range(4)) > 0
    assert any(look_c[i].tokens != look[i].tokens for i in range(4))
    # request 3: alone; in row 1 beside another request; in row 0 after another occupant has run
    cb = _batcher(model, sp, 3, True)
    cb.admit(REQS[3], "alone", _settings()[3])
    alone = _drain(cb, {})["alone"]
    cb.admit_many([REQS[1], REQS[3]], ["x", "row1"], [_settings()[1], _settings()[3]])
    got = _drain(cb, {})
    cb.admit(REQS[3], "later", _settings()[3])  # row 0 again, after "alone" and "x" used it
    got = _drain(cb, got)
    cb.close()
    assert alone.tokens == got["row1"].tokens == got["later"].tokens == plain[3].tokens
    assert got["x"].tokens == plain[1].tokens


def test_per_request_length_cuts_accepted_run(model, plain_greedy):
    """request 1 at K = 3 emits 4 tokens in the verify step that starts at 13 generated tokens: a
    max_new_tokens of 16 must cut that step to exactly 3"""
    em = []
    cb = _batcher(model, GREEDY, 3, True)
    cb.admit(REQS[1], 1)
    full = _drain(cb, {}, None, em)[1]
    lens = [1]
    for e in em:
        lens.append(lens[-1] + e[0])
    assert full.tokens == plain_greedy[1].tokens
    i4 = next(i for i, e in enumerate(em) if e[0] == 4)
    assert lens[i4] == 13  # the step the docstring names
    em2 = []
    cb.admit(REQS[1], "cut", RequestSampling(max_new_tokens=16))
    cut = _drain(cb, {}, None, em2)["cut"]
    cb.close()
    assert [e[0] for e in em2[:i4]] == [e[0] for e in em[:i4]] and em2[i4][0] == 3 and len(em2) == i4 + 1
    assert cut.tokens == plain_greedy[1].tokens[:16] and len(cut.logprobs) == 16
    assert cut.lookup_steps == i4 + 1 and cut.lookup_steps + cut.lookup_accepted == 15


def test_eos_inside_a_multi_token_step_frees_the_row(model, plain_greedy):
    assert plain_greedy[0].tokens[18:20] == [72, 116]  # request 0: EOS candidate after a run of repeats
    em = []
    cb = _batcher(model, GREEDY, 3, eos=(116,))
    cb.admit_many(REQS[:2], [0, 1])
    got = _drain(cb, {}, None, em)
    assert got[0].tokens == plain_greedy[0].tokens[:20]
    last = max(i for i, e in enumerate(em) if e[0] > 0)
    assert em[last][0] >= 2  # the EOS arrived behind an accepted draft token, in one step
    assert cb.free_rows() == MB and int(cb.gen.active.sum()) == 0
    cb.close()


def test_readmitted_row_does_not_draft_from_old_history(model, plain_greedy):
    fresh = _batcher(model, GREEDY, 3)
    fresh.admit(REQS[1], "f")
    f = _drain(fresh, {})["f"]
    f_tot = fresh.lookup_totals
    fresh.close()
    cb = _batcher(model, GREEDY, 3)
    cb.admit(REQS[2], "long")  # 11 tokens of 77, then its answer, fill row 0's history
    _drain(cb, {})
    t0 = cb.lookup_totals
    cb.admit(REQS[1], "short")  # 3 tokens, same row
    assert int(cb.gen._lk.n_draft[0]) == len(brute_draft(REQS[1] + f.tokens[:1], 4, 0, 3, 2))
    s = _drain(cb, {})["short"]
    tot = tuple(a - b for a, b in zip(cb.lookup_totals, t0))
    cb.close()
    assert s.tokens == f.tokens == plain_greedy[1].tokens
    assert (s.lookup_steps, s.lookup_accepted) == (f.lookup_steps, f.lookup_accepted)
    assert tot == f_tot  # also the number of drafted tokens: the same proposals as in a fresh batcher


def test_per_request_draft_length(model, plain_greedy):
    cb = _batcher(model, GREEDY, 3, True)
    cb.admit_many(REQS[:3], [0, 1, 2], [RequestSampling(lookup_tokens=0), RequestSampling(lookup_tokens=1), None])
    em = []
    got = _drain(cb, {}, None, em)
    assert got[0].lookup_accepted == 0 and got[0].lookup_steps == len(got[0].tokens) - 1 == T - 1
    assert max(e[1] for e in em) == 2 and max(e[2] for e in em) > 1  # K = 1: at most 2 tokens per step
    for i in range(3):
        assert got[i].tokens == plain_greedy[i].tokens
    # invalid values take no row
    for bad in (-1, 4, 8, 1.5):
        with pytest.raises(ValueError):
            cb.admit(REQS[0], "bad", RequestSampling(lookup_tokens=bad))
    assert cb.free_rows() == MB
    cb.close()
    off = _batcher(model, GREEDY, 0, True)
    with pytest.raises(ValueError, match="lookup"):
        off.admit(REQS[0], "bad", RequestSampling(lookup_tokens=0))
    assert off.free_rows() == MB
    off.admit(REQS[0], "ok", RequestSampling())
    assert _drain(off, {})["ok"].lookup_steps is None
    off.close()
    with pytest.raises(ValueError):
        RequestSampling(lookup_tokens=9).validate()


def test_refusals(model):
    sp = SamplingParams(max_new_tokens=4, do_sample=False)
    with pytest.raises(NotImplementedError, match="lookup_tokens="):  # points at the keyword
        ContinuousBatcher(Generator(model, 2, 40, "cpu"), dataclasses.replace(sp, lookup_tokens=2))
    for K in (-1, 8):
        with pytest.raises(ValueError):
            _batcher(model, sp, K)
    m = _model()
    m.fused_decode_max_batch = 12
    with pytest.raises(ValueError, match="12"):
        _batcher(m, sp, 3)  # 4 rows x 4 positions
    _batcher(m, sp, 2).close()  # 12 rows fit
    m4 = models.CausalLM(PRESETS["tiny-llama"], dtype=torch.bfloat16, seed=2)  # MXFP4 images quantise bf16 weights
    m4.set_fp4_decode(True)
    with pytest.raises(ValueError, match="16"):
        _batcher(m4, sp, 4)  # 20 rows
    _batcher(m4, sp, 3).close()
    with pytest.raises(NotImplementedError):
        g8 = Generator(model, 2, 40, "cpu", use_graph=False)
        g8.cache.fp8 = True
        ContinuousBatcher(g8, sp, lookup_tokens=3)
    with pytest.raises(NotImplementedError):
        _batcher(_model(preset="tiny-opt"), sp, 3)
    with pytest.raises(NotImplementedError):
        ContinuousBatcher(Generator(model, 2, 40, "cpu", use_graph=False, value_head=lambda h: h[:, 0]), sp,
                          lookup_tokens=3)
    # adapters with lookup, keyword form
    ma = _model()
    bank = models.AdapterBank(ma, slots=2, r_max=8)
    with pytest.raises(ValueError, match="lookup"):
        ContinuousBatcher(Generator(ma, 2, 40, "cpu", use_graph=False), sp, adapters=bank, lookup_tokens=3)
    # room: len + T + K <= max_seq
    cb = _batcher(model, sp, 3, max_batch=2, max_seq=16)
    with pytest.raises(ValueError, match="cache"):
        cb.admit(list(range(1, 11)), "big")  # 10 + 4 + 3 > 16
    assert cb.free_rows() == 2 and cb.active_rows() == 0
    cb.admit(list(range(1, 10)), "fits")  # 9 + 4 + 3 == 16
    assert len(_drain(cb, {})["fits"].tokens) == 4
    cb.close()
    plain = _batcher(model, sp, 0, max_batch=2, max_seq=16)
    plain.admit(list(range(1, 11)), "big")  # without lookup the same prompt fits
    plain.close()


def test_engine_lookup():
    from test_per_request_sampling_cpu import _tiny_pipe

    from rag_tl_domainllm_optimizer_amd.serve import ContinuousEngine, request_sampling

    pipe0, words = _tiny_pipe(max_batch=2, new=12, do_sample=False)
    pipe3, _ = _tiny_pipe(max_batch=2, new=12, do_sample=False, lookup_tokens=3)
    qs = [f"{words[1]} {words[4]}", f"{words[2]} {words[5]}", f"{words[3]} {words[9]}"]
    with ContinuousEngine(pipe0, chunk=2) as e0:
        want = [e0.answer(q, timeout=120) for q in qs]
        assert "lookup_steps" not in e0.stats and "lookup_steps" not in want[0].timings
    with ContinuousEngine(pipe3, chunk=2) as e3:
        assert e3.lookup_tokens == 3
        got = [f.result(120) for f in [e3.submit(q) for q in qs]]
        stats = dict(e3.stats)
    for a, w in zip(got, want):
        assert a.answer == w.answer and a.timings["new_tokens"] == w.timings["new_tokens"]
        assert a.timings["lookup_steps"] + a.timings["lookup_accepted"] == a.timings["new_tokens"] - 1
    assert stats["lookup_steps"] == sum(a.timings["lookup_steps"] for a in got)
    assert stats["lookup_accepted"] == sum(a.timings["lookup_accepted"] for a in got)
    assert stats["lookup_accepted"] <= stats["lookup_drafted"] <= 3 * stats["lookup_steps"]
    with ContinuousEngine(pipe3, chunk=2, per_request_sampling=True) as e3:
        a = e3.answer(qs[0], sampling=RequestSampling(lookup_tokens=0, do_sample=False), timeout=120)
        assert a.answer == want[0].answer and a.timings["lookup_accepted"] == 0
        with pytest.raises(ValueError):
            e3.submit(qs[0], sampling=RequestSampling(lookup_tokens=4))
    with ContinuousEngine(pipe0, chunk=2, per_request_sampling=True) as e0:
        with pytest.raises(ValueError, match="lookup"):
            e0.submit(qs[0], sampling=RequestSampling(lookup_tokens=1))

    class Body:
        temperature = top_k_tokens = top_p = do_sample = seed = max_new_tokens = None
        lookup_tokens = 2

    assert request_sampling(Body(), 12, 3).lookup_tokens == 2
    with pytest.raises(ValueError):
        request_sampling(Body(), 12, 1)


# ----------------------------------------------------------------------------- reference twins
def test_ref_grouped_sample_rows_equals_one_row_calls():
    g = torch.Generator().manual_seed(0)
    B, G, V = 3, 4, 97
    logits = torch.randn(B * G, V, generator=g) * 2
    p = [torch.tensor([1.0, 1 / 0.7, 1.3]), torch.tensor([0, 20, 5], dtype=torch.int32), torch.tensor([1.0, 0.9, 1.0]),
         torch.tensor([1, 0, 0], dtype=torch.uint8), torch.tensor([11, 12, 13]), torch.tensor([0, 7, 21], dtype=torch.int32)]
    active = torch.ones(B * G, dtype=torch.uint8)
    active[2 * G + 1] = 0
    tok, lp = ops.sample_rows(logits, *p, active, group=G)
    for b in range(B):
        for j in range(G):
            r = b * G + j
            one = [t[b:b + 1].clone() for t in p]
            one[5] = one[5] + j
            t1, l1 = ref.sample_rows(logits[r:r + 1], *one, active[r:r + 1])
            assert int(tok[r]) == int(t1) and float(lp[r]) == float(l1), (b, j)
    assert int(tok[2 * G + 1]) == int(logits[2 * G + 1].argmax())  # the masked position: argmax, no draw
    t1, l1 = ops.sample_rows(logits[:B], *p, group=1)
    t0, l0 = ops.sample_rows(logits[:B], *p)
    assert torch.equal(t0, t1) and torch.equal(l0, l1)
    with pytest.raises(ValueError):
        ref.sample_rows(logits[:5], *p, None, 4)


def accept_rows_state(device="cpu"):
    """Five rows, K = 3 (G = 4), T = 10, Smax = 20, EOS = 99 -> (args, kwargs, plain-Python expectation)"""
    G, Tn, Smax = 4, 10, 20
    #        inp              n_draft sampled        gen_len active row_max kv_len
    rows = [([10, 1, 2, 3], 3, [1, 2, 3, 4], 3, 0, 10, 9),      # inactive
            ([10, 1, 2, 3], 3, [1, 2, 3, 4], 3, 1, 6, 9),       # a step would emit 4, row_max_new 6 leaves 3
            ([10, 1, 99, 3], 3, [1, 99, 3, 4], 1, 1, 10, 9),    # EOS mid-run
            ([10, 1, 2, 3], 0, [1, 2, 3, 4], 2, 1, 10, 9),      # row_draft 0 upstream: n_draft 0, one token
            ([10, 1, 2, 3], 3, [1, 2, 3, 4], 2, 1, 10, 17)]     # kv_len + 1 + i reaches Smax: the history guard
    B = len(rows)
    t = dict(sm=torch.tensor([r[2] for r in rows]).reshape(-1), lp=-torch.arange(B * G, dtype=torch.float32) / 4 - 1,
             inp=torch.tensor([r[0] for r in rows]), nd=torch.tensor([r[1] for r in rows], dtype=torch.int32),
             out_t=torch.full((B, Tn), PAD, dtype=torch.long), out_lp=torch.zeros(B, Tn),
             hist=torch.full((B, Smax), 400, dtype=torch.long), act=torch.tensor([r[4] for r in rows], dtype=torch.uint8),
             kv=torch.tensor([r[6] for r in rows], dtype=torch.int32), pos=torch.zeros(B, dtype=torch.int32),
             al=torch.zeros(B, dtype=torch.int32), ks=torch.tensor([0, 1, 0, 0, 2], dtype=torch.int32),
             gl=torch.tensor([r[3] for r in rows], dtype=torch.int32), step=torch.tensor([5]), off=torch.tensor([8]),
             cnt=torch.zeros(3, dtype=torch.long), eos=torch.tensor([99]),
             rmax=torch.tensor([r[5] for r in rows], dtype=torch.int32),
             stats=torch.tensor([[7, 7], [1, 0], [0, 0], [2, 1], [0, 0]], dtype=torch.int32))
    t = {k: v.to(device) for k, v in t.items()}
    # the plain-Python model
    exp = []
    for b, (inp, nd, sm, gl, act, rmax, kv) in enumerate(rows):
        emit, fin = [], False
        if act:
            a = 0
            while a < nd and sm[a] == inp[a + 1]:
                a += 1
            for i in range(a + 1):
                emit.append(sm[i])
                if gl + len(emit) >= min(rmax, Tn) or sm[i] == 99:
                    fin = True
                    break
        exp.append(dict(emit=emit, active=int(act and not fin), gl=gl + len(emit), kv=kv + len(emit)))
    return t, rows, exp


def check_accept_rows(t, rows, exp):
    t = {k: v.cpu() for k, v in t.items()}
    G, Smax = 4, 20
    stats0 = [[7, 7], [1, 0], [0, 0], [2, 1], [0, 0]]
    steps = 0
    for b, (r, e) in enumerate(zip(rows, exp)):
        n, g0, k0 = len(e["emit"]), r[3], r[6]
        assert t["out_t"][b, g0:g0 + n].tolist() == e["emit"] and int((t["out_t"][b] != PAD).sum()) == n, b
        assert torch.equal(t["out_lp"][b, g0:g0 + n], t["lp"][b * G:b * G + n]), b
        want_h = [400] * Smax
        for i, tk in enumerate(e["emit"]):
            if k0 + 1 + i < Smax:
                want_h[k0 + 1 + i] = tk
        assert t["hist"][b].tolist() == want_h, b
        assert (int(t["gl"][b]), int(t["kv"][b]), int(t["act"][b])) == (e["gl"], e["kv"], e["active"]), b
        assert int(t["al"][b]) == e["kv"] + 1 and int(t["pos"][b]) == e["kv"] - int(t["ks"][b]), b
        s = [stats0[b][0] + (1 if r[4] else 0), stats0[b][1] + max(n - 1, 0)]
        assert t["stats"][b].tolist() == s, b
        steps += 1 if r[4] else 0
    assert [len(e["emit"]) for e in exp] == [0, 3, 2, 1, 4]  # what the rows are meant to exercise
    assert t["cnt"].tolist() == [steps, 3 + 3 + 0 + 3, 2 + 1 + 0 + 3]
    assert int(t["step"]) == 6 and int(t["off"]) == 9


def run_accept_rows(t):
    ops.lookup_accept(t["sm"], t["lp"], t["inp"], t["nd"], t["out_t"], t["out_lp"], t["hist"], t["act"], t["kv"],
                      t["pos"], t["al"], t["ks"], t["gl"], t["step"], t["off"], t["cnt"], t["eos"],
                      row_max_new=t["rmax"], row_stats=t["stats"])


def test_ref_accept_rows_equals_python_model():
    t, rows, exp = accept_rows_state()
    run_accept_rows(t)
    check_accept_rows(t, rows, exp)


DRAFT_ROWS = [  # (history, kv_start, active, row_draft) at K = 3, ngram 2
    ([7, 8, 1, 7, 8, 2, 3, 7, 8, 4, 5, 6, 9, 7, 8], 0, 1, 3),
    ([7, 8, 1, 7, 8, 2, 3, 7, 8, 4, 5, 6, 9, 7, 8], 0, 1, 1),
    ([7, 8, 1, 7, 8, 2, 3, 7, 8, 4, 5, 6, 9, 7, 8], 0, 1, 0),
    ([7, 8, 1, 7, 8, 2, 3, 7, 8, 4, 5, 6, 9, 7, 8], 0, 0, 3),   # inactive
    ([1, 2, 3, 4, 1, 2], 0, 1, 9),                              # above K: capped at K, 3 of 4 followers
]


def run_draft_rows(device="cpu"):
    B, K, Smax = len(DRAFT_ROWS), 3, 24
    hist = torch.full((B, Smax), 499, dtype=torch.long)
    for b, (h, _, _, _) in enumerate(DRAFT_ROWS):
        hist[b, :len(h)] = torch.tensor(h)
    kv = torch.tensor([len(r[0]) - 1 for r in DRAFT_ROWS], dtype=torch.int32)
    ks = torch.tensor([r[1] for r in DRAFT_ROWS], dtype=torch.int32)
    act = torch.tensor([r[2] for r in DRAFT_ROWS], dtype=torch.uint8)
    rd = torch.tensor([r[3] for r in DRAFT_ROWS], dtype=torch.int32)
    inp = torch.full((B, K + 1), -7, dtype=torch.long)
    nd = torch.full((B,), -7, dtype=torch.int32)
    ra = torch.full((B * (K + 1),), 9, dtype=torch.uint8)
    a = [x.to(device) for x in (hist, kv, ks, act, inp, nd, ra, rd)]
    ops.lookup_draft(a[0], a[1], a[2], a[3], 2, PAD, a[4], a[5], a[6], row_draft=a[7])
    return a[4].cpu(), a[5].cpu(), a[6].cpu()


def check_draft_rows(inp, nd, ra):
    K = 3
    for b, (h, s, act, rd) in enumerate(DRAFT_ROWS):
        d = brute_draft(h, len(h), s, min(rd, K), 2) if act and rd > 0 else []
        assert int(nd[b]) == len(d), b
        assert inp[b].tolist() == ([h[-1]] + d + [PAD] * (K - len(d)) if act else [PAD] * (K + 1)), b
        assert ra[b * (K + 1):(b + 1) * (K + 1)].tolist() == [act] * (K + 1), b
    assert nd.tolist() == [3, 1, 0, 0, 3]


def test_ref_draft_rows_equals_python_model():
    check_draft_rows(*run_draft_rows())
