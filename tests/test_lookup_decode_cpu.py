"""Prompt-lookup speculative decoding on the CPU path (fp32): the eager twins of the drafter, the
accept bookkeeping and the verify attention, and generation end to end against plain decoding.

``lookup_steps`` is summed over rows, so "fewer steps than plain decoding" reads
``lookup_steps < 47 * rows`` for 48 new tokens (plain: 47 decode steps per row)."""
import pytest
import torch

from rag_tl_domainllm_optimizer_amd import models, ops
from rag_tl_domainllm_optimizer_amd.generation import ContinuousBatcher, Generator, SamplingParams
from rag_tl_domainllm_optimizer_amd.models.config import PRESETS
from rag_tl_domainllm_optimizer_amd.ops import reference as ref
from rag_tl_domainllm_optimizer_amd.train import score_sequences

PROMPTS = [[5, 9, 33, 41, 7, 8, 5, 9, 33, 41], [12, 300, 4], [77] * 11]
PAD = 0


# ----------------------------------------------------------------------------- drafter
def brute_draft(h, end, ks, K, ngram):
    """(draft tokens, n) by the definition: longest n first, latest start, >= 1 token follows."""
    for n in range(ngram, 0, -1):
        if end - n < 0:
            continue
        starts = [i for i in range(ks, end - n) if h[i:i + n] == h[end - n:end]]
        if starts:
            c = max(starts) + n
            return h[c:min(c + K, end)]
    return []


DRAFT_CASES = [
    # (history, kv_start, ngram, K)
    ([1, 2, 3, 4, 5, 6], 0, 2, 3),                      # no match
    ([7, 8, 1, 7, 8, 2, 3, 7, 8, 4, 5, 6, 9, 7, 8], 0, 2, 3),  # several matches: the latest wins
    ([1, 2, 3, 4, 1, 2], 0, 2, 7),                      # continuation shorter than K
    ([9, 5, 1, 2, 3, 4, 6, 5], 0, 2, 3),                # only n = 1 matches after n = 2 fails
    ([0, 0, 0, 4, 0, 0], 3, 2, 3),                      # left pads equal to real tokens must not match
    ([0, 0, 0, 4, 0, 0], 0, 2, 3),                      # ... and do match when they are real
    ([5], 0, 2, 3),                                     # history shorter than n
    ([3, 3], 0, 2, 3),                                  # n = 2 impossible, n = 1 matches itself
    ([4, 4, 4, 4, 4, 4, 4, 4, 4, 4], 0, 3, 7),          # overlapping matches
]


def run_draft(cases, device="cpu"):
    B, Smax = len(cases), 24
    outs = []
    for ngram in sorted({c[2] for c in cases}):
        for K in sorted({c[3] for c in cases}):
            rows = [c for c in cases if c[2] == ngram and c[3] == K]
            if not rows:
                continue
            n = len(rows)
            hist = torch.full((n, Smax), 499, dtype=torch.long)
            kv_len = torch.zeros(n, dtype=torch.int32)
            ks = torch.zeros(n, dtype=torch.int32)
            for b, (h, s, _, _) in enumerate(rows):
                hist[b, :len(h)] = torch.tensor(h)
                kv_len[b], ks[b] = len(h) - 1, s
            act = torch.ones(n, dtype=torch.uint8)
            inp = torch.full((n, K + 1), -7, dtype=torch.long)
            nd = torch.full((n,), -7, dtype=torch.int32)
            ra = torch.zeros(n * (K + 1), dtype=torch.uint8)
            t = [x.to(device) for x in (hist, kv_len, ks, act, inp, nd, ra)]
            ops.lookup_draft(t[0], t[1], t[2], t[3], ngram, PAD, t[4], t[5], t[6])
            outs.append((rows, K, ngram, t[4].cpu(), t[5].cpu(), t[6].cpu()))
    return outs


def test_drafter_matches_brute_force():
    seen = 0
    for rows, K, ngram, inp, nd, ra in run_draft(DRAFT_CASES):
        for b, (h, s, _, _) in enumerate(rows):
            d = brute_draft(h, len(h), s, K, ngram)
            assert int(nd[b]) == len(d), (h, s)
            assert inp[b].tolist() == [h[-1]] + d + [PAD] * (K - len(d)), (h, s)
            seen += 1
        assert bool(ra.all())
    assert seen == len(DRAFT_CASES)
    # what the cases are meant to exercise
    assert brute_draft(DRAFT_CASES[0][0], 6, 0, 3, 2) == []
    assert brute_draft(DRAFT_CASES[1][0], 15, 0, 3, 2) == [4, 5, 6]
    assert brute_draft(DRAFT_CASES[2][0], 6, 0, 7, 2) == [3, 4, 1, 2]
    assert brute_draft(DRAFT_CASES[3][0], 8, 0, 3, 2) == [1, 2, 3]
    assert brute_draft(DRAFT_CASES[4][0], 6, 3, 3, 2) == [0]     # n = 1: the 0 at 4 is followed by 0
    assert brute_draft(DRAFT_CASES[5][0], 6, 0, 3, 2) == [4, 0, 0]  # the bigram of pads at 1..2


def test_drafter_inactive_row_gets_pad():
    hist = torch.tensor([[1, 2, 1, 2, 0, 0]])
    inp = torch.full((1, 4), 9, dtype=torch.long)
    nd = torch.full((1,), 5, dtype=torch.int32)
    ra = torch.ones(4, dtype=torch.uint8)
    ref.lookup_draft(hist, torch.tensor([3], dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                     torch.zeros(1, dtype=torch.uint8), 2, PAD, inp, nd, ra)
    assert inp.tolist() == [[PAD] * 4] and int(nd) == 0 and not bool(ra.any())


# ----------------------------------------------------------------------------- accept
def accept_state(device="cpu"):
    """Six rows, K = 4 (G = 5), T = 8, EOS = 99; returns (args of ops.lookup_accept, expectations)."""
    G, T, Smax = 5, 8, 32
    #        inp (last | draft)      n_draft  sampled              gen_len active
    rows = [([10, 1, 2, 3, 4], 4, [7, 2, 3, 4, 5], 1, 1),     # a = 0
            ([10, 1, 2, 0, 0], 2, [1, 2, 6, 0, 0], 1, 1),     # a = n_draft < K (pad 0 == sampled 0 must not count)
            ([10, 1, 2, 3, 4], 4, [1, 2, 3, 4, 5], 1, 1),     # a = K
            ([10, 1, 99, 3, 4], 4, [1, 99, 3, 4, 5], 1, 1),   # EOS at draft position 1 of 4 accepted
            ([10, 1, 2, 3, 4], 4, [1, 2, 3, 4, 5], 6, 1),     # T reached mid-run
            ([10, 1, 2, 3, 4], 4, [1, 2, 3, 4, 5], 3, 0)]     # inactive
    emit = [[7], [1, 2, 6], [1, 2, 3, 4, 5], [1, 99], [1, 2], []]
    fin = [0, 0, 0, 1, 1, 0]
    B = len(rows)
    inp = torch.tensor([r[0] for r in rows])
    nd = torch.tensor([r[1] for r in rows], dtype=torch.int32)
    sm = torch.tensor([r[2] for r in rows]).reshape(-1)
    lp = -torch.arange(B * G, dtype=torch.float32) / 8 - 0.5
    gl = torch.tensor([r[3] for r in rows], dtype=torch.int32)
    act = torch.tensor([r[4] for r in rows], dtype=torch.uint8)
    kv_len = torch.tensor([12, 13, 14, 15, 16, 17], dtype=torch.int32)
    ks = torch.tensor([0, 2, 0, 0, 0, 0], dtype=torch.int32)
    out_t = torch.full((B, T), PAD, dtype=torch.long)
    out_lp = torch.zeros(B, T)
    hist = torch.full((B, Smax), 400, dtype=torch.long)
    pos, al = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    step, off = torch.tensor([3]), torch.tensor([11])
    cnt = torch.zeros(3, dtype=torch.long)
    eos = torch.tensor([99, 98])
    args = [t.to(device) for t in (sm, lp, inp, nd, out_t, out_lp, hist, act, kv_len, pos, al, ks, gl, step, off, cnt,
                                   eos)]
    return args, dict(rows=rows, emit=emit, fin=fin, G=G, T=T, lp=lp, kv0=kv_len.clone(), ks=ks)


def check_accept(args, ex):
    sm, lp, inp, nd, out_t, out_lp, hist, act, kv_len, pos, al, ks, gl, step, off, cnt, eos = [a.cpu() for a in args]
    G = ex["G"]
    for b, (r, e, f) in enumerate(zip(ex["rows"], ex["emit"], ex["fin"])):
        g0, k0 = r[3], int(ex["kv0"][b])
        assert out_t[b, g0:g0 + len(e)].tolist() == e, b
        assert out_t[b, g0 + len(e):].tolist() == [PAD] * (ex["T"] - g0 - len(e)), b
        assert torch.equal(out_lp[b, g0:g0 + len(e)], ex["lp"][b * G:b * G + len(e)]), b
        assert hist[b, k0 + 1:k0 + 1 + len(e)].tolist() == e and int(hist[b, k0 + 1 + len(e)]) == 400, b
        assert int(gl[b]) == g0 + len(e) and int(kv_len[b]) == k0 + len(e), b
        assert int(act[b]) == (r[4] if not f else 0), b
        assert int(al[b]) == int(kv_len[b]) + 1 and int(pos[b]) == int(kv_len[b]) - int(ex["ks"][b]), b
    assert int(step) == 4 and int(off) == 12
    assert cnt.tolist() == [5, 18, 0 + 2 + 4 + 1 + 1]


def test_accept_twin_hand_cases():
    args, ex = accept_state()
    ops.lookup_accept(*args)
    check_accept(args, ex)


# ----------------------------------------------------------------------------- verify attention
def verify_inputs(B, Hq, Hkv, D, G, Smax, len0, kv_start_row, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B * G, (Hq + 2 * Hkv) * D, generator=g) * 0.5).to(dtype)
    kc = (torch.randn(B, Hkv, Smax, D, generator=g) * 0.5).to(dtype)
    vc = (torch.randn(B, Hkv, Smax, D, generator=g) * 0.5).to(dtype)
    al = torch.tensor([max(1, len0 - 3 * b) for b in range(B)], dtype=torch.int32)
    ks = torch.zeros(B, dtype=torch.int32)
    if kv_start_row is not None and kv_start_row < B:
        ks[kv_start_row] = min(5, int(al[kv_start_row]) - 1)
    pos = (al - 1 - ks).to(torch.int32)
    return qkv, kc, vc, al, ks, pos


def successive_decode(qkv, kc, vc, al, ks, pos, Hq, G, window, cos, sin):
    """the oracle: G successive decode steps on copies of the caches -> (o [B*G, Hq*D], kc, vc)"""
    kc, vc = kc.clone(), vc.clone()
    outs = []
    for j in range(G):
        o = ops.decode_step_attention(qkv[j::G].contiguous(), kc, vc, al - 1 + j, al + j, Hq, pos + j, cos, sin, ks,
                                      window)
        outs.append(o)
    return torch.stack(outs, 1).reshape(qkv.shape[0], -1), kc, vc


@pytest.mark.parametrize("window", [0, 3, 64])
@pytest.mark.parametrize("G", [1, 4, 8])
def test_verify_attention_twin_matches_successive_decode(G, window):
    B, Hq, Hkv, D, Smax = 3, 4, 2, 64, 96
    cos, sin = ref.rope_tables(D, 128)
    qkv, kc, vc, al, ks, pos = verify_inputs(B, Hq, Hkv, D, G, Smax, 70, 1, torch.float32)
    kc[:, :, 75:] = 1e4  # sentinel in the never-written slots
    vc[:, :, 75:] = 1e4
    o_ref, kc_ref, vc_ref = successive_decode(qkv, kc, vc, al, ks, pos, Hq, G, window, cos, sin)
    k2, v2 = kc.clone(), vc.clone()
    o = ops.verify_step_attention(qkv, k2, v2, al - 1, al, Hq, G, pos, cos, sin, ks, window)
    torch.testing.assert_close(o, o_ref, rtol=0, atol=1e-5)
    assert torch.equal(k2, kc_ref) and torch.equal(v2, vc_ref)  # appended rows equal, the rest untouched
    for b in range(B):
        s0 = int(al[b]) - 1
        assert torch.equal(k2[b, :, :s0], kc[b, :, :s0]) and torch.equal(k2[b, :, s0 + G:], kc[b, :, s0 + G:])
        assert not torch.equal(k2[b, :, s0:s0 + G], kc[b, :, s0:s0 + G])


# ----------------------------------------------------------------------------- end to end
def _model(preset, seed):
    return models.CausalLM(PRESETS[preset], dtype=torch.float32, seed=seed)


@pytest.fixture(scope="module")
def plain():
    """plain greedy outputs per (preset, seed, eos, T), computed once"""
    cache = {}

    def get(preset, seed, eos=(-1,), T=48):
        key = (preset, seed, tuple(eos), T)
        if key not in cache:
            m = _model(preset, seed)
            g = Generator(m, 4, 80, device="cpu")
            cache[key] = (m, g.generate(PROMPTS, SamplingParams(max_new_tokens=T, do_sample=False), pad_id=PAD,
                                        eos_ids=list(eos)))
        return cache[key]
    return get


@pytest.mark.parametrize("seed", [2, 4])
@pytest.mark.parametrize("preset", ["tiny-llama", "tiny-mistral"])
def test_greedy_lookup_equals_plain(plain, preset, seed):
    m, ref_out = plain(preset, seed)
    g = Generator(m, 4, 80, device="cpu", sync_every=1)  # the loop stops at the step the last row finishes
    for K in (1, 3, 7):
        o = g.generate(PROMPTS, SamplingParams(max_new_tokens=48, do_sample=False, lookup_tokens=K), pad_id=PAD,
                       eos_ids=[-1])
        assert o.timings["decode_steps"] < 47, o.timings  # verify steps replayed; plain decoding: 47
        assert torch.equal(o.tokens, ref_out.tokens) and torch.equal(o.lengths, ref_out.lengths), K
        torch.testing.assert_close(o.logprobs, ref_out.logprobs, rtol=0, atol=1e-4)
        t = o.timings
        assert t["lookup_accepted"] > 0 and t["lookup_steps"] < 47 * len(PROMPTS), t
        assert t["lookup_accepted"] <= t["lookup_drafted"] <= K * t["lookup_steps"]
        # every token after the first is emitted by a row-step: one per step plus the accepted ones
        assert t["lookup_steps"] + t["lookup_accepted"] == 47 * len(PROMPTS)


def test_greedy_lookup_eos_inside_accepted_run(plain):
    m, ref_out = plain("tiny-llama", 2, eos=(116,))
    n0 = int(ref_out.lengths[0])
    assert ref_out.tokens[0, n0 - 1] == 116 and ref_out.tokens[0, n0 - 3:n0 - 1].tolist() == [72, 72] and n0 < 48
    g = Generator(m, 4, 80, device="cpu")
    for K in (3, 7):
        o = g.generate(PROMPTS, SamplingParams(max_new_tokens=48, do_sample=False, lookup_tokens=K), pad_id=PAD,
                       eos_ids=[116])
        assert torch.equal(o.tokens, ref_out.tokens) and torch.equal(o.lengths, ref_out.lengths)
        assert o.tokens[0, n0:].tolist() == [PAD] * (48 - n0)


def test_greedy_lookup_width_reached_mid_run(plain):
    m, ref_out = plain("tiny-llama", 2, T=5)
    g = Generator(m, 4, 80, device="cpu")
    o = g.generate(PROMPTS, SamplingParams(max_new_tokens=5, do_sample=False, lookup_tokens=7), pad_id=PAD,
                   eos_ids=[-1])
    assert torch.equal(o.tokens, ref_out.tokens) and o.lengths.tolist() == [5, 5, 5]


def test_sampled_lookup_reproducible_and_logprobs_score():
    m = _model("tiny-llama", 2)
    g = Generator(m, 4, 80, device="cpu")
    sp = SamplingParams(max_new_tokens=24, temperature=0.7, top_k=0, seed=3, lookup_tokens=3)
    torch.manual_seed(0)  # the CPU sampler draws from the global generator
    a = g.generate(PROMPTS, sp, pad_id=PAD, eos_ids=[-1])
    torch.manual_seed(0)
    b = g.generate(PROMPTS, sp, pad_id=PAD, eos_ids=[-1])
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.logprobs, b.logprobs)
    with torch.no_grad():
        lp = score_sequences(m, a.prompt_ids, a.prompt_start, a.tokens, a.lengths, 1 / 0.7)[0]
    torch.testing.assert_close(a.logprobs, lp.float(), rtol=0, atol=1e-4)


def test_plain_after_lookup_is_unchanged(plain):
    m, ref_out = plain("tiny-mistral", 4)
    g = Generator(m, 4, 80, device="cpu")
    g.generate(PROMPTS, SamplingParams(max_new_tokens=48, do_sample=False, lookup_tokens=3), pad_id=PAD, eos_ids=[-1])
    o = g.generate(PROMPTS, SamplingParams(max_new_tokens=48, do_sample=False), pad_id=PAD, eos_ids=[-1])
    assert torch.equal(o.tokens, ref_out.tokens) and torch.equal(o.logprobs, ref_out.logprobs)
    assert "lookup_steps" not in o.timings


def test_single_token_answer_reports_zero_counters():
    o = Generator(_model("tiny-llama", 2), 2, 40, device="cpu").generate(
        [[1, 2, 3]], SamplingParams(max_new_tokens=1, do_sample=False, lookup_tokens=3), pad_id=PAD, eos_ids=[-1])
    assert o.lengths.tolist() == [1]
    assert (o.timings["lookup_steps"], o.timings["lookup_drafted"], o.timings["lookup_accepted"]) == (0, 0, 0)


def test_out_of_scope_combinations_raise():
    m = _model("tiny-llama", 2)
    sp = SamplingParams(max_new_tokens=4, do_sample=False, lookup_tokens=3)
    with pytest.raises(ValueError):
        Generator(m, 2, 40, device="cpu").generate([[1, 2]], SamplingParams(max_new_tokens=4, lookup_tokens=8))
    with pytest.raises(AssertionError):  # S + T + K <= max_seq
        Generator(m, 2, 8, device="cpu").generate([[1, 2]], sp)
    with pytest.raises(NotImplementedError):
        Generator(_model("tiny-opt", 2), 2, 40, device="cpu").generate([[1, 2]], sp)
    with pytest.raises(NotImplementedError):
        Generator(m, 2, 40, device="cpu", value_head=lambda h: h[:, 0]).generate([[1, 2]], sp)
    with pytest.raises(NotImplementedError):
        g8 = Generator(m, 2, 40, device="cpu")
        g8.cache.fp8 = True
        g8.generate([[1, 2]], sp)
    with pytest.raises(NotImplementedError):
        ContinuousBatcher(Generator(m, 2, 40, device="cpu"), sp)
