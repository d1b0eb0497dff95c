"""Prompt-lookup speculative decoding on the GPU: the verify attention kernel against the CPU oracle
and against successive decode steps, the drafter / accept kernels against their twins, and generation
end to end (graph == eager, lookup greedy == plain greedy, log-probs == teacher forcing).

Greedy pairs kept: (tiny-llama, seeds 2 and 4) and (tiny-mistral, seed 2, 80 tokens); each is first
checked to give identical plain greedy output at row bucket 1 and row bucket 8 (bf16 kernels at
different row counts may break a near-tie differently: such a pair would say nothing about lookup
decoding). No pair was dropped."""
import pytest
import torch

from rag_tl_domainllm_optimizer_amd import models, ops
from rag_tl_domainllm_optimizer_amd.generation import Generator, SamplingParams
from rag_tl_domainllm_optimizer_amd.models.config import PRESETS
from rag_tl_domainllm_optimizer_amd.ops import reference as ref

import test_lookup_decode_cpu as cpu_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROMPTS = cpu_cases.PROMPTS
LEN0 = [1, 15, 16, 17, 63, 64, 65, 300]


def _close(a, b, rtol=2e-2, atol=2e-2):
    """the tolerance of test_kernels_gpu.test_decode_step_fused against the same kind of oracle"""
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item() + 1e-6
    assert err <= atol + rtol * scale, f"max err {err} (scale {scale})"


def _bits(t):
    return t.contiguous().view(torch.int16)


def _verify_case(B, Hq, Hkv, D, G, Smax, len0, window, cos, sin, seed, successive=False):
    g = torch.Generator().manual_seed(seed)
    W = (Hq + 2 * Hkv) * D
    qkv = torch.randn(B * G, W, generator=g).to(torch.bfloat16)
    kc = torch.randn(B, Hkv, Smax, D, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, Hkv, Smax, D, generator=g).to(torch.bfloat16)
    al = torch.tensor([len0] + [max(1, len0 - 7 * b) for b in range(1, B)], dtype=torch.int32)
    ks = torch.zeros(B, dtype=torch.int32)
    ks[B - 1] = min(5, int(al[B - 1]) - 1)  # one left-padded row
    pos = (al - 1 - ks).to(torch.int32)
    # the slots being appended and every slot after them hold NaN (a fresh cache, a rejected draft)
    tail = torch.arange(Smax)[None, None, :, None] >= (al.long() - 1)[:, None, None, None]
    kc.masked_fill_(tail, float("nan"))
    vc.masked_fill_(tail, float("nan"))
    kd, vd = kc.to(DEV), vc.to(DEV)
    out = ops.verify_step_attention(qkv.to(DEV), kd, vd, (al - 1).to(DEV), al.to(DEV), Hq, G, pos.to(DEV),
                                    cos.to(DEV), sin.to(DEV), ks.to(DEV), window)
    k2, v2 = kc.clone(), vc.clone()
    o_ref = ops.verify_step_attention(qkv, k2, v2, al - 1, al, Hq, G, pos, cos, sin, ks, window)
    assert torch.isfinite(out).all()
    _close(out.cpu(), o_ref)
    amax = qkv.float().abs().max().item()
    for b in range(B):
        s0 = int(al[b]) - 1
        for got, want, old in ((kd[b].cpu(), k2[b], kc[b]), (vd[b].cpu(), v2[b], vc[b])):
            new, exp = got[:, s0:s0 + G].float(), want[:, s0:s0 + G].float()
            # one bf16 ulp of the oracle's value, plus the oracle's own fp32 rounding (two products and
            # a sum of operands up to amax, no fma): where x1 c - x2 s cancels, that error alone exceeds
            # a bf16 ulp of the result (the rope kernel of the prefill differs from it the same way)
            ulp = exp.abs() * 2.0 ** -7 + 3 * 2.0 ** -24 * amax
            assert bool(((new - exp).abs() <= ulp).all()), "appended rows"
            assert torch.equal(_bits(got[:, :s0]), _bits(old[:, :s0])), "slots below slot0 touched"
            assert torch.equal(_bits(got[:, s0 + G:]), _bits(old[:, s0 + G:])), "slots past the new rows touched"
    if successive:
        # G successive launches of the decode step: same rotation code -> the same appended bytes
        ks_d, kc_s, vc_s = ks.to(DEV), kc.to(DEV), vc.to(DEV)
        ws = ops.decode_workspace(B, Hq, Hkv, D, Smax, DEV)
        qd = qkv.to(DEV)
        outs = []
        for j in range(G):
            outs.append(ops.decode_step_attention(qd[j::G].contiguous(), kc_s, vc_s, (al - 1 + j).to(DEV),
                                                  (al + j).to(DEV), Hq, (pos + j).to(DEV), cos.to(DEV), sin.to(DEV),
                                                  ks_d, window, workspace=ws))
        o_s = torch.stack(outs, 1).reshape(B * G, -1)
        _close(out, o_s)
        # head_dim 64: the decode kernel's arithmetic position by position. head_dim 128: the decode
        # kernel's fragments on the same 16-key tiles unless a window moves a later position's start
        # (and the decode step does not split the cache row over workgroups, as it does for long caches)
        if D == 64 or (Smax <= 512 and (window == 0 or window >= len0 + G)):
            assert torch.equal(_bits(out), _bits(o_s)), "not bitwise the successive decode steps"
        assert torch.equal(_bits(kd), _bits(kc_s)) and torch.equal(_bits(vd), _bits(vc_s))
        assert int(ws.tickets.abs().sum()) == 0


@pytest.mark.parametrize("G", [1, 2, 3, 4, 6, 8])
@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (8, 2), (4, 4)])
@pytest.mark.parametrize("D", [64, 128])
def test_verify_kernel_matches_cpu_oracle(D, Hq, Hkv, G):
    cos, sin = ref.rope_tables(D, 512)
    n = 0
    for B in (1, 3):
        for window in (0, 3, 64):
            for len0 in LEN0:
                _verify_case(B, Hq, Hkv, D, G, 512, len0, window, cos, sin, seed=n,
                             successive=(len0 in (17, 300)))
                n += 1


@pytest.mark.parametrize("D,Hq,Hkv,G", [(128, 8, 2, 8), (64, 4, 2, 4), (128, 16, 2, 8)])
def test_verify_kernel_long_cache(D, Hq, Hkv, G):
    cos, sin = ref.rope_tables(D, 4096)
    _verify_case(2, Hq, Hkv, D, G, 4096, 3000, 0, cos, sin, seed=1, successive=True)
    _verify_case(1, Hq, Hkv, D, G, 4096, 3000, 1024, cos, sin, seed=2)


@pytest.mark.parametrize("D,Hq,Hkv,G,len0", [(128, 16, 2, 8, 1), (128, 16, 2, 8, 17),  # 64 rows: four row tiles
                                             (64, 8, 2, 4, 257)])  # two partitions; row 1 ends inside the first
def test_verify_kernel_row_tile_and_partition_edges(D, Hq, Hkv, G, len0):
    cos, sin = ref.rope_tables(D, 512)
    _verify_case(2, Hq, Hkv, D, G, 96 if D == 128 else 512, len0, 0, cos, sin, seed=len0, successive=True)


def test_drafter_kernel_matches_twin():
    for (rows, K, ngram, inp, nd, ra), (_, _, _, inp_c, nd_c, ra_c) in zip(cpu_cases.run_draft(cpu_cases.DRAFT_CASES, DEV),
                                                                         cpu_cases.run_draft(cpu_cases.DRAFT_CASES)):
        assert torch.equal(inp, inp_c) and torch.equal(nd, nd_c) and torch.equal(ra, ra_c), (K, ngram)
    # a long random history over a small alphabet (every thread of the workgroup has candidates)
    g = torch.Generator().manual_seed(0)
    B, Smax, K = 5, 2000, 7
    hist = torch.randint(0, 6, (B, Smax), generator=g)
    kv_len = torch.tensor([1999, 1500, 700, 3, 900], dtype=torch.int32)
    ks = torch.tensor([0, 40, 0, 0, 0], dtype=torch.int32)
    act = torch.tensor([1, 1, 1, 1, 0], dtype=torch.uint8)
    res = []
    for dev in ("cpu", DEV):
        inp = torch.zeros(B, K + 1, dtype=torch.long, device=dev)
        nd = torch.zeros(B, dtype=torch.int32, device=dev)
        ra = torch.zeros(B * (K + 1), dtype=torch.uint8, device=dev)
        ops.lookup_draft(hist.to(dev), kv_len.to(dev), ks.to(dev), act.to(dev), 4, 0, inp, nd, ra)
        res.append((inp.cpu(), nd.cpu(), ra.cpu()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert int(res[0][1][0]) == K


def test_accept_kernel_matches_twin():
    args, ex = cpu_cases.accept_state(DEV)
    ops.lookup_accept(*args)
    cpu_cases.check_accept(args, ex)


# ----------------------------------------------------------------------------- end to end
def _plain(m, prompts, T, max_batch):
    return Generator(m, max_batch, 128, DEV).generate(prompts, SamplingParams(max_new_tokens=T, do_sample=False),
                                                      pad_id=0, eos_ids=[-1])


GREEDY_CASES = [("tiny-llama", 2, 48), ("tiny-llama", 4, 48), ("tiny-mistral", 2, 80)]


def _kept_model(preset, seed, T):
    """the model of a (preset, seed) pair, after the check that keeps the pair: plain greedy output
    of every prompt is the same at row bucket 1 and at row bucket 8"""
    m = models.CausalLM(PRESETS[preset], device=DEV, dtype=torch.bfloat16, seed=seed)
    for p in PROMPTS:
        p1 = _plain(m, [p], T, 1)
        p8 = _plain(m, [p] + [[3, 4, 5]] * 7, T, 8)
        assert torch.equal(p1.tokens[0], p8.tokens[0]), "near-tie in plain decoding: drop this prompt / seed pair"
    return m


@pytest.mark.parametrize("preset,seed,T", GREEDY_CASES)
def test_greedy_lookup_graph_eager_and_state(preset, seed, T):
    """Graph == eager bitwise; lookup greedy == plain greedy; repeated and plain generations on the
    same generator behave as on a fresh one."""
    m = _kept_model(preset, seed, T)
    want = _plain(m, PROMPTS, T, 4)
    for K in (3, 7):
        sp = SamplingParams(max_new_tokens=T, do_sample=False, lookup_tokens=K)
        gg = Generator(m, 4, 128, DEV, use_graph=True)
        a = gg.generate(PROMPTS, sp, pad_id=0, eos_ids=[-1])
        b = Generator(m, 4, 128, DEV, use_graph=False).generate(PROMPTS, sp, pad_id=0, eos_ids=[-1])
        assert torch.equal(a.tokens, b.tokens) and torch.equal(a.logprobs, b.logprobs), "graph != eager"
        assert torch.equal(a.lengths, want.lengths)
        assert torch.equal(a.tokens, want.tokens)
        assert a.timings["lookup_accepted"] > 0
        assert a.timings["lookup_steps"] + a.timings["lookup_accepted"] == (T - 1) * len(PROMPTS)
        # state hygiene: a second lookup generation, then plain decoding on the same generator
        a2 = gg.generate(PROMPTS, sp, pad_id=0, eos_ids=[-1])
        assert torch.equal(a2.tokens, a.tokens) and torch.equal(a2.logprobs, a.logprobs)
        assert a2.timings["lookup_steps"] == a.timings["lookup_steps"]
        pl = gg.generate(PROMPTS, SamplingParams(max_new_tokens=T, do_sample=False), pad_id=0, eos_ids=[-1])
        assert torch.equal(pl.tokens, want.tokens) and torch.equal(pl.logprobs, want.logprobs)
        assert int(gg.workspace.tickets.abs().sum()) == 0


@pytest.mark.parametrize("preset,seed,T", GREEDY_CASES)
def test_greedy_lookup_equals_plain_every_row(preset, seed, T):
    """Lookup greedy tokens == plain greedy tokens for every row of the pairs kept, mismatch zero.
    These outputs contain exact ties of the bf16 logits (e.g. tiny-llama seed 2, row 2, token 37:
    1.0625 vs 1.0625), which any other summation order in the attention breaks the other way: the
    check holds because at head_dim 64 the verify step is the decode kernel's own arithmetic."""
    m = _kept_model(preset, seed, T)
    want = _plain(m, PROMPTS, T, 4)
    for K in (3, 7):
        sp = SamplingParams(max_new_tokens=T, do_sample=False, lookup_tokens=K)
        a = Generator(m, 4, 128, DEV).generate(PROMPTS, sp, pad_id=0, eos_ids=[-1])
        for r in range(len(PROMPTS)):
            assert torch.equal(a.tokens[r], want.tokens[r]), (K, r)


# ---- head_dim 128: the MFMA verify kernel inside the generator (tiny models with Mistral's head shape)
def _cfg128(heads, kv, window=0):
    import dataclasses

    return dataclasses.replace(PRESETS["tiny-mistral" if window else "tiny-llama"], num_heads=heads, num_kv_heads=kv,
                               head_dim=128, sliding_window=window, name=f"tiny-d128-{heads}-{kv}-{window}")


D128_CASES = [  # (q heads, kv heads, window, K, seed, T)
    (2, 1, 0, 3, 2, 48),    # 8 query rows
    (4, 1, 0, 5, 2, 48),    # 24 rows: a partly filled second row tile, 6 / 24 GEMM rows
    (8, 1, 0, 7, 4, 48),    # Q = 8, K = 7: 64 query rows, four row tiles
    (4, 1, 32, 7, 2, 48),   # sliding window shorter than prompt + answer
]


@pytest.mark.parametrize("heads,kv,window,K,seed,T", D128_CASES)
def test_d128_lookup_end_to_end(heads, kv, window, K, seed, T):
    """Graph == eager bitwise, lookup greedy == plain greedy, log-probs == teacher forcing at the
    size and tolerance of test_decode_matches_teacher_forcing. Rows are kept by the rule of the
    head_dim-64 pairs, plain greedy identical at row buckets 1 and 8, and also at the bucket of the
    verify step's GEMM rows (measured: at 32 rows plain decoding itself breaks an exact logit tie,
    1.015625 vs 1.015625, the other way on row 1 of the 4-head model, rows 1 and 2 of the 8-head one:
    those rows are dropped; rows 0 and the 2-head and window models keep all).
    Without a window every position walks the decode kernel's own 16-key tiles, so all T tokens are
    compared. With a window shorter than the sequence the tiles of later positions start at other
    keys than a decode step's, and an exact tie of the bf16 logits may then break differently: there
    the comparison covers the tokens emitted while prompt + answer + K still fits the window."""
    from rag_tl_domainllm_optimizer_amd.train.common import score_sequences

    m = models.CausalLM(_cfg128(heads, kv, window), device=DEV, dtype=torch.bfloat16, seed=seed)
    # rows kept: plain greedy identical at row buckets 1 and 8 and at the bucket of the 4 * (K + 1) rows
    # the verify step's row-local GEMMs run at (all decided by the plain decoder alone)
    nbv = 16 if 4 * (K + 1) <= 16 else 32
    kept = []
    for r, p in enumerate(PROMPTS):
        p1 = _plain(m, [p], T, 1).tokens[0]
        if all(torch.equal(p1, _plain(m, [p] + [[3, 4, 5]] * (mb - 1), T, mb).tokens[0]) for mb in (8, nbv)):
            kept.append(r)
    print(f"rows kept: {kept} of {len(PROMPTS)}")
    assert kept, "no prompt kept"
    want = _plain(m, PROMPTS, T, 4)
    sp = SamplingParams(max_new_tokens=T, do_sample=False, lookup_tokens=K)
    a = Generator(m, 4, 128, DEV, use_graph=True).generate(PROMPTS, sp, pad_id=0, eos_ids=[-1])
    b = Generator(m, 4, 128, DEV, use_graph=False).generate(PROMPTS, sp, pad_id=0, eos_ids=[-1])
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.logprobs, b.logprobs), "graph != eager"
    S = max(len(p) for p in PROMPTS)
    n = T if not window else max(0, min(T, window - S - K))
    assert n > 0 and torch.equal(a.tokens[kept, :n], want.tokens[kept, :n])
    assert a.timings["lookup_accepted"] > 0
    # sampled: behaviour log-probs of the verify forward == teacher forcing
    prompts = [[5, 9, 33, 41, 7, 8, 9, 10], [12, 300, 4]]
    sps = SamplingParams(max_new_tokens=10, temperature=0.7, top_k=0, seed=5, lookup_tokens=K)
    out = Generator(m, 2, 64, DEV).generate(prompts, sps, pad_id=0, eos_ids=[-1])
    with torch.no_grad():
        lp, _, _, _ = score_sequences(m, out.prompt_ids, out.prompt_start, out.tokens, out.lengths, 1 / 0.7)
    print(f"max |logprob - score| = {(lp - out.logprobs).abs().max().item():.5f}")
    torch.testing.assert_close(lp, out.logprobs, rtol=0.0, atol=1e-2)


def test_k5_lookup_end_to_end_tiny():
    """K = 5 (G = 6: not a power of two) on the kept tiny-llama pair: greedy == plain, graph == eager."""
    m = _kept_model("tiny-llama", 2, 48)
    want = _plain(m, PROMPTS, 48, 4)
    sp = SamplingParams(max_new_tokens=48, do_sample=False, lookup_tokens=5)
    a = Generator(m, 4, 128, DEV, use_graph=True).generate(PROMPTS, sp, pad_id=0, eos_ids=[-1])
    b = Generator(m, 4, 128, DEV, use_graph=False).generate(PROMPTS, sp, pad_id=0, eos_ids=[-1])
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.logprobs, b.logprobs)
    assert torch.equal(a.tokens, want.tokens) and a.timings["lookup_accepted"] > 0


def test_sampled_lookup_logprobs_match_teacher_forcing():
    """The method and tolerance of test_models_gpu.test_decode_matches_teacher_forcing (tiny-mistral
    seed 4, its two prompts, 10 new tokens, T 0.7, top_k 0, sampler seed 5, atol 1e-2), with lookup
    decoding on. Measured max |logprob - score|: 0.0055 (K = 3), 0.0066 (K = 7); plain decoding
    0.0081. The bound belongs to that size: at 40 new tokens plain decoding itself reaches 0.0104."""
    from rag_tl_domainllm_optimizer_amd.train.common import score_sequences

    m = models.CausalLM(PRESETS["tiny-mistral"], device=DEV, dtype=torch.bfloat16, seed=4)
    prompts = [[5, 9, 33, 41, 7, 8, 9, 10], [12, 300, 4]]
    for K in (3, 7):
        sp = SamplingParams(max_new_tokens=10, temperature=0.7, top_k=0, seed=5, lookup_tokens=K)
        out = Generator(m, 2, 64, DEV).generate(prompts, sp, pad_id=0, eos_ids=[-1])
        again = Generator(m, 2, 64, DEV).generate(prompts, sp, pad_id=0, eos_ids=[-1])
        assert torch.equal(out.tokens, again.tokens) and torch.equal(out.logprobs, again.logprobs)
        assert out.lengths.tolist() == [10, 10]
        with torch.no_grad():
            lp, _, _, _ = score_sequences(m, out.prompt_ids, out.prompt_start, out.tokens, out.lengths, 1 / 0.7)
        print(f"K={K}: max |logprob - score| = {(lp - out.logprobs).abs().max().item():.5f}")
        torch.testing.assert_close(lp, out.logprobs, rtol=0.0, atol=1e-2)


def test_eos_and_early_stop_modes():
    m = models.CausalLM(PRESETS["tiny-llama"], device=DEV, dtype=torch.bfloat16, seed=2)
    plain = Generator(m, 4, 128, DEV).generate(PROMPTS, SamplingParams(max_new_tokens=48, do_sample=False), pad_id=0,
                                               eos_ids=[116])
    sp = SamplingParams(max_new_tokens=48, do_sample=False, lookup_tokens=7)
    n0 = int(plain.lengths[0])
    assert n0 < 48 and int(plain.tokens[0, n0 - 1]) == 116  # row 0: EOS inside a run of repeats
    first = None
    for mode in (True, False, "async"):
        g = Generator(m, 4, 128, DEV, sync_every=4)
        o = g.generate_async(PROMPTS, sp, pad_id=0, eos_ids=[116], early_stop=mode).result()
        # row 0 (EOS arrives inside an accepted run; pad after it) is plain decoding's, token for token
        assert torch.equal(o.tokens[0], plain.tokens[0]) and int(o.lengths[0]) == n0, mode
        assert torch.equal(o.tokens, plain.tokens) and torch.equal(o.lengths, plain.lengths), mode
        # the three early-exit modes are the same computation
        first = first or o
        assert torch.equal(o.tokens, first.tokens) and torch.equal(o.logprobs, first.logprobs), mode
        assert torch.equal(o.lengths, first.lengths)


def test_rows_times_positions_above_fused_limit_raises():
    m = models.CausalLM(PRESETS["tiny-llama"], device=DEV, dtype=torch.bfloat16, seed=2)
    m.fused_decode_max_batch = 16
    with pytest.raises(ValueError):
        Generator(m, 4, 64, DEV).generate(PROMPTS, SamplingParams(max_new_tokens=4, do_sample=False, lookup_tokens=7),
                                          pad_id=0, eos_ids=[-1])
