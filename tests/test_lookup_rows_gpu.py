"""Prompt-lookup decoding in the continuous batch on the GPU: the grouped per-row sampler against
one-row scalar launches, the extended accept / draft kernels against their CPU twins, and the batcher
end to end (graph == eager bitwise, greedy lookup == the plain continuous run, sampled log-probs ==
teacher forcing, MXFP4 decode).

Rows kept (the rule of test_lookup_decode_gpu): a request is compared only if its plain greedy output
is the same at every row bucket the compared runs put its GEMMs at — 1, the buckets of the staggered
schedule (half the requests, then ``max_batch``) and those times K + 1 for the verify steps
(``_buckets``) — since bf16 kernels at different row counts may break an exact logit tie
differently, which says nothing about lookup decoding. The requests are that file's three prompts
and a fourth cut from the first. Seeds: the pairs of ``GREEDY_CASES``; each case prints the rows it
keeps, needs 3 of 4, and 2 of the 3 cases must qualify or the test fails.

Measured on the MI355X (buckets 2, 4, 8, 16 beside 1): tiny-llama seed 2 drops request 2, tiny-llama
seed 4 drops request 3, tiny-mistral seed 2 drops request 2 — all three cases run with 3 of 4; the
head_dim-128 models (seed 2, buckets 2 and 8) keep both requests with and without the window; under
MXFP4 decode tiny-llama seed 2 drops request 2. Sampled per-request log-probs against teacher
forcing: max |logprob - score| 0.0055, and the tokens were those of the plain per-request run."""
import pytest
import torch

from rag_tl_domainllm_optimizer_amd import models, ops
from rag_tl_domainllm_optimizer_amd.generation import (ContinuousBatcher, Generator, RequestSampling, SamplingParams)
from rag_tl_domainllm_optimizer_amd.models.config import PRESETS

import test_lookup_rows_cpu as rows_cpu
from test_lookup_decode_gpu import GREEDY_CASES, _cfg128, _close
from test_sample_rows_gpu import pick_top_p

pytestmark = pytest.mark.gpu
DEV = "cuda"
REQS = rows_cpu.REQS
FILL = [3, 4, 5]


# ----------------------------------------------------------------------------- grouped sampler
# per request: greedy, top_k, wanted top-p, temperature
MIX = [(True, 0, None, 1.0), (False, 0, None, 0.7), (False, 50, 0.9, 1.3), (False, 2000, None, 0.7)]


def _group_case(dtype, V, G, B=3):
    g = torch.Generator().manual_seed(77 + V + G)
    logits = (torch.randn(B * G, V, generator=g) * 2).to(dtype)
    mix = [MIX[(b + G // 2) % len(MIX)] for b in range(B)]  # G = 2, 4, 6 start the cycle of settings at 1, 2, 3
    p = {"inv_temp": torch.tensor([1.0 if r[0] else 1.0 / r[3] for r in mix], dtype=torch.float32),
         "top_k": torch.tensor([r[1] for r in mix], dtype=torch.int32),
         "greedy": torch.tensor([r[0] for r in mix], dtype=torch.uint8),
         "seed": torch.tensor([31 + b for b in range(B)], dtype=torch.long),
         "counter": torch.tensor([0, 5, 126][:B], dtype=torch.int32)}
    # one top-p per request has to be unambiguous on each of its G rows: the fp32 oracle below runs
    # another kernel. Take the candidate of the row whose half-gap is checked by pick_top_p on every row.
    tp = []
    for b, r in enumerate(mix):
        tp.append(1.0 if r[2] is None else pick_top_p(logits[b * G], 1.0 / r[3], r[1], r[2]))
    p["top_p"] = torch.tensor(tp, dtype=torch.float32)
    active = torch.ones(B * G, dtype=torch.uint8)
    active[B * G - 1] = 0
    return logits.to(DEV), {k: v.to(DEV) for k, v in p.items()}, active.to(DEV), mix


# V 1000: the LDS bodies (search / staged radix); V 1001: the global radix body; one fp32 case
GROUP_CASES = [(G, torch.bfloat16, V) for G in (2, 4, 6) for V in (1000, 1001)] + [(4, torch.float32, 1000)]


@pytest.mark.parametrize("G,dtype,V", GROUP_CASES)
def test_grouped_sample_rows_equals_one_row_scalar_launches(G, dtype, V):
    B = 3
    logits, p, active, mix = _group_case(dtype, V, G)
    tok, lp = ops.sample_rows(logits, p["inv_temp"], p["top_k"], p["top_p"], p["greedy"], p["seed"], p["counter"],
                              active, group=G)
    for b in range(B):
        for j in range(G):
            r = b * G + j
            off = (p["counter"][b:b + 1] + j).long()
            args = (float(p["inv_temp"][b]), int(p["top_k"][b]), float(p["top_p"][b]), bool(p["greedy"][b]),
                    int(p["seed"][b]))
            # the scalar kernels on the same logits: the same row body, so also the same log-prob bits
            t1, l1 = ops.sample(logits[r:r + 1], *args, offset=off, active=active[r:r + 1])
            assert int(tok[r]) == int(t1), (b, j)
            assert torch.equal(lp[r:r + 1], l1), (b, j)
            # the fp32 radix kernel (the oracle of test_sample_rows_gpu): the same token, unless the
            # row's top-p cut is ambiguous at fp32 (only row 0 of a request had its cut placed)
            if j == 0 or mix[b][2] is None:
                t32, _ = ops.sample(logits[r:r + 1].float(), *args, offset=off, active=active[r:r + 1])
                assert int(tok[r]) == int(t32), (b, j)
    # positions of one request draw from different counters
    drawn = [b for b in range(B) if not mix[b][0] and mix[b][1] != 1]
    assert any(len({int(t) for t in tok[b * G:(b + 1) * G]}) > 1 for b in drawn)
    # group = 1 is the call without the argument
    one = {k: v for k, v in p.items()}
    a = ops.sample_rows(logits[:B], one["inv_temp"], one["top_k"], one["top_p"], one["greedy"], one["seed"],
                        one["counter"], active[:B])
    b1 = ops.sample_rows(logits[:B], one["inv_temp"], one["top_k"], one["top_p"], one["greedy"], one["seed"],
                         one["counter"], active[:B], group=1)
    assert torch.equal(a[0], b1[0]) and torch.equal(a[1], b1[1])


def test_grouped_sample_rows_rejects_bad_shapes():
    logits, p, active, _ = _group_case(torch.bfloat16, 1000, 4)
    args = (p["inv_temp"], p["top_k"], p["top_p"], p["greedy"], p["seed"], p["counter"])
    with pytest.raises(RuntimeError):
        ops.sample_rows(logits[:10], *args, group=4)        # 10 rows are no multiple of 4
    with pytest.raises(RuntimeError):
        ops.sample_rows(logits, *args, active[:3], group=4)  # the mask is per logits row
    with pytest.raises(RuntimeError):
        ops.sample_rows(logits, *args, group=9)


# ----------------------------------------------------------------------------- accept / draft kernels
def test_accept_kernel_rows_matches_twin():
    t, rows, exp = rows_cpu.accept_rows_state(DEV)
    rows_cpu.run_accept_rows(t)
    rows_cpu.check_accept_rows(t, rows, exp)
    c, _, _ = rows_cpu.accept_rows_state()
    rows_cpu.run_accept_rows(c)
    for k in t:
        assert torch.equal(t[k].cpu(), c[k]), k


def test_draft_kernel_rows_matches_twin():
    got, want = rows_cpu.run_draft_rows(DEV), rows_cpu.run_draft_rows()
    rows_cpu.check_draft_rows(*got)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------- end to end
def _plain_rows(m, prompts, T, mb, max_seq=128):
    """plain greedy tokens of ``prompts`` decoded in a static batch padded to ``mb`` rows"""
    g, rows = Generator(m, mb, max_seq, DEV), []
    for i in range(0, len(prompts), mb):  # a bucket narrower than the request list: several batches of it
        part = prompts[i:i + mb]
        out = g.generate(part + [FILL] * (mb - len(part)), SamplingParams(max_new_tokens=T, do_sample=False),
                         pad_id=0, eos_ids=[-1])
        rows.append(out.tokens[:len(part)].clone())
    return torch.cat(rows)


def _kept(m, prompts, T, buckets, max_seq=128):
    """indices of the prompts whose plain greedy output is the same at bucket 1 and every bucket given"""
    one = [_plain_rows(m, [p], T, 1, max_seq)[0] for p in prompts]
    wide = [_plain_rows(m, prompts, T, mb, max_seq) for mb in buckets]
    return [i for i in range(len(prompts)) if all(torch.equal(one[i], w[i]) for w in wide)]


def _buckets(n, mb, K):
    """row buckets above 1 that the staggered plain and lookup runs decode at"""
    h = max(1, n // 2)
    return sorted({b for b in (h, mb, h * (K + 1), mb * (K + 1)) if b > 1})


def _staggered(m, prompts, T, K, mb, use_graph, per_request=False, sampling=None, max_seq=128, temp=None):
    """admit the first half, step 3, admit the rest, step to the end -> {index: FinishedRow}"""
    sp = SamplingParams(max_new_tokens=T, do_sample=False) if temp is None else \
        SamplingParams(max_new_tokens=T, temperature=temp, top_k=0, seed=5)
    g = Generator(m, mb, max_seq, DEV, use_graph=use_graph)
    cb = ContinuousBatcher(g, sp, 0, [-1], per_request=per_request, lookup_tokens=K)
    h = len(prompts) // 2
    got = {}
    s = sampling or [None] * len(prompts)
    cb.admit_many(prompts[:h], list(range(h)), s[:h] if per_request else None)
    rows_cpu._drain(cb, got, 3)
    cb.admit_many(prompts[h:], list(range(h, len(prompts))), s[h:] if per_request else None)
    rows_cpu._drain(cb, got)
    cb.close()
    assert int(g.workspace.tickets.abs().sum()) == 0
    return got


def _check_case(m, prompts, T, K, mb, kept, n=None):
    """graph == eager bitwise on every row; lookup greedy == the plain continuous run on the kept rows"""
    plain = _staggered(m, prompts, T, 0, mb, True)
    a = _staggered(m, prompts, T, K, mb, True)
    b = _staggered(m, prompts, T, K, mb, False)
    for i in range(len(prompts)):
        assert a[i].tokens == b[i].tokens and a[i].logprobs == b[i].logprobs, f"graph != eager, request {i}"
        assert a[i].lookup_steps + a[i].lookup_accepted == T - 1
    for i in kept:
        assert a[i].tokens[:n] == plain[i].tokens[:n], f"request {i}"
    assert sum(a[i].lookup_accepted for i in range(len(prompts))) > 0


def test_d64_staggered_graph_eager_and_plain():
    K, mb, ran = 3, 4, 0
    for preset, seed, T in GREEDY_CASES:
        m = models.CausalLM(PRESETS[preset], device=DEV, dtype=torch.bfloat16, seed=seed)
        kept = _kept(m, REQS, T, _buckets(len(REQS), mb, K))
        print(f"{preset} seed {seed}: requests kept {kept} of {len(REQS)}")
        if len(kept) < 3:
            continue
        _check_case(m, REQS, T, K, mb, kept)
        ran += 1
    assert ran >= 2, f"only {ran} of {len(GREEDY_CASES)} cases kept 3 of 4 requests"


@pytest.mark.parametrize("window", [0, 32])
def test_d128_staggered_graph_eager_and_plain(window):
    K, mb, T = 3, 2, 32
    m = models.CausalLM(_cfg128(8, 2, window), device=DEV, dtype=torch.bfloat16, seed=2)
    prompts = [REQS[0], REQS[2]]
    kept = _kept(m, prompts, T, _buckets(len(prompts), mb, K))
    print(f"window {window}: requests kept {kept} of 2")
    assert kept, "no request kept"
    # with a window shorter than the sequence the verify kernel's tiles of later positions start at
    # other keys than a decode step's (test_lookup_decode_gpu.test_d128_lookup_end_to_end): compare the
    # tokens emitted while prompt + answer + K still fits the window
    S = max(len(p) for p in prompts)
    n = None if not window else max(0, min(T, window - S - K))
    assert n is None or n > 0
    _check_case(m, prompts, T, K, mb, kept, n)


def test_sampled_per_request_logprobs_match_teacher_forcing():
    from rag_tl_domainllm_optimizer_amd.train.common import score_sequences

    m = models.CausalLM(PRESETS["tiny-mistral"], device=DEV, dtype=torch.bfloat16, seed=4)
    prompts = [[5, 9, 33, 41, 7, 8, 9, 10], [12, 300, 4]]
    T = 10
    sampling = [RequestSampling(seed=5 + i, temperature=0.7, top_k=0) for i in range(2)]
    got = _staggered(m, prompts, T, 3, 2, True, True, sampling, max_seq=64, temp=0.7)
    again = _staggered(m, prompts, T, 3, 2, True, True, sampling, max_seq=64, temp=0.7)
    plain = _staggered(m, prompts, T, 0, 2, True, True, sampling, max_seq=64, temp=0.7)
    S = max(len(p) for p in prompts)
    ids = torch.zeros(2, S, dtype=torch.long)
    start = torch.zeros(2, dtype=torch.long)
    for b, p in enumerate(prompts):
        ids[b, S - len(p):] = torch.tensor(p)
        start[b] = S - len(p)
    toks = torch.tensor([got[i].tokens for i in range(2)])
    assert toks.shape == (2, T)
    for i in range(2):
        assert got[i].tokens == again[i].tokens and got[i].logprobs == again[i].logprobs
    print("same tokens as the plain per-request run:", [got[i].tokens == plain[i].tokens for i in range(2)])
    with torch.no_grad():
        lp, _, _, _ = score_sequences(m, ids.to(DEV), start.to(DEV), toks.to(DEV), torch.full((2,), T, device=DEV),
                                      1 / 0.7)
    mine = torch.tensor([got[i].logprobs for i in range(2)])
    print(f"max |logprob - score| = {(lp.cpu().float() - mine).abs().max().item():.5f}")
    _close(mine, lp.cpu())


def test_fp4_greedy_lookup_equals_plain_continuous():
    K, mb, T = 3, 4, 32  # 16 rows: the MXFP4 decode kernels' limit
    m = models.CausalLM(PRESETS["tiny-llama"], device=torch.device(DEV), dtype=torch.bfloat16, seed=2)
    m.set_fp4_decode(True)
    kept = _kept(m, REQS, T, _buckets(len(REQS), mb, K), max_seq=96)
    print(f"fp4: requests kept {kept} of {len(REQS)}")
    assert len(kept) >= 3
    plain = _staggered(m, REQS, T, 0, mb, True, max_seq=96)
    look = _staggered(m, REQS, T, K, mb, True, max_seq=96)
    for i in kept:
        assert look[i].tokens == plain[i].tokens, i
    assert sum(look[i].lookup_accepted for i in range(4)) > 0
    with pytest.raises(ValueError, match="16 rows"):
        ContinuousBatcher(Generator(m, 8, 96, DEV), SamplingParams(max_new_tokens=4, do_sample=False), 0, [-1],
                          lookup_tokens=3)
