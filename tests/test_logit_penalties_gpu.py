"""Per-request logit penalties on the GPU: ``logit_rows_penalty_kernel`` against its eager twin, row
independence, and ``ContinuousBatcher(per_request=True, penalties=True)`` end to end on the tiny
Llama preset (graph-replayed)."""
import pytest
import torch

from rag_tl_domainllm_optimizer_amd import models, ops
from rag_tl_domainllm_optimizer_amd.generation import ContinuousBatcher, Generator, RequestSampling, SamplingParams
from rag_tl_domainllm_optimizer_amd.models.config import PRESETS

from test_logit_penalties_cpu import call, pack, ulp_steps

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MAX_SEQ = 128
LENGTHS = [1, 2, 63, 64, 65, MAX_SEQ]  # the staging loop's and the waves' edges


def row_config(i, V):
    """config i of the cycle: history length LENGTHS[i % 6] (left-padded where it fits), tokens from
    a small pool (duplicates, 0 and V - 1), a random prompt / generated split, and one of six
    settings (rho | pi + phi | 16 biases | 1 bias + rho | neutral | inactive)"""
    g = torch.Generator().manual_seed(1000 + i)
    L = LENGTHS[i % 6]
    ks = 0 if L == MAX_SEQ or i % 3 != 1 else min(5, MAX_SEQ - L)
    pool = torch.cat([torch.tensor([0, V - 1]), torch.randint(0, V, (L // 2 + 1,), generator=g)])
    seq = pool[torch.randint(0, pool.numel(), (L,), generator=g)].tolist()
    n_gen = int(torch.randint(0, L + 1, (1,), generator=g))
    prompt, gen = seq[:L - n_gen], seq[L - n_gen:]
    kind = (i // 6 + i) % 6
    rho, pi, phi, bias, act = 1.0, 0.0, 0.0, [], 1
    if kind == 0:
        rho = 1.3
    elif kind == 1:
        pi, phi = 0.75, 1.5
    elif kind == 2:
        toks = list(dict.fromkeys(seq[:8] + [0, V - 1] + torch.randperm(V, generator=g)[:32].tolist()))[:16]
        bias = [(t, float(torch.randn((), generator=g)) * 10) for t in toks]  # in the history and outside it
        rho, phi = 0.9, -0.5
    elif kind == 3:
        rho, bias = 1.7, [(seq[0], -100.0)]
    elif kind == 5:
        rho, pi, bias, act = 1.5, 1.0, [(seq[-1], 50.0)], 0
    return (ks, prompt, gen, rho, pi, phi, bias, act)


def touched_mask(rows, V):
    m = torch.zeros(len(rows), V, dtype=torch.bool)
    for b, (ks, prompt, gen, r, p, f, bias, act) in enumerate(rows):
        if act and not (r == 1.0 and p == 0.0 and f == 0.0 and not bias):
            m[b, torch.tensor(prompt + gen + [t for t, _ in bias])] = True
    return m


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows,V,ld", [(1, 1000, 1000), (3, 1000, 1024), (64, 32000, 32000)])
def test_kernel_against_twin(rows, V, ld, dtype):
    n_cfg = max(rows, 12)
    cfgs = [row_config(i, V) for i in range(n_cfg)]
    g = torch.Generator().manual_seed(V + rows)  # a generator of its own: the global streams stay as they are
    for c0 in range(0, n_cfg, rows):
        batch = cfgs[c0:c0 + rows]
        for append in (True, False):
            a = pack(batch, V, append=append, S=MAX_SEQ)
            full0 = (torch.randn(rows, ld, generator=g) * 4).to(dtype)
            full0[:, V:] = 7.0  # the row padding of a wider leading dimension
            h0 = a["hist"].clone()
            want = call(full0[:, :V].clone(), a, append)  # the twin (CPU tensors)
            want_h = a["hist"]
            d = {k: v.to(DEV) for k, v in pack(batch, V, append=append, S=MAX_SEQ).items()}
            full = full0.to(DEV)
            call(full[:, :V], d, append)
            got = full.cpu()
            steps = ulp_steps(got[:, :V], want)
            print(f"configs {c0}..{c0 + rows - 1} append={append}: max ulp distance {int(steps.max())}")
            assert int(steps.max()) <= 1
            m = touched_mask(batch, V)
            assert torch.equal(got[:, :V][~m], full0[:, :V][~m])  # untouched, neutral, inactive: bitwise
            assert torch.equal(got[:, V:], full0[:, V:])
            # history: the input token at slot kv_len of the served rows, nothing else
            assert torch.equal(d["hist"].cpu(), want_h)
            diff = (want_h != h0).nonzero().tolist()
            assert all(j == int(a["kv_len"][b]) for b, j in diff)
            if append:
                served = [b for b, c in enumerate(batch) if c[7] and len(c[2]) > 0 and bool(m[b].any())]
                assert sorted(b for b, _ in diff) == served


def test_row_independence_and_repeat():
    V = 32000
    cfg = row_config(8, V)  # 63 tokens, 16 biases
    others = [row_config(i, V) for i in range(20, 36)]
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(V, generator=g) * 4).to(torch.bfloat16)

    def launch(batch, r):
        d = {k: v.to(DEV) for k, v in pack(batch, V, S=MAX_SEQ).items()}
        logits = (torch.randn(len(batch), V, generator=g) * 4).to(torch.bfloat16)
        logits[r] = x
        logits = logits.to(DEV)
        call(logits, d)
        return logits[r].cpu()

    alone = launch([cfg], 0)
    mates = others[:9] + [cfg] + others[10:]
    beside = launch(mates, 9)
    assert not torch.equal(alone, x)
    assert torch.equal(alone, beside)
    assert torch.equal(launch(mates, 9), beside)


def test_binding_rejects_bad_arguments():
    V = 100
    a = {k: v.to(DEV) for k, v in pack([row_config(0, V)], V, S=MAX_SEQ).items()}
    x = torch.zeros(1, V, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        call(x.half(), a)
    with pytest.raises(RuntimeError):
        call(x, dict(a, rho=a["rho"].double()))
    with pytest.raises(RuntimeError):
        call(x, dict(a, bias_tok=a["bias_tok"][:, :8].contiguous()))
    with pytest.raises(RuntimeError):
        call(x, dict(a, hist=torch.zeros(1, ops.LOGIT_ROWS_MAX_SEQ + 1, dtype=torch.long, device=DEV)))
    assert ops.native().logit_rows_max_seq() == ops.LOGIT_ROWS_MAX_SEQ


# ---------------------------------------------------------------------------------------- end to end
T = 8
PROMPTS = [[5, 9, 33, 41, 7, 8], [12, 300, 4], [77] * 11, [20, 21, 22, 23, 24, 25, 26, 27]]


@pytest.fixture(scope="module")
def model():
    return models.CausalLM(PRESETS["tiny-llama"], device=DEV, dtype=torch.bfloat16, seed=2)


def _drain(cb, got):
    while cb.active_rows():
        cb.step(2)
        for f in cb.collect():
            got[f.tag] = f
    return got


def _serve(model, sp, settings, penalties=True):
    gen = Generator(model, 4, 64, DEV)
    cb = ContinuousBatcher(gen, sp, pad_id=0, eos_ids=[-1], per_request=True, penalties=penalties)
    cb.admit_many(PROMPTS, [0, 1, 2, 3], settings)
    got = _drain(cb, {})
    cb.close()
    return got, gen


def test_forced_banned_and_neutral_rows(model):
    sp = SamplingParams(max_new_tokens=T, temperature=0.8, top_k=0, seed=5)
    base = [RequestSampling(seed=21), RequestSampling(seed=22, temperature=1.2), RequestSampling(do_sample=False),
            RequestSampling(seed=24, top_p=0.9)]
    plain, gen0 = _serve(model, sp, base, penalties=False)
    assert all("penalties" not in k for k in gen0.runner.graphs) and gen0.penp is None and gen0.hist is None
    first = plain[2].tokens[0]
    mixed = [RequestSampling(seed=21),
             RequestSampling(seed=22, temperature=1.2, logit_bias={77: 100}),
             RequestSampling(do_sample=False, logit_bias={first: -100}),
             RequestSampling(seed=24, top_p=0.9, repetition_penalty=1.0, frequency_penalty=0.0)]
    got, gen = _serve(model, sp, mixed)
    assert all("penalties" in k for k in gen.runner.graphs)
    for i in (0, 3):  # neutral rows: bit for bit the batcher without the feature
        assert got[i].tokens == plain[i].tokens and got[i].logprobs == plain[i].logprobs
    assert got[1].tokens == [77] * T
    assert first not in got[2].tokens and len(got[2].tokens) == T


def test_penalised_greedy_row_matches_twin_teacher_forced(model):
    """the GPU row's own tokens fed to the CPU twin over teacher-forced logits: the reported
    log-probs are those of the penalised distribution (tolerance: the model-numerics tolerance of
    test_per_request_sampling_gpu's rescoring, 1e-2), and every token is its argmax within it"""
    sp = SamplingParams(max_new_tokens=T, do_sample=False)
    prompt = PROMPTS[0]
    rs = RequestSampling(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.7,
                         logit_bias={41: 0.5, 300: -1.0})
    gen = Generator(model, 4, 64, DEV)
    cb = ContinuousBatcher(gen, sp, pad_id=0, eos_ids=[-1], per_request=True, penalties=True)
    cb.admit_many([PROMPTS[1], prompt], ["mate", "x"], [None, rs])
    f = _drain(cb, {})["x"]
    cb.close()
    n = len(f.tokens)
    assert n == T
    with torch.no_grad():
        ids = torch.tensor([prompt + f.tokens], device=DEV)
        logits = model.logits(model.forward(ids)).cpu()[len(prompt) - 1:len(prompt) - 1 + n]
    V = logits.shape[1]
    rho, pi, phi, pairs = rs.resolve_penalties(sp, V)
    for i in range(n):
        row = (0, prompt, f.tokens[:i], rho, pi, phi, list(pairs), 1)
        a = pack([row], V, append=False, S=64)
        x = call(logits[i:i + 1].clone(), a, append=False)
        lp = torch.log_softmax(x[0].float(), -1)
        assert abs(float(lp[f.tokens[i]]) - f.logprobs[i]) <= 1e-2, i
        assert float(lp.max() - lp[f.tokens[i]]) <= 1e-2, i


def test_three_mixes_replay_one_graph_per_bucket(model):
    sp = SamplingParams(max_new_tokens=T, temperature=0.7, top_k=0, seed=5)
    gen = Generator(model, 4, 64, DEV)
    cb = ContinuousBatcher(gen, sp, pad_id=0, eos_ids=[-1], per_request=True, penalties=True)
    mixes = [[RequestSampling(repetition_penalty=1.2), None, RequestSampling(logit_bias={9: 100}), None],
             [RequestSampling(presence_penalty=1.0, frequency_penalty=1.0), RequestSampling(logit_bias={3: -100}),
              RequestSampling(repetition_penalty=0.8, seed=3), RequestSampling(do_sample=False)],
             [None, RequestSampling(logit_bias={i: float(i) for i in range(16)}), None,
              RequestSampling(frequency_penalty=-1.0)]]
    for k, mix in enumerate(mixes):
        cb.admit_many(PROMPTS, [(k, i) for i in range(4)], mix)
        got = _drain(cb, {})
        assert all(len(got[(k, i)].tokens) == T for i in range(4))
        if k == 0:
            assert got[(0, 2)].tokens == [9] * T
    # buckets used: 1 (captured at construction) and 4 — the count does not grow with the settings
    keys = list(gen.runner.graphs)
    assert len(keys) == 2 and all("rows" in k and "penalties" in k for k in keys), keys
    cb.close()


def test_with_adapters_forced_token_beside_neutral_base_row(tmp_path):
    from test_adapter_rows_gpu import _save_adapter

    cfg = models.resolve_preset("tiny-llama")
    _save_adapter(cfg, 1, tmp_path / "sft", 8)
    m = models.CausalLM(cfg, device=DEV, dtype=torch.bfloat16, seed=0)
    bank = models.AdapterBank(m, slots=4, r_max=8)
    bank.load("sft", str(tmp_path / "sft"))
    sp = SamplingParams(max_new_tokens=6, temperature=0.0)
    prompts, names = [[5, 9, 11, 3, 7], [5, 9, 11, 3, 7]], [None, "sft"]

    def serve(penalties, settings):
        gen = Generator(m, max_batch=4, max_seq=64, device=DEV)
        cb = ContinuousBatcher(gen, sp, eos_ids=[-1], per_request=True, adapters=bank, penalties=penalties)
        cb.admit_many(prompts, [0, 1], settings, names)
        got = _drain(cb, {})
        keys = list(gen.runner.graphs)
        cb.close()
        return got, keys

    plain, _ = serve(False, [None, None])
    got, keys = serve(True, [None, RequestSampling(logit_bias={123: 100})])
    assert all("adapters" in k and "penalties" in k for k in keys)
    assert got[1].tokens == [123] * 6 and got[1].adapter == "sft"
    assert got[0].tokens == plain[0].tokens and got[0].logprobs == plain[0].logprobs and got[0].adapter is None
