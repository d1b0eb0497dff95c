"""Per-request sampling in the graph-replayed continuous decode batch (tiny Llama preset)."""
import pytest
import torch

from rag_tl_domainllm_optimizer_amd import models
from rag_tl_domainllm_optimizer_amd.generation import (ContinuousBatcher, Generator, RequestSampling, SamplingParams,
                                                       derive_seed)
from rag_tl_domainllm_optimizer_amd.models.config import PRESETS
from rag_tl_domainllm_optimizer_amd.train.common import score_sequences

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
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


def _check_logprobs(model, prompt, f, temperature):
    """teacher-forced rescoring of prompt + tokens at the row's own temperature"""
    n = len(f.tokens)
    with torch.no_grad():
        lp, _, _, _ = score_sequences(model, torch.tensor([prompt], device=DEV),
                                      torch.zeros(1, dtype=torch.long, device=DEV),
                                      torch.tensor([f.tokens], device=DEV), torch.tensor([n], device=DEV),
                                      1.0 / temperature)
    torch.testing.assert_close(lp[0, :n].cpu(), torch.tensor(f.logprobs), rtol=0.0, atol=1e-2)


def test_mixed_batch_one_graph_per_bucket(model):
    sp = SamplingParams(max_new_tokens=T, temperature=0.7, top_k=0, seed=5)
    greedy = Generator(model, 4, 64, DEV).generate(PROMPTS, SamplingParams(max_new_tokens=T, do_sample=False),
                                                   pad_id=0, eos_ids=[-1]).tokens.tolist()
    gen = Generator(model, 4, 64, DEV)
    cb = ContinuousBatcher(gen, sp, pad_id=0, eos_ids=[-1], per_request=True)
    settings = [RequestSampling(temperature=0.7, max_new_tokens=3, seed=21),
                RequestSampling(temperature=1.3, top_p=0.9, max_new_tokens=5),
                RequestSampling(do_sample=False),
                RequestSampling(top_k=1, temperature=0.9)]
    temps = [0.7, 1.3, 1.0, 0.9]
    cb.admit_many(PROMPTS, [0, 1, 2, 3], settings)
    got = _drain(cb, {})
    assert [len(got[i].tokens) for i in range(4)] == [3, 5, T, T]  # each row stops at its own length
    # graph-replayed rows against the greedy generation of the same prompt (graph-vs-eager decode is
    # compared by token equality)
    assert got[2].tokens == greedy[2] and got[3].tokens == greedy[3]
    for i in range(4):
        _check_logprobs(model, PROMPTS[i], got[i], temps[i])
    assert got[0].seed == 21 and got[1].seed == derive_seed(5, 1)
    # a second wave with other settings into the freed rows: two rows (bucket 2), then one (bucket 1)
    wave2 = [RequestSampling(temperature=0.5, top_k=7, seed=3), RequestSampling(temperature=1.1, top_p=0.8, seed=4,
                                                                              max_new_tokens=6)]
    cb.admit_many(PROMPTS[:2], ["a", "b"], wave2)
    _drain(cb, got)
    cb.admit(PROMPTS[0], "c", RequestSampling(temperature=0.7, max_new_tokens=3, seed=21))
    _drain(cb, got)
    assert len(got["a"].tokens) == T and len(got["b"].tokens) == 6
    _check_logprobs(model, PROMPTS[0], got["a"], 0.5)
    _check_logprobs(model, PROMPTS[1], got["b"], 1.1)
    # the same seed and prompt, another time and other batch mates: the same draw
    assert got["c"].tokens == got[0].tokens
    # buckets used: 1 (captured at construction), 4, 2 — the count does not grow with the settings
    keys = list(gen.runner.graphs)
    assert len(keys) == 3 and all("rows" in k for k in keys), keys
    assert sorted(k[-1] for k in keys) == [1, 2, 4]
    cb.close()


def test_default_path_keeps_scalar_graph_keys(model):
    sp = SamplingParams(max_new_tokens=T, temperature=0.7, top_k=0, seed=5)
    gen = Generator(model, 4, 64, DEV)
    cb = ContinuousBatcher(gen, sp, pad_id=0, eos_ids=[-1])
    cb.admit_many(PROMPTS[:2], [0, 1])
    got = _drain(cb, {})
    assert all("rows" not in k for k in gen.runner.graphs)
    assert (T, sp.inv_temp, 0, 1.0, False, 5, (-1,), 0, 2) in gen.runner.graphs
    assert got[0].seed is None and len(got[0].tokens) == T
    with pytest.raises(ValueError):
        cb.admit(PROMPTS[0], "x", RequestSampling(seed=1))
    cb.close()
