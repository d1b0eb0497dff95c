"""MXFP4 weight-only decode on the CPU: the eager quantiser (the oracle of the GPU kernel) against
the format's definition, ``gemm_decode(..., fp4=...)`` against the dequantised product, the
generator with ``set_fp4_decode`` and the combinations that must raise."""
import pytest
import torch

from rag_tl_domainllm_optimizer_amd import models, ops
from rag_tl_domainllm_optimizer_amd.generation import ContinuousBatcher, Generator, SamplingParams
from rag_tl_domainllm_optimizer_amd.models.config import PRESETS

GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _weight(N, K, lo=-2, hi=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) * torch.logspace(lo, hi, N)[:, None]).to(torch.bfloat16)


def _block(vals):
    """one row of one MX block: ``vals`` then zeros"""
    return torch.tensor(list(vals) + [0.0] * (32 - len(vals)), dtype=torch.float32).to(torch.bfloat16)[None]


def _nibbles(codes):
    return torch.stack((codes & 0xF, codes >> 4), -1).reshape(codes.shape[0], -1)


@pytest.mark.parametrize("N,K", [(64, 256), (64, 4096)])
def test_oracle_self_checks(N, K):
    w = _weight(N, K)
    w[3, 32:64] = 0  # an all-zero block, with negative zeros in it
    w[3, 40:48] = -0.0
    q, s = ops.quantize_mxfp4(w)
    assert q.shape == (N, K // 2) and s.shape == (N, K // 32) and q.dtype == s.dtype == torch.uint8
    d = ops.dequantize_mxfp4(q, s)
    assert d.dtype == torch.float32 and d.shape == (N, K)
    assert torch.equal(d.to(torch.bfloat16).float(), d), "a dequantised value is not a bf16 number"
    q2, s2 = ops.quantize_mxfp4(d.to(torch.bfloat16))
    assert torch.equal(q, q2) and torch.equal(s, s2), "requantising the dequantised weight changed it"
    assert int(s[3, 1]) == 127
    nib = _nibbles(q)[3, 32:64]
    assert set(nib.tolist()) <= {0, 8} and nib[8:16].tolist() == [8] * 8 and nib[:8].tolist() == [0] * 8
    # round-to-nearest MXFP4 on Gaussian weights: ~11 % relative rms error (the documented caveat)
    rel = ((d - w.float()).pow(2).sum() / w.float().pow(2).sum()).sqrt().item()
    assert 0.08 < rel < 0.14, rel


@pytest.mark.parametrize("k", [-20, -3, 0, 5, 30])
def test_hand_cases(k):
    two_k = 2.0 ** k
    # amax exactly 2^k: e = k - 2, the maximum is code 6's neighbour 4 (4 * 2^(k-2) = 2^k)
    q, s = ops.quantize_mxfp4(_block([two_k, -two_k / 2, two_k / 8]))
    assert int(s[0, 0]) == k - 2 + 127
    assert _nibbles(q)[0, :3].tolist() == [6, 8 | 4, 1]
    # amax = 7.5 * 2^k: e = k, 7.5 saturates to 6
    q, s = ops.quantize_mxfp4(_block([7.5 * two_k, -7.5 * two_k, 6 * two_k]))
    assert int(s[0, 0]) == k + 127
    assert _nibbles(q)[0, :3].tolist() == [7, 15, 7]
    assert ops.dequantize_mxfp4(q, s)[0, :3].tolist() == [6 * two_k, -6 * two_k, 6 * two_k]
    # ties round to the even code; the block's amax 6 * 2^k fixes e = k
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    q, s = ops.quantize_mxfp4(_block([6 * two_k] + [t * two_k for t in ties] + [-t * two_k for t in ties]))
    assert int(s[0, 0]) == k + 127
    want = [0, 2, 2, 4, 4, 6, 6]
    assert _nibbles(q)[0, :15].tolist() == [7] + want + [8 | c for c in want]
    d = ops.dequantize_mxfp4(q, s)[0, 1:8]
    assert d.tolist() == [GRID[c] * two_k for c in want]


def test_sign_of_zero_is_kept_and_oracle_is_idempotent():
    w = _block([4.0, -0.1, 0.1, -0.0, 0.0])  # 0.1 / 2^0 rounds to 0: the sign bit stays
    q, s = ops.quantize_mxfp4(w)
    assert _nibbles(q)[0, :5].tolist() == [6, 8, 0, 8, 0]
    d = ops.dequantize_mxfp4(q, s).to(torch.bfloat16)
    assert torch.equal(torch.signbit(d[0, :5]), torch.tensor([False, True, False, True, False]))
    q2, s2 = ops.quantize_mxfp4(d)
    assert torch.equal(q, q2) and torch.equal(s, s2)


def test_supported_and_bad_inputs():
    z = torch.zeros
    assert ops.fp4_supported(z(16, 256)) and ops.fp4_supported(z(64, 512), act=ops.ACT_SWIGLU)
    assert not ops.fp4_supported(z(8, 256)) and not ops.fp4_supported(z(16, 128))
    assert not ops.fp4_supported(z(32, 256), act=ops.ACT_SWIGLU) and not ops.fp4_supported(z(2, 16, 256))
    with pytest.raises(ValueError):
        ops.quantize_mxfp4(z(4, 48, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.quantize_mxfp4(z(4, 64))  # fp32
    with pytest.raises(ValueError):
        ops.dequantize_mxfp4(z(4, 16, dtype=torch.uint8), z(4, 2, dtype=torch.uint8))


@pytest.mark.parametrize("mode", ["plain", "norm_residual", "swiglu"])
@pytest.mark.parametrize("M", [1, 3, 16])
def test_gemm_decode_cpu_is_the_dequantised_product(M, mode):
    N, K = 128, 256
    g = torch.Generator().manual_seed(M)
    w = _weight(N, K, -1, 1, seed=7)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    d = ops.dequantize_mxfp4(*ops.quantize_mxfp4(w))
    y = x.float() @ d.t()
    cache = ops.Fp4Cache()
    if mode == "plain":
        got = ops.gemm_decode(x, w, fp4=cache)
    elif mode == "norm_residual":
        r = torch.randn(M, N, generator=g).to(torch.bfloat16)
        got = ops.gemm_decode(x, w, residual=r, norm_eps=1e-5, fp4=cache)
        y = y * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5) + r.float()
    else:
        got = ops.gemm_decode(x, w, act=ops.ACT_SWIGLU, norm_eps=1e-5, fp4=cache)
        y = y * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)
        y = torch.nn.functional.silu(y[:, :N // 2]) * y[:, N // 2:]
    assert torch.equal(got, y.to(torch.bfloat16))
    # the image follows an in-place change of the weight, at the same address
    ptr = cache["q"].data_ptr()
    w.mul_(0.5)
    q2, s2 = cache.get(w)
    assert q2.data_ptr() == ptr and torch.equal(s2, ops.quantize_mxfp4(w)[1])


def test_gemm_decode_cpu_other_cases_keep_the_bf16_weight():
    g = torch.Generator().manual_seed(0)
    w = _weight(128, 256, -1, 1)
    x17 = torch.randn(17, 256, generator=g).to(torch.bfloat16)
    assert torch.equal(ops.gemm_decode(x17, w, fp4=ops.Fp4Cache()), ops.gemm_decode(x17, w))
    w2 = _weight(24, 128, -1, 1)  # neither N % 16 nor K % 256
    x = torch.randn(2, 128, generator=g).to(torch.bfloat16)
    assert torch.equal(ops.gemm_decode(x, w2, fp4=ops.Fp4Cache()), ops.gemm_decode(x, w2))


def test_tiny_llama_generates_on_cpu_with_fp4_decode():
    m = models.CausalLM(PRESETS["tiny-llama"], dtype=torch.bfloat16, seed=0)
    g = Generator(m, 2, 64, device="cpu")
    prompts = [[5, 6, 7, 8, 9], [3, 4, 5]]
    sp = SamplingParams(max_new_tokens=6, do_sample=False)
    base = g.generate(prompts, sp, pad_id=0, eos_ids=[-1])
    assert m.set_fp4_decode(True) is False
    out = g.generate(prompts, sp, pad_id=0, eos_ids=[-1])
    assert out.tokens.shape == (2, 6) and torch.isfinite(out.logprobs).all()
    assert int(out.tokens.min()) >= 0 and int(out.tokens.max()) < m.cfg.vocab_size
    assert sorted(m.layers[0]._fp4) == ["down", "gate_up", "o", "qkv"]  # all four projections ran on images
    assert not torch.equal(out.logprobs, base.logprobs)  # the quantised weights were really used
    assert m.set_fp4_decode(False) is True
    again = g.generate(prompts, sp, pad_id=0, eos_ids=[-1])
    assert torch.equal(again.tokens, base.tokens) and torch.equal(again.logprobs, base.logprobs)


def test_invalid_combinations_raise():
    m = models.CausalLM(PRESETS["tiny-llama"], dtype=torch.bfloat16, seed=0)
    m.set_fp8(True)
    with pytest.raises(ValueError, match="fp8"):
        m.set_fp4_decode(True)
    m.set_fp8(False)
    m.set_fp4_decode(True)
    with pytest.raises(ValueError, match="set_fp4_decode"):
        m.set_fp8(True)
    opt = models.CausalLM(PRESETS["tiny-opt"], dtype=torch.bfloat16, seed=0)
    with pytest.raises(ValueError, match="opt"):
        opt.set_fp4_decode(True)
    # lookup: 4 rows x (K + 1 = 5) positions > 16 rows
    g = Generator(m, 4, 64, device="cpu")
    with pytest.raises(ValueError, match="16 rows"):
        g.generate([[5, 6, 5, 6, 5]] * 4, SamplingParams(max_new_tokens=4, do_sample=False, lookup_tokens=4), pad_id=0,
                   eos_ids=[-1])
    # ... and 2 rows x 4 positions is served
    o = g.generate([[5, 6, 5, 6, 5]] * 2, SamplingParams(max_new_tokens=4, do_sample=False, lookup_tokens=3), pad_id=0,
                   eos_ids=[-1])
    assert o.tokens.shape == (2, 4)
    from types import SimpleNamespace

    from rag_tl_domainllm_optimizer_amd.serve.continuous import ContinuousEngine
    pipe = SimpleNamespace(sampling=SimpleNamespace(lookup_tokens=0), gen=SimpleNamespace(model=m), max_batch=32)
    with pytest.raises(ValueError, match="max_batch 32"):
        ContinuousEngine(pipe)
    with pytest.raises(ValueError, match="max_batch 32"):
        ContinuousBatcher(Generator(m, 32, 32, device="cpu"), SamplingParams(max_new_tokens=4, do_sample=False))
