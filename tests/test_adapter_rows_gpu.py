"""Per-row LoRA adapters of the decode batch on the GPU: the shrink + 16-row kernel with the adapter
tail against an fp64 oracle of the same bf16 operands, bitwise base rows, bitwise independence of
batch mates, and the continuous batcher end to end (docs/DESIGN.md "Per-request adapters")."""
import pytest
import torch

from rag_tl_domainllm_optimizer_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (name, N, K, first columns of segments 1.., act, norm, residual)
SHAPES = {
    "qkv": (512, 256, (256, 384), 0, False, False),
    "swiglu_norm": (1024, 256, (), ops.ACT_SWIGLU, True, False),
    "res": (256, 512, (), 0, False, True),
}
IDS = {1: [2], 3: [1, -1, 1], 16: [-1, 0, 2, 0, 1, -1, 2, 2, 1, 0, -1, 1, 0, 2, -1, 1]}
SLOTS = 3
EPS = 1e-5

# Error of the EXISTING base-only call (no adapter arguments: the parent's behaviour) against the
# fp64 oracle at the shapes above, max over shapes and M in {1, 3, 16}, measured once on an MI355X
# as max |got - ref| / max |ref| (test_base_only_error_is_the_recorded_one re-measures it). The
# adapter call may be 2x that: its tail adds R more fp32 terms to a sum that is rounded to bf16 once
# (the bf16 output rounding, 2^-9 relative, is what both figures are made of).
BASE_ERR = {"bf16": 2.529e-3, "fp8": 2.575e-3, "fp4": 2.669e-3}


def _case(shape, M, R, seed=0):
    N, K, segs, act, norm, res = SHAPES[shape]
    g = torch.Generator().manual_seed(1000 * seed + N + K + 7 * M + R)
    nseg = 2 if act == ops.ACT_SWIGLU else len(segs) + 1
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    a = (torch.randn(SLOTS, nseg * R, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    b = (torch.randn(SLOTS, N, R, generator=g) * (0.6 / R ** 0.5)).to(torch.bfloat16)
    r = torch.randn(M, N, generator=g).to(torch.bfloat16) if res else None
    ids = torch.tensor(IDS[M], dtype=torch.int32)
    return dict(N=N, K=K, segs=segs, act=act, eps=EPS if norm else 0.0, nseg=nseg, R=R, x=x, w=w, a=a, b=b, r=r, ids=ids)


def _caches(fmt):
    return {"bf16": {"shuf": ops.ShufCache()}, "fp8": {"fp8": ops.Fp8Cache()}, "fp4": {"fp4": ops.Fp4Cache()}}[fmt]


def _weights64(fmt, w_dev):
    """The weights the kernel multiplies by, as fp64 (every image value is exact in fp64)."""
    if fmt == "fp8":
        q, s = ops.quantize_fp8(w_dev)
        return ops.dequantize_fp8(q, s).double().cpu()
    if fmt == "fp4":
        return ops.dequantize_mxfp4(*ops.quantize_mxfp4(w_dev)).double().cpu()
    return w_dev.double().cpu()


def _oracle(c, w64, with_adapters=True):
    """fp64 y of the formula: epilogue(rs (x W'^T + T B^T)) from the bf16 operands; also the rms
    ratio adapter term / base product over the adapted rows."""
    x = c["x"].double()
    N, R = c["N"], c["R"]
    y = x @ w64.t()
    base = y.clone()
    pair = c["act"] == ops.ACT_SWIGLU
    bounds = [N // 2] if pair else list(c["segs"])
    seg = sum((torch.arange(N) >= b0).long() for b0 in bounds) if bounds else torch.zeros(N, dtype=torch.long)
    ratio = None
    if with_adapters:
        rows = [i for i, s in enumerate(c["ids"].tolist()) if s >= 0]
        for i in rows:
            s = int(c["ids"][i])
            t = c["a"][s].double() @ x[i]  # [nseg R]
            idx = seg[:, None] * R + torch.arange(R)[None, :]
            y[i] += (t[idx] * c["b"][s].double()).sum(-1)
        ratio = float((y - base)[rows].pow(2).mean().sqrt() / base[rows].pow(2).mean().sqrt())
    if c["eps"] > 0:
        y = y * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + c["eps"])
    if pair:
        y = torch.nn.functional.silu(y[:, :N // 2]) * y[:, N // 2:]
    if c["r"] is not None:
        y = y + c["r"].double()
    return y, ratio


def _run(c, fmt, adapters=True, ks=0, caches=None, w_dev=None):
    x, w = c["x"].to(DEV), (c["w"].to(DEV) if w_dev is None else w_dev)
    r = c["r"].to(DEV) if c["r"] is not None else None
    kw = dict(act=c["act"], residual=r, norm_eps=c["eps"], **(caches or _caches(fmt)))
    if not adapters:
        return ops.gemm_decode(x, w, **kw)
    ids = c["ids"].to(DEV)
    t = ops.lora_rows_shrink(x, c["a"].to(DEV), ids, ks=ks)
    return ops.gemm_decode(x, w, rows_lora=(t, c["b"].to(DEV), ids, c["segs"]), **kw)


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def base_only_error(fmt, shape, M):
    c = _case(shape, M, 16)
    w_dev = c["w"].to(DEV)
    ref, _ = _oracle(c, _weights64(fmt, w_dev), with_adapters=False)
    return _err(_run(c, fmt, adapters=False, w_dev=w_dev), ref)


@pytest.mark.parametrize("fmt", ["bf16", "fp8", "fp4"])
def test_base_only_error_is_the_recorded_one(fmt):
    worst = max(base_only_error(fmt, shape, M) for shape in SHAPES for M in (1, 3, 16))
    print(f"base-only error {fmt}: {worst:.3e} (recorded {BASE_ERR[fmt]:.3e})")
    assert worst <= BASE_ERR[fmt] * 1.0001


@pytest.mark.parametrize("R", [8, 16])
@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("fmt", ["bf16", "fp8", "fp4"])
def test_kernel_matches_fp64_oracle(fmt, shape, M, R):
    c = _case(shape, M, R)
    w_dev = c["w"].to(DEV)
    ref, ratio = _oracle(c, _weights64(fmt, w_dev))
    assert ratio >= 0.25, ratio  # a dropped or mis-selected adapter cannot pass
    got = _run(c, fmt, w_dev=w_dev)
    e = _err(got, ref)
    print(f"adapter rows {fmt} {shape} M={M} R={R}: err {e:.3e} bound {2 * BASE_ERR[fmt]:.3e} term/base {ratio:.2f}")
    assert e <= 2 * BASE_ERR[fmt]
    # a wrong slot on any adapted row is far outside the bound
    wrong = dict(c, ids=torch.where(c["ids"] >= 0, (c["ids"] + 1) % SLOTS, c["ids"]))
    assert _err(got, _oracle(wrong, _weights64(fmt, w_dev))[0]) > 20 * BASE_ERR[fmt]


@pytest.mark.parametrize("fmt", ["bf16", "fp4"])
def test_shrink_k_slices_sum_in_order(fmt):
    """K = 512 forced into 2 and 8 slices (4 and 1 chunks each: idle waves): same bound; a repeat is bitwise."""
    c = _case("res", 16, 16)
    w_dev = c["w"].to(DEV)
    ref, _ = _oracle(c, _weights64(fmt, w_dev))
    for ks in (2, 8):
        got = _run(c, fmt, ks=ks, w_dev=w_dev)
        assert _err(got, ref) <= 2 * BASE_ERR[fmt]
        assert torch.equal(got, _run(c, fmt, ks=ks, w_dev=w_dev))


# bf16: the existing call takes the 16-row kernel from N / 16 >= 256 row groups and K >= 1024 on
# (below that the split-K kernel, another summation order), so the bf16 bitwise cases use the
# smallest such shapes; fp8 and MXFP4 take the 16-row kernel at every shape.
BITWISE = [("fp8", s) for s in SHAPES] + [("fp4", s) for s in SHAPES] + [("bf16", "big_norm_res"), ("bf16", "big_swiglu")]
SHAPES_BIG = {"big_norm_res": (4096, 1024, (2048, 3072), 0, True, True),
              "big_swiglu": (8192, 1024, (), ops.ACT_SWIGLU, True, False)}


@pytest.mark.parametrize("fmt,shape", BITWISE)
def test_base_rows_bitwise_equal_existing_call(fmt, shape):
    SHAPES.update(SHAPES_BIG)
    try:
        c = _case(shape, 16, 16)
    finally:
        for k in SHAPES_BIG:
            SHAPES.pop(k)
    caches, w_dev = _caches(fmt), c["w"].to(DEV)
    plain = _run(c, fmt, adapters=False, caches=caches, w_dev=w_dev)
    got = _run(c, fmt, caches=caches, w_dev=w_dev)
    base = [i for i, s in enumerate(c["ids"].tolist()) if s < 0]
    assert len(base) == 4
    assert torch.equal(got[base], plain[base])
    adapted = [i for i in range(16) if i not in base]
    assert not torch.equal(got[adapted], plain[adapted])
    # all rows base: the whole result is the existing call's
    allbase = dict(c, ids=torch.full((16,), -1, dtype=torch.int32))
    assert torch.equal(_run(allbase, fmt, caches=caches, w_dev=w_dev), plain)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("fmt", ["bf16", "fp8", "fp4"])
def test_adapter_rows_do_not_depend_on_batch_mates(fmt, shape):
    c = _case(shape, 16, 16)
    caches, w_dev = _caches(fmt), c["w"].to(DEV)
    full = _run(c, fmt, caches=caches, w_dev=w_dev)
    i = 4  # slot 1
    one = dict(c, x=c["x"][i:i + 1], r=None if c["r"] is None else c["r"][i:i + 1], ids=c["ids"][i:i + 1])
    assert torch.equal(_run(one, fmt, caches=caches, w_dev=w_dev)[0], full[i])
    # other neighbours, other ids around it, another position
    o = _case(shape, 16, 16, seed=1)
    x2, ids2 = o["x"].clone(), torch.tensor([(s + 1) % SLOTS if s >= 0 else 0 for s in IDS[16]], dtype=torch.int32)
    x2[11], ids2[11] = c["x"][i], c["ids"][i]
    r2 = None
    if c["r"] is not None:
        r2 = o["r"].clone()
        r2[11] = c["r"][i]
    other = dict(c, x=x2, r=r2, ids=ids2)
    assert torch.equal(_run(other, fmt, caches=caches, w_dev=w_dev)[11], full[i])


# ------------------------------------------------------------------------------------------------
# end to end on tiny-llama: two adapters with non-zero B over one base, one continuous batcher
def _save_adapter(cfg, seed, path, r):
    from rag_tl_domainllm_optimizer_amd import models

    m = models.CausalLM(cfg, device="cpu", dtype=torch.bfloat16, seed=0)
    m.add_lora(r, 16.0, "all", seed=seed)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in m.layers:
            for k, p in layer.lora_params.items():
                if k.endswith("_B"):
                    p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    models.save_adapter(m, str(path))


PROMPTS = [[5, 9, 11, 3, 7], [5, 9, 11, 3, 7], [5, 9, 11, 3, 7], [4, 8, 15]]
NAMES = [None, "sft", "ppo", "sft"]
T_NEW = 6


@pytest.fixture(scope="module")
def served(tmp_path_factory):
    from rag_tl_domainllm_optimizer_amd import models

    d = tmp_path_factory.mktemp("adapters")
    cfg = models.resolve_preset("tiny-llama")
    _save_adapter(cfg, 1, d / "sft", 8)
    _save_adapter(cfg, 2, d / "ppo", 4)   # rank below r_max: zero-padded
    _save_adapter(cfg, 3, d / "sft2", 8)
    model = models.CausalLM(cfg, device=DEV, dtype=torch.bfloat16, seed=0)
    bank = models.AdapterBank(model, slots=4, r_max=8)
    bank.load("sft", str(d / "sft"))
    bank.load("ppo", str(d / "ppo"))
    return cfg, model, bank, d


def _score(model, bank, name, prompt, tokens):
    from rag_tl_domainllm_optimizer_amd.train.common import score_sequences

    P, R = torch.tensor([prompt], device=DEV), torch.tensor([tokens], device=DEV)
    with bank.active(name), torch.no_grad():
        lp = score_sequences(model, P, torch.tensor([0], device=DEV), R, torch.tensor([len(tokens)], device=DEV), 1.0, None)[0]
    return lp[0].float().cpu()


def _batcher(model, bank, max_batch=4):
    from rag_tl_domainllm_optimizer_amd.generation import ContinuousBatcher, Generator, SamplingParams

    gen = Generator(model, max_batch=max_batch, max_seq=64, device=DEV)
    return gen, ContinuousBatcher(gen, SamplingParams(max_new_tokens=T_NEW, temperature=0.0), eos_ids=[-1], per_request=True,
                                  adapters=bank)


def _drain(cb, n):
    out = []
    while len(out) < n:
        cb.step(T_NEW)
        out += cb.collect()
    return sorted(out, key=lambda r: r.tag)


def _e2e(model, bank, d, atol):
    from rag_tl_domainllm_optimizer_amd.generation import RequestSampling

    gen, cb = _batcher(model, bank)
    try:
        cb.admit_many(PROMPTS, tags=[0, 1, 2, 3], adapters=NAMES)
        rows = _drain(cb, 4)
        assert [r.adapter for r in rows] == NAMES
        for r in rows:
            ref = _score(model, bank, r.adapter, PROMPTS[r.tag], r.tokens)
            assert torch.allclose(torch.tensor(r.logprobs), ref, atol=atol), (r.adapter, r.logprobs, ref)
        # the adapters and the base really differ on these tokens (teacher-forced, > 0.1 nat per token)
        lp = {n: _score(model, bank, n, PROMPTS[0], rows[0].tokens) for n in (None, "sft", "ppo")}
        for a, b in ((None, "sft"), (None, "ppo"), ("sft", "ppo")):
            assert float((lp[a] - lp[b]).abs().mean()) > 0.1
        # a second wave with another mix: still one captured graph per bucket
        graphs = len(gen.runner.graphs)
        cb.admit_many(PROMPTS, tags=[0, 1, 2, 3], adapters=["ppo", None, "sft", "ppo"])
        rows2 = _drain(cb, 4)
        assert len(gen.runner.graphs) == graphs
        assert rows2[2].tokens == rows[1].tokens and rows2[1].tokens == rows[0].tokens
        # a seeded sampled request with adapter "ppo": same tokens alone and beside mixed batch mates
        rs = RequestSampling(temperature=0.9, top_k=20, seed=1234)
        cb.admit(PROMPTS[3], tag=0, sampling=rs, adapter="ppo")
        alone = _drain(cb, 1)[0]
        cb.admit_many([PROMPTS[0], PROMPTS[3], PROMPTS[1]], tags=[0, 1, 2], sampling=[None, rs, None],
                      adapters=["sft", "ppo", None])
        mixed = _drain(cb, 3)[1]
        assert mixed.tokens == alone.tokens and mixed.logprobs == alone.logprobs
        # load other weights into "sft" in place: the next answer follows them, no recapture
        graphs = len(gen.runner.graphs)
        bank.load("sft", str(d / "sft2"))
        cb.admit(PROMPTS[1], tag=0, adapter="sft")
        new = _drain(cb, 1)[0]
        assert len(gen.runner.graphs) == graphs
        assert torch.allclose(torch.tensor(new.logprobs), _score(model, bank, "sft", PROMPTS[1], new.tokens), atol=atol)
        assert new.tokens != rows[1].tokens or not torch.allclose(torch.tensor(new.logprobs), torch.tensor(rows[1].logprobs),
                                                                  atol=0.05)
    finally:
        cb.close()
        bank.load("sft", str(d / "sft"))


def test_end_to_end_mixed_adapters(served):
    """[None, sft, ppo, sft] in one per_request batcher: each row's logprobs match score_sequences of
    the model with THAT adapter active unmerged (atol 1e-2: graph-vs-training numerics)."""
    cfg, model, bank, d = served
    _e2e(model, bank, d, atol=1e-2)


def _twin_logprobs(cpu, cbank, name, prompt, tokens):
    """Teacher-forced log-probs of ``tokens`` after ``prompt`` on the eager CPU twin of the serving path:
    the batcher's prefill (adapter ``name`` active unmerged, batch-invariant GEMMs), then one fused
    decode step per token with the per-row adapter oracle over the twin's own weight images."""
    from rag_tl_domainllm_optimizer_amd.generation import Generator

    gen = Generator(cpu, max_batch=1, max_seq=64, device="cpu")
    S = len(prompt)
    zero = torch.zeros(1, dtype=torch.int32)
    ids = torch.full((1,), cbank.slot(name), dtype=torch.int32)
    out = []
    with torch.no_grad():
        with cbank.active(name), ops.batch_invariant():
            h = cpu.prefill(torch.tensor([prompt]), zero, gen.cache)
            out.append(torch.log_softmax(cpu.logits(h).float(), -1)[0, tokens[0]])
        cpu.refresh_decode_weights(1)
        for i, t in enumerate(tokens[:-1]):
            at = torch.full((1,), S + i, dtype=torch.int32)
            h = cpu.decode(torch.tensor([t]), at, at, at + 1, zero, gen.cache, None, adapters=(cbank, ids))
            out.append(torch.log_softmax(cpu.logits(h).float(), -1)[0, tokens[i + 1]])
    return torch.stack(out)


def test_end_to_end_over_mxfp4_base(served):
    """Adapters over the MXFP4 base. The decode streams the 4-bit images, so the reference is the eager
    CPU twin of the same step (the same MXFP4 codes: the quantiser is bitwise the oracle; the same
    formula), teacher-forced on the GPU's tokens: ALL T_NEW log-probs of every row, at the bound of the
    bf16 case (atol 1e-2: both sides multiply the same numbers, the differences are summation order
    and bf16 roundings of the activations). The decoded steps must also tell the adapter from the
    base model and from the other adapter: the same tokens scored on the twin under another slot
    differ by more than 0.1 nat per decoded token on average."""
    from rag_tl_domainllm_optimizer_amd import models

    cfg, model, bank, d = served
    cpu = models.CausalLM(cfg, device="cpu", dtype=torch.bfloat16, seed=0)
    cpu.set_fp4_decode(True)
    cbank = models.AdapterBank(cpu, slots=4, r_max=8)
    cbank.load("sft", str(d / "sft"))
    cbank.load("ppo", str(d / "ppo"))
    model.set_fp4_decode(True)
    try:
        gen, cb = _batcher(model, bank)
        try:
            cb.admit_many(PROMPTS, tags=[0, 1, 2, 3], adapters=NAMES)
            rows = _drain(cb, 4)
        finally:
            cb.close()
        assert [r.adapter for r in rows] == NAMES and all(len(r.tokens) == T_NEW for r in rows)
        for r in rows:
            got = torch.tensor(r.logprobs)
            ref = _twin_logprobs(cpu, cbank, r.adapter, PROMPTS[r.tag], r.tokens)
            print(f"fp4 e2e {r.adapter}: max |gpu - twin| {float((got - ref).abs().max()):.3e}")
            assert torch.allclose(got, ref, atol=1e-2), (r.adapter, got, ref)
            for other in (None, "sft", "ppo"):
                if other != r.adapter:
                    off = _twin_logprobs(cpu, cbank, other, PROMPTS[r.tag], r.tokens)
                    assert float((got[1:] - off[1:]).abs().mean()) > 0.1, (r.adapter, other)  # decode steps only
    finally:
        model.set_fp4_decode(False)


def test_batcher_rejects_what_the_kernels_do_not_cover(served):
    from rag_tl_domainllm_optimizer_amd.generation import ContinuousBatcher, Generator, SamplingParams

    cfg, model, bank, d = served
    with pytest.raises(ValueError, match="16 rows"):
        ContinuousBatcher(Generator(model, max_batch=32, max_seq=32, device=DEV), SamplingParams(max_new_tokens=4),
                          adapters=bank)
    gen, cb = _batcher(model, bank)
    try:
        with pytest.raises(KeyError):
            cb.admit(PROMPTS[0], adapter="nope")
        assert cb.free_rows() == 4
    finally:
        cb.close()
