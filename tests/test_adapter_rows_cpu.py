"""Per-request LoRA adapters on the CPU paths: the eager oracle of ``gemm_decode(rows_lora=...)``,
the AdapterBank, ContinuousBatcher validation and the HTTP ``adapter`` field."""
import pytest
import torch

from rag_tl_domainllm_optimizer_amd import models, ops
from rag_tl_domainllm_optimizer_amd.generation import ContinuousBatcher, Generator, SamplingParams

EPS = 1e-5
U = 2.0 ** -9  # bf16 unit roundoff (round to nearest, 8 significand bits)


def _problem(N, K, segs, pair, R=8, M=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    bounds = [0] + ([N // 2] if pair else list(segs)) + [N]
    nseg = len(bounds) - 1
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    nw = 1 + 0.1 * torch.randn(K, generator=g)
    A = torch.randn(2, nseg, R, K, generator=g) / K ** 0.5   # fp32 masters, s folded in
    B = [[torch.randn(bounds[i + 1] - bounds[i], R, generator=g) * 0.3 for i in range(nseg)] for _ in range(2)]
    ids = torch.tensor([1, -1, 0, 1, -1], dtype=torch.int32)
    res = torch.randn(M, N, generator=g).to(torch.bfloat16)
    return dict(N=N, K=K, segs=segs, pair=pair, R=R, bounds=bounds, nseg=nseg, x=x, w=w, nw=nw, A=A, B=B, ids=ids, res=res)


def _images(p, norm):
    fold = p["nw"][None, :] if norm else 1.0
    a_img = torch.stack([(p["A"][s] * fold).reshape(p["nseg"] * p["R"], p["K"]) for s in range(2)]).to(torch.bfloat16)
    b_img = torch.stack([torch.cat(p["B"][s], 0) for s in range(2)]).to(torch.bfloat16)
    return a_img, b_img


@pytest.mark.parametrize("case", ["qkv", "qkv_norm", "swiglu_norm", "res", "norm_res"])
def test_oracle_matches_dense_fp64(case):
    """Per row: bf16(oracle) vs fp64 epilogue(rs x (W' + B_a A_a')^T), A' = the fp32 s A diag(norm w).

    Tolerance: x and W' are the same bf16 numbers on both sides. The oracle rounds A' and B to bf16
    (relative error <= U each, U = 2^-9), so each product x_k A'_jk B_nj is off by at most (2 U + U^2)
    of its magnitude, and the adapter term by at most 2.01 U * P_n with P = |x| |A'|^T |B|^T; the
    fp32 accumulation adds <= (K + R) 2^-24 of the summed magnitudes (folded into the 2.01 -> 2.1).
    The pre-epilogue error e = 2.1 U rs P passes through: identity (1), SwiGLU (|d silu| <= 1.1:
    1.1 e_g |u| + |silu(g)| e_u + 1.1 e_g e_u), the exact residual add, and one final bf16 rounding
    of the result, U |y|."""
    norm, pair, res = "norm" in case, "swiglu" in case, "res" in case
    N, K, segs = (512, 256, ()) if pair else (256, 128, (128, 192)) if "qkv" in case else (128, 256, ())
    p = _problem(N, K, segs, pair)
    a_img, b_img = _images(p, norm)
    x, w, ids = p["x"], p["w"], p["ids"]
    kw = dict(act=ops.ACT_SWIGLU if pair else 0, residual=p["res"] if res else None, norm_eps=EPS if norm else 0.0)
    t = ops.lora_rows_shrink(x, a_img, ids)
    got = ops.gemm_decode(x, w, rows_lora=(t, b_img, ids, segs), **kw).double()
    plain = ops.gemm_decode(x, w, **kw)
    xd = x.double()
    rs = torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + EPS) if norm else torch.ones(x.shape[0], 1, dtype=torch.float64)
    fold = p["nw"].double()[None, :] if norm else 1.0
    for b, s in enumerate(ids.tolist()):
        if s < 0:
            assert torch.equal(got[b].to(torch.bfloat16), plain[b])  # base rows: exactly the call without rows_lora
            continue
        delta = torch.cat([p["B"][s][i].double() @ (p["A"][s, i].double() * fold) for i in range(p["nseg"])], 0)  # [N, K]
        pabs = torch.cat([p["B"][s][i].double().abs() @ (p["A"][s, i].double() * fold).abs() for i in range(p["nseg"])], 0)
        y = rs[b] * ((w.double() + delta) @ xd[b])
        e = 2.1 * U * rs[b] * (pabs @ xd[b].abs())
        if pair:
            F = N // 2
            gq, uq = y[:F], y[F:]
            sg = torch.nn.functional.silu(gq)
            e = 1.1 * e[:F] * uq.abs() + sg.abs() * e[F:] + 1.1 * e[:F] * e[F:]
            y = sg * uq
        if res:
            y = y + p["res"][b].double()
        tol = e + U * y.abs() + 1e-30
        assert bool(((got[b] - y).abs() <= tol).all()), float(((got[b] - y).abs() / tol).max())
        assert float((rs[b] * (delta @ xd[b])).pow(2).mean().sqrt()) > 0.25 * float((rs[b] * (w.double() @ xd[b])).pow(2).mean().sqrt())


def test_oracle_rejects_bad_arguments():
    p = _problem(256, 128, (128, 192), False)
    a_img, b_img = _images(p, False)
    t = ops.lora_rows_shrink(p["x"], a_img, p["ids"])
    with pytest.raises(ValueError, match="16 rows"):
        ops.gemm_decode(torch.zeros(17, 128, dtype=torch.bfloat16), p["w"], rows_lora=(t, b_img, p["ids"], p["segs"]))
    with pytest.raises(ValueError, match="16 rows"):
        ops.lora_rows_shrink(torch.zeros(17, 128, dtype=torch.bfloat16), a_img, p["ids"])
    with pytest.raises(ValueError):
        ops.gemm_decode(p["x"], p["w"], rows_lora=(t, b_img, p["ids"], (128,)))  # 3 segments in T, 2 given


# ------------------------------------------------------------------------------------------------
def _save(cfg, seed, path, r, targets="all"):
    m = models.CausalLM(cfg, device="cpu", dtype=torch.bfloat16, seed=0)
    m.add_lora(r, 16.0, targets, seed=seed)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in m.layers:
            for k, prm in layer.lora_params.items():
                if k.endswith("_B"):
                    prm.copy_(torch.randn(prm.shape, generator=g) * 0.05)
    m.refresh_lora()
    models.save_adapter(m, str(path))
    return m


@pytest.fixture(scope="module")
def adapters(tmp_path_factory):
    d = tmp_path_factory.mktemp("bank")
    cfg = models.resolve_preset("tiny-llama")
    return cfg, d, _save(cfg, 1, d / "sft", 8), _save(cfg, 2, d / "ppo", 4, ["q_proj", "v_proj", "down_proj"])


def test_bank_round_trip_padding_and_errors(adapters):
    cfg, d, m_sft, m_ppo = adapters
    base = models.CausalLM(cfg, device="cpu", dtype=torch.bfloat16, seed=0)
    with torch.no_grad():
        base.layers[0].ln1_w.mul_(1.5)
    bank = models.AdapterBank(base, slots=2, r_max=8)
    assert bank.load("sft", str(d / "sft")) == 0 and bank.load("ppo", str(d / "ppo")) == 1
    assert bank.loaded() == ["sft", "ppo"] and bank.slot(None) == -1 and bank.slot("ppo") == 1
    Hq = cfg.num_heads * cfg.head_dim
    for name, m, r in (("sft", m_sft, 8), ("ppo", m_ppo, 4)):
        sl, s = bank.slot(name), m.lora_config.scaling
        for li, layer in enumerate(m.layers):
            e = bank.layer(li)["qkv"]
            assert e["segs"] == (Hq, Hq + cfg.num_kv_heads * cfg.head_dim)
            A, B = layer.lora_params["q_proj_A"].detach(), layer.lora_params["q_proj_B"].detach()
            assert torch.equal(e["a_raw"][sl, :r], (A * s).to(torch.bfloat16))
            nw = base.layers[li].ln1_w.detach().float()
            assert torch.equal(e["a_img"][sl, :r], (A * s * nw[None, :]).to(torch.bfloat16))  # folded, rounded once
            assert torch.equal(e["b_img"][sl, :Hq, :r], B.to(torch.bfloat16))
            assert not e["a_img"][sl, r:8].any() and not e["b_img"][sl, :Hq, r:].any()  # rank padding
            o = bank.layer(li)["o"]
            assert o["a_raw"] is o["a_img"]
            if name == "ppo":  # target modules the adapter lacks are zeros
                assert not e["a_img"][sl, 8:16].any() and not o["b_img"][sl].any()
                assert not bank.layer(li)["gate_up"]["b_img"][sl].any() and bank.layer(li)["down"]["b_img"][sl].any()
    ptrs = [bank.layer(0)[g]["b_img"].data_ptr() for g in ("qkv", "o", "gate_up", "down")]
    # a norm weight changed after load and BEFORE the first refresh is re-folded too
    with torch.no_grad():
        base.layers[0].ln1_w.add_(0.25)
    bank.refresh()
    A0 = m_sft.layers[0].lora_params["k_proj_A"].detach() * m_sft.lora_config.scaling
    assert torch.equal(bank.layer(0)["qkv"]["a_img"][0, 8:16],
                       (A0 * base.layers[0].ln1_w.detach().float()[None, :]).to(torch.bfloat16))
    # in place over the same name; a norm-weight change re-folds on refresh
    bank.refresh()
    with torch.no_grad():
        base.layers[1].ln2_w.mul_(0.5)
    bank.refresh()
    A = m_sft.layers[1].lora_params["gate_proj_A"].detach() * m_sft.lora_config.scaling
    assert torch.equal(bank.layer(1)["gate_up"]["a_img"][0, :8],
                       (A * base.layers[1].ln2_w.detach().float()[None, :]).to(torch.bfloat16))
    assert bank.load("sft", str(d / "ppo")) == 0
    assert ptrs == [bank.layer(0)[g]["b_img"].data_ptr() for g in ("qkv", "o", "gate_up", "down")]
    assert not bank.layer(0)["o"]["b_img"][0].any()
    with pytest.raises(ValueError, match="slots"):
        bank.load("third", str(d / "sft"))
    bank.unload("sft")
    assert bank.loaded() == ["ppo"] and not bank.layer(0)["qkv"]["b_img"][0].any()
    with pytest.raises(KeyError):
        bank.slot("sft")
    with pytest.raises(ValueError, match="r_max"):
        models.AdapterBank(base, slots=1, r_max=12)
    small = models.AdapterBank(base, slots=1, r_max=8)
    _save(cfg, 3, d / "r16", 16)
    with pytest.raises(ValueError, match="exceeds"):
        small.load("big", str(d / "r16"))
    # an adapter trained on a base of other shapes: refused, and nothing is written
    import dataclasses

    other = dataclasses.replace(cfg, hidden_size=cfg.hidden_size // 2, intermediate_size=cfg.intermediate_size // 2)
    _save(other, 4, d / "other", 8)
    with pytest.raises(ValueError, match="base model needs"):
        small.load("other", str(d / "other"))
    assert small.loaded() == [] and small.names == [None] and small.version == [0]
    for li in range(cfg.num_layers):
        for e in small.layer(li).values():
            assert not e["a_img"].any() and not e["b_img"].any() and not e["a_raw"].any()
    with pytest.raises(ValueError, match="opt"):
        models.AdapterBank(models.CausalLM(models.resolve_preset("tiny-opt"), device="cpu", dtype=torch.bfloat16, seed=0))


def test_active_slot_is_the_unmerged_adapter(adapters):
    """bank.active(name): the token-parallel forward equals the model that trained the adapter."""
    cfg, d, m_sft, _ = adapters
    base = models.CausalLM(cfg, device="cpu", dtype=torch.bfloat16, seed=0)
    bank = models.AdapterBank(base, slots=2, r_max=8)
    bank.load("sft", str(d / "sft"))
    ids = torch.tensor([[5, 9, 11, 3, 7, 2, 8]])
    with torch.no_grad():
        want = m_sft(ids)
        plain = base(ids)
        with bank.active("sft"):
            got = base(ids)
        with bank.active(None):
            none = base(ids)
        after = base(ids)
    first = lambda o: o[0] if isinstance(o, (tuple, list)) else o  # noqa: E731
    assert torch.equal(first(got), first(want)) and not torch.equal(first(got), first(plain))
    assert torch.equal(first(none), first(plain)) and torch.equal(first(after), first(plain))


def test_batcher_validation_and_rows(adapters):
    cfg, d, _, _ = adapters
    base = models.CausalLM(cfg, device="cpu", dtype=torch.bfloat16, seed=0)
    bank = models.AdapterBank(base, slots=2, r_max=8)
    bank.load("sft", str(d / "sft"))
    sp = SamplingParams(max_new_tokens=3, temperature=0.0)
    with pytest.raises(ValueError, match="16 rows"):
        ContinuousBatcher(Generator(base, max_batch=17, max_seq=32, device="cpu"), sp, adapters=bank)
    with pytest.raises(ValueError, match="lookup"):
        ContinuousBatcher(Generator(base, max_batch=2, max_seq=32, device="cpu"),
                          SamplingParams(max_new_tokens=3, lookup_tokens=2), adapters=bank)
    own = models.CausalLM(cfg, device="cpu", dtype=torch.bfloat16, seed=0)
    own.add_lora(8, 16.0, "all")
    with pytest.raises(ValueError, match="another model"):
        ContinuousBatcher(Generator(own, max_batch=2, max_seq=32, device="cpu"), sp, adapters=bank)
    with pytest.raises(ValueError, match="of its own"):
        ContinuousBatcher(Generator(own, max_batch=2, max_seq=32, device="cpu"), sp,
                          adapters=models.AdapterBank(own, slots=1, r_max=8))
    gen = Generator(base, max_batch=2, max_seq=32, device="cpu")
    plain = ContinuousBatcher(gen, sp, eos_ids=[-1])
    with pytest.raises(ValueError, match="adapters=bank"):
        plain.admit([5, 6, 7], adapter="sft")
    plain.admit([5, 6, 7], tag="b")
    plain.step(3)
    want = plain.collect()[0]
    plain.close()
    cb = ContinuousBatcher(gen, sp, eos_ids=[-1], adapters=bank)
    with pytest.raises(KeyError):
        cb.admit([5, 6, 7], adapter="nope")
    assert cb.free_rows() == 2
    cb.admit_many([[5, 6, 7], [5, 6, 7]], tags=["a", "b"], adapters=["sft", None])
    cb.step(3)
    rows = {r.tag: r for r in cb.collect()}
    cb.close()
    assert rows["a"].adapter == "sft" and rows["b"].adapter is None
    assert rows["b"].tokens == want.tokens  # a base row beside an adapter row: the base model's answer
    assert rows["a"].logprobs != rows["b"].logprobs


def test_http_adapter_field(adapters):
    from fastapi.testclient import TestClient

    from rag_tl_domainllm_optimizer_amd import config as C
    from rag_tl_domainllm_optimizer_amd.rag import RagPipeline
    from rag_tl_domainllm_optimizer_amd.retrieval import Encoder, FlatIndex
    from rag_tl_domainllm_optimizer_amd.serve import create_app
    from rag_tl_domainllm_optimizer_amd.tokenizer import Tokenizer

    cfg, d, _, _ = adapters
    pol = models.CausalLM(cfg, device="cpu", dtype=torch.bfloat16, seed=0)
    enc_m = models.build_model("tiny-bert", device="cpu", dtype=torch.float32, seed=2).eval()
    tok = Tokenizer.synthetic(pol.cfg.vocab_size, pol.cfg.arch)
    enc = Encoder(enc_m, Tokenizer.synthetic(enc_m.cfg.vocab_size, enc_m.cfg.arch), max_length=32)
    words = tok.words()
    docs = [" ".join(words[(7 * i + j) % len(words)] for j in range(12)) for i in range(30)]
    index = FlatIndex(enc.dim, "ip", "cpu")
    index.add(enc.encode(docs))
    pipe = RagPipeline(enc, index, docs, pol, tok, top_k=2, sampling=SamplingParams(max_new_tokens=3, do_sample=False),
                       max_prompt_tokens=96, max_batch=2, use_graph=False)
    bank = models.AdapterBank(pol, slots=2, r_max=8)
    bank.load("sft", str(d / "sft"))
    q = f"{words[1]} {words[4]}"
    with TestClient(create_app(pipe, continuous=True, adapters=bank)) as c:
        assert c.get("/health").json()["adapters"] == ["sft"]
        r = c.post("/answer", json={"query": q, "adapter": "nope"})
        assert r.status_code == 422 and "nope" in r.json()["detail"]
        r = c.post("/answer", json={"query": q, "adapter": "sft"})
        assert r.status_code == 200 and r.json()["timings"]["adapter"] == "sft"
        r = c.post("/answer", json={"query": q})
        assert r.status_code == 200 and r.json()["timings"]["adapter"] is None
    with TestClient(create_app(pipe, continuous=True)) as c:
        assert c.get("/health").json()["adapters"] == []
        r = c.post("/answer", json={"query": q, "adapter": "sft"})
        assert r.status_code == 400 and "serve.adapters" in r.json()["detail"]
        assert "adapter" not in c.post("/answer", json={"query": q}).json()["timings"]
    with pytest.raises(ValueError):
        create_app(pipe, continuous=False, adapters=bank)
    assert C.RunConfig().serve.adapters == {}
