"""MXFP4 weight-only decode on the GPU: the quantiser bitwise against the CPU oracle, the W4A16
16-row GEMV against ``x @ dequantize_mxfp4(...)^T`` within twice the error of the bf16 tile-ordered
kernel on the same (dequantised) weights, rows independent of M, the fused decode layer against
its CPU twin, generation under graph replay with a weight refresh, and prompt-lookup decoding."""
import pytest
import torch

from rag_tl_domainllm_optimizer_amd import models, ops
from rag_tl_domainllm_optimizer_amd.generation import Generator, SamplingParams
from rag_tl_domainllm_optimizer_amd.models.config import PRESETS

import test_lookup_decode_cpu as cpu_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
SHAPES = [(32, 256), (512, 768), (6144, 4096), (5120, 13824)]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _weight(N, K, lo, hi, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) * torch.logspace(lo, hi, N)[:, None]).to(torch.bfloat16)


# ------------------------------------------------------------------------------------- quantiser
def test_quantiser_is_bitwise_the_cpu_oracle():
    N, K = 70 * 16, 4096
    w = _weight(N, K, -3, 3)
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    for i, k in enumerate((-20, -3, 0, 5, 30)):  # the hand cases of the CPU test, one block each
        two_k = 2.0 ** k
        w[i, :32] = 0
        w[i, :3] = torch.tensor([two_k, -two_k / 2, two_k / 8]).to(torch.bfloat16)
        w[i, 32:64] = 0
        w[i, 32:35] = torch.tensor([7.5 * two_k, -7.5 * two_k, 6 * two_k]).to(torch.bfloat16)
        w[i, 64:96] = 0
        w[i, 64:79] = torch.tensor([6 * two_k] + [t * two_k for t in ties] + [-t * two_k for t in ties]).to(torch.bfloat16)
    w[9, 128:160] = 0  # an all-zero block with negative zeros
    w[9, 130:140] = -0.0
    w[10, 0:32] = torch.tensor([4.0, -0.1, 0.1, -0.0] + [0.0] * 28).to(torch.bfloat16)
    qc, sc = ops.quantize_mxfp4(w)
    qg, sg = ops.quantize_mxfp4(w.to(DEV))
    assert qg.is_cuda and qg.dtype == torch.uint8 and sg.dtype == torch.uint8
    assert torch.equal(sg.cpu(), sc), "scales differ from the oracle"
    assert torch.equal(qg.cpu(), qc), "codes differ from the oracle"


def test_cache_refreshes_in_place():
    w = _weight(64, 512, -1, 1).to(DEV)
    c = ops.Fp4Cache()
    img, simg = c.image(w)
    ptrs = (img.data_ptr(), simg.data_ptr())
    s0, i0 = simg.clone(), img.clone()
    assert "q" not in c  # only the image stays resident on the GPU
    assert c.image(w)[0].data_ptr() == ptrs[0]
    w.mul_(0.5)
    img2, simg2 = c.image(w)
    assert (img2.data_ptr(), simg2.data_ptr()) == ptrs
    assert torch.equal(simg2, s0 - 1) and torch.equal(img2, i0)  # half the weight: every exponent one lower
    # a second cache of the same shape shares the staging buffer and leaves this image alone
    ops.Fp4Cache().image(_weight(64, 512, -1, 1, seed=5).to(DEV))
    assert torch.equal(simg2, s0 - 1) and torch.equal(img2, i0)


def test_image_layout():
    """the documented layout of the code and scale images, rebuilt on the host"""
    N, K = 48, 768
    w = _weight(N, K, -2, 2, seed=3).to(DEV)
    c = ops.Fp4Cache()
    img, simg = (t.cpu() for t in c.image(w))
    q, s = (t.cpu() for t in c.get(w))
    nc = K // 256
    blocks = q.reshape(N // 16, 16, nc, 2, 4, 16)  # [G, r, c, h, g, 16 B]
    want = blocks.permute(0, 2, 3, 4, 1, 5).reshape(N, K // 2)  # [G, c, h, g, r, 16 B]
    assert torch.equal(img, want)
    sb = s.reshape(N // 16, 16, nc, 2, 4)  # [G, r, c, h, g]
    swant = sb.permute(0, 2, 4, 1, 3).reshape(N, K // 32)  # [G, c, g, r, h]: lane 16 g + r, bytes h = 0, 1
    assert torch.equal(simg, swant)


# ------------------------------------------------------------------------------------------ GEMV
def _oracle(x, d, mode, r):
    # x @ dequantize(...)^T, summed in float64: in the fp32-output mode the kernels' errors are a few
    # fp32 ulps, the size of a float32 host product's own summation error
    y = x.double() @ d.double().t()
    if mode != "plain":
        y = y * torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + EPS)
    if mode == "swiglu":
        F = d.shape[0] // 2
        y = torch.nn.functional.silu(y[:, :F]) * y[:, F:]
    if mode == "norm_residual":
        y = y + r.double()
    return y


@pytest.fixture(scope="module")
def gemv_case():
    """per (N, K): the weight, its dequantised twin, the caches and 16 rows of X, built once"""
    store = {}

    def get(N, K):
        if (N, K) not in store:
            g = torch.Generator().manual_seed(N + K)
            w = _weight(N, K, -1, 1, seed=N)
            d = ops.dequantize_mxfp4(*ops.quantize_mxfp4(w))
            x = torch.randn(16, K, generator=g).to(torch.bfloat16)
            r = torch.randn(16, N, generator=g).to(torch.bfloat16)
            store[(N, K)] = (w.to(DEV), d, d.to(torch.bfloat16).to(DEV), x, r, ops.Fp4Cache(), ops.ShufCache())
        return store[(N, K)]

    return get


@pytest.mark.parametrize("mode", ["plain", "plain_f32", "norm_residual", "swiglu"])
@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("N,K", SHAPES)
def test_gemv_against_dequantised_product(gemv_case, N, K, M, mode):
    if mode == "swiglu" and N % 64:
        N = 64  # the pair form needs N % 64 == 0: (64, 256) is the one-chunk case of this mode
    _check_gemv(gemv_case, N, K, M, mode)


@pytest.mark.parametrize("K", [256, 1280, 3072, 3328])
def test_gemv_ring_edges(gemv_case, K):
    """depth 3, 256 k per chunk, N = 64 (4 row groups: 8 waves, the pair form 4): 1 chunk (the other
    waves idle), 5 (0-1 per wave at 8 waves, 1-2 at 4: the ring never fills), 12 (exactly DEPTH per
    wave at 4 waves, 1-2 at 8), 13 (DEPTH + 1 for one of 4 waves, an uneven 1-2 at 8)"""
    for M in (1, 16):
        for mode in ("plain", "plain_f32", "norm_residual", "swiglu"):
            _check_gemv(gemv_case, 64, K, M, mode)


def _check_gemv(gemv_case, N, K, M, mode):
    w, d, d_dev, x16, r16, f4, sh = gemv_case(N, K)
    x, r = x16[:M], r16[:M]
    xd, rd = x.to(DEV), r.to(DEV)
    want = _oracle(x, d, "plain" if mode == "plain_f32" else mode, r)
    if mode == "plain_f32":
        got = ops.native().gemv_fp4(xd, *f4.image(w), None, 0, True, None, None, 0.0)
        base = ops.native().gemm(xd, sh.get(d_dev), None, None, None, 0, True, None, None, 0.0, True)
        assert got.dtype == torch.float32
    else:
        kw = {"plain": {}, "norm_residual": {"residual": rd, "norm_eps": EPS},
              "swiglu": {"act": ops.ACT_SWIGLU, "norm_eps": EPS}}[mode]
        got = ops.gemm_decode(xd, w, fp4=f4, **kw)
        base = ops.gemm_decode(xd, d_dev, shuf=sh, **kw)
        assert got.dtype == torch.bfloat16
    assert got.shape == want.shape and torch.isfinite(got).all()
    err = (got.double().cpu() - want).abs().max().item()
    err_base = (base.double().cpu() - want).abs().max().item()
    print(f"fp4 gemv N={N} K={K} M={M} {mode}: err {err:.4g} bf16-kernel err {err_base:.4g} "
          f"ratio {err / max(err_base, 1e-30):.3f}")
    assert err <= 2 * err_base, (err, err_base)


@pytest.mark.parametrize("mode", ["plain", "norm_residual", "swiglu"])
@pytest.mark.parametrize("N,K", SHAPES)
def test_rows_do_not_depend_on_m(gemv_case, N, K, mode):
    if mode == "swiglu" and N % 64:
        N = 64
    w, d, d_dev, x16, r16, f4, sh = gemv_case(N, K)
    xd, rd = x16.to(DEV), r16.to(DEV)
    kw = {"plain": {}, "norm_residual": {"residual": rd, "norm_eps": EPS}, "swiglu": {"act": ops.ACT_SWIGLU, "norm_eps": EPS}}[mode]
    y16 = ops.gemm_decode(xd, w, fp4=f4, **kw)
    for M in (1, 3):
        kwm = dict(kw, residual=rd[:M]) if "residual" in kw else kw
        ym = ops.gemm_decode(xd[:M].contiguous(), w, fp4=f4, **kwm)
        assert torch.equal(_bits(ym), _bits(y16[:M])), f"rows of the M = {M} result differ from the M = 16 result"


def test_bad_shapes_raise():
    C = ops.native()
    f4 = ops.Fp4Cache()
    w = _weight(64, 512, -1, 1).to(DEV)
    img, simg = f4.image(w)
    x = torch.zeros(4, 512, dtype=torch.bfloat16, device=DEV)
    C.gemv_fp4(x, img, simg)
    with pytest.raises(RuntimeError):
        C.gemv_fp4(torch.zeros(17, 512, dtype=torch.bfloat16, device=DEV), img, simg)
    with pytest.raises(RuntimeError):
        C.gemv_fp4(torch.zeros(4, 256, dtype=torch.bfloat16, device=DEV), img, simg)
    with pytest.raises(RuntimeError):
        C.gemv_fp4(x.float(), img, simg)
    with pytest.raises(RuntimeError):
        C.gemv_fp4(x, img, simg[:, :8].contiguous())
    with pytest.raises(RuntimeError):
        C.gemv_fp4(x, img[:32].contiguous(), simg[:32].contiguous(), None, ops.ACT_SWIGLU)  # pair: N % 64
    with pytest.raises(RuntimeError):
        C.gemv_fp4(x, img.cpu(), simg)
    with pytest.raises(RuntimeError):
        C.gemv_fp4(x, img, simg, None, 0, False, None, torch.zeros(4, 32, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(RuntimeError):
        C.gemv_fp4(torch.zeros(4, 1024, dtype=torch.bfloat16, device=DEV)[:, ::2], img, simg)
    with pytest.raises(RuntimeError):
        C.quant_mxfp4(torch.zeros(4, 48, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(RuntimeError):
        C.shuffle_decode_weight_fp4(torch.zeros(8, 128, dtype=torch.uint8, device=DEV),
                                    torch.zeros(8, 8, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError):
        C.shuffle_decode_weight_fp4(torch.zeros(16, 64, dtype=torch.uint8, device=DEV),
                                    torch.zeros(16, 4, dtype=torch.uint8, device=DEV))
    # an unsupported weight keeps the bf16 path
    w2, x2 = _weight(24, 128, -1, 1).to(DEV), torch.randn(2, 128).to(torch.bfloat16).to(DEV)
    assert torch.equal(_bits(ops.gemm_decode(x2, w2, fp4=ops.Fp4Cache())), _bits(ops.gemm_decode(x2, w2)))


# ----------------------------------------------------------------------------------------- layer
def _layer_pair():
    md = models.CausalLM(PRESETS["tiny-llama"], device=torch.device(DEV), dtype=torch.bfloat16, seed=0)
    mc = models.CausalLM(PRESETS["tiny-llama"], dtype=torch.bfloat16, seed=0)
    return md, mc


def _attend(cfg):
    n = cfg.num_heads * cfg.head_dim
    return lambda qkv: qkv[:, :n].contiguous()  # row-local stand-in for attention, the same on both devices


@pytest.mark.parametrize("m", [1, 8])
def test_layer_matches_cpu_twin(m):
    md, mc = _layer_pair()
    ld, lc = md.layers[0], mc.layers[0]
    h = (torch.randn(m, md.cfg.hidden_size, generator=torch.Generator().manual_seed(m)) * 0.5).to(torch.bfloat16)
    att = _attend(md.cfg)
    with torch.no_grad():
        off = (ld.decode_fused(h.to(DEV), att).float().cpu() - lc.decode_fused(h, att).float()).abs().max().item()
        md.set_fp4_decode(True)
        mc.set_fp4_decode(True)
        yd, yc = ld.decode_fused(h.to(DEV), att), lc.decode_fused(h, att)
    assert sorted(ld._fp4) == sorted(lc._fp4) == ["down", "gate_up", "o", "qkv"]
    # the same codes on both sides (the quantiser is bitwise the oracle), here for the folded qkv weight
    qd, sd = ops.quantize_mxfp4(ld._fold["qkv"]["w"])
    assert torch.equal(qd.cpu(), lc._fp4["qkv"]["q"]) and torch.equal(sd.cpu(), lc._fp4["qkv"]["s"])
    on = (yd.float().cpu() - yc.float()).abs().max().item()
    print(f"fp4 layer m={m}: GPU-vs-CPU max diff fp4 on {on:.4g}, off {off:.4g}")
    assert torch.isfinite(yd).all() and on <= 2 * off, (on, off)


def test_option_off_is_the_parent_path():
    md, _ = _layer_pair()
    layer, cfg = md.layers[0], md.cfg
    h = (torch.randn(4, cfg.hidden_size, generator=torch.Generator().manual_seed(1)) * 0.5).to(torch.bfloat16).to(DEV)
    att = _attend(cfg)
    with torch.no_grad():
        got = layer.decode_fused(h, att)
        # the same four calls without the fp4 argument
        wq = ops.FoldCache().get(layer.qkv_w, layer.ln1_w)
        qkv = ops.gemm_decode(h, wq, norm_eps=cfg.norm_eps, shuf=ops.ShufCache())
        h1 = ops.gemm_decode(att(qkv), layer.o_w, residual=h, shuf=ops.ShufCache())
        wgu = ops.FoldCache().get(layer.gate_up_w, layer.ln2_w)
        f = ops.gemm_decode(h1, wgu, act=ops.ACT_SWIGLU, norm_eps=cfg.norm_eps, shuf=ops.ShufCache())
        want = ops.gemm_decode(f, layer.down_w, residual=h1, shuf=ops.ShufCache())
    assert not layer._fp4 and torch.equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------ generation
def test_generation_graph_replay_and_refresh():
    m = models.CausalLM(PRESETS["tiny-mistral"], device=torch.device(DEV), dtype=torch.bfloat16, seed=0)
    m.set_fp4_decode(True)
    prompts = [[5, 9, 33, 41, 7, 8], [12, 300, 4]]
    sp = SamplingParams(max_new_tokens=12, do_sample=False)
    gen = Generator(m, 2, 64, device=torch.device(DEV))
    o1 = gen.generate(prompts, sp, pad_id=0, eos_ids=[-1])
    assert o1.tokens.shape == (2, 12) and torch.isfinite(o1.logprobs).all()
    assert int(o1.tokens.min()) >= 0 and int(o1.tokens.max()) < m.cfg.vocab_size
    assert sorted(m.layers[0]._fp4) == ["down", "gate_up", "o", "qkv"]
    ptr = m.layers[0]._fp4["down"]["img"].data_ptr()
    with torch.no_grad():
        for layer in m.layers:
            layer.down_w.mul_(-0.5)
            layer.o_w.mul_(0.25)
    m.refresh_decode_weights()
    assert m.layers[0]._fp4["down"]["img"].data_ptr() == ptr
    o2 = gen.generate(prompts, sp, pad_id=0, eos_ids=[-1])  # replays the captured step
    fresh = Generator(m, 2, 64, device=torch.device(DEV)).generate(prompts, sp, pad_id=0, eos_ids=[-1])
    assert not torch.equal(o2.logprobs, o1.logprobs)
    assert torch.equal(o2.tokens, fresh.tokens) and torch.equal(o2.logprobs, fresh.logprobs)


@pytest.mark.parametrize("B", [1, 2])
def test_lookup_greedy_equals_plain_under_fp4(B):
    m = models.CausalLM(PRESETS["tiny-llama"], device=torch.device(DEV), dtype=torch.bfloat16, seed=2)
    m.set_fp4_decode(True)
    prompts = [cpu_cases.PROMPTS[0], cpu_cases.PROMPTS[2]][:B]  # both repeat an n-gram
    gen = Generator(m, B, 96, device=torch.device(DEV))
    plain = gen.generate(prompts, SamplingParams(max_new_tokens=32, do_sample=False), pad_id=0, eos_ids=[-1])
    look = gen.generate(prompts, SamplingParams(max_new_tokens=32, do_sample=False, lookup_tokens=3), pad_id=0,
                        eos_ids=[-1])
    assert look.timings["lookup_drafted"] > 0
    assert torch.equal(look.tokens, plain.tokens)
    if B == 2:  # 8 rows x 4 positions do not fit the 16-row kernels
        big = Generator(m, 8, 96, device=torch.device(DEV))
        with pytest.raises(ValueError, match="16 rows"):
            big.generate([prompts[0]] * 8, SamplingParams(max_new_tokens=4, do_sample=False, lookup_tokens=3), pad_id=0,
                         eos_ids=[-1])
