"""Numerics of every HIP kernel against the plain-PyTorch fp32 reference of the same op."""
import contextlib
import math

import pytest
import torch

from rag_tl_domainllm_optimizer_amd import ops
from rag_tl_domainllm_optimizer_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _close(a, b, rtol=2e-2, atol=2e-2):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item() + 1e-6
    assert err <= atol + rtol * scale, f"max err {err} (scale {scale})"


def setup_module(_):
    torch.manual_seed(0)
    assert ops.native_available(), "native extension must load on the GPU box"


@pytest.mark.parametrize("M,N,K", [(256, 256, 256), (300, 1000, 512), (1024, 6144, 1024), (1, 4096, 4096),
                                   (37, 2048, 1024), (64, 512, 384), (129, 136, 128)])
def test_gemm(M, N, K):
    a = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16) / math.sqrt(K)
    _close(ops.gemm(a, w), ref.gemm(a, w, out_f32=True))


@pytest.mark.parametrize("M", [8, 200])
def test_gemm_lora_bias_act(M):
    K, N, R = 512, 384, 64
    a = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16) / math.sqrt(K)
    u = torch.randn(M, R, device=DEV, dtype=torch.bfloat16)
    ub = torch.randn(N, R, device=DEV, dtype=torch.bfloat16) * 0.1
    b = torch.randn(N, device=DEV, dtype=torch.bfloat16)
    for act in (0, 1, 2, 3, 4):
        _close(ops.gemm(a, w, u, ub, b, act), ref.gemm(a, w, u, ub, b, act, out_f32=True))
    y32 = ops.gemm(a, w, u, ub, b, 0, out_f32=True)
    assert y32.dtype == torch.float32
    _close(y32, ref.gemm(a, w, u, ub, b, 0, out_f32=True), rtol=5e-3, atol=5e-3)


def test_gemm_asymmetric_identity():
    # A = I with asymmetric B catches transposed C writes (cdna_hip_programming.md §3)
    n = 128
    a = torch.eye(n, device=DEV, dtype=torch.bfloat16)
    w = (torch.arange(n * n, device=DEV).reshape(n, n) % 97).to(torch.bfloat16)
    out = ops.gemm(a, w)
    assert torch.equal(out.float(), w.t().float())


@pytest.mark.parametrize("M", [96, 40, 600])
def test_linear_lora_autograd(M):
    """LoRA forward (K-extension on the base GEMM's accumulators), NN dX with the dU A_pad extension,
    TN adapter gradients, merged inference weight."""
    torch.manual_seed(1)
    K, N, r = 256, 192, 8
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    w = torch.nn.Parameter((torch.randn(N, K, device=DEV) / 16).to(torch.bfloat16), requires_grad=False)
    a1 = torch.nn.Parameter(torch.randn(r, K, device=DEV) * 0.05)
    b1 = torch.nn.Parameter(torch.randn(N // 2, r, device=DEV) * 0.05)
    a2 = torch.nn.Parameter(torch.randn(r, K, device=DEV) * 0.05)
    b2 = torch.nn.Parameter(torch.randn(N // 2, r, device=DEV) * 0.05)
    grp = ops.LoRAGroup(["q", "v"], [a1, a2], [b1, b2], [0, N // 2], [2.0, 2.0], N)
    y = ops.linear(x, w, lora=grp)
    with torch.no_grad():  # merged inference weight (W + UB A_pad, bf16 GEMM with beta = 1)
        wm = grp.merged_weight(w).float()
        wr = w.float() + torch.cat([2.0 * b1 @ a1, 2.0 * b2 @ a2], 0)
        _close(wm, wr, rtol=1e-2, atol=1e-2)
    g = torch.randn_like(y)
    (y.float() * g.float()).sum().backward()
    # reference
    xr = x.detach().float().requires_grad_(True)
    a1r, b1r, a2r, b2r = [p.detach().clone().requires_grad_(True) for p in (a1, b1, a2, b2)]
    yr = xr @ w.float().t()
    yr = yr + torch.cat([2.0 * (xr @ a1r.t()) @ b1r.t(), 2.0 * (xr @ a2r.t()) @ b2r.t()], 1)
    (yr * g.float()).sum().backward()
    _close(y, yr)
    _close(x.grad, xr.grad)
    for p, pr in ((a1, a1r), (b1, b1r), (a2, a2r), (b2, b2r)):
        _close(p.grad, pr.grad, rtol=3e-2, atol=3e-2)


def test_linear_lora_mixed_scales_grads():
    """Adapters of one projection with different scales: dA_i = s_i dU_i^T X per adapter (the shared
    zero-filled accumulators and the one-launch scale apply only when the scales agree)."""
    torch.manual_seed(3)
    M, K, N, r = 200, 256, 192, 8
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.nn.Parameter((torch.randn(N, K, device=DEV) / 16).to(torch.bfloat16), requires_grad=False)
    ps = [torch.nn.Parameter(torch.randn(*shp, device=DEV) * 0.05) for shp in ((r, K), (N // 2, r), (r, K), (N // 2, r))]
    grp = ops.LoRAGroup(["q", "v"], [ps[0], ps[2]], [ps[1], ps[3]], [0, N // 2], [2.0, 0.5], N)
    y = ops.linear(x, w, lora=grp)
    g = torch.randn_like(y)
    (y.float() * g.float()).sum().backward()
    pr = [p.detach().clone().requires_grad_(True) for p in ps]
    xr = x.float()
    yr = xr @ w.float().t() + torch.cat([2.0 * (xr @ pr[0].t()) @ pr[1].t(), 0.5 * (xr @ pr[2].t()) @ pr[3].t()], 1)
    (yr * g.float()).sum().backward()
    for p, q in zip(ps, pr):
        _close(p.grad, q.grad, rtol=3e-2, atol=3e-2)


@pytest.mark.parametrize("M", [200, 3000])
def test_linear_lora_direct_grads(M):
    """LoRA backward with .grad buffers in place (ops.FlatParams): the adapter gradients go straight
    into them through the native epilogue (the split-K slabs of dA_all / dB_all summed in a fixed
    order: scaled dA rows, each adapter's dB block) — equal to the autograd-returned gradients,
    accumulating across backwards, and bitwise reproducible; autograd still fires the parameters'
    post-accumulate hooks (parallel.GradSync's bucket readiness) exactly once per backward. Three
    adapters with an uncovered middle block of output rows and two scales."""
    torch.manual_seed(5)
    K, N, r = 256, 384, 8
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.nn.Parameter((torch.randn(N, K, device=DEV) / 16).to(torch.bfloat16), requires_grad=False)
    shapes = ((r, K), (128, r), (r, K), (64, r), (r, K), (128, r))
    base = [torch.randn(*shp, device=DEV) * 0.05 for shp in shapes]
    import importlib

    L = importlib.import_module("rag_tl_domainllm_optimizer_amd.ops.linear")
    g = None
    grads = {}
    for mode in ("returned", "direct", "direct"):
        L.DIRECT_LORA_GRADS = mode == "direct"
        ps = [torch.nn.Parameter(t.clone()) for t in base]
        # adapters on rows [0, 128), [192, 256) and [256, 384): rows [128, 192) have none
        grp = ops.LoRAGroup(["q", "k", "v"], ps[0::2], ps[1::2], [0, 192, 256], [2.0, 2.0, 0.5], N)
        calls = []
        if mode == "direct":
            for p in ps:
                p.grad = torch.zeros_like(p)
                p.register_post_accumulate_grad_hook(calls.append)
        for _ in range(2):
            y = ops.linear(x, w, lora=grp)
            if g is None:
                g = torch.randn_like(y)
            (y.float() * g.float()).sum().backward()
        if mode in grads:  # the second direct run: bitwise the first (no arrival-order sums)
            for a, b in zip(grads[mode], ps):
                assert torch.equal(a, b.grad)
        grads[mode] = [p.grad.clone() for p in ps]
        if mode == "direct":
            assert len(calls) == 2 * len(ps)  # one post-accumulate hook per parameter and backward
    L.DIRECT_LORA_GRADS = True
    for a, b in zip(grads["returned"], grads["direct"]):
        _close(b, a, rtol=1e-4, atol=1e-5)


def test_refresh_lora_batched_matches_per_group():
    """One-launch rebuild of every group's bf16 images (scaled A rows, B blocks) is bitwise the
    per-group torch refresh."""
    torch.manual_seed(4)
    groups, ref_imgs = [], []
    for N, K, ranks, scales in ((192, 256, (8, 8), (2.0, 0.5)), (512, 384, (16,), (2.0,)), (96, 128, (4, 4, 4), (1.0,) * 3)):
        n_each = N // len(ranks)
        a = [torch.nn.Parameter(torch.randn(r, K, device=DEV)) for r in ranks]
        b = [torch.nn.Parameter(torch.randn(n_each, r, device=DEV)) for r in ranks]
        grp = ops.LoRAGroup([f"p{i}" for i in range(len(ranks))], a, b, [i * n_each for i in range(len(ranks))],
                            list(scales), N)
        grp.refresh()
        with torch.no_grad():
            for p in a + b:
                p.mul_(1.7).add_(0.1)  # an "optimizer step"
        groups.append(grp)
    for grp in groups:
        g2 = ops.LoRAGroup(grp.names, grp.a, grp.b, grp.col0, grp.scale, grp.n_out)
        g2.refresh()
        ref_imgs.append((g2.a_pad.clone(), g2.ub.clone()))
    assert ops.refresh_lora_batched(groups, torch.bfloat16)
    torch.cuda.synchronize()
    for grp, (ap, ub) in zip(groups, ref_imgs):
        assert torch.equal(grp.a_pad, ap) and torch.equal(grp.ub, ub)
        assert grp.merged_dirty


@pytest.mark.parametrize("M,N,K", [(96, 16384, 256), (300, 512, 8192)])
def test_linear_lora_deep(M, N, K):
    """Deep shapes: a 16384-wide output (deep dX reduction in the NN GEMM) and an 8192-deep K
    with the LoRA K-extension."""
    torch.manual_seed(2)
    r = 16
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    w = torch.nn.Parameter((torch.randn(N, K, device=DEV) / math.sqrt(K)).to(torch.bfloat16), requires_grad=False)
    a = torch.nn.Parameter(torch.randn(r, K, device=DEV) / math.sqrt(K))
    b = torch.nn.Parameter(torch.randn(N, r, device=DEV) * 0.05)
    grp = ops.LoRAGroup(["x"], [a], [b], [0], [2.0], N)
    y = ops.linear(x, w, lora=grp)
    g = torch.randn_like(y)
    (y.float() * g.float()).sum().backward()
    xr = x.detach().float().requires_grad_(True)
    ar, br = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    yr = xr @ w.float().t() + 2.0 * (xr @ ar.t()) @ br.t()
    (yr * g.float()).sum().backward()
    _close(y, yr)
    _close(x.grad, xr.grad)
    _close(a.grad, ar.grad, rtol=3e-2, atol=3e-2)
    _close(b.grad, br.grad, rtol=3e-2, atol=3e-2)
    dy = torch.randn(M, N, device=DEV, dtype=torch.bfloat16)
    _close(ops.gemm_nn(dy, w), dy.float() @ w.float())


@pytest.mark.parametrize("M", [300, 1100])
def test_linear_swiglu_lora_autograd(M):
    """Training SwiGLU projection: one GEMM writes silu(g) * u and keeps the [gate | up]
    pre-activation (epilogue), the LoRA K-extension rows follow the gate / up tile mapping, the
    backward runs the SwiGLU derivative on the kept pre-activation."""
    torch.manual_seed(4)
    K, F, r = 256, 384, 8
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    w = torch.nn.Parameter((torch.randn(2 * F, K, device=DEV) / 16).to(torch.bfloat16), requires_grad=False)
    a = torch.nn.Parameter(torch.randn(r, K, device=DEV) * 0.05)
    b = torch.nn.Parameter(torch.randn(2 * F, r, device=DEV) * 0.05)
    grp = ops.LoRAGroup(["gu"], [a], [b], [0], [2.0], 2 * F)
    y = ops.linear(x, w, act="swiglu", lora=grp)
    assert y.shape == (M, F)
    g = torch.randn_like(y)
    (y.float() * g.float()).sum().backward()
    xr = x.detach().float().requires_grad_(True)
    ar, br = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    pre = xr @ w.float().t() + 2.0 * (xr @ ar.t()) @ br.t()
    yr = torch.nn.functional.silu(pre[:, :F]) * pre[:, F:]
    (yr * g.float()).sum().backward()
    _close(y, yr)
    _close(x.grad, xr.grad)
    _close(a.grad, ar.grad, rtol=3e-2, atol=3e-2)
    _close(b.grad, br.grad, rtol=3e-2, atol=3e-2)


@pytest.mark.parametrize("M,K", [(9632, 4096), (700, 14336)])
def test_lora_narrow_split(M, K):
    """U = X A_pad^T / dU = dY UB with the reduction split over workgroups (fp32 partials)."""
    from rag_tl_domainllm_optimizer_amd.ops.linear import _narrow

    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    ap = (torch.randn(64, K, device=DEV) / 64).to(torch.bfloat16)
    ub = (torch.randn(K, 64, device=DEV) / 64).to(torch.bfloat16)
    for ns in (1, 0, 7):
        _close(_narrow(x, ap, ops.ROW, ns), x.float() @ ap.float().t())
        _close(_narrow(x, ub, ops.KMAJ, ns), x.float() @ ub.float())


def test_linear_lora_dropout():
    """PEFT lora_dropout: the adapter sees drop(X); dX / dA follow the same mask."""
    torch.manual_seed(3)
    M, K, N, r, p = 300, 256, 192, 8, 0.25
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    w = torch.nn.Parameter((torch.randn(N, K, device=DEV) / 16).to(torch.bfloat16), requires_grad=False)
    a = torch.nn.Parameter(torch.randn(r, K, device=DEV) * 0.05)
    b = torch.nn.Parameter(torch.randn(N, r, device=DEV) * 0.05)
    grp = ops.LoRAGroup(["x"], [a], [b], [0], [2.0], N, dropout=p)
    torch.manual_seed(11)
    y = ops.linear(x, w, lora=grp)
    # recover the mask the op drew (same seed, same draw) and check against the masked reference
    torch.manual_seed(11)
    keep = torch.empty(M, K, device=DEV).bernoulli_(1 - p)
    m = (keep / (1 - p)).to(torch.bfloat16).float()
    g = torch.randn_like(y)
    (y.float() * g.float()).sum().backward()
    xr = x.detach().float().requires_grad_(True)
    ar, br = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    yr = xr @ w.float().t() + 2.0 * ((xr * m) @ ar.t()) @ br.t()
    (yr * g.float()).sum().backward()
    _close(y, yr)
    _close(x.grad, xr.grad)
    _close(a.grad, ar.grad, rtol=3e-2, atol=3e-2)
    _close(b.grad, br.grad, rtol=3e-2, atol=3e-2)


@pytest.mark.parametrize("threads", [256, 512])
@pytest.mark.parametrize("H,ns", [(4096, 8), (4096, 5), (5120, 8), (5120, 6)])
def test_norm_split_k_slabs(H, ns, threads):
    """Decode-batch RMSNorm that also reduces the producing GEMM's split-K slabs (256 or 512 threads
    per row; H = 5120: 640 threads) against the fp32 reference: h = bf16(bf16(sum slabs) + residual),
    y = RMSNorm(h) w."""
    B = 256
    slabs = torch.randn(ns, B, H, device=DEV) * 0.2
    r = torch.randn(B, H, device=DEV, dtype=torch.bfloat16)
    w = (1 + 0.1 * torch.randn(H, device=DEV)).to(torch.bfloat16)
    with ops.tuning(norm_slab_threads=threads):
        y, h = ops.rms_norm(ops.SplitK(slabs, ns, B, H, torch.bfloat16), w, 1e-5, r)
    hr = (slabs.sum(0).to(torch.bfloat16).float() + r.float()).to(torch.bfloat16).float()
    yr = hr * torch.rsqrt(hr.pow(2).mean(-1, keepdim=True) + 1e-5) * w.float()
    _close(h, hr)
    _close(y, yr)


@pytest.mark.parametrize("H", [384, 768, 4096, 5120])
@pytest.mark.parametrize("layernorm", [False, True])
def test_norm(H, layernorm):
    T = 67
    x = torch.randn(T, H, device=DEV, dtype=torch.bfloat16)
    r = torch.randn(T, H, device=DEV, dtype=torch.bfloat16)
    w = (1 + 0.1 * torch.randn(H, device=DEV)).to(torch.bfloat16)
    b = (0.1 * torch.randn(H, device=DEV)).to(torch.bfloat16) if layernorm else None
    y, h, rstd, mean = ops.native().norm_fwd(layernorm, x, r, w, b, 1e-5)
    yr, hr, rstdr, meanr = ref.norm(x, w, b, 1e-5, r, layernorm)
    _close(y, yr)
    assert torch.equal(h, hr)
    # backward through the autograd path
    xg = x.clone().requires_grad_(True)
    rg = r.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    if layernorm:
        y1, h1 = ops.layer_norm(xg, wg, b, 1e-5, rg)
    else:
        y1, h1 = ops.rms_norm(xg, wg, 1e-5, rg)
    gy, gh = torch.randn_like(y1), torch.randn_like(h1)
    (y1.float() * gy.float()).sum().add((h1.float() * gh.float()).sum()).backward()
    xf = x.float().requires_grad_(True)
    rf = r.float().requires_grad_(True)
    wf = w.float().requires_grad_(True)
    hf = xf + rf
    if layernorm:
        yf = torch.nn.functional.layer_norm(hf, (H,), wf, b.float(), 1e-5)
    else:
        yf = hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + 1e-5) * wf
    (yf * gy.float()).sum().add((hf * gh.float()).sum()).backward()
    _close(xg.grad, xf.grad)
    _close(rg.grad, rf.grad)
    _close(wg.grad, wf.grad, rtol=3e-2, atol=5e-2)


def test_rope_and_cache():
    B, S, Hq, Hkv, D = 2, 5, 4, 2, 128
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device=DEV, dtype=torch.bfloat16)
    cos, sin = ref.rope_tables(D, 64, device=DEV)
    pos = (torch.arange(S, device=DEV).repeat(B) + 3).int()
    kc = torch.zeros(B, Hkv, 16, D, device=DEV, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    slot = torch.tensor([2, 7], device=DEV, dtype=torch.int32)
    expect = ref.rope_qkv(qkv, pos, cos, sin, Hq, Hkv, D)
    got = ops.rope_qkv_(qkv.clone(), pos, cos, sin, Hq, Hkv, D, S=S, k_cache=kc, v_cache=vc, slot_base=slot)
    _close(got, expect, rtol=1e-2, atol=1e-2)
    k = expect[:, Hq * D:(Hq + Hkv) * D].reshape(B, S, Hkv, D)
    v = expect[:, (Hq + Hkv) * D:].reshape(B, S, Hkv, D)
    for b in range(B):
        s0 = int(slot[b])
        _close(kc[b, :, s0:s0 + S], k[b].transpose(0, 1), rtol=1e-2, atol=1e-2)
        assert torch.equal(vc[b, :, s0:s0 + S], v[b].transpose(0, 1))
    # inverse rotation recovers the input
    back = ops.rope_qkv_(got.clone(), pos, cos, sin, Hq, Hkv, D, sign=-1.0)
    _close(back, qkv, rtol=2e-2, atol=2e-2)


def test_swiglu():
    gu = torch.randn(33, 2 * 1024, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    y = ops.swiglu(gu)
    gy = torch.randn_like(y)
    (y.float() * gy.float()).sum().backward()
    gf = gu.detach().float().requires_grad_(True)
    yf = torch.nn.functional.silu(gf[:, :1024]) * gf[:, 1024:]
    (yf * gy.float()).sum().backward()
    _close(y, yf)
    _close(gu.grad, gf.grad)


def test_embed():
    table = torch.randn(1000, 256, device=DEV, dtype=torch.bfloat16)
    ptable = torch.randn(64, 256, device=DEV, dtype=torch.bfloat16)
    ids = torch.randint(0, 1000, (3, 17), device=DEV)
    pids = torch.randint(0, 64, (3, 17), device=DEV)
    out = ops.embedding(table, ids, ptable, pids)
    _close(out, (table[ids].float() + ptable[pids].float()), rtol=1e-2, atol=1e-2)


def test_embed_grad_fixed_order():
    """Trainable table (full fine-tuning): the gradient is the per-id sum of the output gradient rows
    (fp32 oracle: index_add), summed in a fixed order — two backwards give the same bits."""
    torch.manual_seed(2)
    V, H = 500, 384
    ids = torch.randint(0, V, (7, 300), device=DEV)
    ids[:, :50] = 3  # a heavily repeated id
    g = torch.randn(7, 300, H, device=DEV).to(torch.bfloat16)
    grads = []
    for _ in range(2):
        table = torch.randn(V, H, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0)).to(
            torch.bfloat16).requires_grad_(True)
        out = ops.embedding(table, ids)
        (out.float() * g.float()).sum().backward()
        grads.append(table.grad.clone())
    assert torch.equal(grads[0], grads[1])
    expect = torch.zeros(V, H, device=DEV).index_add_(0, ids.reshape(-1), g.reshape(-1, H).float())
    _close(grads[0], expect, rtol=1e-2, atol=2e-2)


@pytest.mark.parametrize("layernorm", [False, True])
def test_norm_weight_grad_fixed_order(layernorm):
    """RMSNorm / LayerNorm weight (and bias) gradients over many rows per workgroup: per-workgroup
    partial rows summed in a fixed order — equal to the fp32 oracle and bitwise repeatable."""
    torch.manual_seed(3)
    T, H = 5000, 4096
    x = torch.randn(T, H, device=DEV, dtype=torch.bfloat16)
    w = (1 + 0.1 * torch.randn(H, device=DEV)).to(torch.bfloat16)
    b = (0.1 * torch.randn(H, device=DEV)).to(torch.bfloat16) if layernorm else None
    gy = torch.randn(T, H, device=DEV).to(torch.bfloat16)
    runs = []
    for _ in range(2):
        wg = w.clone().requires_grad_(True)
        bg = b.clone().requires_grad_(True) if layernorm else None
        y, _ = ops.layer_norm(x, wg, bg, 1e-5) if layernorm else ops.rms_norm(x, wg, 1e-5)
        (y.float() * gy.float()).sum().backward()
        runs.append((wg.grad.clone(), bg.grad.clone() if layernorm else None))
    assert torch.equal(runs[0][0], runs[1][0])
    if layernorm:
        assert torch.equal(runs[0][1], runs[1][1])
    wf = w.float().requires_grad_(True)
    bf = b.float().requires_grad_(True) if layernorm else None
    xf = x.float()
    yf = torch.nn.functional.layer_norm(xf, (H,), wf, bf, 1e-5) if layernorm else \
        xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5) * wf
    (yf * gy.float()).sum().backward()
    _close(runs[0][0], wf.grad, rtol=3e-2, atol=0.5)
    if layernorm:
        _close(runs[0][1], bf.grad, rtol=3e-2, atol=0.5)


def _qkv(B, S, Hq, Hkv, D):
    return torch.randn(B * S, (Hq + 2 * Hkv) * D, device=DEV, dtype=torch.bfloat16)


@pytest.mark.parametrize("S,causal,window,left", [(64, True, 0, False), (200, True, 0, True), (384, True, 100, False),
                                                  (130, False, 0, False)])
def test_flash_fwd_bwd(S, causal, window, left):
    B, Hq, Hkv, D = 2, 8, 2, 128
    qkv = _qkv(B, S, Hq, Hkv, D)
    kv_start = torch.tensor([0, 37], device=DEV, dtype=torch.int32) if left else None
    x = qkv.clone().requires_grad_(True)
    o = ops.flash_attention_qkv(x, B, S, Hq, Hkv, D, causal, window, kv_start=kv_start)
    go = torch.randn_like(o)
    (o.float() * go.float()).sum().backward()
    xr = qkv.float().requires_grad_(True)
    q, k, v = xr[:, :Hq * D], xr[:, Hq * D:(Hq + Hkv) * D], xr[:, (Hq + Hkv) * D:]
    orf, lse = ref.attention(q, k, v, B, S, S, Hq, Hkv, D, causal, window, None, kv_start)
    valid = torch.ones(B * S, dtype=torch.bool, device=DEV)
    if left:
        valid = (torch.arange(S, device=DEV)[None, :] >= kv_start[:, None]).reshape(-1)
    _close(o[valid], orf[valid])
    (orf[valid].float() * go[valid].float()).sum().backward()
    gx = x.grad.float()
    gr = xr.grad
    _close(gx[:, :Hq * D][valid], gr[:, :Hq * D][valid], rtol=3e-2, atol=3e-2)
    _close(gx[:, Hq * D:], gr[:, Hq * D:], rtol=3e-2, atol=3e-2)


@pytest.mark.parametrize("S,window,left", [(1, 0, False), (31, 0, True), (77, 0, False), (301, 0, True),
                                           (301, 100, False), (700, 0, True)])
@pytest.mark.parametrize("Hq,Hkv", [(32, 8), (16, 16), (16, 8)])
def test_flash_fwd_head_packed_bitwise(S, window, left, Hq, Hkv):
    """The short-sequence causal forward tiles — head-packed (4 query heads x 32 positions per
    workgroup, GQA-4) and 64 positions of one head (other groupings) — write bitwise the output and
    log-sum-exp of the 128-position-per-head form."""
    B, D = 3, 128
    torch.manual_seed(S + window)
    qkv = _qkv(B, S, Hq, Hkv, D)
    q, k, v = qkv[:, :Hq * D], qkv[:, Hq * D:(Hq + Hkv) * D], qkv[:, (Hq + Hkv) * D:]
    kv_start = torch.tensor([0, min(37, S - 1), min(5, S - 1)], device=DEV, dtype=torch.int32) if left else None
    scale = 1.0 / math.sqrt(D)
    outs = []
    for maxs in (4096, 0):
        with ops.tuning(attn_fwd_hp_maxs=maxs):
            outs.append(ops.native().attn_fwd(q, k, v, B, S, S, Hq, Hkv, D, True, window, scale, kv_start, None, None,
                                              0, True))
    (o1, l1), (o2, l2) = outs
    assert torch.equal(o1, o2)
    assert torch.equal(l1, l2)


@pytest.mark.parametrize("S,window,left", [(31, 0, True), (301, 0, True), (301, 100, False), (700, 0, False)])
def test_flash_bwd_dq_head_packed_bitwise(S, window, left):
    """The head-packed dQ kernel (4 query heads x 16 positions per workgroup, GQA-4 causal) gives
    bitwise the gradients of the 64-position-per-head form (dK / dV are the same kernel)."""
    B, Hq, Hkv, D = 3, 32, 8, 128
    torch.manual_seed(S + 3 * window)
    qkv = _qkv(B, S, Hq, Hkv, D)
    kv_start = torch.tensor([0, min(37, S - 1), 5], device=DEV, dtype=torch.int32) if left else None
    go = torch.randn(B * S, Hq * D, device=DEV, dtype=torch.bfloat16)
    grads = []
    for maxs in (4096, 0):
        with ops.tuning(attn_dq_hp_maxs=maxs):
            x = qkv.clone().requires_grad_(True)
            o = ops.flash_attention_qkv(x, B, S, Hq, Hkv, D, True, window, kv_start=kv_start)
            (o.float() * go.float()).sum().backward()
            grads.append(x.grad.clone())
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("S,Hq,Hkv,D,window,left,hp", [(301, 32, 8, 128, 0, True, 1), (301, 32, 8, 128, 0, True, 0),
                                                       (700, 32, 8, 128, 100, False, 1), (301, 12, 12, 64, 0, True, 1),
                                                       (97, 8, 8, 128, 0, False, 1), (1100, 16, 4, 128, 0, True, 1)])
def test_flash_heaviest_first_order_bitwise(S, Hq, Hkv, D, window, left, hp):
    """attn_lpt (causal grids dispatch their heaviest tiles first within each XCD) only permutes
    which workgroup runs when: forward output / LSE and every gradient are bitwise the tile-order
    launch's, on the head-packed, 64-position, 128-position and D = 64 forms and both dQ forms."""
    B = 3
    torch.manual_seed(S + Hq + D + window)
    qkv = _qkv(B, S, Hq, Hkv, D)
    kv_start = torch.tensor([0, min(37, S - 1), 5], device=DEV, dtype=torch.int32) if left else None
    go = torch.randn(B * S, Hq * D, device=DEV, dtype=torch.bfloat16)
    maxs = 4096 if hp else 0
    res = []
    for lpt in (0, 1 << 30):  # tile order / heaviest first whatever the grid size
        with ops.tuning(attn_lpt=lpt, attn_fwd_hp_maxs=maxs, attn_dq_hp_maxs=maxs):
            x = qkv.clone().requires_grad_(True)
            o = ops.flash_attention_qkv(x, B, S, Hq, Hkv, D, True, window, kv_start=kv_start)
            (o.float() * go.float()).sum().backward()
            res.append((o.detach().clone(), x.grad.clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    # and the heaviest-first launch still matches the fp32 oracle
    q, k, v = qkv[:, :Hq * D], qkv[:, Hq * D:(Hq + Hkv) * D], qkv[:, (Hq + Hkv) * D:]
    orf, _ = ref.attention(q, k, v, B, S, S, Hq, Hkv, D, True, window, None, kv_start, None, None, 0)
    rows = torch.ones(B, S, dtype=torch.bool, device=DEV)
    if kv_start is not None:
        for b in range(B):
            rows[b, :int(kv_start[b])] = False  # query rows left of a row's start are padding
    rows = rows.reshape(-1)
    _close(res[1][0][rows], orf[rows])


@pytest.mark.parametrize("D,H", [(32, 12), (64, 12)])
def test_encoder_attention_relbias(D, H):
    B, S = 3, 70
    qkv = _qkv(B, S, H, H, D)
    q, k, v = qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:]
    lens = torch.tensor([70, 31, 5], device=DEV, dtype=torch.int32)
    L = 128
    lut = torch.randn(H, 2 * L - 1, device=DEV) * 0.5
    o = ops.attention(q, k, v, B, S, S, H, H, D, False, kv_len=lens, rel_bias_lut=lut, rb_L=L)
    orf, _ = ref.attention(q, k, v, B, S, S, H, H, D, False, 0, None, None, lens, lut, L)
    _close(o, orf)


@pytest.mark.parametrize("B,Hq,Hkv,D,Smax", [(3, 32, 8, 128, 300), (64, 32, 8, 128, 520), (2, 12, 12, 64, 90)])
def test_decode_attention(B, Hq, Hkv, D, Smax):
    q = torch.randn(B, (Hq + 2 * Hkv) * D, device=DEV, dtype=torch.bfloat16)
    kc = torch.randn(B, Hkv, Smax, D, device=DEV, dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    lens = torch.randint(1, Smax + 1, (B,), device=DEV, dtype=torch.int32)
    start = (torch.rand(B, device=DEV) * lens.float() * 0.3).int()
    for window in (0, 50):
        o = ops.decode_attention(q, kc, vc, lens, Hq, start, window)
        orf = ref.decode_attention(q, kc, vc, lens, Hq, start, window)
        _close(o, orf)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_logprob_entropy(dtype):
    T, V = 45, 32000
    logits = (torch.randn(T, V, device=DEV) * 3).to(dtype).requires_grad_(True)
    tgt = torch.randint(0, V, (T,), device=DEV)
    tgt[3] = -100
    lp, ent = ops.token_logprobs(logits, tgt, 1 / 0.7)
    g1, g2 = torch.randn(T, device=DEV), torch.randn(T, device=DEV)
    ((lp * g1).sum() + (ent * g2).sum()).backward()
    lf = logits.detach().float().requires_grad_(True)
    lpr, entr, _, _ = ref.logprob(lf, tgt, 1 / 0.7)
    ((lpr * g1).sum() + (entr * g2).sum()).backward()
    _close(lp, lpr, rtol=1e-3, atol=1e-3)
    _close(ent, entr, rtol=1e-3, atol=1e-3)
    _close(logits.grad, lf.grad, rtol=2e-2, atol=1e-4)


def test_sampler_greedy_and_topk1():
    logits = torch.randn(16, 32000, device=DEV, dtype=torch.bfloat16)
    tok, lp = ops.sample(logits, 1.0, greedy=True)
    assert torch.equal(tok, logits.float().argmax(-1))
    off = torch.zeros(1, dtype=torch.long, device=DEV)
    tok2, lp2 = ops.sample(logits, 1 / 0.7, top_k=1, seed=5, offset=off)
    # top-1 sampling returns A maximum (bf16 rows can hold tied maxima; argmax picks the first)
    lf = logits.float()
    assert torch.equal(lf.gather(1, tok2[:, None])[:, 0], lf.max(-1).values)
    lpr, _, _, _ = ref.logprob(logits, tok2, 1 / 0.7)
    _close(lp2, lpr, rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sampler_distribution_and_filters(dtype):
    V, B = 8, 20000
    base = torch.tensor([2.0, 1.5, 1.0, 0.5, 0.0, -0.5, -1.0, -3.0], device=DEV)
    logits = base.repeat(B, 1).to(dtype)
    off = torch.zeros(1, dtype=torch.long, device=DEV)
    tok, _ = ops.sample(logits, 1.0, seed=123, offset=off)
    freq = torch.bincount(tok, minlength=V).float() / B
    p = torch.softmax(base, -1)
    assert (freq - p).abs().max().item() < 0.02
    tok, _ = ops.sample(logits, 1.0, top_k=3, seed=7, offset=off)
    assert int(tok.max()) <= 2
    freq = torch.bincount(tok, minlength=V).float() / B
    pk = torch.softmax(base[:3], -1)
    assert (freq[:3] - pk).abs().max().item() < 0.02
    # top-p 0.6: smallest prefix with mass >= 0.6
    tok, _ = ops.sample(logits, 1.0, top_p=0.6, seed=9, offset=off)
    keep = ref.filter_logits(base[None], 1.0, 0, 0.6)[0]
    assert bool(keep[tok].all())
    # different offsets give different draws
    off1 = torch.ones(1, dtype=torch.long, device=DEV)
    t0, _ = ops.sample(logits[:256], 1.0, seed=3, offset=off)
    t1, _ = ops.sample(logits[:256], 1.0, seed=3, offset=off1)
    assert not torch.equal(t0, t1)


@pytest.mark.parametrize("M,N,K", [(64, 28672, 4096), (16, 4096, 14336), (3, 32000, 4096), (64, 6144, 4096),
                                   (1, 1152, 384), (50, 64, 4096)])
def test_decode_gemm_split_k_repeated(M, N, K):
    # split-K with in-launch last-arriver reduction; tickets must re-arm across launches
    a = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16) / math.sqrt(K)
    b = torch.randn(N, device=DEV, dtype=torch.bfloat16)
    ref_ = ref.gemm(a, w, bias=b, act=4, out_f32=True)
    for _ in range(3):
        _close(ops.gemm(a, w, bias=b, act=4), ref_)
    u = torch.randn(M, 64, device=DEV, dtype=torch.bfloat16)
    ub = torch.randn(N, 64, device=DEV, dtype=torch.bfloat16) * 0.1
    _close(ops.gemm(a, w, u, ub, out_f32=True), ref.gemm(a, w, u, ub, out_f32=True), rtol=5e-3, atol=5e-3)


@pytest.mark.parametrize("M,N,K", [(1, 6144, 4096), (5, 4096, 14336), (16, 1040, 448), (12, 2048, 1024),
                                   (1, 28672, 4096)])
def test_decode_gemm_shuffled_weight_bitwise(M, N, K):
    """The tile-ordered weight image feeds the same MFMAs in the same order: at the same split-K the
    results are bitwise equal to the row-major launch, with the in-GEMM norm, SwiGLU pair and
    residual epilogues (the default splits differ per layout: close, not equal)."""
    C = ops.native()
    a = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16) / math.sqrt(K)
    ws = C.shuffle_decode_weight(w)
    # the image is a permutation of w (every element kept)
    assert torch.equal(torch.sort(ws.flatten().float())[0], torch.sort(w.flatten().float())[0])
    res = torch.randn(M, N, device=DEV, dtype=torch.bfloat16)
    for kw in (dict(), dict(norm_eps=1e-5), dict(residual=res), dict(act=ops.ACT_SWIGLU, norm_eps=1e-5)):
        if kw.get("act") == ops.ACT_SWIGLU and N % 64:
            continue
        args = (None, None, None, kw.get("act", 0), False, None, kw.get("residual"), kw.get("norm_eps", 0.0))
        try:
            for split in (0, 2):  # 0: each layout's own split heuristic; forced: the same split-K
                C.set_tuning({"decode_split": split})
                base = C.gemm(a, w, *args)
                for _ in range(2):  # split-K tickets re-arm
                    got = C.gemm(a, ws, *args, True)
                    if split:
                        assert torch.equal(got, base), kw
                    else:
                        _close(got, base, rtol=1e-2, atol=1e-2)
        finally:
            C.set_tuning({"decode_split": 0})
    with pytest.raises(RuntimeError):
        C.gemm(torch.randn(65, K, device=DEV, dtype=torch.bfloat16), ws, w_shuffled=True)


def test_varlen_rows_scatter_gather_autograd():
    """Native varlen scatter (one pass, zero pad rows) / gather and their autograd duals equal the
    index_copy / index_select forms exactly (pure data movement)."""
    R, N, W = 1000, 700, 392
    idx = torch.randperm(R, device=DEV)[:N].sort().values
    inv = ops.packed_inverse(idx, R)
    assert int((inv >= 0).sum()) == N and torch.equal(inv[idx].long(), torch.arange(N, device=DEV))
    base = torch.randn(N, W + 8, device=DEV, dtype=torch.bfloat16)
    src = base[:, :W].detach().requires_grad_(True)  # row stride != W
    grid = ops.scatter_rows(src, idx, inv, R)
    assert torch.equal(grid, torch.zeros(R, W, device=DEV, dtype=torch.bfloat16).index_copy(0, idx, src.detach()))
    g = torch.randn_like(grid)
    grid.backward(g)
    assert torch.equal(src.grad, g.index_select(0, idx))
    full = torch.randn(R, W, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    o = ops.gather_rows(full, idx, inv)
    assert torch.equal(o, full.detach().index_select(0, idx))
    h = torch.randn_like(o)
    o.backward(h)
    assert torch.equal(full.grad, torch.zeros_like(full).index_copy(0, idx, h))


def test_sampler_bf16_topk_topp_vocab():
    # LDS fast path on a realistic vocabulary: only top-k survivors are ever drawn
    B, V = 64, 32000
    logits = (torch.randn(B, V, device=DEV) * 2).to(torch.bfloat16)
    off = torch.zeros(1, dtype=torch.long, device=DEV)
    tok, lp = ops.sample(logits, 1 / 0.7, top_k=50, top_p=0.9, seed=11, offset=off)
    keep = ref.filter_logits(logits.float(), 1 / 0.7, 50, 0.9)
    assert bool(keep.gather(1, tok[:, None]).all())
    lpr, _, _, _ = ref.logprob(logits, tok, 1 / 0.7)
    _close(lp, lpr, rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("top_k,top_p", [(50, 1.0), (50, 0.9), (1000, 0.95), (7, 0.5)])
def test_sampler_search_path_matches_f32_kernel(top_k, top_p):
    """The bf16 binary-search top-k sampler keeps the same set and uses the same Philox stream as the
    fp32 radix kernel, so both draw the same tokens (top-p boundary rounding may flip a rare row)."""
    B, V = 64, 32000
    logits = (torch.randn(B, V, device=DEV) * 2).to(torch.bfloat16)
    off = torch.full((1,), 3, dtype=torch.long, device=DEV)
    tb, lb = ops.sample(logits, 1 / 0.7, top_k=top_k, top_p=top_p, seed=21, offset=off)
    tf, lf = ops.sample(logits.float(), 1 / 0.7, top_k=top_k, top_p=top_p, seed=21, offset=off)
    assert (tb == tf).float().mean().item() >= 0.95
    keep = ref.filter_logits(logits.float(), 1 / 0.7, top_k, top_p)
    assert keep.gather(1, tb[:, None]).float().mean().item() >= 0.98
    _close(lb, ref.logprob(logits, tb, 1 / 0.7)[0], rtol=2e-3, atol=2e-3)


def test_sampler_search_path_tie_plateau():
    # > 2048 tokens tied at the k-th value: survivors overflow the list, the draw falls back to the keys
    V = 32000
    logits = torch.zeros(4, V, device=DEV, dtype=torch.bfloat16)
    logits[:, :3] = 5.0
    off = torch.zeros(1, dtype=torch.long, device=DEV)
    tok, _ = ops.sample(logits, 1.0, top_k=10, seed=2, offset=off)
    assert bool((tok >= 0).all()) and bool((tok < V).all())
    tok, _ = ops.sample(logits, 1.0, top_k=3, seed=2, offset=off)
    assert bool((tok < 3).all())


def test_adamw_matches_torch():
    n = 10007
    p0 = torch.randn(n, device=DEV)
    params = [torch.nn.Parameter(p0[:5000].clone()), torch.nn.Parameter(p0[5000:].clone())]
    flat = ops.FlatParams(params)
    opt = ops.FusedAdamW(flat, lr=1e-2, weight_decay=0.01, max_grad_norm=0.5)
    tp = [torch.nn.Parameter(p0[:5000].clone()), torch.nn.Parameter(p0[5000:].clone())]
    topt = torch.optim.AdamW(tp, lr=1e-2, weight_decay=0.01)
    for _ in range(3):
        g = torch.randn(n, device=DEV)
        opt.zero_grad()
        params[0].grad.copy_(g[:5000])
        params[1].grad.copy_(g[5000:])
        opt.step()
        tp[0].grad = g[:5000].clone()
        tp[1].grad = g[5000:].clone()
        torch.nn.utils.clip_grad_norm_(tp, 0.5)
        topt.step()
    _close(params[0].detach(), tp[0].detach(), rtol=1e-4, atol=1e-5)
    _close(params[1].detach(), tp[1].detach(), rtol=1e-4, atol=1e-5)
    # non-finite gradients skip the update
    before = flat.data.clone()
    opt.zero_grad()
    params[0].grad.fill_(float("nan"))
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(before, flat.data) and int(opt.skipped) == 1


def test_pool_topk_ivf_gae():
    x = torch.randn(4, 33, 384, device=DEV, dtype=torch.bfloat16)
    lens = torch.tensor([33, 10, 1, 20], device=DEV, dtype=torch.int32)
    _close(ops.pool_normalize(x, lens), ref.pool_norm(x, lens), rtol=1e-3, atol=1e-3)
    scores = torch.randn(5, 100003, device=DEV)
    v, i = ops.topk(scores, 10)
    vr, ir = torch.topk(scores, 10)
    assert torch.equal(i, ir) and torch.allclose(v, vr)
    # ivf scan over 3 capacity-padded lists (list 0 holds 7 of its 10 slots), ip and l2
    d = 64
    vecs = torch.randn(50, d, device=DEV, dtype=torch.bfloat16)
    ids = torch.arange(50, device=DEV) + 1000
    lstart = torch.tensor([0, 10, 35], device=DEV, dtype=torch.int32)
    lsize = torch.tensor([7, 25, 15], device=DEV, dtype=torch.int32)
    sq = vecs.float().pow(2).sum(-1)
    q = torch.randn(2, d, device=DEV, dtype=torch.bfloat16)
    probes = torch.tensor([[2, 0], [1, 2]], device=DEV, dtype=torch.int32)
    for l2 in (False, True):
        cand, cid = ops.ivf_scan(q, probes, lstart, lsize, vecs, ids, 32, sq, l2)
        full = q.float() @ vecs.float().t()
        if l2:
            full = 2 * full - sq[None] - q.float().pow(2).sum(-1, keepdim=True)
        for qi in range(2):
            for p in range(2):
                L = int(probes[qi, p])
                a, n = int(lstart[L]), min(int(lsize[L]), 32)
                _close(cand[qi, p * 32:p * 32 + n], full[qi, a:a + n], rtol=1e-2, atol=3e-2)
                assert torch.equal(cid[qi, p * 32:p * 32 + n], ids[a:a + n])
                assert bool((cid[qi, p * 32 + n:(p + 1) * 32] == -1).all())
                assert bool(torch.isinf(cand[qi, p * 32 + n:(p + 1) * 32]).all())
    r = torch.randn(3, 17, device=DEV)
    val = torch.randn(3, 17, device=DEV)
    mask = (torch.arange(17, device=DEV)[None] < torch.tensor([17, 9, 1], device=DEV)[:, None]).float()
    a1, r1 = ops.gae(r, val, mask, 0.99, 0.95)
    a2, r2 = ref.gae(r, val, mask, 0.99, 0.95)
    _close(a1, a2, rtol=1e-4, atol=1e-5)
    _close(r1, r2, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("B,Hq,Hkv,D,Smax,rot,window", [(1, 32, 8, 128, 456, True, 0), (64, 32, 8, 128, 456, True, 0),
                                                        (3, 8, 8, 64, 200, False, 0), (5, 8, 2, 32, 300, True, 64),
                                                        (2, 16, 2, 128, 64, True, 0),
                                                        # B * Hkv < 256, D = 128: the 8-wave MFMA kernel (window; G = 2)
                                                        (3, 32, 8, 128, 300, True, 100), (3, 16, 8, 128, 300, True, 0),
                                                        (1, 40, 40, 128, 456, True, 0),  # G = 1 (Llama-2-13B)
                                                        # D = 128 past 1024 slots at small batch: the 8-wave MFMA
                                                        # kernel over key partitions merged by the last arriver
                                                        (2, 32, 8, 128, 1500, True, 0), (1, 32, 8, 128, 4096, True, 0),
                                                        (1, 32, 8, 128, 8200, True, 4096), (2, 40, 40, 128, 2100, True, 0),
                                                        # B * Hkv >= 256, below and at the one-wave threshold
                                                        # (decode_mw_bh = 320): the MFMA kernel at 1 wave
                                                        # (320 pairs, G = 4) and at 4 waves (256 pairs, G = 8
                                                        # and G = 1)
                                                        (40, 32, 8, 128, 300, True, 64), (32, 64, 8, 128, 200, True, 0),
                                                        (16, 16, 16, 128, 97, False, 0)])
@pytest.mark.parametrize("poison", [False, True])
def test_decode_step_fused(B, Hq, Hkv, D, Smax, rot, window, poison):
    """Fused RoPE + append + attention + in-launch combine == rope_qkv_ + decode_attention.
    ``poison``: the slot being appended and every slot after it hold NaN before the launch (a
    fresh torch.empty cache): masked lanes that re-read the last slot must not see them (0 * NaN)."""
    torch.manual_seed(B + D)
    W = (Hq + 2 * Hkv) * D
    kc = torch.randn(B, Hkv, Smax, D, device=DEV, dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    kv_start = torch.randint(0, 8, (B,), device=DEV, dtype=torch.int32)
    slot = torch.randint(20, Smax - 1, (B,), device=DEV, dtype=torch.int32)
    attn_len = slot + 1
    if poison:
        tail = torch.arange(Smax, device=DEV)[None, None, :, None] >= slot.long()[:, None, None, None]
        kc.masked_fill_(tail, float("nan"))
        vc.masked_fill_(tail, float("nan"))
    pos = (slot - kv_start).to(torch.int32)
    cos, sin = ref.rope_tables(D, 4096, 10000.0, DEV) if rot else (None, None)
    ws = ops.decode_workspace(B, Hq, Hkv, D, Smax, DEV)
    for it in range(3):  # repeated launches: tickets must re-arm
        qkv = torch.randn(B, W, device=DEV, dtype=torch.bfloat16)
        kc2, vc2 = kc.clone(), vc.clone()
        out = ops.decode_step_attention(qkv, kc, vc, slot, attn_len, Hq, pos, cos, sin, kv_start, window,
                                        workspace=ws)
        q_ref = ops.rope_qkv_(qkv.clone(), pos, cos, sin, Hq, Hkv, D, S=1, k_cache=kc2, v_cache=vc2, slot_base=slot)
        o_ref = ref.decode_attention(q_ref, kc2, vc2, attn_len, Hq, kv_start, window, 1.0 / math.sqrt(D))
        assert torch.equal(kc.nan_to_num(), kc2.nan_to_num()) and torch.equal(vc.nan_to_num(), vc2.nan_to_num()), \
            "cache append differs"
        assert torch.isfinite(out).all()
        _close(out, o_ref)
    assert int(ws.tickets.abs().sum()) == 0


def test_quant_fp8_matches_torch_e4m3fn():
    x = (torch.randn(70, 4096, device=DEV) * torch.logspace(-3, 3, 70, device=DEV)[:, None]).to(torch.bfloat16)
    q, s = ops.quantize_fp8(x)
    xf = x.float()
    s_ref = xf.abs().amax(1) / 448.0
    torch.testing.assert_close(s, s_ref, rtol=1e-6, atol=0)
    q_ref = (xf / s_ref[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    # same OCP e4m3fn encoding; the kernel scales by a reciprocal (x * (1/s)) where torch divides,
    # so a few values near a rounding boundary land on the adjacent code
    diff = q != q_ref
    assert diff.float().mean().item() < 5e-3
    assert ((q.int() - q_ref.int()).abs()[diff] <= 1).all()


@pytest.mark.parametrize("M,N,K", [(1, 6144, 4096), (16, 4096, 14336), (64, 1024, 512), (300, 1000, 512),
                                   (2048, 4096, 4096)])
def test_gemm_fp8(M, N, K):
    torch.manual_seed(M)
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).to(torch.bfloat16)
    wq, sw = ops.quantize_fp8(w)
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    b = torch.randn(N, device=DEV, dtype=torch.bfloat16)
    wd = ops.dequantize_fp8(wq, sw)
    xr = x.float() if M <= 64 else ops.dequantize_fp8(*ops.quantize_fp8(x))
    for act in (0, 4):
        y = ops.gemm_fp8(x, wq, sw, b, act)
        yr = ref.apply_act(xr @ wd.t() + b.float(), act)
        _close(y, yr)


def test_model_fp8_generation_gpu():
    from rag_tl_domainllm_optimizer_amd import models
    from rag_tl_domainllm_optimizer_amd.generation import Generator, SamplingParams
    from rag_tl_domainllm_optimizer_amd.models.config import PRESETS

    cfg = PRESETS["tiny-llama"]
    m = models.CausalLM(cfg, device=DEV, dtype=torch.bfloat16, seed=4)
    ids = torch.randint(5, cfg.vocab_size, (2, 150), device=DEV)
    with torch.no_grad():
        ref_h = m(ids).float()
        m.set_fp8(True)
        h = m(ids).float()
    assert ((h - ref_h).abs().max() / ref_h.abs().max()).item() < 0.1
    gen = Generator(m, 2, 200)
    out = gen.generate([list(range(5, 40)), list(range(7, 30))], SamplingParams(max_new_tokens=12, do_sample=False))
    assert out.tokens.shape == (2, 12)
    m.set_fp8(False)


@pytest.mark.parametrize("M", [1, 7, 16, 33, 64])
@pytest.mark.parametrize("F,K", [(512, 256), (14336, 4096)])
def test_gemm_swiglu_pair(M, F, K):
    """SwiGLU fused into the skinny gate/up GEMM (decode) == silu(x g^T) * (x u^T); bf16 and W8."""
    torch.manual_seed(M + F)
    w = (torch.randn(2 * F, K, device=DEV) / math.sqrt(K)).to(torch.bfloat16)
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    g = x.float() @ w[:F].float().t()
    u = x.float() @ w[F:].float().t()
    yr = torch.nn.functional.silu(g) * u
    y = ops.native().gemm(x, w, None, None, None, 5, False, None)
    assert y.shape == (M, F)
    _close(y, yr)
    wq, sw = ops.quantize_fp8(w)
    wd = ops.dequantize_fp8(wq, sw)
    yr8 = torch.nn.functional.silu(x.float() @ wd[:F].t()) * (x.float() @ wd[F:].t())
    _close(ops.native().gemm_fp8(x, None, wq, sw, None, 5, None), yr8)
    # through the layer API (no-grad, GPU)
    with torch.no_grad():
        _close(ops.linear(x, w, act="swiglu"), yr)


@pytest.mark.parametrize("M", [1, 5, 16, 33, 64])
@pytest.mark.parametrize("N,K", [(6144, 4096), (4096, 14336), (512, 256)])
def test_gemm_decode_norm_residual(M, N, K):
    """In-GEMM RMS norm (norm weight folded into W) + residual epilogue == rms_norm -> GEMM -> add."""
    torch.manual_seed(M * 7 + N)
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16) * 3
    lnw = (1 + 0.1 * torch.randn(K, device=DEV)).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).to(torch.bfloat16)
    res = torch.randn(M, N, device=DEV, dtype=torch.bfloat16)
    xn = x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5) * lnw.float()
    yr = xn @ w.float().t() + res.float()
    wf = ops.FoldCache().get(w, lnw)
    y = ops.gemm_decode(x, wf, residual=res, norm_eps=1e-5)
    _close(y, yr)
    # norm only / residual only / swiglu + norm
    _close(ops.gemm_decode(x, wf, norm_eps=1e-5), xn @ w.float().t())
    _close(ops.gemm_decode(x, w, residual=res), x.float() @ w.float().t() + res.float())
    if N % 64 == 0:
        F = N // 2
        g, u = xn @ w[:F].float().t(), xn @ w[F:].float().t()
        _close(ops.gemm_decode(x, wf, act=ops.ACT_SWIGLU, norm_eps=1e-5), torch.nn.functional.silu(g) * u)
    # fp8 weights (W8A16)
    c8 = ops.Fp8Cache()
    q, s = c8.get(wf)
    wd = ops.dequantize_fp8(q, s)
    yr8 = (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)) @ wd.t() + res.float()
    _close(ops.gemm_decode(x, wf, residual=res, norm_eps=1e-5, fp8=c8), yr8)


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("M,N,K,split", [(64, 6144, 4096, 0), (64, 4096, 14336, 8), (33, 28672, 4096, 1),
                                         (64, 4096, 4096, 4), (17, 1152, 384, 0), (64, 32000, 4096, 2),
                                         (48, 4096, 512, 3), (17, 4096, 1024, 0), (40, 6144, 4096, 8)])
def test_m64_kernel_plain_norm_residual_swiglu(M, N, K, split, wide):
    """16 < M <= 64 kernels — the 64-column ring (wide = 0) and the 256-row wide kernel over
    row-major weights (wide = 1, N % 256 == 0) — with every split-K and epilogue (plain, fp32 out,
    in-GEMM RMS norm, residual, SwiGLU pair) against fp32 references; tickets re-arm across launches."""
    C = ops.native()
    C.set_tuning({"m64_split": split, "m64_wide": wide, "wide_split": split})
    try:
        torch.manual_seed(M + N + K)
        x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16) * 2
        w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).to(torch.bfloat16)
        res = torch.randn(M, N, device=DEV, dtype=torch.bfloat16)
        yr = x.float() @ w.float().t()
        for _ in range(2):
            _close(ops.gemm(x, w), yr)
            _close(C.gemm(x, w, None, None, None, 0, False, None), yr)
        _close(C.gemm(x, w, None, None, None, 0, True, None), yr, rtol=1e-4, atol=1e-3)
        rstd = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)
        _close(ops.gemm_decode(x, w, residual=res, norm_eps=1e-5), yr * rstd + res.float())
        if N % 64 == 0:
            F = N // 2
            g, u = (x.float() * rstd) @ w[:F].float().t(), (x.float() * rstd) @ w[F:].float().t()
            _close(ops.gemm_decode(x, w, act=ops.ACT_SWIGLU, norm_eps=1e-5), torch.nn.functional.silu(g) * u)
    finally:
        C.set_tuning({"m64_split": 0, "m64_wide": 1, "wide_split": 0})


@pytest.mark.parametrize("kl", [None, 0.05])
@pytest.mark.parametrize("vclip", [None, 0.2])
@pytest.mark.parametrize("B,T", [(16, 128), (3, 37), (64, 300)])
def test_ppo_loss_fused(B, T, vclip, kl):
    """Fused PPO objective + closed-form gradient == eager autograd of the reference formulas
    (with and without the in-loss k3 reference-KL term)."""
    torch.manual_seed(B * T)
    lp = (torch.randn(B, T, device=DEV) * 0.3 - 2).requires_grad_(True)
    vals = torch.randn(B, T, device=DEV).requires_grad_(True)
    ent = (torch.rand(B, T, device=DEV) * 3).requires_grad_(True)
    old = lp.detach() + torch.randn(B, T, device=DEV) * 0.2
    adv, ret, vold = torch.randn(B, T, device=DEV), torch.randn(B, T, device=DEV), torch.randn(B, T, device=DEV)
    refl = lp.detach() + torch.randn(B, T, device=DEV) * 0.3 if kl else None
    lens = torch.randint(1, T + 1, (B,), device=DEV)
    mask = torch.arange(T, device=DEV)[None] < lens[:, None]
    loss, st = ops.ppo_loss(lp, vals, ent, old, adv, ret, mask, 0.2, 0.5, 0.01, vclip, vold, refl, kl or 0.0)
    (2.0 * loss).backward()
    g = [t.grad.clone() for t in (lp, vals, ent)]
    for t in (lp, vals, ent):
        t.grad = None
    rl, rst = ref.ppo_loss(lp, old, adv, vals, ret, ent, mask.float(), 0.2, 0.5, 0.01, vclip, vold, refl, kl or 0.0)
    (2.0 * rl).backward()
    torch.testing.assert_close(st, rst, rtol=1e-4, atol=1e-5)
    for a, t in zip(g, (lp, vals, ent)):
        torch.testing.assert_close(a, t.grad, rtol=1e-4, atol=1e-6)


def test_ppo_advantages_kernel():
    """Fused token rewards + GAE + whitening == the fp32 oracle (ragged lengths incl. 0 and T)."""
    torch.manual_seed(5)
    B, T = 300, 128
    old, refl, vals = (torch.randn(B, T, device=DEV) for _ in range(3))
    scores = torch.randn(B, device=DEV)
    lens = torch.randint(0, T + 1, (B,), device=DEV)
    lens[0], lens[1] = 0, T
    for whiten in (False, True):
        got = ops.ppo_advantages(old, refl, vals, scores, lens, 0.05, 0.99, 0.95, whiten)
        want = ref.ppo_advantages(old.cpu(), refl.cpu(), vals.cpu(), scores.cpu(), lens.cpu(), 0.05, 0.99, 0.95, whiten)
        for a, b in zip(got, want):
            _close(a.cpu(), b, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("waves", [0, 4, 8, 16])
@pytest.mark.parametrize("M,N,K", [(1, 6144, 4096), (5, 4096, 14336), (16, 4096, 4096), (1, 28672, 4096),
                                   (3, 32000, 4096)])
def test_gemv16_no_split_matches_fp32(M, N, K, waves):
    """Decode GEMV without split-K (M <= 16 over the tile-ordered image, N / 16 >= 256 workgroups):
    in-GEMM RMS norm, residual, SwiGLU pair vs an fp32 PyTorch reference; 4, 8 or 16 waves per row group
    or the automatic choice (tuning gemv16_waves = 0; the SwiGLU pair form stays at 4)."""
    with ops.tuning(gemv16_waves=waves):
        _gemv16_case(M, N, K)


def _gemv16_case(M, N, K):
    torch.manual_seed(M + N)
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16) * 2
    lnw = (1 + 0.1 * torch.randn(K, device=DEV)).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).to(torch.bfloat16)
    res = torch.randn(M, N, device=DEV, dtype=torch.bfloat16)
    wf = ops.FoldCache().get(w, lnw)
    xn = x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5) * lnw.float()
    shuf = ops.ShufCache()
    _close(ops.gemm_decode(x, w, shuf=shuf), x.float() @ w.float().t())
    shuf_f = ops.ShufCache()
    _close(ops.gemm_decode(x, wf, residual=res, norm_eps=1e-5, shuf=shuf_f), xn @ w.float().t() + res.float())
    if N % 32 == 0 and N <= 28672:
        F = N // 2
        g, u = xn @ w[:F].float().t(), xn @ w[F:].float().t()
        _close(ops.gemm_decode(x, wf, act=ops.ACT_SWIGLU, norm_eps=1e-5, shuf=shuf_f),
               torch.nn.functional.silu(g) * u)


@pytest.mark.parametrize("M", [1, 3, 16, 17, 40, 64])
@pytest.mark.parametrize("N,K", [(512, 256), (6144, 4096), (5120, 13824)])
@pytest.mark.parametrize("mode", ["plain", "norm_res", "swiglu"])
def test_gemm_fp8_decode_w8a16(M, N, K, mode):
    """W8A16 decode GEMMs (config 5): tile-ordered fp8 image on the no-split 16-row kernel (M <= 16)
    and the fp8 LDS-DMA ring (M > 16), with the in-GEMM RMS norm + residual and SwiGLU pair
    epilogues, against an fp32 oracle on the dequantised weights."""
    torch.manual_seed(M * 7 + N + K)
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).to(torch.bfloat16)
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    cache = ops.Fp8Cache()
    wq, sw = cache.get(w)
    wd = ops.dequantize_fp8(wq, sw)
    act = 5 if mode == "swiglu" else 0
    eps = 1e-5 if mode == "norm_res" else 0.0
    Nout = N // 2 if act == 5 else N
    res = torch.randn(M, Nout, device=DEV, dtype=torch.bfloat16) if mode == "norm_res" else None
    xf = x.float()
    y = xf @ wd.t()
    if eps:
        y = y * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    if act == 5:
        y = torch.nn.functional.silu(y[:, :N // 2]) * y[:, N // 2:]
    if res is not None:
        y = y + res.float()
    out = ops.gemm_decode(x, w, act=act, residual=res, norm_eps=eps, fp8=cache)
    _close(out, y)
    if K % 128 == 0:
        # the tile-ordered image was built and used; row-major launch of the same product agrees
        assert "qs" in cache
        y2 = ops.native().gemm_fp8(x, None, wq, sw, None, act, None, res, eps)
        _close(y2, y)
        # refreshing the source rebuilds the image in place (graph-safe address)
        qs_ptr = cache["qs"].data_ptr()
        with torch.no_grad():
            w.mul_(0.5)
        out2 = ops.gemm_decode(x, w, act=act, residual=res, norm_eps=eps, fp8=cache)
        assert cache["qs"].data_ptr() == qs_ptr
        y3 = xf @ ops.dequantize_fp8(*cache.get(w)).t()
        if eps:
            y3 = y3 * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        if act == 5:
            y3 = torch.nn.functional.silu(y3[:, :N // 2]) * y3[:, N // 2:]
        if res is not None:
            y3 = y3 + res.float()
        _close(out2, y3)


# ------------------------------------------- 16-row GEMV: ring edges, rows vs M, image layout
# One kernel serves the bf16, fp8 and MXFP4 images (S = 1, 2, 4; a 2-KiB chunk = 64 S k). Its waves
# split the chunks of a 16-row group and each runs a DEPTH-deep register ring, so K picks the ring
# case: waves with no chunk, fewer than DEPTH - 1 chunks, exactly DEPTH, DEPTH + 1 unevenly split.
# (The MXFP4 cases are in test_fp4_decode_gpu.py.)
_G16 = {}


def _g16_data(fmt, N, K):
    """weight (bf16: its tile-ordered image; fp8: image + scales), 16 rows of X, residual and the
    fp32 products x w^T / rstd(x), built once per shape and left unchanged"""
    if (fmt, N, K) not in _G16:
        g = torch.Generator().manual_seed(N + K)
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).to(DEV)
        x = (torch.randn(16, K, generator=g) * 2).to(torch.bfloat16).to(DEV)
        res = torch.randn(16, N, generator=g).to(torch.bfloat16).to(DEV)
        if fmt == "fp8":
            q, s = ops.quantize_fp8(w)
            wd, img = ops.dequantize_fp8(q, s), (ops.native().shuffle_decode_weight_fp8(q), s)
        else:
            wd, img = w.float(), ops.native().shuffle_decode_weight(w)
        y = x.float() @ wd.t()
        rstd = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)
        _G16[(fmt, N, K)] = (img, x, res, y, rstd)
    return _G16[(fmt, N, K)]


def _g16_run(fmt, N, K, rows, mode):
    """mode plain / plain_f32 (bf16 image only) / norm_res / pair on X rows `rows` -> (got, oracle)"""
    img, x, res, y, rstd = _g16_data(fmt, N, K)
    xs, rs, y, rstd = x[rows].contiguous(), res[rows].contiguous(), y[rows], rstd[rows]
    act = ops.ACT_SWIGLU if mode == "pair" else 0
    r, eps = (rs, 1e-5) if mode == "norm_res" else (None, 1e-5 if mode == "pair" else 0.0)
    if fmt == "fp8":
        got = ops.native().gemm_fp8(xs, None, img[0], img[1], None, act, None, r, eps, True)
    else:
        got = ops.native().gemm(xs, img, None, None, None, act, mode == "plain_f32", None, r, eps, True)
    if mode == "pair":
        want = torch.nn.functional.silu(y[:, :N // 2] * rstd) * (y[:, N // 2:] * rstd)
    else:
        want = y * rstd + rs.float() if mode == "norm_res" else y
    return got, want


def _g16_check(fmt, N, K, M, mode):
    got, want = _g16_run(fmt, N, K, slice(0, M), mode)
    assert got.dtype == (torch.float32 if mode == "plain_f32" else torch.bfloat16) and got.shape == want.shape
    if mode == "plain_f32":
        _close(got, want, rtol=1e-4, atol=1e-3)
    else:
        _close(got, want)


@pytest.mark.parametrize("K", [128, 640, 2048, 2432])
def test_gemv16_fp8_ring_edges(K):
    """fp8 image, depth 4, 4 waves, 128 k per chunk: 1 chunk (three waves idle), 5 (1-2 per wave: the
    ring never fills), 16 (exactly DEPTH each), 19 (4-5 per wave: one full turn plus a drain)."""
    for M in (1, 16):
        for mode in ("plain", "norm_res", "pair"):
            _g16_check("fp8", 64, K, M, mode)


@pytest.mark.parametrize("K,depth,waves", [(1024, 4, 4), (1024, 4, 8), (1024, 4, 16), (1088, 4, 4), (1088, 4, 8),
                                           (1088, 4, 16), (1088, 6, 0), (1088, 8, 0)])
def test_gemv16_bf16_ring_edges(K, depth, waves):
    """bf16 image, 64 k per chunk: K = 1024 is 16 chunks (exactly DEPTH per wave at 4 waves, 2 at 8,
    1 at 16), K = 1088 is 17 (4-5 per wave at 4 waves; 8 and 16 waves split unevenly below DEPTH - 1;
    depth 6 and 8 never fill their ring). The route needs N / 16 >= 256 row groups: N = 4096, and
    N = 8192 for the SwiGLU pair, which always runs depth 4 with 4 waves."""
    with ops.tuning(gemv16_depth=depth, gemv16_waves=waves):
        for M in (1, 16):
            for mode in ("plain", "plain_f32", "norm_res"):
                _g16_check("bf16", 4096, K, M, mode)
            _g16_check("bf16", 8192, K, M, "pair")


@pytest.mark.parametrize("fmt,N,K", [("bf16", 4096, 1024), ("fp8", 64, 128)])
@pytest.mark.parametrize("mode", ["plain", "norm_res", "pair"])
def test_gemv16_rows_do_not_depend_on_m(fmt, N, K, mode):
    """row r of the 16-row result is bitwise the 1-row result of row r alone: the form is chosen by
    the shape, and the MFMA rows past M repeat row M - 1"""
    if fmt == "bf16" and mode == "pair":
        N = 8192  # N / 32 >= 256 row-group pairs
    y16, _ = _g16_run(fmt, N, K, slice(0, 16), mode)
    for r in range(16):
        y1, _ = _g16_run(fmt, N, K, slice(r, r + 1), mode)
        assert torch.equal(y1.view(torch.int16), y16[r:r + 1].view(torch.int16)), f"row {r} differs"


def _image_from_rule(rows, S):
    """The documented image of row-major weight bytes `rows` [N, 16 K / (8 S)] (a 16-B unit = 8 S k
    of one row): unit i = lane l = i & 63 of load h = (i >> 6) & 1 of tile i >> 7 = (G, c) holds row
    16 G + (l & 15) at k = c KC + h KC / 2 + (l >> 4) 8 S, KC = 64 S. Returns (image, row, k)."""
    N, per_row = rows.shape[0], rows.shape[1] // 16
    nc = per_row * 8 * S // (64 * S)
    i = torch.arange(N * per_row)
    l, h, tile = i & 63, (i >> 6) & 1, i >> 7
    row = 16 * (tile // nc) + (l & 15)
    k = (tile % nc) * 64 * S + h * 32 * S + (l >> 4) * 8 * S
    return rows.reshape(N, per_row, 16)[row, k // (8 * S)].reshape(N, per_row * 16), row, k


@pytest.mark.parametrize("S", [1, 2, 4])
def test_decode_weight_images_follow_the_s_rule(S):
    N, K = 32, 512
    w = (torch.randn(N, K, generator=torch.Generator().manual_seed(S)) * torch.logspace(-2, 2, N)[:, None]).to(torch.bfloat16)
    C = ops.native()
    if S == 1:
        rows, got = w.view(torch.uint8), C.shuffle_decode_weight(w.to(DEV)).cpu().view(torch.uint8)
    elif S == 2:
        q, _ = ops.quantize_fp8(w.to(DEV))
        rows, got = q.cpu(), C.shuffle_decode_weight_fp8(q).cpu()
    else:
        q, s = ops.quantize_mxfp4(w.to(DEV))
        got, simg = (t.cpu() for t in C.shuffle_decode_weight_fp4(q, s))
        rows, s = q.cpu(), s.cpu()
    want, row, k = _image_from_rule(rows, S)
    assert got.shape == want.shape and torch.equal(got, want)
    if S == 4:
        # scale word i = lane i & 63 of tile i >> 6: the scale bytes of that lane's loads h = 0 (low
        # byte) and h = 1 (high byte) = the MX blocks k / 32 and k / 32 + 4 of its unit with h = 0
        u = torch.arange(N * K // 64)
        u = ((u >> 6) << 7) | (u & 63)
        swant = torch.stack((s[row[u], k[u] // 32], s[row[u], k[u] // 32 + 4]), -1).reshape(N, K // 32)
        assert torch.equal(simg, swant)


# ------------------------------------------------------------------ fp8 K/V cache (config 5)
def test_kv_store_fp8_matches_cpu_reference():
    torch.manual_seed(11)
    B, S, Hq, Hkv, D, Smax = 3, 37, 8, 4, 128, 50
    W = (Hq + 2 * Hkv) * D
    qkv = (torch.randn(B * S, W, device=DEV) * torch.logspace(-2, 1, B * S, device=DEV)[:, None]).to(torch.bfloat16)
    kc = torch.zeros(B, Hkv, Smax, D, device=DEV, dtype=torch.uint8)
    vc = torch.zeros_like(kc)
    ks = torch.zeros(B, Hkv, 64, device=DEV)
    vs = torch.zeros_like(ks)
    ops.kv_store_fp8(qkv, kc, vc, ks, vs, B, S, Hq)
    kc2, vc2, ks2, vs2 = kc.cpu().zero_(), vc.cpu().zero_(), ks.cpu().zero_(), vs.cpu().zero_()
    ops.kv_store_fp8(qkv.cpu(), kc2, vc2, ks2, vs2, B, S, Hq)
    torch.testing.assert_close(ks.cpu(), ks2, rtol=1e-6, atol=0)
    torch.testing.assert_close(vs.cpu(), vs2, rtol=1e-6, atol=0)
    for a, b in ((kc.cpu(), kc2), (vc.cpu(), vc2)):
        diff = a != b
        assert diff.float().mean().item() < 5e-3  # reciprocal-scale rounding boundary cases only
        assert ((a.int() - b.int()).abs()[diff] <= 1).all()


@pytest.mark.parametrize("B,Hq,Hkv,Smax,window", [(64, 40, 40, 456, 0),   # Llama-2-13B rollout: MFMA, G = 1
                                                  (40, 32, 8, 300, 64),   # MFMA, G = 4, sliding window
                                                  (1, 40, 40, 456, 0),    # batch-1 8-wave kernel
                                                  (3, 16, 8, 300, 0),     # 8-wave, G = 2
                                                  (2, 32, 8, 1500, 0)])   # 8-wave over key partitions
def test_decode_step_fused_fp8kv(B, Hq, Hkv, Smax, window):
    """fp8 cache decode step (RoPE + quantised append + attention over e4m3 K/V with per-slot
    scales) == fp32 attention over the dequantised cache, and the appended bytes / scales equal the
    reference quantisation of the rotated k_new / v_new."""
    torch.manual_seed(B + Smax)
    D = 128
    W = (Hq + 2 * Hkv) * D
    S = Smax - 40
    smaxp = (Smax + 15) // 16 * 16
    prompt = torch.randn(B * S, W, device=DEV, dtype=torch.bfloat16)
    kc = torch.zeros(B, Hkv, Smax, D, device=DEV, dtype=torch.uint8)
    vc = torch.zeros_like(kc)
    ks = torch.zeros(B, Hkv, smaxp, device=DEV)
    vs = torch.zeros_like(ks)
    ops.kv_store_fp8(prompt, kc, vc, ks, vs, B, S, Hq)
    kv_start = torch.randint(0, 8, (B,), device=DEV, dtype=torch.int32)
    slot = torch.randint(S, Smax - 4, (B,), device=DEV, dtype=torch.int32)
    attn_len = slot + 1
    pos = (slot - kv_start).to(torch.int32)
    cos, sin = ref.rope_tables(D, 4096, 10000.0, DEV)
    ws = ops.decode_workspace(B, Hq, Hkv, D, Smax, DEV)
    for it in range(2):
        qkv = torch.randn(B, W, device=DEV, dtype=torch.bfloat16)
        out = ops.decode_step_attention(qkv, kc, vc, slot, attn_len, Hq, pos, cos, sin, kv_start, window,
                                        workspace=ws, k_scale=ks, v_scale=vs)
        q = ops.rope_qkv_(qkv.clone(), pos, cos, sin, Hq, Hkv, D, S=1)
        kq, ksn = ops.kv_quantize_rows(q[:, Hq * D:(Hq + Hkv) * D].reshape(B, Hkv, D), True)
        vq, vsn = ops.kv_quantize_rows(q[:, (Hq + Hkv) * D:].reshape(B, Hkv, D), False)
        bi = torch.arange(B, device=DEV)
        torch.testing.assert_close(ks[bi, :, slot.long()], ksn, rtol=1e-6, atol=0)
        torch.testing.assert_close(vs[bi, :, slot.long()], vsn, rtol=1e-6, atol=0)
        assert (kc[bi, :, slot.long()].int() - kq.int()).abs().max().item() <= 1
        assert (vc[bi, :, slot.long()].int() - vq.int()).abs().max().item() <= 1
        kd = ops.kv_dequantize(kc, ks[..., :Smax], True)
        vd = ops.kv_dequantize(vc, vs[..., :Smax], False)
        o_ref = ref.decode_attention(q.float(), kd, vd, attn_len, Hq, kv_start, window, 1.0 / math.sqrt(D))
        assert torch.isfinite(out).all()
        _close(out, o_ref)
    assert int(ws.tickets.abs().sum()) == 0


def _decode_edge_case(B, Hq, Hkv, D, Smax, lens, kv_start=0, window=0, fp8=False, PS=None, tune=None):
    """Two successive fused decode steps at chosen lengths (row b: lens[b % len(lens)], then one more)
    against the references of test_decode_step_fused / test_decode_step_fused_fp8kv."""
    g = torch.Generator().manual_seed(Smax + D + Hq)
    W = (Hq + 2 * Hkv) * D
    cos, sin = ref.rope_tables(D, 4096, 10000.0, DEV)
    ks = vs = None
    if fp8:
        prompt = torch.randn(B * Smax, W, generator=g).to(torch.bfloat16).to(DEV)
        kc = torch.zeros(B, Hkv, Smax, D, device=DEV, dtype=torch.uint8)
        vc = torch.zeros_like(kc)
        ks = torch.zeros(B, Hkv, (Smax + 15) // 16 * 16, device=DEV)
        vs = torch.zeros_like(ks)
        ops.kv_store_fp8(prompt, kc, vc, ks, vs, B, Smax, Hq)
    else:
        kc = torch.randn(B, Hkv, Smax, D, generator=g).to(torch.bfloat16).to(DEV)
        vc = torch.randn(B, Hkv, Smax, D, generator=g).to(torch.bfloat16).to(DEV)
    ws = ops.decode_workspace(B, Hq, Hkv, D, Smax, DEV, PS=PS)
    bi = torch.arange(B, device=DEV)
    for step in range(2):
        attn_len = torch.tensor([lens[b % len(lens)] + step for b in range(B)], dtype=torch.int32, device=DEV)
        slot = attn_len - 1
        kvs = torch.clamp(slot, max=kv_start).to(torch.int32)
        pos = (slot - kvs).to(torch.int32)
        qkv = torch.randn(B, W, generator=g).to(torch.bfloat16).to(DEV)
        kc2, vc2 = kc.clone(), vc.clone()
        with ops.tuning(**tune) if tune else contextlib.nullcontext():
            out = ops.decode_step_attention(qkv, kc, vc, slot, attn_len, Hq, pos, cos, sin, kvs, window, workspace=ws,
                                            k_scale=ks, v_scale=vs)
        assert torch.isfinite(out).all()
        if fp8:
            q = ops.rope_qkv_(qkv.clone(), pos, cos, sin, Hq, Hkv, D, S=1)
            kq, ksn = ops.kv_quantize_rows(q[:, Hq * D:(Hq + Hkv) * D].reshape(B, Hkv, D), True)
            vq, vsn = ops.kv_quantize_rows(q[:, (Hq + Hkv) * D:].reshape(B, Hkv, D), False)
            torch.testing.assert_close(ks[bi, :, slot.long()], ksn, rtol=1e-6, atol=0)
            torch.testing.assert_close(vs[bi, :, slot.long()], vsn, rtol=1e-6, atol=0)
            assert (kc[bi, :, slot.long()].int() - kq.int()).abs().max().item() <= 1
            assert (vc[bi, :, slot.long()].int() - vq.int()).abs().max().item() <= 1
            kd = ops.kv_dequantize(kc, ks[..., :Smax], True)
            vd = ops.kv_dequantize(vc, vs[..., :Smax], False)
            o_ref = ref.decode_attention(q.float(), kd, vd, attn_len, Hq, kvs, window, 1.0 / math.sqrt(D))
        else:
            q_ref = ops.rope_qkv_(qkv.clone(), pos, cos, sin, Hq, Hkv, D, S=1, k_cache=kc2, v_cache=vc2, slot_base=slot)
            o_ref = ref.decode_attention(q_ref, kc2, vc2, attn_len, Hq, kvs, window, 1.0 / math.sqrt(D))
            assert torch.equal(kc, kc2) and torch.equal(vc, vc2), "cache append differs"
        _close(out, o_ref)
    assert int(ws.tickets.abs().sum()) == 0


def test_decode_step_one_wave_mfma_g16_edges():
    """16 query heads per kv head on the one-wave MFMA form (B * Hkv = 320), rows of 1 .. 47 keys"""
    _decode_edge_case(160, 32, 2, 128, 48, [1, 15, 16, 17, 32, 33, 47])


@pytest.mark.parametrize("attn_len,kv_start,window", [(1, 0, 0), (16, 0, 0), (17, 0, 0), (95, 0, 0),
                                                      (95, 40, 0),  # the first two partitions are empty
                                                      (95, 0, 8)])
@pytest.mark.parametrize("fp8", [False, True])
def test_decode_step_eight_wave_partition_edges(attn_len, kv_start, window, fp8):
    """The 8-wave MFMA form over six 16-key partitions of a 96-slot cache: waves and partitions without
    a tile, a full and a one-key last tile, empty leading partitions, a window inside one partition."""
    _decode_edge_case(2, 8, 2, 128, 96, [attn_len], kv_start, window, fp8, PS=16,
                      tune=dict(decode_mw_smax=32, decode_mw_kpp=16))


def test_decode_step_valu_empty_leading_partition():
    """The fused VALU kernel (head_dim 64) over three 128-key partitions with kv_start past the first:
    partition 0 publishes an empty record, partition 2 holds no key of the 200-key rows either."""
    _decode_edge_case(3, 8, 2, 64, 300, [200, 131, 258], kv_start=130, PS=128)


def test_generation_fp8kv_matches_teacher_forcing():
    """Generation on an fp8 K/V cache: the behaviour log-probs stay close to a full-precision
    teacher-forced rescoring of the same tokens (head_dim 128 model)."""
    import dataclasses

    from rag_tl_domainllm_optimizer_amd import models
    from rag_tl_domainllm_optimizer_amd.generation import Generator, SamplingParams
    from rag_tl_domainllm_optimizer_amd.models.config import PRESETS
    from rag_tl_domainllm_optimizer_amd.train.common import score_sequences

    cfg = dataclasses.replace(PRESETS["tiny-llama"], hidden_size=512, num_heads=4, num_kv_heads=2, head_dim=128,
                              intermediate_size=1024, name="tiny-llama-d128")
    m = models.CausalLM(cfg, device=DEV, dtype=torch.bfloat16, seed=4)
    prompts = [[5, 9, 33, 41, 7, 8, 9, 10], [12, 300, 4], list(range(20, 90))]
    p = SamplingParams(max_new_tokens=16, temperature=0.7, top_k=0, seed=5)
    gen = Generator(m, 3, 128, DEV, kv_fp8=True)
    assert gen.cache.fp8 and gen.cache.k.dtype == torch.uint8
    out = gen.generate(prompts, p, pad_id=0, eos_ids=[-1])
    with torch.no_grad():
        lp, _, _, _ = score_sequences(m, out.prompt_ids, out.prompt_start, out.tokens, out.lengths, 1 / 0.7)
    d = (lp - out.logprobs).abs()
    assert torch.isfinite(out.logprobs).all()
    assert d.mean().item() < 0.1 and d.max().item() < 0.6, (d.mean().item(), d.max().item())


@pytest.mark.parametrize("M,F,K", [(300, 512, 256), (2048, 1024, 512), (777, 2304, 384)])
def test_gemm_fp8_w8a8_swiglu_fused(M, F, K):
    """W8A8 [gate; up] with SwiGLU in the gemm_big fp8 epilogue == silu(g) * u over the
    dequantised operands (and the plain W8A8 product for every planner split)."""
    torch.manual_seed(M)
    w = (torch.randn(2 * F, K, device=DEV) / math.sqrt(K)).to(torch.bfloat16)
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    wq, sw = ops.quantize_fp8(w)
    xq, sx = ops.quantize_fp8(x)
    xd, wd = ops.dequantize_fp8(xq, sx), ops.dequantize_fp8(wq, sw)
    y = ops.native().gemm_fp8(xq, sx, wq, sw, None, 5, None)
    assert y.shape == (M, F)
    g, u = xd @ wd[:F].t(), xd @ wd[F:].t()
    _close(y, torch.nn.functional.silu(g) * u)
    _close(ops.native().gemm_fp8(xq, sx, wq, sw, None, 0, None), xd @ wd.t())


def test_fp8_training_forward_loss_parity():
    """config 5 ``model.fp8_train``: the frozen base product of LoRA training forwards on W8A8
    (adapter as a bf16 K-extension, bf16 backward) keeps the loss and the adapter gradients of
    the bf16 forward (tiny Llama, 2 x 120 tokens: every projection takes the fp8 path)."""
    from rag_tl_domainllm_optimizer_amd import models

    cfg = models.resolve_preset("tiny-llama")
    m = models.CausalLM(cfg, device=DEV, dtype=torch.bfloat16, seed=7)
    m.add_lora(8, 16.0, "all")
    m.freeze_base()
    for p in m.lora_parameters():  # non-zero B so the adapter term matters
        p.data.normal_(0, 0.05)
    m.refresh_lora()
    ids = torch.randint(3, cfg.vocab_size, (2, 120), device=DEV)

    def run():
        for p in m.lora_parameters():
            p.grad = None
        logits = m.logits(m(ids)).float().view(ids.shape[0], ids.shape[1], -1)
        loss = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), ids[:, 1:].reshape(-1))
        loss.backward()
        return loss.item(), torch.cat([p.grad.flatten().float() for p in m.lora_parameters()])

    l16, g16 = run()
    m.set_fp8(True, train=True)
    try:
        l8, g8 = run()
        assert "q" in m.layers[0]._fp8["qkv"].train_cache(), "fp8 training forward did not run"
    finally:
        m.set_fp8(False, train=False)
    assert abs(l8 - l16) <= 0.02 * abs(l16), (l8, l16)
    cos = torch.nn.functional.cosine_similarity(g8, g16, dim=0).item()
    assert cos > 0.98, cos


def test_swiglu_bwd_epilogue_and_fused_mlp_bitwise():
    """ACT_DSWIGLU (the SwiGLU backward in the down projection's dX GEMM epilogue) is bitwise the
    separate GEMM + swiglu_bwd pair, and the fused MLP node (ops.swiglu_mlp) gives bitwise the
    two-linear outputs and gradients with LoRA on gate, up and down."""
    def _r(*shape, s=1.0):
        return (torch.randn(*shape, device=DEV) * s).to(torch.bfloat16)

    torch.manual_seed(0)
    M, H, F, R = 700, 512, 1024, 64
    dd, wd = _r(M, H), _r(H, F, s=1 / math.sqrt(H))
    pre = _r(M, 2 * F)
    du, ap = _r(M, R), _r(R, F, s=0.05)
    out = torch.empty(M, 2 * F, device=DEV, dtype=torch.bfloat16)
    for bn in (0, 128, 256):
        fused = ops.gemm_big(dd, wd, ops.ROW, ops.KMAJ, du, ap, act=ops.ACT_DSWIGLU, out=out, residual=pre, bn=bn)
        df = ops.gemm_big(dd, wd, ops.ROW, ops.KMAJ, du, ap, bn=bn)
        assert torch.equal(fused, ops.native().swiglu_bwd(pre, df))
    from rag_tl_domainllm_optimizer_amd import models

    cfg = models.resolve_preset("tiny-mistral")
    m = models.CausalLM(cfg, device=DEV, dtype=torch.bfloat16, seed=3)
    m.add_lora(8, 16.0, "all")
    layer = m.layers[0]
    with torch.no_grad():
        for p in m.lora_parameters():
            p.normal_(0, 0.02)
    m.refresh_lora()
    x = _r(300, cfg.hidden_size).requires_grad_(True)
    gy = _r(300, cfg.hidden_size)
    params = [x] + list(layer.lora_params.values())

    def run(fused):
        if fused:
            y = ops.swiglu_mlp(x, layer.gate_up_w, layer.down_w, layer.lora["gate_up"], layer.lora["down"])
            assert y is not None
        else:
            f = ops.linear(x, layer.gate_up_w, act="swiglu", lora=layer.lora["gate_up"])
            y = ops.linear(f, layer.down_w, lora=layer.lora["down"])
        return y, torch.autograd.grad((y.float() * gy.float()).sum(), params, allow_unused=True)

    y1, g1 = run(True)
    y2, g2 = run(False)
    assert torch.equal(y1, y2)
    for a, b in zip(g1, g2):
        assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 8, 2), (64, 4, 2)])
def test_gemm_rope_epilogue_bitwise(D, Hq, Hkv):
    """gemm_rope (the rotary embedding in the qkv projection's GEMM epilogue, E_ROPE) is bitwise the
    GEMM + rope_qkv pair — with a LoRA K-extension, a bias, both tile widths and the planner's
    split into 256- and 128-wide tiles — and close to the fp32 oracle."""
    from rag_tl_domainllm_optimizer_amd.ops import reference as ref

    torch.manual_seed(1)
    M, K, R = 1000, 512, 64
    N = (Hq + 2 * Hkv) * D
    x = (torch.randn(M, K, device=DEV) * 0.5).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).to(torch.bfloat16)
    u = (torch.randn(M, R, device=DEV) * 0.1).to(torch.bfloat16)
    ub = (torch.randn(N, R, device=DEV) * 0.1).to(torch.bfloat16)
    bias = (torch.randn(N, device=DEV) * 0.1).to(torch.bfloat16)
    cos, sin = ref.rope_tables(D, 4096, 10000.0, DEV)
    pos = torch.randint(0, 4096, (M,), device=DEV, dtype=torch.int32)
    cols = (Hq + Hkv) * D
    for ext, b in ((False, None), (True, None), (True, bias)):
        uu, uub = (u, ub) if ext else (None, None)
        for bn in (0, 128, 256):
            fused = ops.native().gemm_rope(x, w, uu, uub, b, pos, cos, sin, cols, D, bn=bn)
            plain = ops.gemm_big(x, w, ops.ROW, ops.ROW, uu, uub, b, bn=bn)
            ops.rope_qkv_(plain, pos, cos, sin, Hq, Hkv, D)
            assert torch.equal(fused, plain), (ext, b is not None, bn)
    y32 = x.float() @ w.float().t() + u.float() @ ub.float().t() + bias.float()
    want = ref.rope_qkv(y32.cpu(), pos.cpu(), cos.cpu(), sin.cpu(), Hq, Hkv, D)
    _close(fused.float().cpu(), want, 0.02)


def test_rope_epilogue_model_bitwise():
    """A LoRA policy's scoring forward + backward (padded and packed) and its prefill give bitwise
    the same log-probs, values, adapter gradients and greedy tokens with the rotary embedding in the
    qkv GEMM epilogue as with the separate rope pass (ops.linear.ROPE_EPILOGUE off)."""
    import numpy as np

    from rag_tl_domainllm_optimizer_amd import models
    from rag_tl_domainllm_optimizer_amd.generation import Generator, SamplingParams
    from rag_tl_domainllm_optimizer_amd.models import ValueHead
    import importlib

    lin = importlib.import_module("rag_tl_domainllm_optimizer_amd.ops.linear")  # (ops.linear is a function)
    from rag_tl_domainllm_optimizer_amd.train.common import score_sequences

    cfg = models.resolve_preset("tiny-mistral")
    m = models.CausalLM(cfg, device=DEV, dtype=torch.bfloat16, seed=5)
    m.add_lora(8, 16.0, None, seed=2)
    with torch.no_grad():
        for p in m.lora_parameters():
            p.normal_(0, 0.02)
    m.refresh_lora()
    vh = ValueHead(cfg.hidden_size, device=DEV, seed=3)
    g = torch.Generator().manual_seed(0)
    B, S, T = 6, 80, 24
    st = np.array([0, 30, 7, 50, 12, 64])
    rl = np.array([24, 3, 17, 1, 20, 9])
    pid = torch.randint(5, cfg.vocab_size, (B, S), generator=g)
    resp = torch.randint(5, cfg.vocab_size, (B, T), generator=g)
    for b in range(B):
        pid[b, :st[b]] = 0
        resp[b, rl[b]:] = 0
    pid, resp = pid.to(DEV), resp.to(DEV)
    start = torch.tensor(st, dtype=torch.int32, device=DEV)
    rlen = torch.tensor(rl, device=DEV)
    prompts = [list(range(7, 7 + n)) for n in (60, 5, 33, 17, 41, 70)]
    res = {}
    try:
        for flag in (True, False):
            lin.ROPE_EPILOGUE = flag
            outs = []
            for lengths in (None, (st, rl)):
                for p in m.lora_parameters():
                    p.grad = None
                lp, ent, val, mask = score_sequences(m, pid, start, resp, rlen, 1.0, vh, lengths=lengths)
                ((lp + 0.5 * val) * mask).sum().backward()
                outs.append((lp.detach(), val.detach(), [p.grad.clone() for p in m.lora_parameters()]))
            gen = Generator(m, max_batch=6, max_seq=96, device=DEV)
            gen.use_graph = False
            toks = gen.generate(prompts, SamplingParams(max_new_tokens=6, do_sample=False), pad_id=0, eos_ids=[-5]).tokens
            res[flag] = (outs, toks.cpu())
    finally:
        lin.ROPE_EPILOGUE = True
    (o1, t1), (o2, t2) = res[True], res[False]
    for (lp1, v1, g1), (lp2, v2, g2) in zip(o1, o2):
        assert torch.equal(lp1, lp2) and torch.equal(v1, v2)
        for a, b in zip(g1, g2):
            assert torch.equal(a, b)
    assert torch.equal(t1, t2)


def test_attention_bwd_fused_rope_bitwise(monkeypatch):
    """The RoPE backward fused into the attention backward's dQ / dK stores gives bitwise the
    gradient of the separate inverse-rotation pass."""
    import importlib

    att = importlib.import_module("rag_tl_domainllm_optimizer_amd.ops.attention")  # (ops.attention is a function)
    from rag_tl_domainllm_optimizer_amd.ops import reference as ref

    torch.manual_seed(3)
    B, S, Hq, Hkv, D = 3, 150, 8, 2, 128
    W = (Hq + 2 * Hkv) * D
    cos, sin = ref.rope_tables(D, 4096, 10000.0, DEV)
    start = torch.tensor([0, 37, 100], dtype=torch.int32, device=DEV)
    pos = (torch.arange(S, device=DEV)[None, :] - start[:, None].long()).clamp(min=0).reshape(-1).to(torch.int32)
    base = (torch.randn(B * S, W, device=DEV) * 0.5).to(torch.bfloat16)
    do = (torch.randn(B * S, Hq * D, device=DEV) * 0.1).to(torch.bfloat16)
    grads = []
    for fused in (True, False):
        monkeypatch.setattr(att, "ROPE_BWD_FUSED", fused)
        x = base.clone().requires_grad_(True)
        o = ops.flash_attention_qkv(x * 1, B, S, Hq, Hkv, D, True, 0, kv_start=start, rope=(pos, cos, sin))
        (g,) = torch.autograd.grad(o, x, do)
        grads.append(g)
    assert torch.equal(grads[0], grads[1])


def test_attention_bwd_writes_every_row():
    """attn_bwd writes every row and column of dq / dk / dv (masked / left-padded rows as zeros), so
    the autograd node hands out an uninitialised buffer: NaN-poisoned outputs come back NaN-free."""
    torch.manual_seed(5)
    B, S, Hq, Hkv, D = 2, 130, 8, 2, 128
    W = (Hq + 2 * Hkv) * D
    qkv = (torch.randn(B * S, W, device=DEV) * 0.5).to(torch.bfloat16)
    start = torch.tensor([0, 77], dtype=torch.int32, device=DEV)
    q, k, v = qkv[:, :Hq * D], qkv[:, Hq * D:(Hq + Hkv) * D], qkv[:, (Hq + Hkv) * D:]
    o, lse = ops.native().attn_fwd(q, k, v, B, S, S, Hq, Hkv, D, True, 0, 1 / math.sqrt(D), start, None, None, 0, True)
    do = (torch.randn(B * S, Hq * D, device=DEV) * 0.1).to(torch.bfloat16)
    d = torch.full((B * S, W), float("nan"), device=DEV, dtype=torch.bfloat16)
    ops.native().attn_bwd(q, k, v, o, do, lse, d[:, :Hq * D], d[:, Hq * D:(Hq + Hkv) * D], d[:, (Hq + Hkv) * D:],
                          B, S, Hq, Hkv, D, True, 0, 1 / math.sqrt(D), start)
    assert not torch.isnan(d).any()
    # left-pad keys of row 1 get no gradient
    assert float(d[S:S + 77, Hq * D:].float().abs().max()) == 0.0


@pytest.mark.parametrize("top_k", [1, 7, 50, 300, 1024])
def test_sampler_search_kth_exact(top_k):
    """Radix select of the k-th largest bf16 logit: with distinct logits every draw is one of the
    exact top-k tokens, over many offsets (top-p off); top-p on top: the draw lies in the nucleus of
    the top-k set (survivors sorted in one wave when <= 64)."""
    B = 32
    g = torch.Generator(device="cpu").manual_seed(7)
    # 2048 distinct bf16 values (8 binades x 128 mantissas, both signs): every logit is unique
    pos = torch.tensor([2.0 ** e * (1 + m / 128) for e in range(-4, 4) for m in range(128)])
    grid = torch.cat([pos, -pos])
    V = grid.numel()
    logits = torch.stack([grid[torch.randperm(V, generator=g)] for _ in range(B)]).to(torch.bfloat16).to(DEV)
    assert int(torch.unique(logits[0].float()).numel()) == V
    topi = logits.float().topk(top_k, dim=1).indices
    for o in range(4):
        off = torch.full((1,), o, dtype=torch.long, device=DEV)
        tok, _ = ops.sample(logits, 1 / 0.7, top_k=top_k, top_p=1.0, seed=5, offset=off)
        assert bool((topi == tok[:, None]).any(1).all())
        tok, _ = ops.sample(logits, 1 / 0.7, top_k=top_k, top_p=0.6, seed=5, offset=off)
        keep = ref.filter_logits(logits.float(), 1 / 0.7, top_k, 0.6)
        assert keep.gather(1, tok[:, None]).float().mean().item() >= 0.97




@pytest.mark.parametrize("top_k,top_p,scale", [(50, 1.0, 2.0), (50, 0.9, 2.0), (7, 0.5, 0.3), (300, 0.95, 8.0),
                                               (1024, 1.0, 1.0), (50, 0.9, 0.02)])
def test_sampler_window_path_bitwise(top_k, top_p, scale):
    """Top-k candidates from a window below the row maximum (one wave finds the k-th key) vs the 16
    block-wide counting passes over the whole row: the same k-th key, kept set, Philox draw and
    behaviour log-prob, bitwise — over logit scales that pick different windows (and, at tiny
    scales, the full-row fallback when no window holds <= 2048 keys)."""
    B, V = 48, 32000
    g = torch.Generator(device="cpu").manual_seed(top_k)
    logits = (torch.randn(B, V, generator=g) * scale).to(torch.bfloat16).to(DEV)
    logits[3, 100:140] = logits[3].max()  # ties at the top
    off = torch.full((1,), 5, dtype=torch.long, device=DEV)
    with ops.tuning(sample_window=1):
        t1, l1 = ops.sample(logits, 1 / 0.7, top_k=top_k, top_p=top_p, seed=9, offset=off)
    with ops.tuning(sample_window=0):
        t0, l0 = ops.sample(logits, 1 / 0.7, top_k=top_k, top_p=top_p, seed=9, offset=off)
    assert torch.equal(t1, t0)
    assert torch.equal(l1, l0)
    keep = ref.filter_logits(logits.float(), 1 / 0.7, top_k, top_p)
    assert keep.gather(1, t1[:, None]).float().mean().item() >= 0.97


@pytest.mark.parametrize("window", [0, 1])
@pytest.mark.parametrize("top_k,top_p,scale", [(50, 1.0, 2.0), (50, 0.9, 2.0), (64, 0.8, 1.0), (7, 0.5, 0.3),
                                               (50, 0.9, 0.02)])
def test_sampler_fast64_path_bitwise(top_k, top_p, scale, window):
    """<= 64 survivors (top-k 50): the wave-0 register fast path vs the block-wide sort / nucleus /
    Gumbel path (tuning sample_fast64=0) — the same token and behaviour log-prob bitwise, with ties
    at the top and at the k-th value, under both candidate searches."""
    B, V = 48, 32000
    g = torch.Generator(device="cpu").manual_seed(top_k + 1000)
    logits = (torch.randn(B, V, generator=g) * scale).to(torch.bfloat16).to(DEV)
    logits[3, 100:140] = logits[3].max()  # 40-way tie at the top
    kth = logits[5].float().topk(top_k).values[-1]
    logits[5, 200:230] = kth.to(torch.bfloat16)  # ties at the k-th value (survivor count > k)
    outs = []
    for fast in (1, 0):
        with ops.tuning(sample_window=window, sample_fast64=fast):
            res = []
            for o in range(3):
                off = torch.full((1,), o, dtype=torch.long, device=DEV)
                res.append(ops.sample(logits, 1 / 0.7, top_k=top_k, top_p=top_p, seed=11, offset=off))
        outs.append(res)
    for (t1, l1), (t0, l0) in zip(*outs):
        assert torch.equal(t1, t0)
        assert torch.equal(l1, l0)


@pytest.mark.parametrize("M,N,K", [(256, 15360, 5120), (256, 5120, 13824), (200, 4096, 4096), (130, 1000, 512)])
def test_gemm_fp8_splitk_slabs(M, N, K):
    """W8A8 split-K into fp32 slabs (config-5 decode at batch > 64): the summed slabs equal the
    dequantised product; the register-row quantiser's scales / codes match torch's e4m3fn cast."""
    torch.manual_seed(N + K)
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).to(torch.bfloat16)
    wq, sw = ops.quantize_fp8(w)
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    xq, sx = ops.quantize_fp8(x)
    # reference codes: torch's e4m3fn cast of x * (1 / s) with the kernel's scales
    s_ref = x.float().abs().amax(1) / 448.0
    torch.testing.assert_close(sx, s_ref, rtol=1e-6, atol=0)
    q_ref = (x.float() * (1.0 / sx)[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    assert (xq != q_ref).float().mean().item() < 5e-3
    yr = ops.dequantize_fp8(xq, sx) @ ops.dequantize_fp8(wq, sw).t()
    for ns, bn in ((1, 128), (3, 128), (5, 256)):
        slabs = torch.full((ns * M * N,), float("nan"), device=DEV)
        ops.native().gemm_fp8_splitk_raw(xq, sx, wq, sw, ns, slabs, bn)
        y = slabs.view(ns, M, N).sum(0)
        torch.testing.assert_close(y, yr, rtol=2e-3, atol=2e-3 * float(yr.abs().max()))


def test_fp8_linear_deferred_splitk():
    """Config-5 decode at batch > 64: ``linear_deferred`` with an fp8 cache returns split-K partials
    (ops.SplitK) whose reduce matches the unsplit W8A8 ``linear``; the slab-summing norm consumes
    them like the bf16 ones."""
    from rag_tl_domainllm_optimizer_amd.ops.fp8 import Fp8Cache
    from rag_tl_domainllm_optimizer_amd.ops.linear import SplitK

    torch.manual_seed(3)
    M, N, K = 96, 2048, 4096
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).to(torch.bfloat16)
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    cache = Fp8Cache()
    with torch.no_grad():
        d = ops.linear_deferred(x, w, fp8=cache)
        y = ops.linear(x, w, fp8=cache)
        assert isinstance(d, SplitK) and d.nsplit > 1
        yd = d.reduce()
        _close(yd.float(), y.float(), rtol=2e-2, atol=2e-2 * float(y.float().abs().max()))
        res = torch.randn(M, N, device=DEV, dtype=torch.bfloat16)
        nw = torch.rand(N, device=DEV, dtype=torch.bfloat16) + 0.5
        y1, h1 = ops.rms_norm(d, nw, 1e-5, res)
        y2, h2 = ops.rms_norm(yd, nw, 1e-5, res)
    _close(h1.float(), h2.float(), rtol=2e-2, atol=2e-2)
    _close(y1.float(), y2.float(), rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("Hq,Hkv", [(40, 40), (32, 8)])
def test_decode_step_fp8kv_from_splitk_slabs(Hq, Hkv):
    """Config-5 decode at batch > 64 hands the attention the qkv GEMM's split-K partials: the fused
    step over the slabs (summed in the kernel prologue) equals the step over the reduced qkv —
    same appended bytes and scales, same output."""
    from rag_tl_domainllm_optimizer_amd.ops.linear import SplitK

    torch.manual_seed(Hq)
    B, D, Smax = 96, 128, 320
    W = (Hq + 2 * Hkv) * D
    S = Smax - 40
    smaxp = (Smax + 15) // 16 * 16
    prompt = torch.randn(B * S, W, device=DEV, dtype=torch.bfloat16)
    kc = torch.zeros(B, Hkv, Smax, D, device=DEV, dtype=torch.uint8)
    vc = torch.zeros_like(kc)
    ks = torch.zeros(B, Hkv, smaxp, device=DEV)
    vs = torch.zeros_like(ks)
    ops.kv_store_fp8(prompt, kc, vc, ks, vs, B, S, Hq)
    kv_start = torch.zeros(B, device=DEV, dtype=torch.int32)
    slot = torch.randint(S, Smax - 4, (B,), device=DEV, dtype=torch.int32)
    attn_len = slot + 1
    pos = slot.clone()
    cos, sin = ref.rope_tables(D, 4096, 10000.0, DEV)
    part = torch.randn(2, B, W, device=DEV)
    qkv = part.sum(0).to(torch.bfloat16)  # the reduce's rounding of the two partials
    sk = SplitK(part.reshape(-1).contiguous(), 2, B, W, torch.bfloat16)
    assert torch.equal(sk.reduce(), qkv)
    caches = [(kc.clone(), vc.clone(), ks.clone(), vs.clone()) for _ in range(2)]
    outs = []
    for src, (k_, v_, ks_, vs_) in zip((qkv, sk), caches):
        ws = ops.decode_workspace(B, Hq, Hkv, D, Smax, DEV)
        outs.append(ops.decode_step_attention(src, k_, v_, slot, attn_len, Hq, pos, cos, sin, kv_start, 0,
                                              workspace=ws, k_scale=ks_, v_scale=vs_))
    for a, b in zip(caches[0], caches[1]):
        assert torch.equal(a, b)
    assert torch.isfinite(outs[1]).all()
    _close(outs[1], outs[0].float(), rtol=1e-2, atol=1e-2)


def test_generation_fp8_deferred_splitk_matches_reduced():
    """Config-5 decode at batch > 64 (W8A8 split-K partials summed in the norms / attention
    prologue) vs the same model with the partials reduced eagerly: same greedy tokens, close
    behaviour log-probs (MHA, fp8 K/V, projections wide enough to split)."""
    import dataclasses

    from rag_tl_domainllm_optimizer_amd import models
    from rag_tl_domainllm_optimizer_amd.generation import Generator, SamplingParams
    from rag_tl_domainllm_optimizer_amd.models.config import PRESETS

    cfg = dataclasses.replace(PRESETS["tiny-llama"], hidden_size=2048, num_heads=16, num_kv_heads=16, head_dim=128,
                              intermediate_size=4096, name="tiny-llama-w2048")
    m = models.CausalLM(cfg, device=DEV, dtype=torch.bfloat16, seed=6)
    m.set_fp8(True)
    g = torch.Generator(device="cpu").manual_seed(2)
    prompts = [torch.randint(5, cfg.vocab_size, (int(n),), generator=g).tolist()
               for n in torch.randint(8, 40, (96,), generator=g)]
    p = SamplingParams(max_new_tokens=8, do_sample=False)
    outs = []
    for defer in (False, True):
        m.defer_splitk = defer
        gen = Generator(m, 96, 64, DEV, kv_fp8=True)
        outs.append(gen.generate(prompts, p, pad_id=0, eos_ids=[-1]))
    m.defer_splitk = True
    # each path against a teacher-forced rescoring of its own tokens (token-parallel forward)
    from rag_tl_domainllm_optimizer_amd.train.common import score_sequences

    gaps = []
    with torch.no_grad():
        for o in outs:
            lp, _, _, _ = score_sequences(m, o.prompt_ids, o.prompt_start, o.tokens, o.lengths, 1.0)
            gaps.append((lp - o.logprobs).abs())
    m.set_fp8(False)
    same = (outs[0].tokens == outs[1].tokens).float().mean(0)
    print("token match by position", [round(v, 3) for v in same.tolist()])
    print("teacher-forced gap reduced / deferred by position",
          [round(v, 4) for v in gaps[0].mean(0).tolist()], [round(v, 4) for v in gaps[1].mean(0).tolist()])
    assert torch.isfinite(outs[1].logprobs).all()
    assert same[0].item() == 1.0  # prefill token: no decode step involved
    assert gaps[1].mean().item() < 1.5 * gaps[0].mean().item() + 0.01, (gaps[0].mean().item(), gaps[1].mean().item())
