"""The attention forward / backward kernels against an fp64 oracle, tensor by tensor.

Every case compares o, lse, dq, dk and dv separately with tests/attention_oracle.py::oracle64:
  * o, dq, dk, dv: relative Frobenius error  e_kernel <= 2 * e_twin,  e_twin being the error of the
    rounding-point twin (twin32) on the same inputs. The twin reproduces every bf16 rounding point of
    the kernels; what is left (summation order, the hardware exp2) cannot double a rounding-dominated
    error.
  * a tensor whose oracle is exactly zero must be exactly zero — except dq / dk where every query
    sees a single key (S = 1, causal window 1): they are zero only by cancellation (p = 1 and
    dS = dP - delta is the difference of the same D products summed in two orders), the relative error
    is undefined, and exact zeros would demand one summation order, which no kernel form promises.
    Their norm is bounded by the worst-case fp32 accumulation error
    (attention_oracle.cancellation_floor); measured on the MI355X the kernels leave ~2e-6 there, the
    twin ~2e-6 (or exactly 0), the bound is ~1e-2 — orders of magnitude below a mask error's O(1).
  * lse, over the rows that see a key: max |err| <= 4 * (the same error of the fp32
    ops/reference.py::attention) + 4 fp32 ulps of max |lse|. With RoPE, o and lse are taken against the
    oracle on the rotated bf16 rows the forward left in place (the rotation's rounding is an input of
    the attention, not part of its error); the gradients are always those of the unrotated rows.
  * exactly zero: dk / dv of keys left of kv_start, dq of causal queries left of it; rows that see no
    key have o == 0 and lse == +inf.
Set ATTN_GRAD_RATIOS to a file name to append the measured figures, one line per case and tensor
(profiles/r10/attn_grad_error_ratios.txt is such a recording).
"""
import importlib
import math
import os

import pytest
import torch

from attention_oracle import (Case, cancellation_floor, make_inputs, oracle64, rel_err, rotate_rows, table, twin32,
                              visible)
from rag_tl_domainllm_optimizer_amd import ops
from rag_tl_domainllm_optimizer_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TABLE = table()
att = importlib.import_module("rag_tl_domainllm_optimizer_amd.ops.attention")  # (ops.attention is a function)


def setup_module(_):
    assert ops.native_available(), "native extension must load on the GPU box"


def _record(line):
    path = os.environ.get("ATTN_GRAD_RATIOS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _tuning(case):
    t = {}
    if case.hp is not None:
        t.update(attn_fwd_hp_maxs=case.hp, attn_dq_hp_maxs=case.hp)
    if case.lpt is not None:
        t["attn_lpt"] = case.lpt
    return ops.tuning(**t)


def _args(case, kv_start, rope=None):
    return (case.B, case.S, case.Hq, case.Hkv, case.D, case.causal, case.window, kv_start, rope)


def _compare_tensor(case, name, x, x64, t, floor):
    x, t = x.double(), t.double()
    if not x64.any():
        if case.single_key and name in ("dq", "dk"):
            fl = floor()[0 if name == "dq" else 1]
            _record(f"attn grad {case.name} {name}: zero by cancellation, |kernel| {float(x.norm()):.4g} "
                    f"|twin| {float(t.norm()):.4g} fp32 bound {fl:.4g}")
            assert float(x.norm()) <= fl, f"{name}: {float(x.norm())} > fp32 accumulation bound {fl}"
        else:
            _record(f"attn grad {case.name} {name}: exact zero (mask)")
            assert not x.any(), f"{name}: the oracle is exactly zero, kernel max {float(x.abs().max())}"
        return
    ek, et = rel_err(x, x64), rel_err(t, x64)
    _record(f"attn grad {case.name} {name}: err {ek:.4g} twin err {et:.4g} ratio {ek / et if et else 0.0:.3f}")
    assert math.isfinite(ek) and ek <= 2 * et, f"{name}: e_kernel {ek:.4g} > 2 * e_twin {et:.4g}"


def _compare_lse(case, lse, lse64, qkv_rows, kv_start):
    B, S, Hq, Hkv, D = case.B, case.S, case.Hq, case.Hkv, case.D
    seen = torch.isfinite(lse64)
    assert bool((torch.isinf(lse[~seen]) & (lse[~seen] > 0)).all()), "lse of a row that sees no key is not +inf"
    assert torch.isfinite(lse[seen]).all()
    q, k, v = qkv_rows[:, :Hq * D], qkv_rows[:, Hq * D:(Hq + Hkv) * D], qkv_rows[:, (Hq + Hkv) * D:(Hq + 2 * Hkv) * D]
    lse32 = ref.attention(q, k, v, B, S, S, Hq, Hkv, D, case.causal, case.window, None, kv_start)[1]
    assert lse32.dtype == torch.float32
    err = float((lse.double()[seen] - lse64[seen]).abs().max())
    err32 = float((lse32.double()[seen] - lse64[seen]).abs().max())
    ulp = 2.0 ** (math.floor(math.log2(float(lse64[seen].abs().max()))) - 23)
    bound = 4 * err32 + 4 * ulp
    _record(f"attn grad {case.name} lse: err {err:.4g} fp32-ref err {err32:.4g} bound {bound:.4g}")
    assert err <= bound, f"lse: max err {err:.4g} > 4 * {err32:.4g} + 4 * {ulp:.4g}"


def _exact_properties(case, kv_start, o, lse, dq, dk, dv):
    B, S = case.B, case.S
    seen = visible(B, S, case.causal, case.window, kv_start).any(-1)  # [B, S]
    keyless = ~seen.reshape(-1)
    assert not o[keyless].any(), "o of a row that sees no key is not 0"
    assert not dq[keyless].any(), "dq of a row that sees no key is not 0"
    l = lse.permute(0, 2, 1).reshape(B * S, -1)[keyless]
    assert bool((torch.isinf(l) & (l > 0)).all()), "lse of a row that sees no key is not +inf"
    if kv_start is not None:
        pad = (torch.arange(S)[None, :] < kv_start[:, None].long()).reshape(-1)
        assert not dk[pad].any() and not dv[pad].any(), "keys left of kv_start got a gradient"
        if case.causal:
            assert bool((keyless | ~pad).all())
    for t in (o, dq, dk, dv):
        assert torch.isfinite(t.float()).all()


def _check(case, got, qkv, do, kv_start, rope=None, fwd_rows=None, lse=True):
    """got: (o, lse, dq, dk, dv) CPU tensors of the kernels. fwd_rows: the rows the forward attended
    (RoPE: rotated in place), default qkv."""
    o, klse, dq, dk, dv = got
    r64, r32 = oracle64(qkv, do, *_args(case, kv_start, rope)), twin32(qkv, do, *_args(case, kv_start, rope))
    f64, f32 = r64, r32
    if fwd_rows is not None:
        f64, f32 = oracle64(fwd_rows, do, *_args(case, kv_start)), twin32(fwd_rows, do, *_args(case, kv_start))
    cache = []

    def floor():
        if not cache:
            cache.append(cancellation_floor(qkv, do, *_args(case, kv_start, rope)))
        return cache[0]

    _exact_properties(case, kv_start, o, klse if lse else f64.lse, dq, dk, dv)
    _compare_tensor(case, "o", o, f64.o, f32.o, floor)
    if lse:
        _compare_lse(case, klse, f64.lse, fwd_rows if fwd_rows is not None else qkv, kv_start)
    _compare_tensor(case, "dq", dq, r64.dq, r32.dq, floor)
    _compare_tensor(case, "dk", dk, r64.dk, r32.dk, floor)
    _compare_tensor(case, "dv", dv, r64.dv, r32.dv, floor)


def _run_kernels(case, qkv, do, kv_start, rope=None):
    """One forward + backward through ops.flash_attention_qkv; returns CPU (o, lse, dq, dk, dv), the
    trailing-column gradient and the rows the forward attended."""
    B, S, Hq, Hkv, D = case.B, case.S, case.Hq, case.Hkv, case.D
    x = qkv.to(DEV).requires_grad_(True)
    ks = kv_start.to(DEV) if kv_start is not None else None
    rp = tuple(t.to(DEV) for t in rope) if rope is not None else None
    with _tuning(case):
        xin = x * 1 if rope is not None else x  # the forward rotates its input rows in place
        o = ops.flash_attention_qkv(xin, B, S, Hq, Hkv, D, case.causal, case.window, kv_start=ks, rope=rp)
        lse = o.grad_fn.saved_tensors[2].clone()  # the lse the backward will read
        (g,) = torch.autograd.grad(o, x, do.to(DEV))
    g = g.cpu()
    W = (Hq + 2 * Hkv) * D
    got = (o.detach().cpu(), lse.cpu(), g[:, :Hq * D], g[:, Hq * D:(Hq + Hkv) * D], g[:, (Hq + Hkv) * D:W])
    return got, g[:, W:], xin.detach().cpu()


@pytest.mark.parametrize("case", TABLE, ids=[c.name for c in TABLE])
def test_attention_grad_table(case, monkeypatch):
    monkeypatch.setattr(att, "ROPE_BWD_FUSED", case.fused)
    qkv, do, kv_start, rope = make_inputs(case)
    got, _, rows = _run_kernels(case, qkv, do, kv_start, rope)
    _check(case, got, qkv, do, kv_start, rope, fwd_rows=rows if rope is not None else None)


PAD_CASES = [Case("bigpad-D128-hp", 3, 200, 8, 2, 128, starts=(0, 1, 63), hp=4096),
             Case("bigpad-D128-nohp-w65", 3, 200, 8, 2, 128, window=65, starts=(64, 65, 199), hp=0),
             Case("bigpad-D64", 3, 321, 4, 2, 64, starts=(0, 130, 199)),
             Case("bigpad-D64-w130", 3, 200, 4, 1, 64, window=130, starts=(64, 65, 199))]


@pytest.mark.parametrize("case", PAD_CASES, ids=[c.name for c in PAD_CASES])
def test_attention_grad_large_pad_rows(case):
    """Rows left of kv_start holding 1e4 in qkv and do: rows that see no key still have o == 0 and
    lse == +inf, every gradient is finite (delta = sum(o * do) of such a row multiplies p = 0), the
    gradients of the pad rows are exactly zero and the rest matches the oracle."""
    qkv, do, kv_start, _ = make_inputs(case, pad_value=1e4)
    got, _, _ = _run_kernels(case, qkv, do, kv_start)
    _check(case, got, qkv, do, kv_start)


WIDE_CASES = [Case("wide-D128", 2, 65, 4, 1, 128, starts=(0, 17)), Case("wide-D64", 2, 129, 4, 2, 64, window=64)]


@pytest.mark.parametrize("case", WIDE_CASES, ids=[c.name for c in WIDE_CASES])
def test_attention_grad_wide_rows(case):
    """qkv rows with 64 columns beyond q | k | v: their gradient is exactly zero."""
    qkv, do, kv_start, _ = make_inputs(case, extra_cols=64)
    got, tail, _ = _run_kernels(case, qkv, do, kv_start)
    assert tail.shape[1] == 64 and not tail.any()
    _check(case, got, qkv, do, kv_start)


PACKED_CASES = [Case("packed-D128", 3, 70, 4, 1, 128, starts=(69, 0, 37)),
                Case("packed-D64-w33", 3, 70, 4, 2, 64, window=33, starts=(69, 0, 37))]


@pytest.mark.parametrize("case", PACKED_CASES, ids=[c.name for c in PACKED_CASES])
def test_attention_grad_packed(case):
    """flash_attention_packed on ragged rows (lengths 1, S and 33): output and gradient of the packed
    rows against the oracle on the equivalent left-padded grid (pad rows zero, no gradient)."""
    B, S, Hq, Hkv, D = case.B, case.S, case.Hq, case.Hkv, case.D
    qkv, do, kv_start, _ = make_inputs(case)
    real = (torch.arange(S)[None, :] >= kv_start[:, None].long()).reshape(-1)
    idx = real.nonzero()[:, 0]
    assert idx.numel() == 1 + 70 + 33
    qkv[~real] = 0
    do[~real] = 0
    x = qkv[idx].to(DEV).requires_grad_(True)
    o = ops.flash_attention_packed(x, idx.to(DEV), B, S, Hq, Hkv, D, case.causal, case.window,
                                   kv_start=kv_start.to(DEV))
    (g,) = torch.autograd.grad(o, x, do[idx].to(DEV))

    def grid(rows):  # packed rows on the grid, zeros elsewhere (what the oracle gives the pad rows)
        out = torch.zeros(B * S, rows.shape[1], dtype=rows.dtype)
        out[idx] = rows.cpu()
        return out

    g = grid(g)
    got = (grid(o.detach()), None, g[:, :Hq * D], g[:, Hq * D:(Hq + Hkv) * D], g[:, (Hq + Hkv) * D:])
    _check(case, got, qkv, do, kv_start, lse=False)


ROPE_DONE = [Case("ropedone-D64", 3, 150, 4, 2, 64, starts=(0, 37, 100), rope=True),
             Case("ropedone-D128", 3, 150, 8, 2, 128, starts=(0, 37, 100), rope=True)]


@pytest.mark.parametrize("source", ["rows", "linear_rope"])
@pytest.mark.parametrize("case", ROPE_DONE, ids=[c.name for c in ROPE_DONE])
def test_attention_grad_rope_done(case, source):
    """rope_done=True: the rows arrive rotated (by hand, or from the GEMM epilogue of ops.linear_rope)
    and only the backward inverse-rotates. The gradient handed to the producer of the rows is the
    inverse rotation of the attention gradient at the rotated rows."""
    B, S, Hq, Hkv, D = case.B, case.S, case.Hq, case.Hkv, case.D
    W = (Hq + 2 * Hkv) * D
    qkv, do, kv_start, rope = make_inputs(case)
    pos, cos, sin = rope
    rp = tuple(t.to(DEV) for t in rope)
    if source == "rows":
        rot = qkv.clone()
        rot[:, :(Hq + Hkv) * D] = rotate_rows(qkv[:, :(Hq + Hkv) * D], pos, cos, sin, B, S, Hq + Hkv, D).to(torch.bfloat16)
        y = rot.to(DEV).requires_grad_(True)
    else:
        g = torch.Generator().manual_seed(5)
        xin = torch.randn(B * S, 64, generator=g).to(torch.bfloat16).to(DEV).requires_grad_(True)
        w = (torch.randn(W, 64, generator=g) / 8).to(torch.bfloat16).to(DEV)
        y, rotated = ops.linear_rope(xin, w, rope=(rp[0], rp[1], rp[2], (Hq + Hkv) * D, D))
        assert rotated, "ops.linear_rope did not rotate in its epilogue at this shape"
    o = ops.flash_attention_qkv(y, B, S, Hq, Hkv, D, True, 0, kv_start=kv_start.to(DEV), rope=rp, rope_done=True)
    lse = o.grad_fn.saved_tensors[2].clone()
    (gy,) = torch.autograd.grad(o, y, do.to(DEV))
    gy, rows = gy.cpu(), y.detach().cpu()
    plain = case._replace(rope=False)
    r64, r32 = oracle64(rows, do, *_args(plain, kv_start)), twin32(rows, do, *_args(plain, kv_start))

    def unrot(t, H):
        return rotate_rows(t, pos, cos, sin, B, S, H, D, -1.0)

    noflo = lambda: (_ for _ in ()).throw(AssertionError("no cancellation case here"))  # noqa: E731
    _exact_properties(plain, kv_start, o.detach().cpu(), lse.cpu(), gy[:, :Hq * D], gy[:, Hq * D:(Hq + Hkv) * D],
                      gy[:, (Hq + Hkv) * D:])
    _compare_tensor(case, "o", o.detach().cpu(), r64.o, r32.o, noflo)
    _compare_lse(plain._replace(name=case.name + "-" + source), lse.cpu(), r64.lse, rows, kv_start)
    _compare_tensor(case, "dq", gy[:, :Hq * D], unrot(r64.dq, Hq), unrot(r32.dq, Hq).to(torch.bfloat16), noflo)
    _compare_tensor(case, "dk", gy[:, Hq * D:(Hq + Hkv) * D], unrot(r64.dk, Hkv), unrot(r32.dk, Hkv).to(torch.bfloat16),
                    noflo)
    _compare_tensor(case, "dv", gy[:, (Hq + Hkv) * D:], r64.dv, r32.dv, noflo)


def test_attention_bwd_unsupported_head_dim_raises():
    """The backward exists for D = 64 and 128 only; D = 32 (which the forward serves) must raise, not
    return with the gradient buffers untouched."""
    B, S, H, D = 1, 20, 2, 32
    qkv = torch.randn(B * S, 3 * H * D, device=DEV, dtype=torch.bfloat16)
    q, k, v = qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:]
    o, lse = ops.native().attn_fwd(q, k, v, B, S, S, H, H, D, True, 0, 1 / math.sqrt(D), None, None, None, 0, True)
    d = torch.zeros_like(qkv)
    with pytest.raises(RuntimeError):
        ops.native().attn_bwd(q, k, v, o, torch.ones_like(o), lse, d[:, :H * D], d[:, H * D:2 * H * D], d[:, 2 * H * D:],
                              B, S, H, H, D, True, 0, 1 / math.sqrt(D), None)
