"""Independent references for the flash attention forward / backward kernels.

``oracle64``: the mathematics in fp64 on the bf16 inputs (no rounding anywhere).
``twin32``:   the same mathematics in fp32 with the kernels' rounding points (csrc/kernels/attention.hip):
  * forward: the unnormalised P = exp(s - m) is rounded to bf16 before P.V (pack_bf16x8 of the S^T
    accumulators), the row sum l stays fp32, o = (P.V) / l is rounded to bf16;
  * backward: P = exp(s - lse) is rounded to bf16 before dO^T.P, delta = sum(o * do) uses the bf16 o,
    dS = P (dP - delta) is rounded to bf16 before dS.K and Q^T.dS, and dq / dk (after the scale) / dv
    are rounded to bf16;
  * RoPE: q / k are rounded to bf16 after the forward rotation (rope_qkv_kernel, in place), and
    dq / dk are rounded a second time after the inverse rotation (the store epilogues of
    attn_bwd_kernel and attn_bwd_dq_kernel rotate the bf16-rounded values).
Both are written from the mathematics with plain torch and call no project op, so an error shared
by every kernel form cannot hide in them. They run on the device of ``qkv`` (the tests use the CPU).

Layouts are the kernels': qkv [B*S, >= (Hq + 2 Hkv) D] token-major rows, head h at column h*D, query
head h reads kv head h // (Hq // Hkv); do / o / dq [B*S, Hq*D]; dk / dv [B*S, Hkv*D] (summed over the
group); lse [B, Hq, S]. Masks are those of ops/reference.py::attention: key <= query (causal),
query - key < window (window > 0), key >= kv_start[b]. A query that sees no key has o = 0,
lse = +inf and contributes no gradient.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch


class AttnGrads(NamedTuple):
    o: torch.Tensor
    lse: torch.Tensor
    dq: torch.Tensor
    dk: torch.Tensor
    dv: torch.Tensor


def visible(B, S, causal, window, kv_start, device=None):
    """bool [B, S(query), S(key)]: which keys each query attends."""
    qi = torch.arange(S, device=device)[:, None]
    ki = torch.arange(S, device=device)[None, :]
    m = torch.ones(S, S, dtype=torch.bool, device=device)
    if causal:
        m = m & (ki <= qi)
    if window and window > 0:
        m = m & ((qi - ki) < window)
    m = m[None].expand(B, S, S)
    if kv_start is not None:
        m = m & (ki[None] >= kv_start.to(device).long().view(B, 1, 1))
    return m


def _split(qkv, B, S, Hq, Hkv, D, dt):
    G = Hq // Hkv
    x = qkv[:, : (Hq + 2 * Hkv) * D].to(dt)
    q = x[:, : Hq * D].reshape(B, S, Hkv, G, D).permute(0, 2, 3, 1, 4)           # [B, Hkv, G, S, D]
    k = x[:, Hq * D:(Hq + Hkv) * D].reshape(B, S, Hkv, D).permute(0, 2, 1, 3)    # [B, Hkv, S, D]
    v = x[:, (Hq + Hkv) * D:].reshape(B, S, Hkv, D).permute(0, 2, 1, 3)
    return q, k, v


def _rows_q(x, B, S, Hq, D):  # [B, Hkv, G, S, D] -> [B*S, Hq*D]
    return x.permute(0, 3, 1, 2, 4).reshape(B * S, Hq * D)


def _rows_k(x, B, S, Hkv, D):  # [B, Hkv, S, D] -> [B*S, Hkv*D]
    return x.permute(0, 2, 1, 3).reshape(B * S, Hkv * D)


def _angles(rope, B, S, dt):
    pos, cos, sin = rope
    c = cos.to(dt)[pos.long().reshape(-1)].reshape(B, S, -1)  # [B, S, D/2]
    s = sin.to(dt)[pos.long().reshape(-1)].reshape(B, S, -1)
    return c, s


def _rotate(x, c, s, sign):
    """Rotate the (d, d + D/2) pairs of x [B, ..., S, D] by sign * angle; c / s [B, S, D/2]."""
    while c.dim() < x.dim():
        c, s = c.unsqueeze(1), s.unsqueeze(1)
    h = x.shape[-1] // 2
    x1, x2 = x[..., :h], x[..., h:]
    s = s * sign
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def rotate_rows(rows, pos, cos, sin, B, S, H, D, sign=1.0):
    """fp64 rotation of token-major rows [B*S, H*D] (every head); sign = -1: the inverse."""
    c, s = _angles((pos, cos, sin), B, S, torch.float64)
    x = rows.double().reshape(B, S, H, D).permute(0, 2, 1, 3)
    return _rotate(x, c, s, sign).permute(0, 2, 1, 3).reshape(B * S, H * D)


def _bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _forward(q, k, v, vis, scale, round_p):
    s = torch.einsum("bhgqd,bhkd->bhgqk", q, k) * scale
    s = s.masked_fill(~vis[:, None, None], float("-inf"))
    m = s.amax(-1, keepdim=True)
    seen = torch.isfinite(m)
    m0 = torch.where(seen, m, torch.zeros_like(m))
    e = torch.exp(s - m0)  # masked entries: exp(-inf) = 0
    l = e.sum(-1, keepdim=True)
    lse = torch.where(seen, m0 + torch.log(l), torch.full_like(m, float("inf")))
    inv = torch.where(seen, 1.0 / l.clamp_min(torch.finfo(l.dtype).tiny), torch.zeros_like(l))
    o = torch.einsum("bhgqk,bhkd->bhgqd", _bf(e) if round_p else e, v) * inv
    return s, lse, o, seen


def _run(qkv, do, B, S, Hq, Hkv, D, causal, window, kv_start, rope, dt, rounded):
    G = Hq // Hkv
    scale = 1.0 / math.sqrt(D)
    rnd = _bf if rounded else (lambda x: x)
    q, k, v = _split(qkv, B, S, Hq, Hkv, D, dt)
    if rope is not None:
        c, sn = _angles(rope, B, S, dt)
        q, k = rnd(_rotate(q, c, sn, 1.0)), rnd(_rotate(k, c, sn, 1.0))
    vis = visible(B, S, causal, window, kv_start, qkv.device)
    s, lse, o, seen = _forward(q, k, v, vis, scale, rounded)
    o = rnd(o)
    dO = do.to(dt).reshape(B, S, Hkv, G, D).permute(0, 2, 3, 1, 4)
    lse0 = torch.where(seen, lse, torch.zeros_like(lse))
    p = torch.where(vis[:, None, None] & seen, torch.exp(s - lse0), torch.zeros_like(s))
    dP = torch.einsum("bhgqd,bhkd->bhgqk", dO, v)
    delta = (o * dO).sum(-1, keepdim=True)
    dS = rnd(p * (dP - delta))
    dq = rnd(torch.einsum("bhgqk,bhkd->bhgqd", dS, k) * scale)
    dk = rnd(torch.einsum("bhgqk,bhgqd->bhkd", dS, q) * scale)
    dv = rnd(torch.einsum("bhgqk,bhgqd->bhkd", rnd(p), dO))
    if rope is not None:
        dq, dk = rnd(_rotate(dq, c, sn, -1.0)), rnd(_rotate(dk, c, sn, -1.0))
    return AttnGrads(_rows_q(o, B, S, Hq, D), lse.squeeze(-1).reshape(B, Hq, S), _rows_q(dq, B, S, Hq, D),
                     _rows_k(dk, B, S, Hkv, D), _rows_k(dv, B, S, Hkv, D))


def oracle64(qkv, do, B, S, Hq, Hkv, D, causal, window, kv_start, rope=None):
    """fp64 forward and backward; with rope = (pos, cos, sin) the gradient w.r.t. the unrotated qkv."""
    return _run(qkv, do, B, S, Hq, Hkv, D, causal, window, kv_start, rope, torch.float64, False)


def twin32(qkv, do, B, S, Hq, Hkv, D, causal, window, kv_start, rope=None):
    """fp32 with the kernels' bf16 rounding points (module docstring)."""
    return _run(qkv, do, B, S, Hq, Hkv, D, causal, window, kv_start, rope, torch.float32, True)


def rel_err(x, x64):
    """Relative Frobenius error of one tensor against its fp64 oracle."""
    return float((x.double() - x64).norm() / x64.norm())


def cancellation_floor(qkv, do, B, S, Hq, Hkv, D, causal, window, kv_start, rope=None, u=2.0 ** -23):
    """(|dq| bound, |dk| bound) in the Frobenius norm for gradients that are zero only by
    cancellation: a query that sees exactly ONE key has p = 1 and dS = dP - delta = 0, where
    dP = sum_d do.v and delta = sum_d o.do (o = v) are the same D products summed in two orders. In
    fp64 both sums are exact; in fp32 each carries at most D.u.sum|terms| of rounding (the standard
    bound for a length-D sum with unit roundoff u, whatever the order; u = 2^-23 covers any faithful
    accumulator). That error, pushed through dq = dS.K.scale and dk = Q^T.dS.scale and the two bf16
    roundings on the way ((1 + 2^-8)^2 < 1.01), is all a correct kernel may leave there."""
    G = Hq // Hkv
    scale = 1.0 / math.sqrt(D)
    dt = torch.float64
    q, k, v = _split(qkv, B, S, Hq, Hkv, D, dt)
    if rope is not None:  # a rotation preserves the norm of every (d, d + D/2) pair
        c, sn = _angles(rope, B, S, dt)
        q, k = _rotate(q, c, sn, 1.0), _rotate(k, c, sn, 1.0)
    vis = visible(B, S, causal, window, kv_start, qkv.device)
    s, lse, o, seen = _forward(q, k, v, vis, scale, False)
    lse0 = torch.where(seen, lse, torch.zeros_like(lse))
    p = torch.where(vis[:, None, None] & seen, torch.exp(s - lse0), torch.zeros_like(s))
    dO = do.to(dt).reshape(B, S, Hkv, G, D).permute(0, 2, 3, 1, 4).abs()
    E = p * (D * u) * (torch.einsum("bhgqd,bhkd->bhgqk", dO, v.abs()) + (o.abs() * dO).sum(-1, keepdim=True))
    fq = torch.einsum("bhgqk,bhkd->bhgqd", E, k.abs()) * scale
    fk = torch.einsum("bhgqk,bhgqd->bhkd", E, q.abs()) * scale
    return 1.01 * float(fq.norm()), 1.01 * float(fk.norm())


# ------------------------------------------------------------------------------- the case table
class Case(NamedTuple):
    name: str
    B: int
    S: int
    Hq: int
    Hkv: int
    D: int
    causal: bool = True
    window: int = 0
    starts: tuple = None   # kv_start per batch row
    hp: int = None         # attn_fwd_hp_maxs = attn_dq_hp_maxs (None: the defaults)
    lpt: int = None        # attn_lpt (None: the default)
    rope: bool = False
    fused: bool = True     # ROPE_BWD_FUSED

    @property
    def single_key(self):
        """every query sees at most one key: dq and dk are zero by cancellation (p = 1)"""
        return self.S == 1 or (self.causal and self.window == 1)


S_FORMS = (1, 15, 16, 17, 63, 64, 65, 129, 257)
WINDOWS = (0, 1, 2, 63, 64, 65, 130, 1000)


def _start_sets(S):
    return (None, (0, 1, 63), (64, 65, S - 1), (0, 130, 199))


def table():
    cases = []
    # kernel form x head layout (tile edges: 16 HP dQ, 32 HP forward, 64 dK/dV and dQ, 128 forward)
    for Hq, Hkv in ((4, 1), (8, 2)):
        for hp in (4096, 0):
            for S in S_FORMS:
                cases.append(Case(f"form-D128-Hq{Hq}-Hkv{Hkv}-hp{hp}-S{S}", 2, S, Hq, Hkv, 128, hp=hp))
    for Hq, Hkv in ((2, 2), (4, 2), (8, 1)):
        for S in S_FORMS:
            cases.append(Case(f"form-D128-Hq{Hq}-Hkv{Hkv}-S{S}", 2, S, Hq, Hkv, 128))
    for Hq, Hkv in ((2, 2), (4, 2), (4, 1), (8, 1)):
        for S in S_FORMS:
            cases.append(Case(f"form-D64-Hq{Hq}-Hkv{Hkv}-S{S}", 2, S, Hq, Hkv, 64))
    # masks: causal x window x kv_start (every batch row differs)
    for S in (200, 321):
        for si, st in enumerate(_start_sets(S)):
            for w in WINDOWS:
                cases.append(Case(f"mask-D128-S{S}-w{w}-ks{si}", 3, S, 4, 1, 128, True, w, st))
            for w in (1, 64, 65, 130):
                cases.append(Case(f"mask-D64-S{S}-w{w}-ks{si}", 3, S, 4, 2, 64, True, w, st))
            for D in (64, 128):
                for w in (0, 65):
                    cases.append(Case(f"mask-noncausal-D{D}-S{S}-w{w}-ks{si}", 3, S, 4, 2, D, False, w, st))
    # launch order, one case per kernel form (head-packed, 64-row dQ with the 128-row forward, the
    # 64-row forward of other groupings, D = 64)
    for lpt in (0, 1 << 30):
        cases.append(Case(f"lpt{lpt}-D128-hp", 3, 257, 8, 2, 128, starts=(0, 37, 5), hp=4096, lpt=lpt))
        cases.append(Case(f"lpt{lpt}-D128-nohp", 3, 257, 8, 2, 128, starts=(0, 37, 5), hp=0, lpt=lpt))
        cases.append(Case(f"lpt{lpt}-D128-mha", 3, 257, 4, 4, 128, starts=(0, 37, 5), hp=4096, lpt=lpt))
        cases.append(Case(f"lpt{lpt}-D64", 3, 257, 4, 2, 64, starts=(0, 37, 5), lpt=lpt))
    # RoPE inside the attention node, fused into the stores or as the separate pass
    for D, Hq, Hkv in ((64, 4, 2), (128, 8, 2)):
        for fused in (True, False):
            cases.append(Case(f"rope-D{D}-fused{int(fused)}", 3, 150, Hq, Hkv, D, starts=(0, 37, 100), rope=True,
                              fused=fused))
            cases.append(Case(f"rope-D{D}-w65-fused{int(fused)}", 3, 150, Hq, Hkv, D, window=65, starts=(0, 37, 100),
                              rope=True, fused=fused))
    return cases


def rope_tables(D, max_pos, theta=10000.0):
    inv = theta ** (-torch.arange(0, D, 2, dtype=torch.float64) / D)
    ang = torch.arange(max_pos, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().float(), ang.sin().float()


def make_inputs(case, extra_cols=0, pad_value=None):
    """Seeded CPU inputs of a case: (qkv bf16, do bf16 — non-zero on every row —, kv_start int32 or
    None, rope = (pos int32, cos, sin) or None). ``pad_value``: the rows left of kv_start of qkv and
    do are set to it (large but finite: they must not reach any result)."""
    import zlib

    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    B, S, Hq, Hkv, D = case.B, case.S, case.Hq, case.Hkv, case.D
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D + extra_cols, generator=g).to(torch.bfloat16)
    do = torch.randn(B * S, Hq * D, generator=g).to(torch.bfloat16)
    do[do == 0] = 1.0
    kv_start = torch.tensor(case.starts, dtype=torch.int32) if case.starts is not None else None
    if pad_value is not None:
        pad = (torch.arange(S)[None, :] < kv_start[:, None].long()).reshape(-1)
        qkv[pad] = pad_value
        do[pad] = pad_value
    rope = None
    if case.rope:
        st = kv_start.long() if kv_start is not None else torch.zeros(B, dtype=torch.long)
        pos = (torch.arange(S)[None, :] - st[:, None]).clamp(min=0).reshape(-1).to(torch.int32)
        rope = (pos,) + rope_tables(D, 512)
    return qkv, do, kv_start, rope
