"""Bit-level fingerprint of the decode / verify attention step (csrc/kernels/attention.hip):
    python tools/attn_decode_bits.py [--out profiles/r12/attn_decode_bits_this.txt]
From fixed seeds it runs every branch of rt_attn_decode_fused and rt_attn_verify — the fp8 MHA VALU
kernel, the MFMA kernel at 1 / 4 / 8 waves (bf16 and fp8 caches, the split-K slab form, key
partitions), the fused VALU kernel (head_dim 32 / 64 / 128, one and several partitions), both verify
kernels, and the fp8 prompt store — each crossed with: rotary on / off, kv_start > 0 (past whole
partitions where there are any), a window shorter than the row, and per-row lengths 1, 15, 16, 17,
32, 33, 47 and up (waves without a tile, len % 16 in {0, 1, 15}, the new slot in a clamped last tile,
partitions with no visible key). Every case runs two successive steps on one workspace (the ticket
re-arm) and prints one sha256 over its results in order: per step the output, then the K and V
caches after the step, then for fp8 caches both scale arrays (--each prints one sha256 per result
instead, to locate a difference). Tickets must be zero at the end. Two builds compute the same thing
when their listings are identical (RAGTL_EXT_PATH selects another build of the extension)."""
import argparse
import contextlib
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

LENS = (1, 15, 16, 17, 32, 33, 47)
MW = dict(decode_mw_smax=32, decode_mw_kpp=16)  # 96 slots: six partitions of 16 keys


def raw(t):
    return t.contiguous().cpu().view(torch.uint8).numpy().tobytes()


def decode_forms():
    """(name, B, Hq, Hkv, D, Smax, fp8, PS, tuning, slabs, extra lens, kv_start of the kv_start edge)"""
    big = dict(B=160, Hkv=2, D=128, Smax=48, PS=None, tune={}, more=(), ks=20)  # B * Hkv = 320
    yield dict(big, name="g1fp8", G=1, fp8=True)
    for G in (1, 2, 4, 8, 16):
        yield dict(big, name="mfma_w1", G=G)
    for G in (2, 4, 8):
        yield dict(big, name="mfma_w1", G=G, fp8=True)
    yield dict(big, name="mfma_w1_slabs", G=4, slabs=True)
    for G in (1, 4):
        yield dict(big, name="mfma_w1_slabs", G=G, fp8=True, slabs=True)
    small = dict(B=8, Hkv=2, D=128, Smax=96, PS=None, tune={}, more=(94,), ks=40)
    for fp8 in (False, True):
        for G in (1, 2, 4, 8):
            yield dict(small, name="mfma_w8", G=G, fp8=fp8)
            yield dict(small, name="mfma_w8_np6", G=G, fp8=fp8, PS=16, tune=MW)
    for G in (1, 2, 4, 8):
        yield dict(big, name="mfma_w4", B=128, G=G)  # 256 <= B * Hkv < 320
    yield dict(small, name="mfma_w4_np6", B=128, G=4, PS=16, tune=MW)
    # fused VALU kernel: a partition is a multiple of the chunk (256 / 128 / 64 keys at D = 32 / 64 / 128)
    for D, chunk in ((32, 256), (64, 128)):
        for G in (1, 2, 4, 8):
            v = dict(B=12, Hkv=2, D=D, Smax=300, G=G, tune={}, more=(chunk - 1, chunk, chunk + 1, 257, 298),
                     ks=chunk + 2)
            yield dict(v, name="valu_np1", PS=2 * chunk if D == 32 else 3 * chunk)
            yield dict(v, name=f"valu_np{-(-300 // chunk)}", PS=chunk)
    for G in (1, 2, 4, 8):  # head_dim 128 reaches this kernel with several partitions at B * Hkv >= 320 only
        yield dict(big, name="valu_np3", G=G, Smax=160, PS=64, more=(63, 64, 65, 129, 158), ks=66)


def verify_forms():
    for G in (1, 4, 8):
        for Q in (1, 4, 8):
            yield dict(name="verify_mfma", B=8, Hkv=2, Q=Q, G=G, D=128, Smax=96, PS=None, more=(78,), ks=40)
    v = dict(B=12, Hkv=2, Q=2, G=4, D=64, Smax=300, more=(125, 127, 128, 129, 290), ks=130)
    yield dict(v, name="verify_valu_np1", PS=384)
    yield dict(v, name="verify_valu_np3", PS=128)


def edges():
    """(name, rotary, kv_start edge, window)"""
    return (("plain", True, False, 0), ("norot", False, False, 0), ("kvstart", True, True, 0), ("window", True, False, 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--each", action="store_true", help="one sha256 per result, not per case")
    a = ap.parse_args()
    from rag_tl_domainllm_optimizer_amd import ops
    from rag_tl_domainllm_optimizer_amd.ops import reference as ref
    from rag_tl_domainllm_optimizer_amd.ops.linear import SplitK

    dev = torch.device("cuda")
    lines = []

    def say(digest, name):
        lines.append(f"{digest}  {name}")
        print(lines[-1], flush=True)

    def caches(f, g, steps):
        """cache tensors (+ scales) and the per-row first length: LENS and the form's own, cycled over rows"""
        B, Hkv, D, Smax = f["B"], f["Hkv"], f["D"], f["Smax"]
        ls = LENS + tuple(f["more"])
        len0 = torch.tensor([min(ls[b % len(ls)], Smax - steps) for b in range(B)], dtype=torch.int32)
        if f.get("fp8"):
            W = (f["Hq"] + 2 * Hkv) * D
            prompt = (torch.randn(B * Smax, W, generator=g) * torch.logspace(-1, 1, B * Smax)[:, None]).to(torch.bfloat16)
            kc = torch.zeros(B, Hkv, Smax, D, dtype=torch.uint8, device=dev)
            vc = torch.zeros_like(kc)
            ks = torch.zeros(B, Hkv, (Smax + 15) // 16 * 16, device=dev)
            vs = torch.zeros_like(ks)
            ops.kv_store_fp8(prompt.to(dev), kc, vc, ks, vs, B, Smax, f["Hq"])
            return [kc, vc, ks, vs], len0
        kc = torch.randn(B, Hkv, Smax, D, generator=g).to(torch.bfloat16).to(dev)
        vc = torch.randn(B, Hkv, Smax, D, generator=g).to(torch.bfloat16).to(dev)
        return [kc, vc], len0

    case = [None]  # the running sha256 of the current case

    def report(tag, out, cs, last=True):
        """a step's results (out = None: the caches alone) into the case's digest; `last` prints it"""
        if case[0] is None:
            case[0] = hashlib.sha256()
        for nm, t in zip(("out", "kcache", "vcache", "kscale", "vscale"), [out] + cs):
            if t is None:
                continue
            case[0].update(raw(t))
            if a.each:
                say(hashlib.sha256(raw(t)).hexdigest(), f"{tag} {nm}")
        if last:
            if not a.each:
                say(case[0].hexdigest(), tag)
            case[0] = None

    for f in decode_forms():
        f = dict(f, Hq=f["G"] * f["Hkv"])
        B, Hq, Hkv, D, Smax = f["B"], f["Hq"], f["Hkv"], f["D"], f["Smax"]
        W = (Hq + 2 * Hkv) * D
        fp8 = bool(f.get("fp8"))
        cos, sin = ref.rope_tables(D, 512, 10000.0, dev)
        for ename, rot, kvs, window in edges():
            g = torch.Generator().manual_seed(1000 * D + 10 * Hq + Smax + len(ename))
            cs, len0 = caches(f, g, 2)
            if fp8 and ename == "plain":
                report(f"kv_store_fp8 {f['name']} G={f['G']}", None, cs)
            ws = ops.decode_workspace(B, Hq, Hkv, D, Smax, dev, PS=f["PS"])
            for step in range(2):
                attn_len = (len0 + step).to(dev)
                slot = attn_len - 1
                # the kv_start edge: whole leading partitions hidden; short rows see their new key only
                kv_start = torch.clamp(slot, max=f["ks"]).to(torch.int32) if kvs else None
                pos = slot if kv_start is None else (slot - kv_start).to(torch.int32)
                if f.get("slabs"):
                    part = torch.randn(2, B, W, generator=g)
                    qkv = SplitK(part.to(dev).reshape(-1).contiguous(), 2, B, W, torch.bfloat16)
                else:
                    qkv = torch.randn(B, W, generator=g).to(torch.bfloat16).to(dev)
                with ops.tuning(**f["tune"]) if f["tune"] else contextlib.nullcontext():
                    out = ops.decode_step_attention(qkv, cs[0], cs[1], slot, attn_len, Hq, pos if rot else None,
                                                    cos if rot else None, sin if rot else None, kv_start, window,
                                                    workspace=ws, k_scale=cs[2] if fp8 else None,
                                                    v_scale=cs[3] if fp8 else None)
                report(f"{f['name']} {'fp8' if fp8 else 'bf16'} D={D} G={f['G']} B={B} Smax={Smax} {ename}" +
                       (f" step={step}" if a.each else ""), out, cs, last=step == 1)
            assert int(ws.tickets.abs().sum()) == 0, f"tickets not re-armed: {f}"

    for f in verify_forms():
        f = dict(f, Hq=f["Q"] * f["Hkv"])
        B, Hq, Hkv, D, Smax, G = f["B"], f["Hq"], f["Hkv"], f["D"], f["Smax"], f["G"]
        W = (Hq + 2 * Hkv) * D
        cos, sin = ref.rope_tables(D, 512, 10000.0, dev)
        for ename, rot, kvs, window in edges():
            g = torch.Generator().manual_seed(2000 * D + 10 * Hq + G + len(ename))
            cs, len0 = caches(f, g, 2 * G)
            ws = ops.decode_workspace(B, Hq, Hkv, D, Smax, dev, PS=f["PS"])
            for step in range(2):
                attn_len0 = (len0 + step * G).to(dev)
                slot0 = attn_len0 - 1
                kv_start = torch.clamp(slot0, max=f["ks"]).to(torch.int32) if kvs else None
                pos0 = slot0 if kv_start is None else (slot0 - kv_start).to(torch.int32)
                qkv = torch.randn(B * G, W, generator=g).to(torch.bfloat16).to(dev)
                out = ops.verify_step_attention(qkv, cs[0], cs[1], slot0, attn_len0, Hq, G, pos0 if rot else None,
                                                cos if rot else None, sin if rot else None, kv_start, window,
                                                workspace=ws)
                report(f"{f['name']} D={D} Q={f['Q']} G={G} B={B} Smax={Smax} {ename}" +
                       (f" step={step}" if a.each else ""), out, cs, last=step == 1)

    torch.cuda.synchronize()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
