"""Bit-level fingerprint of the 16-row decode GEMV (gemv16_kernel) and of the weight-image builders:
    python tools/gemv16_bits.py [--out profiles/r11/gemv16_bits_this.txt]
From fixed seeds it runs every form the launcher can reach — image (bf16 / fp8 / MXFP4) x plain /
SwiGLU pair x in-GEMM norm (+ residual) on / off x bf16 / fp32 output x waves x depth — at M = 1, 5
and 16, on the ring-edge shapes of the tests (chunks per wave: none for some waves, fewer than
DEPTH - 1, exactly DEPTH, DEPTH + 1 with an uneven split) and one real shape per image, and prints
one sha256 per result and per built image. Two builds compute the same thing when their listings
are identical (RAGTL_EXT_PATH selects another build of the extension)."""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

EPS = 1e-5
MS = (1, 5, 16)
# plain N = 4096 (the bf16 route needs N / 16 >= 256, K >= 1024), pair N = 8192 (N / 32 >= 256)
BF16_K = (1024, 1088, 14336)
FP8 = [(64, 128), (64, 640), (64, 2048), (64, 2432), (4096, 14336)]
# N = 6144: 384 row groups, more than one per CU, so the plain form runs 4 waves (8 below that)
FP4 = [(64, 256), (64, 1280), (64, 3072), (64, 3328), (6144, 1280), (4096, 14336)]


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from rag_tl_domainllm_optimizer_amd import ops

    C = ops.native()
    dev = torch.device("cuda")
    lines = []

    def say(digest, name):
        lines.append(f"{digest}  {name}")
        print(lines[-1], flush=True)

    def data(N, K, seed):
        g = torch.Generator().manual_seed(seed)
        w = (torch.randn(N, K, generator=g) * torch.logspace(-1, 1, N)[:, None] / K ** 0.5).to(torch.bfloat16)
        x = torch.randn(16, K, generator=g).to(torch.bfloat16)
        r = torch.randn(16, N, generator=g).to(torch.bfloat16)
        return w.to(dev), x.to(dev), r.to(dev)

    def modes(N, pair_ok, f32_ok):
        """(name, act, normed, residual?, out_f32)"""
        for f32 in (False, True) if f32_ok else (False,):
            for normed in (False, True):
                yield f"plain{'_norm_res' if normed else ''}{'_f32' if f32 else ''}", 0, normed, normed, f32
                if pair_ok:
                    yield f"pair{'_norm' if normed else ''}{'_f32' if f32 else ''}", ops.ACT_SWIGLU, normed, False, f32

    # ---- bf16 image: waves and depth are tuning knobs (depth 6 / 8 and the pair form run 4 waves)
    knobs = [(4, 0), (4, 4), (4, 8), (4, 16), (6, 0), (8, 0)]
    for K in BF16_K:
        for N, pair in ((4096, False), (8192, True)):
            w, x, r = data(N, K, N + K)
            img = C.shuffle_decode_weight(w)
            say(sha(img), f"image bf16 N={N} K={K}")
            for M in MS:
                for name, act, normed, res, f32 in modes(N, pair, True):
                    if (act != 0) != pair:
                        continue
                    for depth, waves in (knobs if not pair else [(4, 0)]):
                        with ops.tuning(gemv16_depth=depth, gemv16_waves=waves):
                            y = C.gemm(x[:M], img, None, None, None, act, f32, None, r[:M] if res else None,
                                       EPS if normed else 0.0, True)
                        say(sha(y), f"bf16 N={N} K={K} M={M} {name} depth={depth} waves={waves}")

    # ---- fp8 image: depth 4, 4 waves, bf16 output
    for N, K in FP8:
        w, x, r = data(N, K, N + K + 1)
        q, s = ops.quantize_fp8(w)
        img = C.shuffle_decode_weight_fp8(q)
        say(sha(img), f"image fp8 N={N} K={K}")
        for M in MS:
            for name, act, normed, res, _ in modes(N, True, False):
                y = C.gemm_fp8(x[:M], None, img, s, None, act, None, r[:M] if res else None, EPS if normed else 0.0, True)
                say(sha(y), f"fp8 N={N} K={K} M={M} {name}")

    # ---- MXFP4 image: depth 3, waves by the grid rule
    for N, K in FP4:
        w, x, r = data(N, K, N + K + 2)
        img, simg = C.shuffle_decode_weight_fp4(*ops.quantize_mxfp4(w))
        say(sha(img), f"image mxfp4 codes N={N} K={K}")
        say(sha(simg), f"image mxfp4 scales N={N} K={K}")
        for M in MS:
            for name, act, normed, res, f32 in modes(N, True, True):
                y = C.gemv_fp4(x[:M].contiguous(), img, simg, None, act, f32, None, r[:M] if res else None,
                               EPS if normed else 0.0)
                say(sha(y), f"mxfp4 N={N} K={K} M={M} {name}")

    torch.cuda.synchronize()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
