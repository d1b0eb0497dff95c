"""Cost of MXFP4 weight-only decode (Mistral-7B, random init, 173-token prompt, graph replay):
    python tools/fp4_decode_cost.py [--prompt 173] [--new 64] [--rounds 7] [--log profiles/r9/fp4_decode.log]
One process, the variants (bf16, fp8, fp4) alternated per round, medians and spread reported:
  * the decode step at batch 1, 4, 8, 16 and at batch 1 with prompt-lookup K = 3 (every step of a
    generation is enqueued, early_stop=False, so decode time / steps is the step cost);
  * per projection (qkv, o, gate_up + SwiGLU, down) the GEMV alone at M = 1 and 16: one captured
    graph of the launch over 32 distinct weights (a layer stack's worth, so the weights come from
    HBM as in a decode step), bf16 tile-ordered image against the fp8 and MXFP4 images. These
    settle which projections ``fp4_projection`` sends to the MXFP4 kernel.
Random-init answers are no quality result: MXFP4 has ~11 % relative rms weight error."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=173)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", default="mistral-7b")
    ap.add_argument("--batches", default="1,4,8,16")
    ap.add_argument("--log", default=None)
    ap.add_argument("--skip-steps", action="store_true")
    a = ap.parse_args()
    from rag_tl_domainllm_optimizer_amd import ops
    from rag_tl_domainllm_optimizer_amd.generation import Generator, SamplingParams
    from rag_tl_domainllm_optimizer_amd.models import build_model

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda")
    m = build_model(a.model, device=dev, dtype=torch.bfloat16, seed=0, fast_init=True)
    cfg = m.cfg
    say(f"# {a.model} random init, prompt {a.prompt}, {a.new} new tokens, {a.rounds} rounds after {a.warmup} warm-up, "
        f"{torch.cuda.get_device_name(0)}")

    def mode(name):
        m.set_fp4_decode(False)
        m.set_fp8(False)
        if name == "fp8":
            m.set_fp8(True)
        elif name == "fp4":
            m.set_fp4_decode(True)

    if not a.skip_steps:
        g = torch.Generator().manual_seed(0)
        prompt = torch.randint(5, cfg.vocab_size, (a.prompt,), generator=g).tolist()
        smax = a.prompt + a.new + 16
        cases = [(f"batch{b}", b, 0) for b in (int(x) for x in a.batches.split(","))] + [("batch1_lookupK3", 1, 3)]
        variants = {}
        for cname, b, K in cases:
            for v in ("bf16", "fp8", "fp4"):
                # one generator per (case, variant): its captured step belongs to that variant
                variants[(cname, v)] = (Generator(m, b, smax, dev), [prompt] * b,
                                        SamplingParams(max_new_tokens=a.new, do_sample=False, lookup_tokens=K))
        times = {k: [] for k in variants}
        for r in range(a.warmup + a.rounds):
            for (cname, v), (gen, prompts, sp) in variants.items():
                mode(v)
                out = gen.generate_async(prompts, sp, pad_id=0, eos_ids=[-1], early_stop=False).result()
                if r >= a.warmup:
                    times[(cname, v)].append(out.timings["decode_s"] / out.timings["decode_steps"] * 1e3)
        mode("bf16")
        say("# decode step, ms (median [min .. max]); ratio = variant / bf16 of the same run")
        for cname, _, _ in cases:
            base = statistics.median(times[(cname, "bf16")])
            for v in ("bf16", "fp8", "fp4"):
                t = times[(cname, v)]
                say(f"{cname:16s} {v:5s} {statistics.median(t):.4f} [{min(t):.4f} .. {max(t):.4f}]  "
                    f"ratio {statistics.median(t) / base:.4f}")
        del variants
        torch.cuda.empty_cache()

    # ---- the projections alone
    H, F = cfg.hidden_size, cfg.intermediate_size
    shapes = [("qkv", cfg.qkv_dim, H, 0, True), ("o", H, cfg.num_heads * cfg.head_dim, 0, False),
              ("gate_up", 2 * F, H, ops.ACT_SWIGLU, True), ("down", H, F, 0, False)]
    L = 32
    say(f"# GEMV alone, us per launch (median of 7 graph replays over {L} distinct weights); ratio = variant / bf16")
    for name, N, K, act, normed in shapes:
        ws = [(torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02) for _ in range(L)]
        caches = {"bf16": [ops.ShufCache() for _ in range(L)], "fp8": [ops.Fp8Cache() for _ in range(L)],
                  "fp4": [ops.Fp4Cache() for _ in range(L)]}
        for M in (1, 16):
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            res = None if act else torch.randn(M, N, device=dev, dtype=torch.bfloat16)
            kw = {"act": act, "residual": res, "norm_eps": cfg.norm_eps if normed else 0.0}
            graphs = {}
            for v, key in (("bf16", "shuf"), ("fp8", "fp8"), ("fp4", "fp4")):
                def run(v=v, key=key):
                    for i in range(L):
                        ops.gemm_decode(x, ws[i], **kw, **{key: caches[v][i]})
                run()  # builds the images
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    run()
                graphs[v] = gr
            t = {v: [] for v in graphs}
            for r in range(9):
                for v, gr in graphs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    gr.replay()
                    e1.record()
                    e1.synchronize()
                    if r >= 2:
                        t[v].append(e0.elapsed_time(e1) / L * 1e3)
            base = statistics.median(t["bf16"])
            say(f"{name:8s} N={N:6d} K={K:6d} M={M:2d}  " + "  ".join(
                f"{v} {statistics.median(t[v]):.2f} [{min(t[v]):.2f} .. {max(t[v]):.2f}] x{statistics.median(t[v]) / base:.3f}"
                for v in ("bf16", "fp8", "fp4")))
            del graphs
        del ws, caches
        torch.cuda.empty_cache()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
