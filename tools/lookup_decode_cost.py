"""Cost of a prompt-lookup verify step (Mistral-7B, random init, batch 1, graph replay):
    python tools/lookup_decode_cost.py [--prompt 173] [--new 64] [--rounds 7]
Same process, variants alternated per round, medians reported:
  * plain decode step at 1 row;
  * for K in 3, 5, 7: the verify step (K + 1 positions of one row) and its comparator, the plain
    decode step at K + 1 rows (the same GEMVs on the same number of rows);
  * the attention kernels alone (back-to-back launches between two events, launch overhead included).
Every step of a generation is enqueued (early_stop=False), so decode time / steps is the step cost
whatever the acceptance. Random-init acceptance is printed but is not a result."""
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
    ap.add_argument("--ks", default="3,5,7")
    a = ap.parse_args()
    from rag_tl_domainllm_optimizer_amd import ops
    from rag_tl_domainllm_optimizer_amd.generation import Generator, SamplingParams
    from rag_tl_domainllm_optimizer_amd.models import build_model
    from rag_tl_domainllm_optimizer_amd.ops import reference as ref

    dev = torch.device("cuda")
    m = build_model(a.model, device=dev, dtype=torch.bfloat16, seed=0, fast_init=True)
    cfg = m.cfg
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(5, cfg.vocab_size, (a.prompt,), generator=g).tolist()
    ks = [int(k) for k in a.ks.split(",")]
    smax = a.prompt + a.new + 16
    variants = {"plain_1": (Generator(m, 1, smax, dev), [prompt], SamplingParams(max_new_tokens=a.new, do_sample=False))}
    for K in ks:
        variants[f"plain_{K + 1}"] = (Generator(m, K + 1, smax, dev), [prompt] * (K + 1),
                                      SamplingParams(max_new_tokens=a.new, do_sample=False))
        variants[f"verify_K{K}"] = (Generator(m, 1, smax, dev), [prompt],
                                    SamplingParams(max_new_tokens=a.new, do_sample=False, lookup_tokens=K))
    times = {k: [] for k in variants}
    acc = {}
    for r in range(a.warmup + a.rounds):
        for name, (gen, prompts, sp) in variants.items():
            out = gen.generate_async(prompts, sp, pad_id=0, eos_ids=[-1], early_stop=False).result()
            if r >= a.warmup:
                times[name].append(out.timings["decode_s"] / out.timings["decode_steps"] * 1e3)
            if "lookup_steps" in out.timings:
                acc[name] = (out.timings["lookup_steps"], out.timings["lookup_drafted"], out.timings["lookup_accepted"])
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print(f"{k:12s} median {med[k]:.4f} ms/step  min {min(v):.4f} max {max(v):.4f}  (n={len(v)})")
    for K in ks:
        tv, tc, t1 = med[f"verify_K{K}"], med[f"plain_{K + 1}"], med["plain_1"]
        verdict = "passes" if tv / tc <= 1.03 else "MISSES"
        print(f"K={K}: verify / plain at {K + 1} rows = {tv / tc:.4f} ({verdict} the bound of 1.03)   r_K = verify / plain at 1 row = "
              f"{tv / t1:.4f}   break-even: mean accepted tokens per step > {tv / t1 - 1:.4f}")
    for k, v in acc.items():
        print(f"{k}: random-init row-steps {v[0]}, drafted {v[1]}, accepted {v[2]} (not a result)")

    # ---- the attention kernels alone, at the layer's shapes
    Hq, Hkv, D = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim
    cos, sin = ref.rope_tables(D, 4096, cfg.rope_theta, dev)
    len0 = a.prompt + a.new // 2
    N = 200

    def timed(fn):
        for _ in range(20):
            fn()
        best = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(N):
                fn()
            e1.record()
            e1.synchronize()
            best.append(e0.elapsed_time(e1) / N * 1e3)
        return statistics.median(best)

    for K in ks:
        G = K + 1
        kc = torch.randn(G, Hkv, smax, D, device=dev, dtype=torch.bfloat16)
        vc = torch.randn_like(kc)
        qkv = torch.randn(G, (Hq + 2 * Hkv) * D, device=dev, dtype=torch.bfloat16)
        al1 = torch.full((1,), len0, dtype=torch.int32, device=dev)
        alg = torch.full((G,), len0, dtype=torch.int32, device=dev)
        ws = ops.decode_workspace(G, Hq, Hkv, D, smax, dev)
        out_v = torch.empty(G, Hq * D, device=dev, dtype=torch.bfloat16)
        out_d = torch.empty_like(out_v)
        tv = timed(lambda: ops.verify_step_attention(qkv, kc[:1], vc[:1], al1 - 1, al1, Hq, G, al1 - 1, cos, sin, None,
                                                     cfg.sliding_window, out=out_v))
        td = timed(lambda: ops.decode_step_attention(qkv, kc, vc, alg - 1, alg, Hq, alg - 1, cos, sin, None,
                                                     cfg.sliding_window, workspace=ws, out=out_d))
        print(f"attention per layer, {len0} keys: verify K={K} {tv:.2f} us   decode step at {G} rows {td:.2f} us")


if __name__ == "__main__":
    main()
