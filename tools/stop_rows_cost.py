"""Cost of per-request stop strings in the continuous decode batch (Mistral-7B, random init, graph replay):
    python tools/stop_rows_cost.py [--prompt 173] [--steps 48] [--rounds 7] [--log profiles/r16/stop_rows.log]
One process; per row bucket (1, 16, 64) three per-request batchers on generators of their own, alternated per round:
  * off     — ContinuousBatcher(per_request=True): the comparator, no stop launch in the captured step;
  * neutral — stops=True, no request with stops (each row leaves the kernel on its first branch);
  * four    — stops=True, every request with four 32-byte stop strings that never match.
A round admits the bucket's rows, runs 2 untimed steps and times ``--steps`` graph-replayed decode
steps between two device events (no row finishes inside the window). Medians over the rounds after
the warm-up rounds, with min .. max; ``delta`` is the median minus the ``off`` median of the same
run, to be read against the ``off`` form's own spread."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=173)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", default="mistral-7b")
    ap.add_argument("--buckets", default="1,16,64")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds: at least 5, the spread is part of the result")
    if not torch.cuda.is_available():
        sys.exit("stop_rows_cost: needs the GPU (a CPU timing says nothing about the decode step)")
    from rag_tl_domainllm_optimizer_amd import ops
    from rag_tl_domainllm_optimizer_amd.generation import ContinuousBatcher, Generator, RequestSampling, SamplingParams
    from rag_tl_domainllm_optimizer_amd.models import build_model
    from rag_tl_domainllm_optimizer_amd.tokenizer import Tokenizer

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda")
    m = build_model(a.model, device=dev, dtype=torch.bfloat16, seed=0, fast_init=True)
    tb = ops.TokenBytes.from_tokenizer(Tokenizer.synthetic(m.cfg.vocab_size, m.cfg.arch), dev)
    T = a.steps + 8  # no row reaches its answer length inside the timed window
    sp = SamplingParams(max_new_tokens=T, temperature=0.7, top_k=50, seed=0)
    say(f"# {a.model} random init, prompt {a.prompt}, {a.steps} timed decode steps per round, {a.rounds} rounds after "
        f"{a.warmup} warm-up, defaults temperature {sp.temperature} top_k {sp.top_k}, {torch.cuda.get_device_name(0)}")
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(5, m.cfg.vocab_size, (a.prompt,), generator=g).tolist()
    # the synthetic vocabulary is lowercase words: upper-case strings cannot occur in the stream text
    four = RequestSampling(stop=[c * 32 for c in "QWXZ"])
    forms = ("off", "neutral", "four")
    buckets = [int(x) for x in a.buckets.split(",")]
    gens = {(b, f): Generator(m, b, a.prompt + T + 16, dev) for b in buckets for f in forms}
    times = {k: [] for k in gens}
    for r in range(a.warmup + a.rounds):
        for (b, f), gen in gens.items():
            kw = {} if f == "off" else dict(stops=True, token_bytes=tb)
            cb = ContinuousBatcher(gen, sp, pad_id=0, eos_ids=[-1], per_request=True, **kw)
            cb.admit_many([prompt] * b, None, [four] * b if f == "four" else None)
            cb.step(2)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cb.step(a.steps)
            e1.record()
            e1.synchronize()
            assert cb.active_rows() == b and not cb.collect(), "a row finished inside the timed window"
            cb.close()
            if r >= a.warmup:
                times[(b, f)].append(e0.elapsed_time(e1) / a.steps)
    say("# decode step, ms: median [min .. max]; delta = median - off median (us); off spread = max - min (us)")
    for b in buckets:
        base = times[(b, "off")]
        bm, spread = statistics.median(base), (max(base) - min(base)) * 1e3
        for f in forms:
            t = times[(b, f)]
            say(f"bucket{b:<3d} {f:8s} {statistics.median(t):.4f} [{min(t):.4f} .. {max(t):.4f}]  "
                f"delta {(statistics.median(t) - bm) * 1e3:+8.2f} us  off spread {spread:.2f} us  "
                f"graphs {len(gens[(b, f)].runner.graphs)}")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
