"""Cost of per-request logit penalties in the continuous decode batch (Mistral-7B, random init, graph replay):
    python tools/penalty_rows_cost.py [--prompt 173] [--steps 48] [--rounds 7] [--log profiles/r15/penalty_rows.log]
One process; per row bucket (1, 16, 64) four per-request batchers on generators of their own, alternated per round:
  * off     — ContinuousBatcher(per_request=True): the comparator, no penalty launch in the captured step;
  * neutral — penalties=True, every request neutral (each row leaves the kernel on its first branch);
  * rho     — penalties=True, every request with repetition_penalty = 1.1;
  * mix     — penalties=True, requests cycling neutral / rho = 1.1 / presence + frequency / 16 biases.
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
        sys.exit("penalty_rows_cost: needs the GPU (a CPU timing says nothing about the decode step)")
    from rag_tl_domainllm_optimizer_amd.generation import ContinuousBatcher, Generator, RequestSampling, SamplingParams
    from rag_tl_domainllm_optimizer_amd.models import build_model

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda")
    m = build_model(a.model, device=dev, dtype=torch.bfloat16, seed=0, fast_init=True)
    T = a.steps + 8  # no row reaches its answer length inside the timed window
    sp = SamplingParams(max_new_tokens=T, temperature=0.7, top_k=50, seed=0)
    say(f"# {a.model} random init, prompt {a.prompt}, {a.steps} timed decode steps per round, {a.rounds} rounds after "
        f"{a.warmup} warm-up, defaults temperature {sp.temperature} top_k {sp.top_k}, {torch.cuda.get_device_name(0)}")
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(5, m.cfg.vocab_size, (a.prompt,), generator=g).tolist()
    rho = RequestSampling(repetition_penalty=1.1)
    mix = [None, rho, RequestSampling(presence_penalty=0.5, frequency_penalty=0.5),
           RequestSampling(logit_bias={1000 + 37 * i: float(i - 8) for i in range(16)})]
    forms = ("off", "neutral", "rho", "mix")
    buckets = [int(x) for x in a.buckets.split(",")]
    gens = {(b, f): Generator(m, b, a.prompt + T + 16, dev) for b in buckets for f in forms}
    times = {k: [] for k in gens}
    for r in range(a.warmup + a.rounds):
        for (b, f), gen in gens.items():
            cb = ContinuousBatcher(gen, sp, pad_id=0, eos_ids=[-1], per_request=True, penalties=f != "off")
            sampling = {"off": None, "neutral": None, "rho": [rho] * b,
                        "mix": [mix[i % len(mix)] for i in range(b)]}[f]
            cb.admit_many([prompt] * b, None, sampling)
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
