"""Cost of a verify step of prompt-lookup decoding in the continuous decode batch (Mistral-7B, random
init, graph replay):
    python tools/lookup_rows_cost.py [--prompt 173] [--steps 48] [--rounds 7] [--log profiles/r14/lookup_rows.log]
Configurations (row bucket x K): 1x3, 4x3, 16x3 and 8x7. Each runs in a child process of its own
under its own time limit (``--limit`` seconds; the parent never opens the GPU and stops at the first
child that fails). A child holds three batchers on generators of their own, alternated per round:
  * plain       — ContinuousBatcher without lookup, the comparator: the plain continuous decode step;
  * verify      — lookup_tokens=K, the scalar sampler on bucket * (K + 1) rows;
  * verify-rows — lookup_tokens=K with per_request=True: the grouped per-row sampler.
A round admits the bucket's rows, runs 2 untimed steps and times ``--steps`` graph-replayed steps
between two device events; the answer length leaves room for K + 1 tokens per step, so no row
finishes inside the window. Medians over the rounds after the warm-up rounds, with min .. max;
``ratio`` = verify median / plain median of the same run; ``break-even`` = ratio - 1 is the mean
number of accepted draft tokens per row-step above which verify steps finish an answer sooner than
plain steps (a verify step emits 1 + accepted tokens per row). ``accepted/row-step`` is what this
random-weight model accepted, reported only to show that the draft path ran: it says nothing about
real text."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = "1x3,4x3,16x3,8x7"


def child(a, bucket, K):
    import torch

    if not torch.cuda.is_available():
        sys.exit("lookup_rows_cost: needs the GPU (a CPU timing says nothing about the decode step)")
    from rag_tl_domainllm_optimizer_amd.generation import ContinuousBatcher, Generator, SamplingParams
    from rag_tl_domainllm_optimizer_amd.models import build_model

    dev = torch.device("cuda")
    m = build_model(a.model, device=dev, dtype=torch.bfloat16, seed=0, fast_init=True)
    T = (a.steps + 2) * (K + 1) + 8  # no row reaches its answer length inside the timed window
    sp = SamplingParams(max_new_tokens=T, temperature=0.7, top_k=50, seed=0)
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(5, m.cfg.vocab_size, (a.prompt,), generator=g).tolist()
    forms = ("plain", "verify", "verify-rows")
    gens = {f: Generator(m, bucket, a.prompt + T + K + 16, dev) for f in forms}
    times = {f: [] for f in forms}
    acc = {f: [0, 0] for f in forms}
    for r in range(a.warmup + a.rounds):
        for f, gen in gens.items():
            cb = ContinuousBatcher(gen, sp, pad_id=0, eos_ids=[-1], per_request=f == "verify-rows",
                                   lookup_tokens=0 if f == "plain" else K)
            cb.admit_many([prompt] * bucket)
            cb.step(2)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cb.step(a.steps)
            e1.record()
            e1.synchronize()
            assert cb.active_rows() == bucket and not cb.collect(), "a row finished inside the timed window"
            if f != "plain" and r >= a.warmup:
                c = gen._lk.counters.tolist()
                acc[f][0] += int(c[0])
                acc[f][1] += int(c[2])
            cb.close()
            if r >= a.warmup:
                times[f].append(e0.elapsed_time(e1) / a.steps)
    base = times["plain"]
    bm, spread = statistics.median(base), (max(base) - min(base)) * 1e3
    for f in forms:
        t = times[f]
        med = statistics.median(t)
        tail = f"plain spread {spread:.2f} us"
        if f != "plain":
            tail = (f"ratio {med / bm:.4f}  break-even {med / bm - 1:+.4f} accepted/row-step  {tail}  "
                    f"accepted/row-step here {acc[f][1] / max(acc[f][0], 1):.3f}")
        print(f"RESULT bucket{bucket:<3d} K{K} rows{bucket * (K + 1 if f != 'plain' else 1):<3d} {f:11s} {med:.4f} "
              f"[{min(t):.4f} .. {max(t):.4f}]  {tail}  graphs {len(gens[f].runner.graphs)}", flush=True)
    print(f"DEVICE {torch.cuda.get_device_name(0)}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=173)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", default="mistral-7b")
    ap.add_argument("--configs", default=CONFIGS, help="row bucket x K, comma separated")
    ap.add_argument("--limit", type=int, default=240, help="seconds per configuration (its own process)")
    ap.add_argument("--log", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds: at least 5, the spread is part of the result")
    if a.one:
        b, k = a.one.split("x")
        return child(a, int(b), int(k))
    lines, device = [], "?"
    results = []
    for cfg in a.configs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", cfg, "--prompt", str(a.prompt), "--steps", str(a.steps),
               "--rounds", str(a.rounds), "--warmup", str(a.warmup), "--model", a.model]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired as e:
            print(e.stdout or "", flush=True)
            sys.exit(f"lookup_rows_cost: configuration {cfg} exceeded {a.limit} s; nothing further is launched")
        if r.returncode != 0:
            print(r.stdout, flush=True)
            sys.exit(f"lookup_rows_cost: configuration {cfg} failed ({r.returncode}); nothing further is launched")
        for ln in r.stdout.splitlines():
            if ln.startswith("RESULT "):
                results.append(ln[len("RESULT "):])
                print(results[-1], flush=True)
            elif ln.startswith("DEVICE "):
                device = ln[len("DEVICE "):]
    lines.append(f"# {a.model} random init, prompt {a.prompt}, {a.steps} timed steps per round, {a.rounds} rounds after "
                 f"{a.warmup} warm-up, temperature 0.7 top_k 50, one process per configuration, {device}")
    lines.append("# step, ms: median [min .. max]; ratio = verify / plain of the same run; break-even = ratio - 1 = mean "
                 "accepted draft tokens per row-step at which the verify step wins; plain spread = max - min (us)")
    lines += results
    print("\n".join(lines[:2]), flush=True)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
