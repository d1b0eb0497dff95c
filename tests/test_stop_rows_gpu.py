"""Per-request stop strings and stop token ids on the GPU: ``stop_rows_kernel`` against its eager twin
(bitwise on every state buffer), and ``ContinuousBatcher(per_request=True, stops=True)`` end to end on
the tiny Llama preset (graph-replayed), alone and with prompt-lookup decoding and logit penalties."""
import random

import pytest
import torch

from rag_tl_domainllm_optimizer_amd import models, ops
from rag_tl_domainllm_optimizer_amd.generation import ContinuousBatcher, Generator, RequestSampling, SamplingParams
from rag_tl_domainllm_optimizer_amd.models.config import PRESETS
from rag_tl_domainllm_optimizer_amd.tokenizer import Tokenizer

from test_stop_rows_cpu import pack_rows, straddling_stop

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ------------------------------------------------------------------------------ kernel against oracle
def hand_table():
    """64 entries of 0, 1, 7 and 256 bytes (and a few of 2..3) over a small alphabet; the first
    entries are fixed, the rest drawn from a generator of its own"""
    rng = random.Random(64)
    fixed = [b"", b"a", b"b", b" ", b"ab", b" a", b"abababa", b"b" * 255 + b"a", b"\n", b" b", b"ba", b"", b"a b a b"]
    entries = fixed + [bytes(rng.choice(b"ab \n") for _ in range(rng.choice([0, 1, 1, 2, 3, 7]))) for _ in range(64 - len(fixed))]
    assert len(entries) == 64 and {len(e) for e in entries} >= {0, 1, 7, 256}
    offsets = [0]
    for e in entries:
        offsets.append(offsets[-1] + len(e))
    return entries, (torch.tensor(offsets, dtype=torch.int32), torch.tensor(list(b"".join(entries)), dtype=torch.uint8), True)


# the case list of tests/test_stop_rows_cpu.py on this table (ids: 1 "a", 2 "b", 3 " ", 4 "ab", 5 " a",
# 6 "abababa", 7 the 256-byte entry, 8 newline, 0 and 11 empty): (tokens, stop strings, stop ids)
CASE_ROWS = [
    ([2, 2, 6, 2], [b"bab"], []),                      # inside one token
    ([2, 1, 2, 2], [b"ab"], []),                       # straddling two
    ([2, 2, 1, 2, 1, 2], [b"aba"], []),                # straddling three
    ([2, 2, 1, 4, 2], [b"aab", b"baab"], []),          # two stops complete at one token: the earlier start wins
    ([2, 1, 4, 2], [b"ab"], [4]),                      # a stop id where a string completes
    ([4, 2], [b"ab"], []),                             # at the very first token
    ([5, 2, 2, 2], [b" a"], []),                       # needs the stripped space: no match
    ([2, 2, 2, 2, 1, 4, 2, 2], [b"baa"], []),          # the second token of a G = 4 step
    ([2, 7, 1, 2], [b"ba" + b"a"], []),                # ends right behind the 256-byte entry
    ([7, 7, 2, 2], [b"b" * 32], []),                   # 32 bytes inside the 256-byte entry
    ([1, 7, 7, 7, 7, 7, 7, 7, 7, 3, 1], [b"a a"], []),  # 2048 bytes in one G = 9 step, then a match
    ([0, 11, 0, 5, 0, 2], [b"ab"], [11]),              # empty entries; a stop id with no text
    ([2, 3, 3, 1, 8, 8, 2], [b"\n\nb", b"  a"], []),
    ([3, 1, 2], [b" ab", b"ab"], []),                  # the first string needs the stripped space, the second matches
]


def random_rows(n, T, seed):
    rng = random.Random(seed)
    alphabet = [b"ab", b" a", b"a b", b"aba", b"\n", b"b\na", b"bb", b"a  b", b" ab a", b"b" * 31 + b"a", b"ba b"]
    rows = []
    for _ in range(n):
        toks = [rng.choice([0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 12] + list(range(13, 64))) for _ in range(rng.randrange(1, T + 1))]
        if rng.random() < 0.15:
            toks[rng.randrange(len(toks))] = 7
        rows.append((toks, rng.sample(alphabet, rng.randrange(0, 5)), rng.sample(range(64), rng.randrange(0, 4))))
    return rows


def step_both(table, rows, T, G):
    """The kernel and the oracle stepped G tokens at a time over rows + a row with seen == gen_len + a
    row without stops (sentinel state). Each side advances its own gen_len / active from its own
    previous outputs; every buffer is compared after every step. Returns the final (gen_len,
    stop_hit, stop_at) of the rows."""
    B = len(rows) + 2
    rows = rows + [([2, 1, 2, 1], [b"ab"], [1]), ([2, 1, 2, 1, 4, 4], [], [])]
    out, st = pack_rows(rows, T)
    tb_c, tb_g = ops.TokenBytes(*table), ops.TokenBytes(*table, device=DEV)
    lens = torch.tensor([len(r[0]) for r in rows], dtype=torch.int32)
    gen_len = torch.zeros(B, dtype=torch.int32)
    active = torch.ones(B, dtype=torch.uint8)
    # the two untouched rows: stops but nothing new (seen == gen_len == 4); no stops at all
    gen_len[B - 2], st.seen[B - 2], st.nbytes[B - 2], st.stop_at[B - 2] = 4, 4, 777, 12345
    st.nbytes[B - 1], st.stop_at[B - 1], st.stop_hit[B - 1] = 99, 4242, -7
    dev = [t.clone().to(DEV) for t in st.tensors()]
    out_g, gen_g, act_g, lens_g = out.to(DEV), gen_len.clone().to(DEV), active.clone().to(DEV), lens.clone().to(DEV)

    def advance(gl, act, ln):
        """what the bookkeeping does to a side's own state: G more tokens for its active rows, and a
        row that reaches its length finishes (and is still scanned)"""
        grow = act.bool()
        grow[B - 2] = False
        gl.copy_(torch.where(grow, torch.minimum(gl + G, ln), gl))
        act.copy_(torch.where(grow & (gl >= ln), torch.zeros_like(act), act))

    for _ in range(0, T, G):
        advance(gen_len, active, lens)
        advance(gen_g, act_g, lens_g)
        ops.stop_rows(out, gen_len, active, tb_c, *st.tensors())
        ops.stop_rows(out_g, gen_g, act_g, tb_g, *dev)
        assert torch.equal(gen_g.cpu(), gen_len) and torch.equal(act_g.cpu(), active)
        for name, a, b in zip(("n_stop", "stop_len", "stop_bytes", "n_stop_tok", "stop_tok", "seen", "nbytes", "stop_hit",
                               "stop_at"), dev, st.tensors()):
            assert torch.equal(a.cpu(), b), (name, G, a.cpu().tolist(), b.tolist())
    assert (int(st.seen[B - 2]), int(st.nbytes[B - 2]), int(st.stop_hit[B - 2]), int(st.stop_at[B - 2])) == (4, 777, -1, 12345)
    assert (int(st.seen[B - 1]), int(st.nbytes[B - 1]), int(st.stop_hit[B - 1]), int(st.stop_at[B - 1])) == (0, 99, -7, 4242)
    assert int(gen_len[B - 1]) == 6 and int(gen_len[B - 2]) == 4 and int(active[B - 2]) == 1
    return [(int(gen_len[b]), int(st.stop_hit[b]), int(st.stop_at[b])) for b in range(B - 2)]


@pytest.mark.parametrize("G", [1, 4, 9])
def test_kernel_against_oracle(G):
    entries, table = hand_table()
    T = 16
    rows = CASE_ROWS + random_rows(16, T, 7)
    got = []
    for i in range(0, len(rows), 3):  # B = 5: three rows of the list and the two untouched ones
        got += step_both(table, rows[i:i + 3], T, G)
    want = {0: (3, 0, 1), 1: (3, 0, 1), 2: (5, 0, 2), 3: (4, 1, 1), 4: (3, 4, 2), 5: (1, 0, 0), 6: (4, -1, 0),
            7: (6, 0, 3), 8: (3, 0, 255), 9: (1, 0, 0), 10: (11, 0, 2048), 11: (2, 4, 0), 13: (3, 1, 0)}
    for i, w in want.items():
        assert got[i] == w, (i, got[i], w)
    kinds = {h for _, h, _ in got}
    assert kinds >= {-1, 0, 1, 4}, kinds


# ---------------------------------------------------------------------------------------- end to end
T = 24
PROMPTS = [[5, 9, 33, 41, 7, 8], [12, 300, 4], [77] * 11, [20, 21, 22, 23, 24, 25, 26, 27]]
SEEDS = [31, 32, 33, 34, 35, 36, 37, 38]


@pytest.fixture(scope="module")
def model():
    return models.CausalLM(PRESETS["tiny-llama"], device=DEV, dtype=torch.bfloat16, seed=2)


@pytest.fixture(scope="module")
def tok(model):
    return Tokenizer.synthetic(model.cfg.vocab_size, model.cfg.arch)


def _drain(cb, got):
    while cb.active_rows():
        cb.step(1)
        for f in cb.collect():
            got[f.tag] = f
    return got


def _batcher(model, sp, rows=4, **kw):
    gen = Generator(model, rows, 96, DEV)
    return ContinuousBatcher(gen, sp, pad_id=0, eos_ids=[-1], per_request=True, **kw), gen


def test_end_to_end(model, tok):
    sp = SamplingParams(max_new_tokens=T, temperature=1.0, top_k=0, seed=5)
    tb = ops.TokenBytes.from_tokenizer(tok, DEV)
    cb, gen0 = _batcher(model, sp)
    # the first run, flag off: for each of three rows the first seed of the list whose text holds a
    # stop string that begins and ends inside tokens and completes between token 3 and token T - 3
    seeds, picks, plain = [], [], {}
    for i in range(4):
        for s in SEEDS:
            cb.admit(PROMPTS[i], "probe", RequestSampling(seed=s + 10 * i))
            f = _drain(cb, {})["probe"]
            pick = straddling_stop(tok, f.tokens, 3, T - 3)
            if pick is not None or i == 3:
                break
        assert pick is not None or i == 3, f"row {i}: none of the 8 seeds gives a stop string"
        seeds.append(s + 10 * i)
        picks.append(pick)
    # the run the stop run is compared with: the same admissions, flag off
    cb.admit_many(PROMPTS, [0, 1, 2, 3], [RequestSampling(seed=s) for s in seeds])
    plain = _drain(cb, {})
    assert all(straddling_stop(tok, plain[i].tokens, 3, T - 3) == picks[i] for i in range(3))
    cb.close()
    assert all("stops" not in k for k in gen0.runner.graphs) and gen0.stopp is None
    cb, gen = _batcher(model, sp, stops=True, token_bytes=tb)
    settings = [RequestSampling(seed=seeds[i], stop=["not there", picks[i][0]]) for i in range(3)] + \
        [RequestSampling(seed=seeds[3])]
    cb.admit_many(PROMPTS, [0, 1, 2, 3], settings)
    got, steps = {}, {}
    while cb.active_rows():
        cb.step(1)
        for f in cb.collect():
            got[f.tag], steps[f.tag] = f, cb.steps
    for i in range(3):
        stop, n, keep = picks[i]
        print(f"row {i}: stop {stop!r} completes at token {n}, keeps {keep} bytes; got {len(got[i].tokens)} tokens")
        assert got[i].tokens == plain[i].tokens[:n] and got[i].logprobs == plain[i].logprobs[:n]
        assert steps[i] == n - 1  # the first token comes from the admission, then one per step
        assert (got[i].finish_reason, got[i].stop, got[i].text_bytes) == ("stop", stop, keep)
    assert got[3].tokens == plain[3].tokens and got[3].logprobs == plain[3].logprobs  # bit for bit
    assert got[3].finish_reason == "length" and got[3].text_bytes is None
    # a freed row takes a new request, which finishes at its own stop
    assert cb.free_rows() == 4
    cb.admit(PROMPTS[1], "again", RequestSampling(seed=seeds[1], stop=picks[1][0]))
    again = _drain(cb, {})["again"]
    assert again.tokens == got[1].tokens and again.text_bytes == picks[1][2] and again.finish_reason == "stop"
    # buckets used: 1 (captured at construction) and 4, whatever the rows' stops
    keys = list(gen.runner.graphs)
    assert len(keys) == 2 and all("rows" in k and "stops" in k for k in keys), keys
    assert len(keys) == len(gen0.runner.graphs)
    cb.close()


def test_with_lookup_greedy(model, tok):
    """2 rows, greedy, lookup_tokens = 3: the answer text is the plain stop run's"""
    sp = SamplingParams(max_new_tokens=T, do_sample=False)
    tb = ops.TokenBytes.from_tokenizer(tok, DEV)
    prompts = [PROMPTS[0] * 3, PROMPTS[3] * 2]

    def serve(settings, **kw):
        cb, gen = _batcher(model, sp, rows=2, stops=True, token_bytes=tb, **kw)
        cb.admit_many(prompts, [0, 1], settings)
        got = _drain(cb, {})
        cb.close()
        return got

    plain = serve(None)
    picks = [straddling_stop(tok, plain[i].tokens, 3, T - 3) for i in (0, 1)]
    i = 0 if picks[0] is not None else 1
    assert picks[i] is not None, [tok.decode(plain[j].tokens) for j in (0, 1)]
    settings = [None, None]
    settings[i] = RequestSampling(stop=picks[i][0])
    want, got = serve(settings), serve(settings, lookup_tokens=3)
    assert want[i].tokens == plain[i].tokens[:picks[i][1]] and want[i].text_bytes == picks[i][2]
    for j in (0, 1):
        text = [tok.decode(r[j].tokens).encode()[:r[j].text_bytes] for r in (want, got)]
        print(f"row {j}: {len(want[j].tokens)} / {len(got[j].tokens)} tokens, accepted {got[j].lookup_accepted}")
        assert text[0] == text[1] and got[j].finish_reason == want[j].finish_reason
    assert got[i].tokens == want[i].tokens


def test_with_penalties(model, tok):
    sp = SamplingParams(max_new_tokens=T, temperature=1.0, top_k=0, seed=5)
    tb = ops.TokenBytes.from_tokenizer(tok, DEV)
    base = [RequestSampling(seed=41), RequestSampling(seed=42, logit_bias={77: 100}), RequestSampling(seed=43)]

    def serve(settings, **kw):
        cb, gen = _batcher(model, sp, penalties=True, **kw)
        cb.admit_many(PROMPTS[:3], [0, 1, 2], settings)
        got = _drain(cb, {})
        cb.close()
        return got, gen

    plain, _ = serve(base)
    assert plain[1].tokens == [77] * T
    pick = None
    for s in SEEDS:
        plain, _ = serve([RequestSampling(seed=s)] + base[1:])
        pick = straddling_stop(tok, plain[0].tokens, 3, T - 3)
        if pick is not None:
            break
    assert pick is not None
    word = tok.decode([77]).encode()
    forced_stop = (word[1:] + b" " + word + b" " + word[:1]).decode()  # completes inside the third forced token
    got, gen = serve([RequestSampling(seed=s, stop=pick[0]),
                      RequestSampling(seed=42, logit_bias={77: 100}, stop=forced_stop), base[2]], stops=True, token_bytes=tb)
    assert got[0].tokens == plain[0].tokens[:pick[1]] and got[0].text_bytes == pick[2]
    assert got[1].tokens == [77] * 3 and got[1].finish_reason == "stop" and got[1].text_bytes == 1
    assert got[2].tokens == plain[2].tokens and got[2].logprobs == plain[2].logprobs
    assert all("penalties" in k and "stops" in k for k in gen.runner.graphs)


def test_two_tables_on_one_generator(model, tok):
    """Two stop batchers that follow each other on ONE generator with different byte tables (the
    second vocabulary spells every token differently): the captured step of the first must not serve
    the second, whose stops are searched in its own table after the first table has been dropped."""
    sp = SamplingParams(max_new_tokens=T, temperature=1.0, top_k=0, seed=5)
    tok2 = Tokenizer.synthetic(model.cfg.vocab_size, model.cfg.arch, seed=99)
    gen = Generator(model, 4, 96, DEV)
    cb = ContinuousBatcher(gen, sp, pad_id=0, eos_ids=[-1], per_request=True)
    pick = pick2 = None
    for s in SEEDS:
        cb.admit(PROMPTS[0], "probe", RequestSampling(seed=s))
        plain = _drain(cb, {})["probe"]
        pick, pick2 = straddling_stop(tok, plain.tokens, 3, T - 3), straddling_stop(tok2, plain.tokens, 3, T - 3)
        if pick is not None and pick2 is not None and pick[0] != pick2[0]:
            break
    cb.close()
    assert pick is not None and pick2 is not None and pick[0] not in tok2.decode(plain.tokens)
    keys = []
    for t, (stop, n, keep) in ((tok, pick), (tok2, pick2)):
        tb = ops.TokenBytes.from_tokenizer(t, DEV)
        keys.append(tb.key)
        cb = ContinuousBatcher(gen, sp, pad_id=0, eos_ids=[-1], per_request=True, stops=True, token_bytes=tb)
        cb.admit_many([PROMPTS[0], PROMPTS[1]], ["x", "mate"], [RequestSampling(seed=s, stop=stop), None])
        got = _drain(cb, {})["x"]
        cb.close()
        assert got.tokens == plain.tokens[:n] and (got.finish_reason, got.stop, got.text_bytes) == ("stop", stop, keep)
        del tb, cb
        gen.token_bytes = None  # the graphs alone keep the table they read
        torch.cuda.empty_cache()
    stops = [k for k in gen.runner.graphs if "stops" in k]
    assert {k[k.index("stops") + 1] for k in stops} == set(keys) and len(stops) == 4  # buckets 1 and 2 per table
