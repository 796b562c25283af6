"""The KV cache of a running request, held to the committed text: float64 reference, metric and bar, planted workloads, a CPU play of the
whole speculative loop and the named faults the plan must expose (numpy + torch + transformers + the CPU oracle; no product import).

THE INVARIANT.  A speculative step writes the K / V rows of its n draft nodes at cache rows [L, L + n), node i rotated at position
L + depth(i); it accepts a root-to-node path of a nodes, moves their rows to [L, L + a) (kv_index[j] -> j, K rows and V rows or V^T
columns, every layer) and advances L by a.  So after any number of steps rows [0, L) of every layer are the K (after RoPE) and V of the
committed text t[0 .. L), as ONE teacher-forced forward of that text computes them -- whatever was drafted and rejected on the way.

REFERENCE.  `master`: a seeded tiny decoder in float64 (weights drawn in fp32, so every model-dtype copy is one rounding of the same
numbers; rotary angles in float64, where HF's own module stops at fp32).  reference_cache(master, text) -> [layers, K|V, H_kv, N, D].
`twin`: the same module cast to the model dtype, rotary frequencies kept in fp32: the arithmetic the reference project itself runs.

METRIC, per (layer, K|V):  e = max over rows r < L and heads h of |got - want|_inf / max(|want[r, h]|_inf, floor), floor = a quarter of
the tensor's largest |want| -- a row-wise relative error that a near-zero row cannot inflate.  A NaN anywhere makes e NaN.

BAR, per (layer, K|V) and dtype:  1.5 x e_twin + 2 ulp, e_twin = the same metric on the twin's cache over the same text, ulp = 2^-11
(fp16) or 2^-8 (bf16).  The 1.5 is the margin of every runner-against-HF comparison of this suite (another summation order of the same
roundings); the ulp term covers tensors that the twin happens to round almost exactly (layer-0 V: one GEMM behind an exact embedding).

WORKLOADS.  Documents are planted in FAMILIES: a main path that forks several times; at every fork the other children are short stubs
that occur MORE often than the main path, so the static automaton's best-first tree draft lists them first and the main path's nodes come
late in the draft.  The target text walks main paths: the accepted path of such a tree draft is not its first nodes and compaction has
rows to move.  Between families the target copies spans of the prompt (sequence drafts from the dynamic automaton, long accepts) and
emits tokens that no document continues (everything but the root rejected).  simulate() plays the loop with the oracle; assert_plan()
holds every workload to the conditions that make the plan bite.

FAULTS rewrite the float64 reference with the step records, touching only the rows the fault would touch; no defective kernel is built."""
import copy
from functools import lru_cache

import numpy as np
import torch

from oracle import sam_oracle as O
from scripted_lm import ScriptedLM

VOCAB, EOS = 1024, 2
CFG = dict(hidden_size=512, intermediate_size=768, num_hidden_layers=2, num_attention_heads=4, vocab_size=VOCAB, max_position_embeddings=1024,
           rms_norm_eps=1e-5, head_dim=128)
ULP = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
MARGIN = 1.5
BUCKETS = (1, 8, 16, 32, 48, 64, 128)
NAMES = ("layer0 K", "layer0 V", "layer1 K", "layer1 V")


# ---- models ----------------------------------------------------------------------------------------------------------------------------
def tiny_llama(kv_heads, seed, device="cpu"):
    """fp32 LlamaForCausalLM of the planting geometry; weights from a CPU generator (std 0.02, norm weights 1 +- 0.05), so the same numbers on
    every device"""
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(**CFG, num_key_value_heads=kv_heads, tie_word_embeddings=False)
    cfg._attn_implementation = "eager"
    torch.manual_seed(seed)
    lm = LlamaForCausalLM(cfg).float().eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, p in lm.named_parameters():
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            else:
                p.copy_(1 + 0.05 * torch.randn(p.shape, generator=g))
    return lm.to(device)


def tiny_qwen(kind, seed):
    """Qwen2-shaped (q|k|v bias) or Qwen3-shaped (per-head q / k norm) fp32 module of the same geometry, by the builder of
    tests/test_gpu_qwen.py (which draws on the GPU; that module imports the product, so it is imported here, on a GPU machine, only)"""
    from test_gpu_qwen import hf_qwen
    return hf_qwen(kind, dict(intermediate_size=CFG["intermediate_size"], num_attention_heads=CFG["num_attention_heads"]), seed=seed)


def as_master(lm32):
    """the float64 master of an fp32 module, on the CPU, with rotary angles in float64"""
    master = copy.deepcopy(lm32).to("cpu").double().eval()
    rot = master.model.rotary_emb
    inv = lm32.model.rotary_emb.inv_freq.detach().to("cpu").double()
    scaling = float(getattr(rot, "attention_scaling", 1.0))

    def forward(x, position_ids):
        ang = position_ids[:, :, None].double() * inv[None, None, :].to(position_ids.device)
        emb = torch.cat((ang, ang), dim=-1)
        return (emb.cos() * scaling).to(x.dtype), (emb.sin() * scaling).to(x.dtype)
    rot.forward = forward
    master.inv_freq64 = inv
    return master


def low_precision_twin(lm32, dtype, device=None):
    """the reference's own arithmetic: the module cast to the serving dtype, rotary frequencies kept in fp32"""
    twin = copy.deepcopy(lm32).to(dtype)
    if device is not None:
        twin = twin.to(device)
    inv = lm32.model.rotary_emb.inv_freq.detach().clone().float().to(next(twin.parameters()).device)
    twin.model.rotary_emb.inv_freq = inv
    if hasattr(twin.model.rotary_emb, "original_inv_freq"):
        twin.model.rotary_emb.original_inv_freq = inv.clone()
    return twin.eval()


# ---- reference -------------------------------------------------------------------------------------------------------------------------
def _layers_of(cache):
    if hasattr(cache, "layers"):
        return [(l.keys, l.values) for l in cache.layers]
    return list(zip(cache.key_cache, cache.value_cache))


def _prefix_cache(lm, text):
    from transformers import DynamicCache
    dev = next(lm.parameters()).device
    cache = DynamicCache()
    with torch.no_grad():
        lm(input_ids=torch.tensor([list(text)], device=dev), past_key_values=cache, use_cache=True, logits_to_keep=1)
    return cache


def reference_cache(lm, text):
    """K (after RoPE) and V of every layer for every position of `text` from one teacher-forced forward: float64 [layers, K|V, H_kv, N, D] on
    the CPU (of the master; of a twin, its own rows widened)"""
    rows = _layers_of(_prefix_cache(lm, text))
    return torch.stack([torch.stack([k[0], v[0]]) for k, v in rows]).double().cpu()


def draft_rows(master, text, rec):
    """the rows a step's verify forward writes for ALL n draft nodes (node i sees text[:L] and its own root path, at position L + depth):
    float64 [layers, K|V, H_kv, n, D]"""
    L, n, anc = rec["L"], rec["n"], rec["anc"]
    cache = _prefix_cache(master, text[:L])
    mask = torch.full((1, 1, n, L + n), torch.finfo(torch.float64).min, dtype=torch.float64)
    mask[..., :L] = 0
    for i in range(n):
        j = i
        while j != -1:
            mask[0, 0, i, L + j] = 0
            j = anc[j]
    with torch.no_grad():
        master(input_ids=torch.tensor([rec["tokens"]]), position_ids=torch.tensor([[L + d for d in rec["depth"]]]), attention_mask=mask,
               past_key_values=cache, use_cache=True)
    return torch.stack([torch.stack([k[0, :, L:], v[0, :, L:]]) for k, v in _layers_of(cache)]).double()


# ---- metric and bar --------------------------------------------------------------------------------------------------------------------
def cache_error(got, want):
    """[layers, 2] float64: the metric of the module docstring over all rows of `want`; got, want [layers, K|V, H_kv, N, D]"""
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    size = want.abs().amax(dim=-1)                                             # [layers, 2, H, N]
    floor = 0.25 * want.abs().amax(dim=(2, 3, 4))[:, :, None, None]
    return ((got - want).abs().amax(dim=-1) / torch.maximum(size, floor)).amax(dim=(2, 3))


def bar(e_twin, dtype):
    return MARGIN * e_twin + 2 * ULP[dtype]


# ---- workloads -------------------------------------------------------------------------------------------------------------------------
class _Pool:
    """distinct tokens first, random ones once they run out"""

    def __init__(self, rng):
        self.rng, self.free = rng, rng.permutation(np.arange(3, VOCAB)).tolist()

    def take(self, k):
        out = [self.free.pop() if self.free else int(self.rng.integers(3, VOCAB)) for _ in range(k)]
        return out


def _family(rng, pool, segments, stubs_per_fork, stub_len):
    """one planted family.  main = seg_0 | seg_1 | ... ; a fork sits in front of every seg_i, i >= 1, where seg_i's first token competes with
    stubs_per_fork[i - 1] stubs.  Every stub document occurs more often than all documents that pass the fork along the main path together,
    so the stubs outrank the main path's child there.  -> (documents with multiplicity, main path)"""
    segs = [pool.take(k) for k in segments]
    main = [t for s in segs for t in s]
    docs, passing = [(main, 1)], 1
    for i in range(len(segs) - 1, 0, -1):                                      # deepest fork first: `passing` documents run through seg_i
        prefix = [t for s in segs[:i] for t in s]
        mults = [passing + 1 + k + int(rng.integers(0, 2)) for k in range(stubs_per_fork[i - 1])]
        for mult in mults:
            docs.append((prefix + pool.take(int(rng.integers(stub_len[0], stub_len[1] + 1))), mult))
        passing += sum(mults)
    return docs, main


def _segments(rng, n_forks, first, later):
    return [int(rng.integers(first[0], first[1] + 1))] + [int(rng.integers(later[0], later[1] + 1)) for _ in range(n_forks)]


WORKLOADS = {
    # name: seed, prompt length, max_predicts, steps, max_cache_len, families (count, forks, first segment, later segments), copy spans
    "base": dict(seed=11, prompt=96, max_predicts=40, steps=42, max_cache_len=512, families=10, forks=(3, 4), first=(1, 7), later=(1, 5), copies=(14, 22)),
    "sweep": dict(seed=13, prompt=120, max_predicts=64, steps=45, max_cache_len=512, families=9, forks=(2, 4), first=(1, 14), later=(1, 9), copies=(10, 40)),
    "wide": dict(seed=35, prompt=64, max_predicts=128, steps=45, max_cache_len=512, families=10, forks=(2, 4), first=(1, 26), later=(1, 5), copies=(20, 30)),
    "end": dict(seed=7, prompt=88, max_predicts=12, steps=200, max_cache_len=128, families=3, forks=(2, 2), first=(1, 3), later=(2, 3), copies=(6, 8)),
}
ALPHA, TOPK, LEN_BIAS = 4.0, 8, 0


@lru_cache(maxsize=None)
def build_workload(name):
    """-> dict(prompt, target, docs, max_predicts, alpha, K, len_bias, steps, max_cache_len, vocab, eos); deterministic"""
    w = WORKLOADS[name]
    rng = np.random.default_rng(w["seed"])
    pool = _Pool(rng)
    prompt = pool.take(w["prompt"])
    docs, mains = [], []
    for _ in range(w["families"]):
        n_forks = int(rng.integers(w["forks"][0], w["forks"][1] + 1))
        fam, main = _family(rng, pool, _segments(rng, n_forks, w["first"], w["later"]), [int(rng.integers(1, 3)) for _ in range(n_forks)], (1, 3))
        mains.append(main)
        for doc, mult in fam:
            for _ in range(mult):
                docs.append(doc)
                docs.append([int(rng.integers(3, VOCAB))])   # a one-token document behind every copy: what follows the EOS varies
    singles = rng.permutation(np.arange(3, VOCAB))[:VOCAB // 2].tolist()         # half the vocabulary has a document of its own
    docs += [[int(t)] for t in singles]
    target = list(prompt)
    for k, main in enumerate(mains):
        target += pool.take(int(rng.integers(1, 3)))                            # tokens that no document continues
        target += main
        target += pool.take(int(rng.integers(1, 3)))
        if k % 2 == 0:
            span = int(rng.integers(w["copies"][0], w["copies"][1] + 1))
            q = int(rng.integers(0, len(prompt) - span))
            target += prompt[q:q + span]
    while len(target) < w["max_cache_len"] + 2 * w["max_predicts"] + 8:          # never exhausted inside the cache
        span = int(rng.integers(w["copies"][0], w["copies"][1] + 1))
        q = int(rng.integers(0, len(prompt) - span))
        target += pool.take(int(rng.integers(1, 4))) + prompt[q:q + span]
    return dict(name=name, prompt=prompt, target=target, docs=docs, max_predicts=w["max_predicts"], alpha=ALPHA, K=TOPK, len_bias=LEN_BIAS,
                steps=w["steps"], max_cache_len=w["max_cache_len"], vocab=VOCAB, eos=EOS)


def _depths(anc):
    depth = [0] * len(anc)
    for i in range(1, len(anc)):
        depth[i] = depth[anc[i]] + 1
    return depth


def _node_argmax(lm, committed, toks, anc):
    """the scripted arg-max of every draft node (tests/scripted_lm.py's rule; samd_scripted_argmax is its device twin)"""
    out = []
    for i in range(len(toks)):
        path, j = [], i
        while j != -1:
            path.append(toks[j])
            j = anc[j]
        out.append(lm.next_token(committed + path[::-1]))
    return out


def simulate(w, on_step=None):
    """the whole loop on the CPU oracle: DraftModel lookup, gen_buffers, scripted arg-max, eval_posterior, update -- SamdModel._run's loop
    with its stopping rule.  -> one record per step: type (0 sequence, 1 tree), n, tokens, anc, depth, a (accept length), kv_index[:a],
    accepted tokens, L before and L1 after.  on_step(draft_model, start_token): a hook for the step-by-step cross-check."""
    lm = ScriptedLM(w["target"], w["vocab"])
    d = O.DraftModel(w["max_predicts"], w["alpha"], w["K"], w["len_bias"], sam_static=O.StaticSAM.build(w["docs"], w["eos"]))
    d.reset()
    ids = list(w["prompt"])
    d.update(ids)
    start = lm.next_token(ids)
    records = []
    for _ in range(w["steps"]):
        L = len(ids)
        if L + w["max_predicts"] >= w["max_cache_len"]:
            break
        if on_step is not None:
            on_step(d, start)
        ty, toks, anc = d.lookup_raw(start)
        am = _node_argmax(lm, ids, toks, anc)
        ret = None if ty == 0 else O.gen_buffers(anc)["tree_retrieve_indices"]
        best, a, nn = O.eval_posterior(am, toks, ret)
        path = list(range(a)) if ret is None else [int(x) for x in ret[best][:a]]
        new = [toks[j] for j in path]
        assert w["eos"] not in new and all(j >= 0 for j in path)
        d.update(new)
        start = int(am[nn])
        ids.extend(new)
        records.append(dict(type=ty, n=len(toks), tokens=list(toks), anc=list(anc), depth=_depths(anc), a=a, kv_index=path, accepted=new, L=L, L1=len(ids)))
    assert ids == w["target"][:len(ids)], "the scripted run is lossless"
    return records


def bucket_of(n):
    return next(b for b in BUCKETS if n <= b)


def moved(rec):
    """a tree step whose accepted path is not its first nodes: compaction has rows to move"""
    return rec["type"] == 1 and rec["kv_index"] != list(range(rec["a"]))


def assert_plan(name, records):
    """the conditions under which the workload exercises compaction, the exact-row graphs and every bucket it is meant for.  `end` has 40 rows
    of cache behind its prompt and max_predicts 12: the general conditions do not fit there (8 moved steps, an accept of 6 and one of 8 need more
    rows than it commits); it has its own, below."""
    mv = [r for r in records if moved(r)]
    if name != "end":
        assert len(mv) >= 8, (name, len(mv))
        assert any(r["a"] >= 6 for r in mv), name
        assert any(max(k - j for j, k in enumerate(r["kv_index"])) >= 3 for r in mv), name
        assert sum(r["a"] == 1 for r in records) >= 3, name
        assert any(r["type"] == 0 and r["a"] >= 8 for r in records), name
        assert {5, 9} <= {r["n"] for r in records}, name
    if name == "sweep":
        assert {8, 16, 32, 48, 64} <= {bucket_of(r["n"]) for r in records}, sorted({bucket_of(r["n"]) for r in records})
    if name == "wide":
        assert any(bucket_of(r["n"]) == 128 for r in mv), name
    if name == "end":
        w = build_workload(name)
        assert len(mv) >= 2 and len(records) < w["steps"] and records[-1]["L1"] + w["max_predicts"] >= w["max_cache_len"], name
        assert any(r["L"] + bucket_of(r["n"]) > w["max_cache_len"] for r in records), "a bucket's padding rows reach past the cache"


# ---- named faults ------------------------------------------------------------------------------------------------------------------------
def _rotate(k_rows, delta, inv_freq):
    """K rows [..., D] rotated by `delta` further positions (HF's half-split pairs)"""
    ang = float(delta) * inv_freq
    cos, sin = torch.cat((ang, ang)).cos(), torch.cat((ang, ang)).sin()
    half = k_rows.shape[-1] // 2
    rot = torch.cat((-k_rows[..., half:], k_rows[..., :half]), dim=-1)
    return k_rows * cos + rot * sin


def _sibling_or_next(rec, node):
    sib = [i for i in range(rec["n"]) if i != node and rec["anc"][i] == rec["anc"][node] and node > 0]
    return sib[0] if sib else min(node + 1, rec["n"] - 1)


FAULTS = ("no_compaction", "neighbour_row", "rope_by_node_index", "rope_from_new_length", "k_moved_v_left", "v_moved_k_left", "length_minus_one",
          "length_plus_one", "wrap_into_next_head")
ON_EVERY_TENSOR = ("no_compaction", "neighbour_row", "length_minus_one", "length_plus_one")


def apply_fault(fault, want, master, text, records, max_steps=2):
    """the cache a run with the named fault would leave: `want` (reference_cache of text) rewritten on the rows the fault touches, at the
    first max_steps tree steps that move rows"""
    got = want.clone()
    N = want.shape[3]
    steps = [r for r in records if moved(r) and r["L1"] <= N][:max_steps]
    assert steps, "no step to damage"
    inv = master.inv_freq64
    if fault in ("no_compaction", "neighbour_row", "k_moved_v_left", "v_moved_k_left"):
        for r in steps:
            rows = draft_rows(master, text, r)
            for j, node in enumerate(r["kv_index"]):
                src = j if fault != "neighbour_row" else _sibling_or_next(r, node)
                if src == node:
                    continue
                halves = {"no_compaction": (0, 1), "neighbour_row": (0, 1), "k_moved_v_left": (1,), "v_moved_k_left": (0,)}[fault]
                for h in halves:
                    got[:, h, :, r["L"] + j] = rows[:, h, :, src]
    elif fault == "rope_by_node_index":
        for r in steps:
            for j, node in enumerate(r["kv_index"]):
                got[:, 0, :, r["L"] + j] = _rotate(want[:, 0, :, r["L"] + j], node - j, inv)
    elif fault == "rope_from_new_length":
        for r in steps:
            for j in range(r["a"]):
                got[:, 0, :, r["L"] + j] = _rotate(want[:, 0, :, r["L"] + j], r["a"], inv)
    elif fault == "length_minus_one":
        s = steps[0]["L1"] - 1                                                  # every later row lands one row early
        got[:, :, :, s:N - 1] = want[:, :, :, s + 1:]
    elif fault == "length_plus_one":
        s = steps[0]["L1"]                                                      # ... one row late; row s keeps a rejected node's rows
        got[:, :, :, s + 1:] = want[:, :, :, s:N - 1]
        r = steps[0]
        left = [i for i in range(r["n"]) if i not in r["kv_index"]]
        got[:, :, :, s] = draft_rows(master, text, r)[:, :, :, left[0]]
    elif fault == "wrap_into_next_head":
        got[:, :, 1:, 0] = want[:, :, :-1, N - 1]                               # head h's row behind the end is head h + 1's row 0
    else:
        raise KeyError(fault)
    return got
