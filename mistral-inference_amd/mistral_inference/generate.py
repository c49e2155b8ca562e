"""`generate()` with the reference's contract (generate.py:43-170), minus its host round trips.

Same arguments, same return value: `(tokens, logprobs)` where logprobs hold prompt tokens 1..n-1 then the
generated tokens, `tokens == []` when nothing was generated, sequences keep generating until ALL have hit
`eos_id`, top-p is fixed at 0.8 at the call site (generate.py:126).

What changes is where the bookkeeping runs.  The reference reads one logprob per token with `.item()`
(one device sync per prompt token, generate.py:107,111, and per generated token, :134-136), allocates the
K/V buffers on the host before moving them (:69-78) and rebuilds mask metadata per layer per step.  Here
the cache is allocated in HBM once per call, logprobs are gathered on the device and copied back once at
the end, and a decode step is a single native call with no host metadata; the only per-token sync left
is the EOS test, and only when `eos_id` is given.
"""
import contextlib
import functools
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from .cache import BufferCache, check_kv_dtype
from .transformer import Transformer


@dataclass
class SpeculativeArgs:
    """Speculative decoding for `generate(speculative=...)`: every step drafts up to `k` tokens on the host and the model
    scores them in ONE pass over its weights (`Transformer.verify_step`), keeping the drafts its own argmaxes confirm - the
    tokens are those of the plain greedy loop.  The default drafter is prompt lookup (`ngram_draft`); `drafter` replaces it with
    any callable history -> drafts (history: prompt plus everything emitted so far; more than `k` drafts are cut).

    `sample=True` opts in to speculation at temperature > 0 (without it such a call is refused): a verify step then accepts a
    draft with its probability under the nucleus distribution and draws a replacement from the rest of that distribution at the
    first rejection (include/mistral_hip.h, `mi_verify_sample`).  What changes against the plain sampling loop: the generation
    has the plain sampler's DISTRIBUTION and is reproducible per `torch.manual_seed`, but it is not the plain sampler's tokens
    for a given seed.  At temperature 0 `sample` changes nothing: the greedy path."""
    k: int = 3
    ngram_max: int = 3
    ngram_min: int = 1
    drafter: Optional[Callable[[List[int]], Sequence[int]]] = None
    sample: bool = False

    def __post_init__(self) -> None:
        if not 1 <= self.k <= 7:
            raise ValueError(f"SpeculativeArgs.k = {self.k}: a verify step takes the last token and 1 .. 7 drafts")
        if not 1 <= self.ngram_min <= self.ngram_max:
            raise ValueError(f"SpeculativeArgs: 1 <= ngram_min <= ngram_max, got {self.ngram_min} .. {self.ngram_max}")

    def draft(self, history: List[int]) -> List[int]:
        d = self.drafter(history) if self.drafter is not None else ngram_draft(history, self.k, self.ngram_max, self.ngram_min)
        return [int(t) for t in list(d)[: self.k]]


def ngram_draft(history: Sequence[int], k: int, ngram_max: int = 3, ngram_min: int = 1) -> List[int]:
    """Prompt lookup: the longest suffix n-gram of `history` (n from ngram_max down to ngram_min) that occurs earlier in it; of
    its earlier occurrences the most recent one; the (up to) k tokens that followed it there.  No match: []."""
    h = list(history)
    L = len(h)
    for n in range(min(ngram_max, L - 1), ngram_min - 1, -1):
        suffix = h[L - n:]
        for start in range(L - n - 1, -1, -1):  # most recent earlier occurrence first
            if h[start: start + n] == suffix:
                return h[start + n: start + n + k]
    return []


def refuse_speculative(model, n_prompts: int, temperature: float, kv_dtype: Optional[torch.dtype],
                       speculative: Optional[SpeculativeArgs] = None) -> None:
    """What generate(speculative=...) does not take, by name, before anything runs."""
    if temperature > 0 and not (speculative is not None and speculative.sample):
        raise NotImplementedError(f"speculative decoding at temperature {temperature} > 0 verifies by sampling, which changes the tokens "
                                  "a seed gives (not their distribution): opt in with SpeculativeArgs(sample=True), or pass temperature=0")
    if n_prompts != 1:
        raise NotImplementedError(f"speculative decoding of {n_prompts} prompts is not implemented: one prompt per call")
    if kv_dtype == torch.float8_e4m3fn:
        raise NotImplementedError("speculative decoding on an FP8 K/V cache (kv_dtype=float8_e4m3fn) is not implemented; "
                                  "use the model's own bf16 rings")
    if not hasattr(model, "verify_step"):
        raise NotImplementedError("speculative decoding: this model has no verify_step")
    if hasattr(model, "refuse_verify"):
        model.refuse_verify(None, model_only=True)  # (the model's own refusals but the cache's: pipeline ranks, storage dtype, un-merged LoRA)


def _unpins_adapters(fn):
    """generate() pins its per-sequence adapter slots on the model (`adapters=`) for the length of the call: whatever way the
    call ends, forward() decides them per call again afterwards."""
    @functools.wraps(fn)
    def wrapper(encoded_prompts, model, *args, **kwargs):
        try:
            return fn(encoded_prompts, model, *args, **kwargs)
        finally:
            if hasattr(model, "unpin_adapters"):
                model.unpin_adapters()
    return wrapper


@_unpins_adapters
@torch.inference_mode()
def generate(
    encoded_prompts: List[List[int]],
    model: Transformer,
    images: List[List] = [],
    *,
    max_tokens: int,
    temperature: float,
    chunk_size: Optional[int] = None,
    eos_id: Optional[int] = None,
    adapters: Optional[List[int]] = None,
    kv_dtype: Optional[torch.dtype] = None,
    speculative: Optional[SpeculativeArgs] = None,
) -> Tuple[List[List[int]], List[List[float]]]:
    # speculative (one prompt, bf16 rings, one stage; temperature > 0 only with sample=True): the decode loop runs verify steps -
    # see SpeculativeArgs; at temperature 0 the returned tokens and log-probs are the plain loop's, at temperature > 0 their
    # distribution is; max_tokens truncation and EOS stop are the plain loop's.  None: the plain loop.
    if speculative is not None:
        refuse_speculative(model, len(encoded_prompts), temperature, kv_dtype, speculative)
    # kv_dtype: dtype of the K/V rings; None: the model's.  torch.float8_e4m3fn (bf16 models on the tuned path): rings of e4m3 bytes
    # at half the size, written and read by the rule of cache.kv_quantize / kv_dequantize; such a generation takes the launch path.
    kv_dtype = check_kv_dtype(kv_dtype, model.dtype)   # (before anything is pinned or allocated)
    # adapters (a model built with `lora`, Transformer.set_lora_slots): one adapter slot per prompt, -1 = the base model; written
    # to the device ONCE here, before the first prefill chunk - every forward, prompt_logprobs call and the decode session below
    # run with it.  None: slot 0 for every sequence.
    if hasattr(model, "pin_adapters"):
        model.pin_adapters(adapters, len(encoded_prompts))
    elif adapters is not None:
        raise ValueError("adapters=...: this model runs one adapter set")
    images_torch: List[List[torch.Tensor]] = []
    if images:  # reference generate.py:54-60: one list of [C, H, W] arrays per sample; no chunking with images
        assert chunk_size is None
        images_torch = [[torch.as_tensor(im).to(device=model.device, dtype=model.dtype) for im in images_for_sample]
                        for images_for_sample in images]
    flattened_images: List[torch.Tensor] = sum(images_torch, [])
    model = model.eval()

    # K/V rings, straight in device memory (reference generate.py:67-78)
    cache_window = max(len(x) for x in encoded_prompts) + max_tokens
    cache = BufferCache(model.n_local_layers, model.args.max_batch_size, cache_window, model.args.n_kv_heads,
                        model.args.head_dim, model.args.sliding_window, device=model.device, dtype=kv_dtype)
    cache.reset()

    last_token_prelogits, lp_chunks = _run_prompt(encoded_prompts, model, cache, chunk_size, flattened_images)

    # ---- decode (reference generate.py:120-140): exactly one decoder runs, or none
    generated: List[torch.Tensor] = []
    gen_lp: List[torch.Tensor] = []
    spec_out: Optional[Tuple[List[int], List[float]]] = None
    decoder = _pick_decoder(model, model.device.type, temperature, max_tokens, speculative)
    if decoder == "speculative":
        spec_out = _decode_speculative(model, cache, last_token_prelogits, max_tokens, temperature, eos_id,
                                       speculative, encoded_prompts[0])
    elif decoder == "session":
        generated, gen_lp = _decode_session(model, cache, last_token_prelogits, max_tokens, temperature, eos_id)
    elif decoder == "loop":
        generated, gen_lp = _decode_loop(model, cache, last_token_prelogits, max_tokens, temperature, eos_id)

    result = _copy_back(len(encoded_prompts), lp_chunks, generated, gen_lp, spec_out)
    _raise_if_flagged(model)
    return result


# ---- which decoder: every read of the model's decode capabilities is here
def _pp_ranks(model) -> int:
    return getattr(model, "num_pipeline_ranks", 1)


def _pick_decoder(model, device_type: str, temperature: float, max_tokens: int, speculative: Optional[SpeculativeArgs]) -> str:
    """Which decoder generate() runs: "none", "speculative" (_decode_speculative), "session" (_decode_session) or "loop"
    (_decode_loop)."""
    if max_tokens <= 0:
        return "none"
    if speculative is not None:
        return "speculative"
    if (hasattr(model, "greedy_session")
            and (device_type == "cuda" or (temperature == 0 and getattr(model, "greedy_session_any_device", False)))  # (CPU stand-ins: tests)
            and (_pp_ranks(model) == 1 or getattr(model, "greedy_session_pp", False))
            and getattr(model, "softmax_fp32", True)
            and getattr(model, "fused_greedy", True)):  # (model.fused_greedy = False: the host loop, for A/B)
        return "session"
    return "loop"


def _loop_shares_seed(model, temperature: float) -> bool:
    """_decode_loop under pipeline parallelism at temperature > 0: every stage samples the same broadcast logits and must draw
    the same variate whatever state its own CPU generator is in - step i uses (the agreed seed, offset i)."""
    return temperature > 0 and _pp_ranks(model) > 1 and hasattr(model, "pp_comm")


def _graph_context(model, cache: BufferCache):
    """Inside it decode steps replay a captured hipGraph (single rank; no-op otherwise)."""
    return model.graphed_decode(cache) if hasattr(model, "graphed_decode") else contextlib.nullcontext()


def _fused_prompt_logprobs(model) -> bool:
    """The prompt route: True - `model.prompt_logprobs` reduces the logits to the wanted log-probabilities inside the LM head
    GEMM; False - `forward` returns the [T, V] logits and generate() takes their log_softmax."""
    return bool(getattr(model, "supports_prompt_logprobs", False) and getattr(model, "softmax_fp32", True)
                and (model.device.type == "cuda" or getattr(model, "prompt_logprobs_any_device", False)))


# ---- prompt, by chunks (reference generate.py:91-118)
def _run_prompt(encoded_prompts: List[List[int]], model, cache: BufferCache, chunk_size: Optional[int],
                images: List[torch.Tensor]) -> Tuple[torch.Tensor, List[Tuple[int, torch.Tensor]]]:
    """(logits after every prompt's last token [B, V], the prompt's log-prob pieces).  The pieces stay on the device:
    (sequence, tensor) in emission order."""
    B, V, dev = len(encoded_prompts), model.args.vocab_size, model.device
    lp_chunks: List[Tuple[int, torch.Tensor]] = []
    last_token_prelogits: Optional[torch.Tensor] = None
    max_prompt_len = max(len(x) for x in encoded_prompts)
    if chunk_size is None:
        chunk_size = max_prompt_len
    for s in range(0, max_prompt_len, chunk_size):
        prompt_chunks = [p[s: s + chunk_size] for p in encoded_prompts]
        assert all(len(p) > 0 for p in prompt_chunks)
        flat_ids = sum(prompt_chunks, [])
        if min(flat_ids) < 0 or max(flat_ids) >= V:  # the prompt is host data: raise where nn.Embedding would (transformer.py:193)
            raise IndexError("index out of range in self")
        flat = torch.tensor(flat_ids, device=dev, dtype=torch.long)
        # token i+1 of each chunk is scored by position i
        rows, cols, owners = [], [], []
        offset = 0
        for b, seq in enumerate(prompt_chunks):
            n = len(seq) - 1
            rows += list(range(offset, offset + n))
            cols += seq[1:]
            owners.append((b, n))
            offset += len(seq)
        if _fused_prompt_logprobs(model):
            # the [T, V] logits are never materialised: the LM head GEMM reduces them to the wanted log-probabilities
            tgt = torch.full((flat.numel(),), -1, dtype=torch.int32)
            if rows:
                tgt[rows] = torch.tensor(cols, dtype=torch.int32)
            lp_rows, last_rows = model.prompt_logprobs(flat, [len(p) for p in prompt_chunks], cache, tgt.to(dev), images=images)
            picked_rows = lp_rows[torch.tensor(rows, device=dev, dtype=torch.long)] if rows else None
        else:
            prelogits = model.forward(flat, seqlens=[len(p) for p in prompt_chunks], cache=cache, images=images)
            logits = torch.log_softmax(prelogits, dim=-1)
            picked_rows = None
            if rows:
                idx = torch.tensor([rows, cols], device=dev, dtype=torch.long)
                picked_rows = logits[idx[0], idx[1]]
            ends = torch.tensor([len(p) for p in prompt_chunks], device=dev).cumsum(dim=0) - 1
            last_rows = prelogits.index_select(0, ends)

        if last_token_prelogits is not None:
            # first token of this chunk is scored by the previous chunk's last position
            firsts = torch.tensor([p[0] for p in prompt_chunks], device=dev, dtype=torch.long)
            picked = _logprob_of(last_token_prelogits, firsts)
            for b in range(B):
                lp_chunks.append((b, picked[b: b + 1]))
        if picked_rows is not None:
            o = 0
            for b, n in owners:
                if n:
                    lp_chunks.append((b, picked_rows[o: o + n]))
                o += n
        last_token_prelogits = last_rows
        assert last_token_prelogits.shape == (B, V)
    assert last_token_prelogits is not None
    return last_token_prelogits, lp_chunks


# ---- the pieces the decoders share
def _logprob_of(prelogits: torch.Tensor, tokens: torch.Tensor) -> torch.Tensor:
    return torch.log_softmax(prelogits, dim=-1).gather(1, tokens[:, None])[:, 0]


def _first_token(prelogits: torch.Tensor, temperature: float, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The token after the prompt and its log-prob, [B] each, as a decoder that samples on the device itself draws it: the
    argmax at temperature 0, else the native nucleus draw at an offset no decode step of the same seed reaches."""
    if temperature > 0:
        from . import _hip
        return _hip.sample_top_p(prelogits.contiguous(), temperature, 0.8, seed=seed, offset=1 << 63)
    token = sample(prelogits, temperature=0.0, top_p=0.8)
    return token, _logprob_of(prelogits, token)


def _agree_seed(model) -> int:
    """ONE seed per generation, from torch's default generator (torch.manual_seed makes a generation reproducible).  The
    reference's pipeline ranks stay in step only because they share torch's default seed (generate.py:126 on every rank); here
    rank 0's seed is the generation's seed on every stage, agreed over `model.pp_comm` - where the model and its pipeline
    communicator are known.  `sample()` itself issues no collective: a data-parallel job, or ranks that generate different
    things, never meet in it (the reference's sample() has none either, generate.py:151-159)."""
    seed_t = torch.randint(0, 2 ** 62, (1,))
    if _pp_ranks(model) > 1:
        seed_t = seed_t.to(model.device)
        model.pp_comm.broadcast(seed_t, src=0)
    return int(seed_t.item())


# ---- the three decoders: (model, cache, last_token_prelogits, max_tokens > 0, temperature, eos_id, ...)
def _decode_speculative(model, cache: BufferCache, last_token_prelogits: torch.Tensor, max_tokens: int, temperature: float,
                        eos_id: Optional[int], speculative: SpeculativeArgs, prompt: List[int]) -> Tuple[List[int], List[float]]:
    """One prompt: (tokens, logprobs) as host lists.  Token 0 comes from the prompt's last logits as in the plain loop; every
    later step scores [last emitted token] + drafts and emits the rows the step confirms - at temperature 0 the argmaxes, at
    temperature > 0 (SpeculativeArgs.sample) the sampled verification with one seed per generation from torch's default
    generator and the step's index as the Philox counter.  One synchronisation per step (n_accept), which also brings the tokens."""
    V, dev = model.args.vocab_size, model.device
    seed = _agree_seed(model) if temperature > 0 else 0
    t0, lp0 = _first_token(last_token_prelogits, temperature, seed)
    toks, lps = [int(t0[0])], [float(lp0[0])]
    if eos_id is not None and toks[0] == eos_id:
        return [], []
    history = list(prompt) + toks
    done = False
    step = 0
    while not done and len(toks) < max_tokens:
        drafts = speculative.draft(history)[: max_tokens - len(toks) - 1]
        if any(d < 0 or d >= V for d in drafts):
            raise IndexError("index out of range in self (a drafted token)")
        ids = torch.tensor([history[-1]] + drafts, device=dev, dtype=torch.long)
        if temperature > 0:
            tok, lp, n_accept = model.verify_step(ids, [len(drafts) + 1], cache, temperature=temperature, top_p=0.8, seed=seed, offset=step)
        else:
            tok, lp, n_accept = model.verify_step(ids, [len(drafts) + 1], cache)
        step += 1
        new_t, new_lp = tok[: n_accept[0] + 1].tolist(), lp[: n_accept[0] + 1].tolist()
        for t, l in zip(new_t, new_lp):
            if eos_id is not None and t == eos_id:  # generate.py:128-132: the EOS token itself is not returned
                done = True
                break
            if len(toks) == max_tokens:
                break
            toks.append(int(t))
            lps.append(float(l))
            history.append(int(t))
    return toks, lps


def _decode_session(model, cache: BufferCache, last_token_prelogits: torch.Tensor, max_tokens: int, temperature: float,
                    eos_id: Optional[int]) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
    """The sample rides on the LM head inside the step (GreedySession): argmax + log-softmax at temperature 0, the native
    nucleus draw (csrc/sampling.hip, generate.py:151-170 in one kernel) otherwise.  It feeds the next step on the device, and
    the tokens come back in one copy per chunk of steps.  The session is one HIP stage, or pipeline stages with a session
    each; the sample then crosses from the last stage to the first as 8 bytes per sequence instead of the reference's
    [B, vocab] logits broadcast.  Temperature 0: the same values as _decode_loop (token i+1 = first argmax of the logits after
    token i; its logprob = log_softmax at it).  Temperature > 0: the same distribution as _decode_loop, drawn from a Philox
    stream seeded from torch's default generator (torch.multinomial's own stream cannot be reproduced by any other sampler);
    only the last stage draws."""
    generated: List[torch.Tensor] = []
    gen_lp: List[torch.Tensor] = []
    is_finished = torch.zeros(last_token_prelogits.shape[0], dtype=torch.bool, device=model.device)
    seed = _agree_seed(model) if temperature > 0 else 0
    next_token, first_lp = _first_token(last_token_prelogits, temperature, seed)
    if eos_id is not None:
        is_finished = is_finished | (next_token == eos_id)
        if bool(is_finished.all()):
            return generated, gen_lp
    generated.append(next_token)
    gen_lp.append(first_lp)
    sess = (model.greedy_session(cache, next_token, temperature=temperature, top_p=0.8, seed=seed) if temperature > 0
            else model.greedy_session(cache, next_token))
    need = max_tokens - 1            # (the reference's last forward only feeds a sample nobody draws)
    chunk = 32 if eos_id is not None else sess.HIST
    stop = False
    while need > 0 and not stop:
        n = min(need, chunk)
        sess.run(n)
        toks, lps = sess.collect(n)  # [n, B] each; one synchronisation per chunk
        keep = n
        if eos_id is not None:       # generate.py:128-132: stop BEFORE the step at which every sequence has hit EOS
            fin = is_finished[None, :] | ((toks == eos_id).cumsum(0) > 0)
            all_fin = fin.all(dim=1)
            if bool(all_fin.any()):
                keep = int(torch.nonzero(all_fin)[0, 0])
                stop = True
            is_finished = fin[keep - 1] if keep > 0 else is_finished
        for j in range(keep):
            generated.append(toks[j])
            gen_lp.append(lps[j])
        need -= n
    return generated, gen_lp


def _decode_loop(model, cache: BufferCache, last_token_prelogits: torch.Tensor, max_tokens: int, temperature: float,
                 eos_id: Optional[int]) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
    """The reference's loop: sample on the host side of the logits, one `forward` per token."""
    B, V = last_token_prelogits.shape
    generated: List[torch.Tensor] = []
    gen_lp: List[torch.Tensor] = []
    is_finished = torch.zeros(B, dtype=torch.bool, device=model.device)
    pp_seed = _agree_seed(model) if _loop_shares_seed(model, temperature) else None
    with _graph_context(model, cache):  # (the only place the context is entered)
        for step in range(max_tokens):
            next_token = sample(last_token_prelogits, temperature=temperature, top_p=0.8, seed=pp_seed, offset=step)
            if eos_id is not None:
                is_finished = is_finished | (next_token == eos_id)
                if bool(is_finished.all()):  # the one remaining per-token sync, only with an eos_id
                    break
            gen_lp.append(_logprob_of(last_token_prelogits, next_token))
            generated.append(next_token)
            # under the graph the returned tensor is the graph's output buffer (overwritten by the next step);
            # everything derived from it (next token, logprob) is computed before that happens
            last_token_prelogits = model.forward(next_token, seqlens=[1] * B, cache=cache)
            assert last_token_prelogits.shape == (B, V)
    return generated, gen_lp


# ---- one copy back
def _copy_back(B: int, lp_chunks: List[Tuple[int, torch.Tensor]], generated: List[torch.Tensor], gen_lp: List[torch.Tensor],
               spec_out: Optional[Tuple[List[int], List[float]]]) -> Tuple[List[List[int]], List[List[float]]]:
    logprobs: List[List[float]] = [[] for _ in range(B)]
    if lp_chunks:
        flat_lp = torch.cat([t for _, t in lp_chunks]).tolist()
        o = 0
        for b, t in lp_chunks:
            n = t.numel()
            logprobs[b].extend(flat_lp[o: o + n])
            o += n
    generated_tokens: List[List[int]] = []
    if generated:
        generated_tokens = torch.stack(generated, 1).tolist()
        lp = torch.stack(gen_lp, 1).tolist()
        for b in range(B):
            logprobs[b].extend(lp[b])
    elif spec_out is not None and spec_out[0]:
        generated_tokens = [spec_out[0]]
        logprobs[0].extend(spec_out[1])
    return generated_tokens, logprobs


def _raise_if_flagged(model) -> None:
    """The copies back synchronised the stream: the place to turn device-side flags (an out-of-range token id seen by the
    embedding kernel, a timed-out wait of the decode engine) into the exceptions the reference would have raised."""
    backend = getattr(model, "_backend", None)
    if hasattr(backend, "raise_if_flagged"):
        backend.raise_if_flagged()


def sample(logits: torch.Tensor, temperature: float, top_p: float, seed: Optional[int] = None, offset: int = 0) -> torch.Tensor:
    """Greedy for temperature 0, else nucleus sampling (reference generate.py:151-159).  fp32 logits on a HIP device: ONE
    native launch (mi_sample_top_p: no sort of the vocabulary, no host sync).

    Seeding contract: `seed=None` draws one 62-bit seed per call from torch's DEFAULT (CPU) generator, i.e. `torch.manual_seed`
    makes a generation reproducible; a seeded CUDA generator (what the reference's torch.multinomial consumes) does not enter.
    A caller that needs several ranks to draw the same token (pipeline stages sampling the same broadcast logits) agrees on a
    seed itself and passes it with a per-step `offset` - `generate()` does, over the model's pipeline communicator; this
    function never communicates."""
    if temperature > 0 and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2:
        from . import _hip
        if seed is None:
            seed, offset = int(torch.randint(0, 2 ** 62, (1,)).item()), 0
        tok, _ = _hip.sample_top_p(logits.contiguous(), temperature, top_p, seed=seed, offset=offset)
        return tok.reshape(-1)
    if temperature > 0:
        probs = torch.softmax(logits / temperature, dim=-1)
        next_token = sample_top_p(probs, top_p)
    else:
        next_token = torch.argmax(logits, dim=-1).unsqueeze(0)
    return next_token.reshape(-1)


def sample_top_p(probs: torch.Tensor, p: float) -> torch.Tensor:
    """Reference generate.py:162-170: keep the smallest prefix of the sorted distribution whose mass
    before the token is <= p, renormalise, draw one."""
    assert 0 <= p <= 1
    sorted_probs, order = torch.sort(probs, dim=-1, descending=True)
    mass_before = torch.cumsum(sorted_probs, dim=-1) - sorted_probs
    sorted_probs = sorted_probs.masked_fill(mass_before > p, 0.0)
    sorted_probs = sorted_probs / sorted_probs.sum(dim=-1, keepdim=True)
    pick = torch.multinomial(sorted_probs, num_samples=1)
    return torch.gather(order, -1, pick)
