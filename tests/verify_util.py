"""Shared by tests/test_gpu_verify_step.py and tests/test_gpu_speculative.py: the two small models of the verify-step tests (a
dense one and a 4-expert top-2 one, two layers, rings of 32 slots), their checkpoints, cache helpers; no test functions here."""
import torch

import mistral_oracle as mo
from hip_util import write_checkpoint

BF = torch.bfloat16
W = 32
DENSE = mo.OracleArgs(dim=512, n_layers=2, head_dim=128, hidden_dim=1024, n_heads=4, n_kv_heads=2, norm_eps=1e-5, vocab_size=512,
                      sliding_window=W)
MOE = mo.OracleArgs(dim=512, n_layers=2, head_dim=128, hidden_dim=1024, n_heads=4, n_kv_heads=2, norm_eps=1e-5, vocab_size=512,
                    sliding_window=W, num_experts=4, num_experts_per_tok=2)
ARGS = {"dense": DENSE, "moe": MOE}
SEED = 21
ALPHA = 5.0


def weights(kind):
    """mistral_oracle.synth_weights with a CONFIDENT LM head: output[v] += ALPHA / dim * tok_embeddings[perm[v]] for a fixed random
    permutation.  With the plain synthetic head the top-2 logit margin of a greedy step is below one bf16 ulp of the logits at
    about one step in three (512 nearly exchangeable logits), so no 48-step generation can be compared token by token between two
    summation orders.  With the added term the row of the current token's successor under the permutation leads by 1.5 or more
    (CPU oracle, test_gpu_speculative.py) while attention and FFN still move every logit."""
    a = ARGS[kind]
    w = mo.synth_weights(a, seed=SEED)
    perm = torch.randperm(a.vocab_size, generator=torch.Generator().manual_seed(SEED + 1000))
    w["output.weight"] = (w["output.weight"].float() + ALPHA / a.dim * w["tok_embeddings.weight"].float()[perm]).to(BF)
    return w


def make_folder(kind, tmp_path_factory):
    return write_checkpoint(tmp_path_factory.mktemp("verify_" + kind) / "bf16", ARGS[kind], weights(kind))


def load(folder, B=2, **kw):
    from mistral_inference.transformer import Transformer
    return Transformer.from_folder(folder, max_batch_size=B, device="cuda", dtype=BF, **kw)


def new_cache(B, max_seq_len=160):
    from mistral_inference.cache import BufferCache
    return BufferCache(DENSE.n_layers, B, max_seq_len, DENSE.n_kv_heads, DENSE.head_dim, W, device="cuda", dtype=BF)


def clone_cache(c):
    """A cache of the same geometry holding the same bytes and the same positions."""
    from mistral_inference.cache import BufferCache
    n = BufferCache(c.n_layers, c.max_batch_size, c.max_seq_len, c.n_kv_heads, c.head_dim, W, device=c.device, dtype=c.cache_k[0].dtype)
    assert n.cache_sizes == c.cache_sizes
    for i in range(c.n_layers):
        n.cache_k[i].copy_(c.cache_k[i])
        n.cache_v[i].copy_(c.cache_v[i])
    n.kv_seqlens = c.kv_seqlens.clone()
    n._seen = list(c._seen)
    return n


def bits(t):
    """A ring's payload as integers (a never-written slot may hold NaN bits, which compare unequal as numbers)."""
    return t.contiguous().view(torch.int16)


def prompt(n, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    return torch.randint(0, DENSE.vocab_size, (n,), generator=g).tolist()
