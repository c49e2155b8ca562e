"""Cases of the verify-step attention (mi_attn_verify) on the structured inputs of attn_cases.py, unchanged: helpers for
test_attn_verify_host.py and test_gpu_attn_verify.py; no test functions here.

A verify step of m rows on a sequence with `seen` cached positions is a prefill chunk of m rows as far as the expected output
goes (attn_cases.prefill_sequences / ref_attention64): row i at position seen + i sees seen + i - W < kp <= seen + i.  What is
new is where the keys are: NONE of the step's rows is in the ring, so on a wrapped ring slot (seen + j) % W still holds position
seen + j - W, which row i < j must read and rows i >= j must not.  The existing branches write the step's rows into the ring first;
`overwritten_first` is that defect as a mutant of the operation."""
import torch

import attn_cases as ac

HEADS = [(4, 4), (8, 2), (12, 2)]
RINGS = [16, 300, 4096]
ROWS = [1, 2, 5, 8]
BATCH2 = (300, (299, 603), (3, 5))      # W, seen, m: one B = 2 launch, a ring about to wrap beside one wrapped twice


def seen_values(W):
    """Cached positions before the step: the empty ring, then attn_cases.decode_lens (split edges, W - 1, W, W + 7, 2 W + 3)."""
    return [0] + ac.decode_lens(W)


def n_pos(W):
    return 2 * W + 3 + max(ROWS) + 1


def overwritten_first(qpos, kpos, W):
    """weight [s, n] of the mutant "the step's rows were written into the ring before the attention": row i finds, in the slot
    of every later row j, position seen + j where seen + j - W belongs - that key is lost and a future one is seen.  None where
    no row loses a key (the ring does not wrap under the step)."""
    w = ac.visibility(qpos, kpos, W, True).double()
    honest = w.clone()
    seen, m = int(qpos[0]), len(qpos)
    for i in range(m):
        for j in range(i + 1, m):
            lost = seen + j - W
            if lost >= 0 and lost > seen + i - W:       # a ring key inside row i's window
                w[i, kpos == lost] = 0
                w[i, kpos == seen + j] = 1
    return None if torch.equal(w, honest) else w
