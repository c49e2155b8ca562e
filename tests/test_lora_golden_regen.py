"""The un-merged LoRA fixtures (tests/golden/lora_*) against the unmodified reference, where its source exists (the build
container; skipped elsewhere):

* tests/make_golden_lora.py regenerates them bit for bit;
* `lora_util.lora_linear_ref` - the numerics contract of csrc/lora.hip written out in torch - equals the reference's
  `LoRALinear.forward` exactly on CPU bf16 inputs;
* teeth: in every forward of every case the stored logits are further from those of the same model WITHOUT adapters (run here by
  the reference, teacher-forced on the stored tokens) than four times the tolerance of the GPU replay at that logit's magnitude,
  so a build that ignores an adapter cannot pass tests/test_gpu_lora.py.

One subprocess does all three (it imports the reference under the package name the product also uses)."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MISTRAL_REFERENCE_SRC", "/root/reference/src")
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "mistral_inference")), reason="reference source not present")

SCRIPT = textwrap.dedent("""
    import json, os, sys, torch
    sys.path.insert(0, os.path.join({root!r}, "tests"))
    import make_golden_lora as mg
    import lora_util
    from safetensors.torch import load_file
    res = {{"regen_bad": [], "ref_maxdiff": {{}}, "teeth": {{}}}}
    mg.main({out!r})
    new_index = json.load(open(os.path.join({out!r}, "lora_index.json")))
    res["index_equal"] = new_index == lora_util.lora_index()
    for name, (over, rank, prompts, max_tokens, chunk) in mg.CASES.items():
        files = [name] + [f"{{name}}.adapters.{{l}}" for l in range(mg.TINY["n_layers"])]
        for fn in files:
            new = load_file(os.path.join({out!r}, fn + ".safetensors"))
            old = load_file(os.path.join(lora_util.GOLDEN, fn + ".safetensors"))
            if set(new) != set(old):
                res["regen_bad"].append((fn, "keys"))
                continue
            for k in old:
                a, b = new[k], old[k]
                if a.dtype != b.dtype or a.shape != b.shape or not torch.equal(torch.nan_to_num(a.double(), nan=7.0),
                                                                                torch.nan_to_num(b.double(), nan=7.0)):
                    res["regen_bad"].append((fn, k))
        # teeth: the same model with the zero adapters of a base checkpoint, teacher-forced on the stored tokens
        stored = load_file(os.path.join(lora_util.GOLDEN, name + ".safetensors"))
        _, _, base = mg.build(over, rank, None)
        outs = mg.replay(base, prompts, stored["tokens"].tolist(), chunk, max_tokens)
        n_pre = sum(1 for k in stored if k.startswith("prefill_logits."))
        keys = [f"prefill_logits.{{c}}" for c in range(n_pre)] + [f"decode_logits.{{s}}" for s in range(len(outs) - n_pre)]
        margins = []
        for key, o in zip(keys, outs):
            ref = stored[key]
            tol = torch.minimum(torch.full_like(ref, 4e-2), 3.0 * ref.abs().clamp(min=1.0) * 2.0 ** -7)  # tests/test_gpu_lora.py
            margins.append(float(((o - ref).abs() / tol).max()))
        res["teeth"][name] = margins
    # the restatement against LoRALinear.forward itself, every rank of the fixtures, 5 rows
    g = torch.Generator().manual_seed(5)
    for rank in (8, 16, 64):
        for fin, fout in ((256, 512), (512, 256)):
            m = mg.LoRALinear(fin, fout, rank, 2.0).to(torch.bfloat16)
            with torch.no_grad():
                m.linear.weight.copy_(torch.randn(fout, fin, generator=g) / fin ** 0.5)
                m.lora_A.weight.copy_(torch.randn(rank, fin, generator=g) / fin ** 0.5)
                m.lora_B.weight.copy_(torch.randn(fout, rank, generator=g) / rank ** 0.5)
                x = torch.randn(5, fin, generator=g).to(torch.bfloat16)
                ref = m(x)
            got = lora_util.lora_linear_ref(x, m.linear.weight, m.lora_A.weight, m.lora_B.weight, 2.0)
            res["ref_maxdiff"][f"{{rank}}:{{fin}}x{{fout}}"] = float((got.float() - ref.float()).abs().max())
    print("RESULT " + json.dumps(res))
""")


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    out = tmp_path_factory.mktemp("lora_regen")
    r = subprocess.run([sys.executable, "-c", SCRIPT.format(root=ROOT, out=str(out))], capture_output=True, text=True,
                       env=dict(os.environ, MISTRAL_REFERENCE_SRC=REF), timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(lines[-1][len("RESULT "):])


def test_lora_goldens_regenerate_bit_for_bit(result):
    assert result["index_equal"]
    assert not result["regen_bad"], result["regen_bad"]


def test_restatement_equals_the_reference_lora_linear_exactly(result):
    assert len(result["ref_maxdiff"]) == 6
    assert all(v == 0.0 for v in result["ref_maxdiff"].values()), result["ref_maxdiff"]


def test_every_forward_of_every_case_tells_the_adapters_from_none(result):
    assert sorted(result["teeth"]) == ["lora_dense_bf16", "lora_r64_bf16", "lora_swa_chunk_bf16"]
    for name, margins in result["teeth"].items():
        print(name, [round(m, 1) for m in margins])
        assert len(margins) >= 5 and min(margins) > 4.0, (name, margins)
