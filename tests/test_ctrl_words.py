"""The workspace's control words have one definition on each side of the C ABI - the CTRL_* enum of csrc/kernels.h and
_hip.CTRL_WORDS - and the two agree in order and in value.  CPU only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mistral-inference_amd", "csrc")


def _c_enum():
    text = open(os.path.join(CSRC, "kernels.h")).read()
    bodies = [b for b in re.findall(r"enum\s*(?::\s*\w+\s*)?\{(.*?)\}", text, flags=re.S) if "CTRL_EPOCH" in b]
    assert len(bodies) == 1, "kernels.h: exactly one enum defines the control words"
    body = re.sub(r"//[^\n]*", "", bodies[0])
    pairs = re.findall(r"\b(CTRL_[A-Z0-9_]+)\s*=\s*(\d+)", body)
    assert len(pairs) == len([e for e in body.split(",") if e.strip()]), "every enumerator is CTRL_<NAME> = <number>"
    return [(n, int(v)) for n, v in pairs]


def test_c_enum_and_python_tuple_name_the_same_words_in_the_same_order():
    from mistral_inference import _hip
    enum = _c_enum()
    assert [v for _, v in enum] == list(range(len(enum)))                       # word i is enumerator i: no gap, no alias
    assert tuple(n[len("CTRL_"):].lower() for n, _ in enum) == _hip.CTRL_WORDS
    assert len(_hip.CTRL_WORDS) == 10 and _hip.CTRL_WORDS.index("bad_id") == 3 and _hip.CTRL_WORDS.index("steps") == 5


def test_no_source_indexes_a_control_word_by_number():
    pat = re.compile(r"ctrl *\[ *[0-9]|ctrl \+ [0-9]")
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h", ".cuh")):
            for i, line in enumerate(open(os.path.join(CSRC, f)), 1):
                assert not pat.search(line.split("//")[0]), f"{f}:{i}: {line.strip()}"


def test_helpers_touch_exactly_the_named_word():
    """ctrl_clear / ctrl_set on a host tensor laid out like a workspace; decode_engine_status keeps its keys."""
    import torch
    from mistral_inference import _hip
    ws = torch.arange(1, 65, dtype=torch.uint8)
    before = ws.clone()
    _hip.ctrl_clear(ws, "bad_id")
    assert ws[12:16].tolist() == [0, 0, 0, 0] and torch.equal(ws[:12], before[:12]) and torch.equal(ws[16:], before[16:])
    _hip.ctrl_set(ws, "steps", 0x01020304)
    assert ws[20:24].tolist() == [4, 3, 2, 1] and torch.equal(ws[16:20], before[16:20]) and torch.equal(ws[24:], before[24:])
    _hip.ctrl_set(ws, "steps", -1)
    assert ws[20:24].view(torch.int32).item() == 0x7FFFFFFF
    keys = [_hip._STATUS_KEYS.get(n, n) for n in _hip.CTRL_WORDS[:7]]
    assert keys == ["epoch", "status", "abort", "bad_id", "engine_launches", "steps", "arrivals"]
