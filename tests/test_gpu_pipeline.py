"""The HIP pipeline path with 2 ranks: real kernels, per-rank layer ranges, device-tensor send/recv, the prompt's
log-probability broadcast and the decode loop's GreedySession per stage (activations forward, the sample back to stage 0 as 8
bytes).  On a 1-GPU box both ranks share the GPU and the transport is gloo (RCCL refuses two ranks on one device); the same
cases are COLLECTED for "nccl" = RCCL with both transports and run wherever two GPUs are visible (bench.py --gpus N)."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, name, tmp, q, backend="gloo", transport="torch"):
    for p in (os.path.join(ROOT, "mistral-inference_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      MI_PP_TRANSPORT=transport, HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = "cuda:0" if backend == "gloo" else f"cuda:{rank}"   # gloo: both ranks share the box's one GPU
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        from golden_util import Case
        from hip_util import write_checkpoint
        from mistral_inference.generate import generate
        from mistral_inference.transformer import Transformer
        case = Case(name)
        folder = os.path.join(tmp, "ckpt")
        if rank == 0:
            write_checkpoint(folder, case.args, case.weights())
        dist.barrier()
        m = Transformer.from_folder(folder, max_batch_size=case.max_batch_size, num_pipeline_ranks=world, device=dev,
                                    dtype=torch.bfloat16)
        comm, big = m.pp_comm, []
        B, V = len(case.prompts), case.args.vocab_size

        class Recorder:  # what crosses between the stages at decode
            def send(self, t, dst):
                comm.send(t, dst)

            def recv(self, t, src):
                comm.recv(t, src)

            def broadcast(self, t, src):
                if tuple(t.shape) == (B, V):
                    big.append(tuple(t.shape))
                comm.broadcast(t, src)
        m._pp_comm = Recorder()
        prompts = case.prompts if rank == 0 else [[0] * len(p) for p in case.prompts]
        toks, lps = generate(prompts, m, max_tokens=case.max_tokens, temperature=0.0, chunk_size=case.chunk_size)
        q.put((rank, toks, lps, m.n_local_layers, sorted(m.layers.keys()), len(big), type(comm).__name__))
    finally:
        dist.destroy_process_group()


def _two_gpus():
    return torch.cuda.is_available() and torch.cuda.device_count() >= 2


@pytest.mark.parametrize("backend,transport", [
    ("gloo", "torch"),
    # collected everywhere, run where two GPUs exist (the driver's 8-GPU node): the reference's own transport over RCCL ...
    pytest.param("nccl", "torch", marks=pytest.mark.skipif(not _two_gpus(), reason="needs 2 GPUs (RCCL refuses two ranks on one device)")),
    # ... and the stream-ordered C-ABI communicator (mi_rccl_send / recv / bcast), hops captured in the decode hipGraph
    pytest.param("nccl", "rccl", marks=pytest.mark.skipif(not _two_gpus(), reason="needs 2 GPUs (RCCL refuses two ranks on one device)")),
])
@pytest.mark.parametrize("name", ["dense_bf16", "swa_chunk_bf16", "moe_bf16"])
def test_two_stage_pipeline_on_hip(name, backend, transport, tmp_path):
    from golden_util import Case
    case = Case(name)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + (os.getpid() % 500) + (sum(map(ord, name + backend + transport)) % 97)  # a fresh port per case (no TIME_WAIT reuse)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, name, str(tmp_path), q, backend, transport)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ref_toks, ref_lps = case.tokens(), case.logprobs()
    (_, t0, lp0, n0, k0, big0, comm0), (_, t1, lp1, n1, k1, big1, comm1) = res
    assert (n0, n1) == (1, 1) and k0 == ["0"] and k1 == ["1"]
    assert t0 == t1  # the last stage's samples, broadcast once per collect()
    # [B, vocab] broadcasts: exactly one per prompt chunk (the last rows generate() samples the first token from, reference
    # generate.py:101-118) and NONE per decode token - the sample crosses as 8 bytes per sequence (the reference: one per token)
    chunk = case.chunk_size or max(len(p) for p in case.prompts)
    n_chunks = -(-max(len(p) for p in case.prompts) // chunk)
    assert big0 == n_chunks and big1 == n_chunks, (big0, big1, n_chunks)
    assert comm0 == comm1 == ("RcclComm" if transport == "rccl" else "TorchDistComm")
    for b, (mine, ref) in enumerate(zip(t0, ref_toks)):
        n = next((i for i, (x, y) in enumerate(zip(mine, ref)) if x != y), len(ref))
        # every greedy token of the reference (round 6: the gloo hops of this rig are ordered behind the producing stream -
        # distributed.TorchDistComm; before, a stage could read a hidden state its kernel had not finished and the sequences
        # left the reference's after 2-3 tokens, differently from run to run)
        assert n == len(ref), (name, b, mine, ref)
        npl = len(case.prompts[b]) - 1 + n
        dev = max(abs(x - y) for x, y in zip(lp0[b][:npl], ref_lps[b][:npl]))
        print(f"{name} [{backend}/{transport}] sequence {b}: tokens agree for {n}/{len(ref)}, max |logprob - reference| {dev:.4f} over {npl}", flush=True)
        assert dev <= 6e-2


def test_bench_two_ranks_prints_one_json_line():
    """bench.py's N > 1 path (pipeline stages, max-over-ranks timing, rank-0 report, orderly shutdown) with two ranks
    sharing this box's GPU over gloo; on a multi-GPU node the same code runs over RCCL."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # (two ranks on ONE GPU: the persistent engine of one rank cannot be resident beside the other's when both decode at the
    # same time - the interleaved measurement - so this rig takes the launch path; one rank per GPU keeps the engine)
    env = dict(os.environ, MI_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MI_DECODE_ENGINE="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29377", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2",
           "--layers", "4", "--prefill", "256", "--mixtral-layers", "2", "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    # N > 1 headline = the BASELINE metric: ONE sequence relayed through the stages (strong scaling, the reference's pipeline);
    # the throughput mode (one sequence per stage in flight) in its own object, with the host cost per tick of its loop
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["scaling"] == "strong" and d["value"] > 0
    assert d["metric"].startswith("decode tokens/sec/GPU (batch=1")
    pt = d["pipeline_throughput"]
    assert pt["sequences_in_flight"] == 2 and pt["scaling"] == "weak" and pt["tokens_per_s"] > 0 and pt["tick_host_us"] > 0
    assert abs(pt["tokens_per_s_per_gpu"] * 2 - pt["tokens_per_s"]) < 0.02
    assert d["distributed"] == {"backend": "gloo", "world_size": 2, "transport": "TorchDistComm", "rccl_comm_ranks": None}
    assert d["roofline"]["bound"] == "hbm"
    cb = d["cpu_baseline"]   # round 6: computed by rank 0 at every N (the whole headline model on the host cores)
    assert cb["kind"] in ("reference", "port") and cb["value"] > 0 and cb["cores"] >= 1
    per_rank = d["roofline_per_rank"]
    assert [r["rank"] for r in per_rank] == [0, 1] and [r["lm_head"] for r in per_rank] == [False, True]
    assert all(0 < r["frac"] < 1 and r["layers"] == 2 for r in per_rank)
    # north_star's multi-GPU model: a Mixtral sub-measurement over the same stages (8x7B dims for N < 8, layer-truncated here)
    mx = d["mixtral"]
    assert "Mixtral-8x7B" in mx["model"] and mx["tokens_per_s"] > 0 and 0 < mx["hbm_roofline_frac"] < 1 and mx["prefill_tokens_per_s"] > 0
    assert mx["pipeline_throughput"]["sequences_in_flight"] == 2 and mx["pipeline_throughput"]["tokens_per_s"] > 0


def test_plain_bench_invocation_spawns_its_own_ranks():
    """`python bench.py --gpus 2` with NO torchrun environment (the shape of the driver's N = 1 command with another N) must
    start its two ranks itself and still print exactly one JSON line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["MI_DIST_BACKEND"] = "gloo"  # two ranks on this box's one GPU (RCCL refuses that); "nccl" on a multi-GPU node
    env["MI_DECODE_ENGINE"] = "0"    # (see above: two engines cannot share one GPU)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2", "--layers", "2",
           "--prefill", "128", "--no-mixtral"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["value"] > 0 and "pp2" in d["config"]["parallelism"]


def _interleaved_worker(rank, world, port, name, tmp, q, backend, n_dec):
    for p in (os.path.join(ROOT, "mistral-inference_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      MI_PP_TRANSPORT="torch", HSA_ENABLE_IPC_MODE_LEGACY="0")
    if backend == "gloo":
        os.environ["MI_DECODE_ENGINE"] = "0"  # both stages decode at the same time on ONE GPU here: no room for two engines
    dev = "cuda:0" if backend == "gloo" else f"cuda:{rank}"
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        from golden_util import Case
        from hip_util import write_checkpoint
        from mistral_inference.cache import BufferCache
        from mistral_inference.pipeline_decode import InterleavedDecoder
        from mistral_inference.transformer import Transformer
        case = Case(name)
        folder = os.path.join(tmp, "ckpt")
        if rank == 0:
            write_checkpoint(folder, case.args, case.weights())
        dist.barrier()
        m = Transformer.from_folder(folder, max_batch_size=1, num_pipeline_ranks=world, device=dev, dtype=torch.bfloat16)
        a = m.args
        caches, first = [], []
        for pr in case.prompts[:world]:
            c = BufferCache(m.n_local_layers, 1, len(pr) + n_dec + 4, a.n_kv_heads, a.head_dim, a.sliding_window, device=dev,
                            dtype=torch.bfloat16)
            c.reset()
            ids = torch.tensor(pr if rank == 0 else [0] * len(pr), dtype=torch.long)
            logits = m.forward(ids, [len(pr)], c)
            first.append(torch.argmax(logits[-1:], dim=-1))
            caches.append(c)
        dec = InterleavedDecoder(m, caches, torch.cat(first))
        toks, lps = dec.run(n_dec)
        q.put((rank, [int(f) for f in first], toks.tolist(), lps.tolist()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("backend", [
    "gloo",
    pytest.param("nccl", marks=pytest.mark.skipif(not _two_gpus(), reason="needs 2 GPUs (RCCL refuses two ranks on one device)")),
])
@pytest.mark.parametrize("name", ["dense_bf16", "swa_bf16"])
def test_interleaved_decoder_on_hip(name, backend, tmp_path):
    """pipeline_decode.InterleavedDecoder on the real kernels: two sequences through two stages, both stages busy every tick.
    Every sequence's tokens and log-probabilities equal decoding it ALONE on one stage (generate() on the whole model, same
    kernels per layer: the stage boundary moves bf16 activations, nothing is recomputed differently)."""
    from golden_util import Case
    from hip_util import write_checkpoint
    from mistral_inference.generate import generate
    from mistral_inference.transformer import Transformer
    case = Case(name)
    n_dec = 6
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 30300 + (os.getpid() % 500) + (sum(map(ord, name + backend)) % 97)
    procs = [ctx.Process(target=_interleaved_worker, args=(r, 2, port, name, str(tmp_path), q, backend, n_dec)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    from mistral_inference import _hip
    folder = write_checkpoint(tmp_path / "single", case.args, case.weights())
    single = Transformer.from_folder(folder, max_batch_size=1, device="cuda", dtype=torch.bfloat16)
    (_, f0, t0, lp0), (_, f1, t1, lp1) = res
    assert f0 == f1 and t0 == t1  # every stage returns the same tokens
    prev = _hip.set_decode_engine(False) if backend == "gloo" else None  # the same path as the workers took
    try:
        for j, pr in enumerate(case.prompts[:2]):
            ref_t, ref_lp = generate([pr], single, max_tokens=n_dec + 1, temperature=0.0)
            assert f0[j] == ref_t[0][0], (j, f0, ref_t)
            assert [row[j] for row in t0] == ref_t[0][1:], (j, t0, ref_t)
            gen_lp = ref_lp[0][len(pr) - 1:]
            assert max(abs(row[j] - x) for row, x in zip(lp0, gen_lp[1:])) <= 1e-5
    finally:
        if prev is not None:
            _hip.set_decode_engine(bool(prev))
