"""GPU: the training calls captured into a HIP graph replay the eager bits.

What is captured here and nowhere else in the suite: the pooled branch the two-branch training forward
runs on a side stream at D=128 (autograd.FORK_POOLED_BRANCH), the persistent (work-queue) launch of both
training forwards at D=128, the backward's ForkScope (dQ on a library-owned side stream between two event
record/wait pairs, csrc/vb_attn_bwd_host.cpp), and a backward at all.

One protocol for every case (``_check_capture``):
  1. the eager result on the current stream for two independent draws of the inputs;
  2. static inputs holding draw 0, the identical call warmed up twice on a side stream s that waits for
     the current stream first (torch's capture contract: whatever the call creates on first use, the
     work queue, the side streams and their events, the occupancy query, exists before the capture);
  3. the capture on s, the gradients taken inside it with torch.autograd.grad, so they are static tensors;
  4. replay, compare with eager draw 0; copy draw 1 into the static inputs (dout included), replay,
     compare with eager draw 1; replay once more, compare again.
All comparisons are torch.equal: the kernels are deterministic and the forks are scheduling only
(test_wan_training_path_forks_are_bit_identical_to_one_stream asserts both eagerly). Where a D=128 case
launches a persistent form, the queue of stream s must exist and sum to zero after the replays.

Group C is the work queue's own rule (ops.work_queue): a capture never creates a queue. Without a
warm-up the captured persistent call takes the one-workgroup-per-q-block form and leaves no queue
behind; with a warm-up, graphs captured on one stream share that stream's eagerly zeroed queue and replay
in any order."""
import functools
import math

import pytest
import torch

import bsa_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vblade
    vblade.load_library()


def _draw(B, H, L, D, seed, dtype=torch.bfloat16, blhd_dout=False):
    """q, k, v, dout on the device: clustered q/k (a centroid per 128-token block, as
    test_gpu_backward._realistic draws them), so the softmax is peaked the way trained heads are.
    ``blhd_dout``: dout as the [B,H,L,D] view of [B,L,H,D] memory, what a projection's backward hands on."""
    g = torch.Generator().manual_seed(seed)
    cent = torch.randn(B, H, L // 128 + 1, D, generator=g).repeat_interleave(128, 2)[:, :, :L]
    q = (torch.randn(B, H, L, D, generator=g) + 2 * cent).to(dtype).to(DEV)
    k = (torch.randn(B, H, L, D, generator=g) + 2 * cent).to(dtype).to(DEV)
    v = torch.randn(B, H, L, D, generator=g).to(dtype).to(DEV)
    do = torch.randn(B, H, L, D, generator=g).to(dtype).to(DEV)
    if blhd_dout:
        do = do.transpose(1, 2).contiguous().transpose(1, 2)
    return q, k, v, do


def _like(t):
    """A new tensor with t's values and t's strides (a static input of a capture)."""
    s = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device)
    return s.copy_(t)


def _step(fn, q, k, v, do, extra=None, grad=True):
    """One training step of ``fn(q, k, v) -> out``: (out, dq, dk, dv) + extra(). ``grad=False``: the
    inference call, (out,) + extra()."""
    if not grad:
        with torch.no_grad():
            return (fn(q, k, v),) + (tuple(extra()) if extra else ())
    qd, kd, vd = (t.detach().requires_grad_(True) for t in (q, k, v))
    out = fn(qd, kd, vd)
    dq, dk, dv = torch.autograd.grad(out, (qd, kd, vd), do)
    return (out.detach(), dq, dk, dv) + (tuple(extra()) if extra else ())


def _same(got, want, what, names):
    assert len(got) == len(want) == len(names)
    for name, a, b in zip(names, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name)
        assert torch.equal(a, b), (what, name)


def _check_capture(fn, draws, extra=None, queue=False, grad=True):
    from vblade import ops
    names = (("out", "dq", "dk", "dv") if grad else ("out",)) + (("mask",) if extra else ())
    n = len(names) - (1 if extra else 0)
    step = functools.partial(_step, extra=extra, grad=grad)
    cur = torch.cuda.current_stream()
    eager = [tuple(t.clone() for t in step(fn, *d)) for d in draws]
    for e in eager:   # the comparison is not of blanks, and the two draws tell a stale replay from a fresh one
        assert all(bool(torch.isfinite(t.float()).all()) and bool(t.float().abs().sum() > 0) for t in e)
    assert not any(torch.equal(a, b) for a, b in zip(eager[0][:n], eager[1][:n]))
    static = [_like(t) for t in draws[0]]
    assert all(s.stride() == t.stride() for s, t in zip(static, draws[0]))
    s = torch.cuda.Stream()
    s.wait_stream(cur)
    with torch.cuda.stream(s):
        for _ in range(2):
            step(fn, *static)
    cur.wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        got = step(fn, *static)
    graph.replay()
    _same(got, eager[0], "replay 1, draw 0", names)
    for t, src in zip(static, draws[1]):
        t.copy_(src)
    graph.replay()
    _same(got, eager[1], "replay 2, draw 1", names)
    graph.replay()
    _same(got, eager[1], "replay 3, draw 1", names)
    if queue:
        with torch.cuda.stream(s):
            wq = ops._WORK_QUEUES.get((torch.cuda.current_device(), s.cuda_stream))
            assert wq is not None and wq is ops.work_queue(torch.device(DEV))
            assert int(wq.abs().sum()) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------
# A. the autograd functions, mask and row table given
# ----------------------------------------------------------------------------------------------
# the smallest shapes that still run every launch: more than one q-block, a ragged last block, and
# pool_split's psplit = nbq > 1, so the pooled-gradient reduce launch is in the graph too
SHAPE = {128: dict(L=360, gap=30, heavy_rows=0), 64: dict(L=520, gap=15, heavy_rows=2)}
B, H = 1, 2


def _mask_and_rows(L, seed):
    nb = (L + 127) // 128
    mask = O.block_mask_from_density(B, H, nb, nb, 0.5, seed=seed)   # the diagonal is kept: no empty row
    assert bool(mask.any(-1).all())
    g = torch.Generator().manual_seed(seed + 1)
    rows = torch.randperm(L, generator=g).to(torch.int32)
    return mask.to(DEV), rows.to(DEV)


@pytest.mark.parametrize("form,D,dtype,io_layout", [
    ("split", 128, torch.bfloat16, "bhld"),    # side-stream pooled branch, persistent main launch, combine, ForkScope
    ("split", 128, torch.bfloat16, "blhd"),    # strided combine, strided gradients, dout through its strides
    ("split", 64, torch.bfloat16, "bhld"),     # one stream throughout
    ("joint", 128, torch.float16, "bhld"),
    ("joint", 64, torch.bfloat16, "bhld"),
], ids=["split-128-bf16", "split-128-bf16-blhd", "split-64-bf16", "joint-128-fp16", "joint-64-bf16"])
def test_autograd_function_replays_the_eager_bits(form, D, dtype, io_layout):
    from vblade import autograd as va
    L, gap, heavy = SHAPE[D]["L"], SHAPE[D]["gap"], SHAPE[D]["heavy_rows"]
    mask, rows = _mask_and_rows(L, seed=31 + D)
    draws = [_draw(B, H, L, D, seed=100 + D + i, dtype=dtype, blhd_dout=io_layout == "blhd") for i in range(2)]
    if io_layout == "blhd":
        assert not draws[0][3].is_contiguous()
    if form == "split":
        fn = lambda q, k, v: va.adaptive_split_attention(q, k, v, mask, rows, gap, heavy_rows=heavy,  # noqa: E731
                                                         io_layout=io_layout)
    else:
        bias = float(torch.log(torch.tensor(float(gap), dtype=dtype)).item())
        fn = lambda q, k, v: va.adaptive_joint_attention(q, k, v, mask, rows, gap, bias, heavy_rows=heavy,  # noqa: E731
                                                         io_layout=io_layout)
    _check_capture(fn, draws, queue=D == 128)


# ----------------------------------------------------------------------------------------------
# B. the modules
# ----------------------------------------------------------------------------------------------
def _offsets(Hh):
    return torch.zeros(1, Hh, 32, dtype=torch.int32, device=DEV) + torch.arange(32, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("grad_combine", ["reference", "joint"])
def test_wan_module_training_step_replays_the_eager_bits(grad_combine):
    """AdaptiveBlockSparseAttn("wan") on test_gpu_backward._small_module's grid (L = 360, D = 128), the
    predictor in the graph too. The sampling offsets are given, so the eager and the captured calls predict
    from the same samples; the mask is one of the compared outputs."""
    import vblade
    m = vblade.AdaptiveBlockSparseAttn("wan", log_every=0, width=10, height=6, depth=6, sample_gap=30,
                                       min_retain_ratio=0.3, max_retain_ratio=0.6, grad_combine=grad_combine)
    L = m.gilbert_rearranger.seq_len
    offs = _offsets(H)
    draws = [_draw(1, H, L, 128, seed=200 + i) for i in range(2)]
    fn = lambda q, k, v: m(q, k, v, q_off=offs, k_off=offs)  # noqa: E731
    _check_capture(fn, draws, extra=lambda: (m.last_mask,), queue=True)


def test_multilevel_module_training_step_replays_the_eager_bits():
    """multilevel.AdaptiveBlockSparseAttnTrain built as test_gpu_ml_backward's module test builds it, with
    persistent=True: one training step, forward then backward. (The option reaches the module's inference
    launch, captured by the next test; the autograd op launches one workgroup per q-block.)"""
    from vblade import multilevel
    w, h, d, text = 14, 10, 6, 26
    L = w * h * d + text
    m = multilevel.AdaptiveBlockSparseAttnTrain(width=w, height=h, depth=d, text_length=text, log_every=0,
                                                persistent=True).to(DEV)
    offs = _offsets(H)
    draws = [_draw(1, H, L, 64, seed=300 + i) for i in range(2)]
    fn = lambda q, k, v: m(q, k, v, q_off=offs, k_off=offs)  # noqa: E731
    _check_capture(fn, draws, extra=lambda: (m.last_mask,))


def test_multilevel_module_inference_call_replays_the_eager_bits():
    """The same module's inference call with persistent=True: the pyramid pass in the predictor's launch and
    the persistent multi-level launch (ops.ml_attention_fwd's work queue, made by the warm-up)."""
    from vblade import multilevel
    w, h, d, text = 14, 10, 6, 26
    L = w * h * d + text
    m = multilevel.AdaptiveBlockSparseAttnTrain(width=w, height=h, depth=d, text_length=text, log_every=0,
                                                persistent=True).to(DEV)
    offs = _offsets(H)
    draws = [_draw(1, H, L, 64, seed=310 + i) for i in range(2)]
    fn = lambda q, k, v: m(q, k, v, q_off=offs, k_off=offs)  # noqa: E731
    _check_capture(fn, draws, extra=lambda: (m.last_mask,), queue=True, grad=False)


# ----------------------------------------------------------------------------------------------
# C. the work queue and captures
# ----------------------------------------------------------------------------------------------
def _lse_problem(seed):
    L, D = SHAPE[128]["L"], 128
    q, k, v, _ = _draw(B, H, L, D, seed=seed)
    nb = (L + 127) // 128
    mask = O.block_mask_from_density(B, H, nb, nb, 0.5, seed=seed).to(DEV)
    return q, k, v, mask


def _capture_lse_forward(s, prob):
    from vblade import ops
    q, k, v, mask = prob
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        res = ops.attention_fwd(q, k, v, block_mask=mask, need_lse=True, persistent=True)
    return graph, res


def _key(s):
    return (torch.cuda.current_device(), s.cuda_stream)


def _eager_lse_forward(prob):
    from vblade import ops
    q, k, v, mask = prob
    out, lse = ops.attention_fwd(q, k, v, block_mask=mask, need_lse=True)    # one workgroup per q-block
    assert bool(torch.isfinite(lse).all())
    return out.clone(), lse.clone()


def test_a_capture_without_warm_up_creates_no_queue(monkeypatch):
    """Two graphs captured on one fresh stream with no eager persistent call before: neither creates a
    queue (each launches the one-workgroup-per-q-block form), so replaying the second first finds nothing
    unzeroed. Both equal the eager non-persistent bits."""
    from vblade import ops
    monkeypatch.setattr(ops, "_WORK_QUEUES", {})   # torch's pooled stream handles can alias an earlier test's key
    probs = [_lse_problem(41), _lse_problem(42)]
    eager = [_eager_lse_forward(p) for p in probs]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    (ga, ra), (gb, rb) = (_capture_lse_forward(s, p) for p in probs)
    assert _key(s) not in ops._WORK_QUEUES and ops._WORK_QUEUES == {}
    gb.replay()
    ga.replay()
    torch.cuda.synchronize()
    for got, want, what in ((rb, eager[1], "graph B"), (ra, eager[0], "graph A")):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), what


def test_graphs_captured_after_a_warm_up_share_the_streams_queue(monkeypatch):
    """With the warm-up torch asks for, the stream's queue is created and zeroed eagerly; two graphs
    captured on that stream launch the persistent form on it and replay A, B, A in sequence with the eager
    bits, leaving the queue zero."""
    from vblade import ops
    monkeypatch.setattr(ops, "_WORK_QUEUES", {})
    probs = [_lse_problem(43), _lse_problem(44)]
    eager = [_eager_lse_forward(p) for p in probs]
    cur = torch.cuda.current_stream()
    s = torch.cuda.Stream()
    s.wait_stream(cur)
    with torch.cuda.stream(s):
        for p in probs:
            q, k, v, mask = p
            warm = ops.attention_fwd(q, k, v, block_mask=mask, need_lse=True, persistent=True)
    cur.wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(warm[0], eager[1][0]) and torch.equal(warm[1], eager[1][1])
    wq = ops._WORK_QUEUES.get(_key(s))
    assert wq is not None and list(ops._WORK_QUEUES) == [_key(s)]
    (ga, ra), (gb, rb) = (_capture_lse_forward(s, p) for p in probs)
    assert list(ops._WORK_QUEUES) == [_key(s)] and ops._WORK_QUEUES[_key(s)] is wq
    for graph, got, want, what in ((ga, ra, eager[0], "A"), (gb, rb, eager[1], "B"), (ga, ra, eager[0], "A again")):
        got[0].zero_()
        got[1].fill_(math.nan)
        graph.replay()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), what
    assert int(wq.abs().sum()) == 0
    torch.cuda.synchronize()
