"""CPU: the persistent forward's work queue is never created inside a graph capture.

A queue made by ``torch.zeros`` during a capture is zeroed by a graph node, not eagerly, and lives in the
graph's private pool: a second graph captured on the same stream would find it cached and, replayed
first, launch on memory that was never zeroed. So while the current stream is capturing and has no queue,
``ops.work_queue`` reports "no queue" (None), allocates nothing and caches nothing, and the two users
(``attention_fwd``, ``ml_attention_fwd``) hand the library a null queue: the one-workgroup-per-q-block
launch. Everything here is monkeypatched: no device is touched and nothing is launched."""
import pytest
import torch

from vblade import _lib, ops

_STREAM = 0x5EED


class _Queue:
    """Stands in for the device tensor torch.zeros would return."""

    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


@pytest.fixture
def env(monkeypatch):
    """ops with a fixed stream handle, an empty queue table and a counting torch.zeros; ``capturing``
    is what torch.cuda.is_current_stream_capturing answers."""
    state = {"capturing": True, "stream": _STREAM, "zeros": []}
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: state["capturing"])
    monkeypatch.setattr(ops, "_stream", lambda dev: state["stream"])
    monkeypatch.setattr(ops, "_WORK_QUEUES", {})

    def zeros(*args, **kw):
        if state["capturing"]:
            raise AssertionError("torch.zeros called while the stream is capturing")
        state["zeros"].append((args, kw))
        return _Queue(0x1000 * len(state["zeros"]))

    monkeypatch.setattr(torch, "zeros", zeros)
    return state


def test_no_queue_is_created_while_the_stream_is_capturing(env):
    for _ in range(2):
        assert ops.work_queue("cuda:0") is None
        assert ops._work_queue_ptr("cuda:0", True) is None
        assert ops._work_queue_ptr("cuda:0", False) is None
    assert ops._WORK_QUEUES == {} and env["zeros"] == []


def test_an_eager_call_creates_the_queue_once_and_reuses_it(env):
    env["capturing"] = False
    wq = ops.work_queue("cuda:0")
    assert isinstance(wq, _Queue)
    assert list(ops._WORK_QUEUES) == [(0, _STREAM)]
    (args, kw), = env["zeros"]
    assert args == (_lib.VB_WORK_QUEUE_INTS,) and kw["dtype"] == torch.int32
    assert kw["device"] == torch.device("cuda:0")
    for _ in range(3):
        assert ops.work_queue("cuda:0") is wq
        assert ops._work_queue_ptr("cuda:0", True) == wq.data_ptr()
    assert ops._work_queue_ptr("cuda:0", False) is None    # not asked for: no queue handed on
    assert len(env["zeros"]) == 1 and len(ops._WORK_QUEUES) == 1


def test_a_queue_warmed_up_eagerly_is_used_inside_a_capture(env):
    env["capturing"] = False
    wq = ops.work_queue("cuda:0")
    env["capturing"] = True            # torch.zeros raises from here on
    assert ops.work_queue("cuda:0") is wq
    assert ops._work_queue_ptr("cuda:0", True) == wq.data_ptr()
    # another stream of the same device has no queue: none is made for it inside the capture
    env["stream"] = _STREAM + 1
    assert ops.work_queue("cuda:0") is None
    assert ops._work_queue_ptr("cuda:0", True) is None
    assert list(ops._WORK_QUEUES) == [(0, _STREAM)] and len(env["zeros"]) == 1


@pytest.mark.parametrize("persistent,capturing,want", [(True, True, None), (True, False, 0x1000),
                                                       (False, False, None)])
def test_both_forwards_hand_the_library_the_looked_up_queue(env, monkeypatch, persistent, capturing, want):
    """attention_fwd and ml_attention_fwd fill vb_attn_args.work_queue / vb_ml_attn_args.work_queue from
    the lookup above: null (the per-q-block launch) inside a capture without a queue, the queue's
    address otherwise. The library call is intercepted; nothing is launched."""
    env["capturing"] = capturing
    seen = {}
    real = _lib.load()

    class _Lib:
        vb_kv_pyramid_rows = staticmethod(real.vb_kv_pyramid_rows)   # host arithmetic only

        def vb_attn_fwd(self, a, stream):
            seen["attn"] = a._obj.work_queue
            return 0

        def vb_ml_attn_fwd(self, a, stream):
            seen["ml"] = a._obj.work_queue
            return 0

    monkeypatch.setattr(_lib, "load", lambda: _Lib())
    monkeypatch.setattr(ops, "_require_gpu", lambda *ts: torch.device("cuda:0"))
    B, H, L, D = 1, 1, 256, 64
    q = torch.empty(B, H, L, D, dtype=torch.bfloat16)
    out = torch.empty_like(q)          # given, so the ops allocate nothing on the (absent) device
    ops.attention_fwd(q, q, q, persistent=persistent, out=out)
    R = ops.kv_pyramid_rows(L)
    pyr = torch.empty(B, H, R, D, dtype=torch.bfloat16)
    mask = torch.ones(B, H, 2, 2, dtype=torch.uint8)
    ops.ml_attention_fwd(q, pyr, pyr, mask, persistent=persistent, out=out)
    assert seen == {"attn": want, "ml": want}
    assert len(ops._WORK_QUEUES) == (1 if want else 0)
