"""`backend._Workspace` and `backend.workspace_owner` without a device: the stream / capture queries of torch.cuda are replaced by a fake
whose current stream and capture state the test sets, and the buffers are host tensors."""
import pytest
import torch

from imcui_hip import backend
from imcui_hip.lib_loader import ImcuiHipError

CPU = torch.device("cpu", 0)


@pytest.fixture
def fake_cuda(monkeypatch):
    class State:
        stream = 1
        capturing = False

    st = State()
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: type("S", (), {"cuda_stream": st.stream})())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: st.capturing)
    return st


def test_eager_buffers_are_per_stream_and_grow(fake_cuda):
    ws = backend._Workspace()
    with ws.use(100, CPU) as a:
        pass
    with ws.use(50, CPU) as b:
        assert b is a  # grow-only: a smaller request re-uses the buffer
    fake_cuda.stream = 2
    with ws.use(50, CPU) as c:
        assert c is not a  # another stream never shares scratch
    fake_cuda.stream = 1
    with ws.use(200, CPU) as d:
        assert d.numel() == 200 and d is not a
    assert len(ws._bufs) == 2


def test_owner_table_is_separate_pinned_at_capture_and_released(fake_cuda):
    ws, other = backend._Workspace(), backend._Workspace()
    with ws.use(100, CPU) as eager:
        pass
    table = {}
    with backend.workspace_owner(table):
        with ws.use(300, CPU) as warm:  # warm-up: the owner's buffer, whatever the stream
            assert warm is not eager
        fake_cuda.stream = 7
        with ws.use(200, CPU) as b:
            assert b is warm
        with other.use(10, CPU) as o:
            assert o is not warm
        fake_cuda.capturing = True
        with ws.use(300, CPU) as cap:
            assert cap is warm
        with pytest.raises(ImcuiHipError, match="captured HIP graph"):
            with ws.use(301, CPU):
                pass
        fake_cuda.capturing = False
    assert set(table) == {(ws, 0), (other, 0)}
    # the stream table saw none of it and is never pinned: an eager call of any size on the graph's stream grows its own buffer
    fake_cuda.stream = 7
    with ws.use(10_000, CPU) as big:
        assert big.numel() == 10_000
    fake_cuda.stream = 1
    with ws.use(100, CPU) as again:
        assert again is eager


def test_capture_outside_an_owner_scope_raises(fake_cuda):
    ws = backend._Workspace()
    fake_cuda.capturing = True
    with pytest.raises(ImcuiHipError, match="workspace_owner"):
        with ws.use(10, CPU):
            pass
    assert not ws._bufs


def test_owner_scope_is_per_thread_and_restored(fake_cuda):
    import threading

    ws = backend._Workspace()
    outer, inner, seen = {}, {}, {}
    with backend.workspace_owner(outer):
        with backend.workspace_owner(inner):
            with ws.use(10, CPU):
                pass

            def other_thread():
                with ws.use(10, CPU) as b:
                    seen["buf"] = b

            t = threading.Thread(target=other_thread)
            t.start()
            t.join()
        with ws.use(10, CPU):
            pass
    assert list(inner) == [(ws, 0)] and list(outer) == [(ws, 0)]
    assert list(ws._bufs) == [(0, 1)] and ws._bufs[(0, 1)][0] is seen["buf"]  # the other thread ran eagerly
