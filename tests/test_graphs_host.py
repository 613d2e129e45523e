"""feanet_amd.graphs.GraphCache with a stub capture backend (no GPU): the eager / capture / replay order per key,
no issuing on a replay, enabled=False, a capture that raises, and the confirm step between capture and replay."""
import pytest

from feanet_amd.graphs import GraphCache


class StubCapture:
    """Records what a capture would: calls issue() (whose work lands in `log` as usual), returns a graph whose
    replay() logs ("replay", id)."""

    def __init__(self, log, fail=None):
        self.log, self.fail, self.count = log, fail, 0

    def __call__(self, issue):
        self.log.append("capture")
        issue()
        if self.fail is not None:
            raise self.fail
        self.count += 1
        stub, n = self, self.count

        class Graph:
            def replay(self):
                stub.log.append(("replay", n))
        return Graph()


def cache(fail=None):
    log = []
    c = GraphCache(capture=StubCapture(log, fail))
    return c, log


def test_eager_capture_replay_per_key():
    c, log = cache()
    issue = {k: (lambda k=k: log.append(("issue", k, c.capturing))) for k in "xy"}
    assert c.run("x", issue["x"]) and len(c) == 0 and "x" not in c
    assert log == [("issue", "x", False)]
    assert c.run("y", issue["y"])  # another key starts its own sequence
    assert c.run("x", issue["x"])
    assert log[2:] == ["capture", ("issue", "x", True), ("replay", 1)]
    assert "x" in c and "y" not in c and list(c) == ["x"] and len(c) == 1
    del log[:]
    for _ in range(3):
        assert c.run("x", issue["x"])
    assert log == [("replay", 1)] * 3  # the issuing callable is not invoked on a replay
    assert c.run("y", issue["y"])
    assert log[3:] == ["capture", ("issue", "y", True), ("replay", 2)]
    assert sorted(c) == ["x", "y"] and not c.capturing


def test_disabled_never_captures():
    c, log = cache()
    for _ in range(4):
        assert c.run("x", lambda: log.append("issue"), enabled=False)
    assert log == ["issue"] * 4 and len(c) == 0 and not list(c)
    # and leaves no eager-run record: the first enabled run is the eager one
    assert c.run("x", lambda: log.append("issue"))
    assert log == ["issue"] * 5 and len(c) == 0


def test_capture_error_reaches_the_caller():
    c, log = cache(fail=RuntimeError("stream is capturing"))
    c.run("x", lambda: log.append("issue"))
    with pytest.raises(RuntimeError, match="stream is capturing"):
        c.run("x", lambda: log.append("issue"))
    assert "x" not in c and len(c) == 0 and not c.capturing
    assert log == ["issue", "capture", "issue"]  # nothing replayed


def test_clear_and_discard_restart_the_sequence():
    c, log = cache()
    for key in (("cap", 1), ("cap", 2), ("seg", 1)):
        c.run(key, lambda: None)
        c.run(key, lambda: None)
    assert len(c) == 3
    c.discard(lambda k: k[0] == "cap")
    assert list(c) == [("seg", 1)]
    del log[:]
    c.run(("cap", 1), lambda: log.append("issue"))
    assert log == ["issue"]  # eager again
    c.clear()
    assert len(c) == 0
    c.run(("seg", 1), lambda: log.append("issue"))
    assert log == ["issue"] * 2


@pytest.mark.parametrize("keep", [True, False])
def test_confirm_runs_between_capture_and_first_replay(keep):
    c, log = cache()

    def confirm(error):
        log.append(("confirm", error))
        return keep
    issue = lambda: log.append("issue")
    assert c.run("x", issue, confirm=confirm)
    assert log == ["issue"]  # the eager run asks nobody
    assert c.run("x", issue, confirm=confirm) is keep
    if keep:
        assert log[1:] == ["capture", "issue", ("confirm", None), ("replay", 1)] and "x" in c
        assert c.run("x", issue, confirm=confirm) and log[-1] == ("replay", 1) and len(log) == 6  # not asked again
    else:  # discarded: nothing replayed, no graph under the key
        assert log[1:] == ["capture", "issue", ("confirm", None)] and "x" not in c and len(c) == 0


def test_confirm_sees_the_capture_error():
    err = RuntimeError("operation not permitted when stream is capturing")
    c, log = cache(fail=err)
    seen = []
    c.run("x", lambda: None, confirm=lambda e: seen.append(e) or False)
    assert c.run("x", lambda: None, confirm=lambda e: seen.append(e) or False) is False
    assert seen == [err] and "x" not in c and not c.capturing

    def raising(e):
        raise ValueError("decided elsewhere")
    with pytest.raises(ValueError, match="decided elsewhere"):
        c.run("x", lambda: None, confirm=raising)
    assert len(c) == 0


@pytest.mark.parametrize("fail", [False, True])
def test_stream_capture_holds_the_cyclic_collector(monkeypatch, fail):
    """StreamCapture runs issue() with Python's cyclic collector off and restores it, also when the capture raises:
    a dead solver in a reference cycle owns captured graphs, and collecting it inside a capture destroys them while a
    stream captures — HIP refuses that inside a destructor and the process aborts.  torch.cuda's pieces are stubs."""
    import contextlib
    import gc

    import torch
    from feanet_amd.graphs import StreamCapture

    class Stream:
        def __init__(self, device=None):
            pass

        def wait_stream(self, other):
            pass

    @contextlib.contextmanager
    def graph(g, stream=None, **kw):
        yield

    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: Stream())
    monkeypatch.setattr(torch.cuda, "Stream", Stream)
    monkeypatch.setattr(torch.cuda, "CUDAGraph", object)
    monkeypatch.setattr(torch.cuda, "graph", graph)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: None)
    seen = []

    def issue():
        seen.append(gc.isenabled())
        if fail:
            raise RuntimeError("operation not permitted when stream is capturing")
    assert gc.isenabled()
    if fail:
        with pytest.raises(RuntimeError):
            StreamCapture("cuda")(issue)
    else:
        assert StreamCapture("cuda")(issue) is not None
    assert seen == [False] and gc.isenabled()
    gc.disable()  # a caller that had it off keeps it off
    try:
        StreamCapture("cuda")(lambda: None)
        assert not gc.isenabled()
    finally:
        gc.enable()
