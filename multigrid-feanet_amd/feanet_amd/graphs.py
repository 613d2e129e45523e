"""GraphCache: work that is issued eagerly once, captured as a HIP graph the second time and replayed after.

Every solver replays fixed launch sequences (a V-cycle, a block of joined cycles, a block of PCG iterations, a
decomposed rank's kernel segment or whole block of cycles).  The first run of a sequence is eager — lazy buffers,
pointer arrays and communicator plans exist afterwards — the second run is captured and replayed, later runs
replay.  That state machine and the capture mechanics (a side stream, joined with the current one before and
after, torch's capture_error_mode) live here, once; the callers pass a callable that issues the work, so a replay
builds no launch list.
"""
import gc

import torch


class StreamCapture:
    """issue() captured into a HIP graph on a side stream of `device`.  mode: torch.cuda.graph's
    capture_error_mode (None: torch's default; "thread_local" where other threads of the process — a
    communicator's watchdog — keep making HIP calls during the capture).  A capture that raises RuntimeError
    leaves the device synchronised and the streams joined, then raises it on."""

    def __init__(self, device, mode=None):
        self.device = device
        self.kw = {} if mode is None else {"capture_error_mode": mode}

    def __call__(self, issue):
        stream = torch.cuda.current_stream(self.device)
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(self.device)
        side.wait_stream(stream)
        # No cyclic garbage collection inside the capture.  A dead solver that sits in a reference cycle (a DDSolver
        # does) keeps its captured graphs until the collector finds it; found during a capture, its graphs are
        # destroyed while a stream captures, which HIP refuses ("operation not permitted when stream is
        # capturing") — inside ~CUDAGraph, so the process aborts.  torch collects ahead of a capture only under
        # torch.compiler.config.force_cudagraph_gc.
        collecting = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(g, stream=side, **self.kw):
                issue()
        except RuntimeError:
            torch.cuda.synchronize(self.device)
            stream.wait_stream(side)
            raise
        finally:
            if collecting:
                gc.enable()
        stream.wait_stream(side)
        return g


class GraphCache:
    """key -> None (ran eagerly once) | captured graph.  len(), iteration and `in` see the captured keys only.

    capture: callable(issue) -> an object with replay() (default: StreamCapture(device, mode); tests pass a stub).
    capturing: True while a capture runs, for callers whose issuing differs inside one."""

    def __init__(self, device=None, mode=None, capture=None):
        self._capture = capture if capture is not None else StreamCapture(device, mode)
        self._graphs = {}
        self.capturing = False

    def __len__(self):
        return sum(g is not None for g in self._graphs.values())

    def __iter__(self):
        return iter([k for k, g in self._graphs.items() if g is not None])

    def __contains__(self, key):
        return self._graphs.get(key) is not None

    def clear(self):
        self._graphs.clear()

    def discard(self, match):
        """Forget every key with match(key) (graph and eager-run record)."""
        self._graphs = {k: g for k, g in self._graphs.items() if not match(k)}

    def run(self, key, issue, enabled=True, confirm=None):
        """Run issue()'s work under `key`: eager the first time, captured and replayed the second, replayed after
        (issue is not called on a replay).  enabled=False: always eager, nothing recorded.

        confirm(error) runs between the capture and the first replay, error being the RuntimeError the capture
        raised or None: it returns whether to keep the graph (it may raise instead).  Not kept, or not captured:
        the key is left as after its eager run, nothing is replayed and run() returns False — the caller issues
        the work another way.  Without confirm a capture's error is raised to the caller.  Returns True otherwise."""
        if not enabled:
            issue()
            return True
        try:
            g = self._graphs[key]
        except KeyError:
            self._graphs[key] = None
            issue()
            return True
        if g is None:
            error = None
            self.capturing = True
            try:
                g = self._capture(issue)
            except RuntimeError as e:
                if confirm is None:
                    raise
                error = e
            finally:
                self.capturing = False
            if confirm is not None and not (confirm(error) and error is None):
                return False
            self._graphs[key] = g
        g.replay()
        return True
