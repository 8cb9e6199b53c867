"""A stretch of device solves recorded once into a HIP graph and replayed with one host call (include/fastmpc.h, "Recording
solves into a HIP graph").  The reference replays a realisation step by step through Fast_MPC2(...).mpc_fixed_log_newton
(README.md:548-556); when the inputs of the steps are known in advance -- a replay batch -- the host does not have to submit
them one by one: inside a graph the launches follow each other more closely than the host can submit them."""
from . import _lib
from ._lib import FastMPCError


class RecordedSolves:
    """record_fn(): any number of solve_device / solve-like calls on torch tensors that all exist already (status and iters
    included: nothing may be allocated while the calls are recorded).  It is run once eagerly (the handle builds its constants
    and workspaces), then once under capture.  replay() runs the recorded launches on torch's current stream; it refuses when
    any handle of the process has allocated or released device memory since the recording (the graph holds addresses).

    fuse=True (default): both passes run inside a stretch bracket (fmpc_stretch_begin / fmpc_stretch_end, include/fastmpc.h):
    consecutive cold-start steps that take the affine form are recorded as chains of up to 16 steps, two or three launches per
    chain instead of two per step, with the same results bit for bit.  The bracket's contract is this class's own: record_fn
    enqueues nothing but solve calls.  Anything else on the stream between two solves is detected while recording and raises
    FastMPCError (FMPC_E_UNSUPPORTED); pass fuse=False for such a record_fn."""

    def __init__(self, record_fn, fuse=True):
        import gc
        import torch
        self._lib = _lib.load()
        self._record_fn = record_fn           # (keeps the tensors the closure refers to alive: the graph holds their addresses)
        self._fuse = bool(fuse)
        self._bracketed(torch.cuda.current_stream(), record_fn)
        torch.cuda.synchronize()
        self._stream = torch.cuda.Stream()
        self.graph = torch.cuda.CUDAGraph()
        # No garbage collection while the stream is capturing: a collection that happens to run inside the capture may destroy
        # objects whose release is not allowed then -- another graph with its memory pool (hipFree), a stream -- and the
        # runtime aborts the process (seen in the test suite: the previous test's recording was collected here).
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.stream(self._stream):
                with torch.cuda.graph(self.graph, stream=self._stream):
                    self._bracketed(self._stream, record_fn)
        finally:
            if gc_was_on:
                gc.enable()
        torch.cuda.synchronize()
        self._gen = int(self._lib.fmpc_alloc_generation())

    def _bracketed(self, stream, record_fn):
        """record_fn() between fmpc_stretch_begin and fmpc_stretch_end on `stream` (fuse=True)."""
        if not self._fuse:
            record_fn()
            return
        import ctypes
        sp = ctypes.c_void_p(stream.cuda_stream)
        rc = self._lib.fmpc_stretch_begin(sp)
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_stretch_begin")
        try:
            record_fn()
        except FastMPCError as e:
            self._lib.fmpc_stretch_end(sp)
            if e.code == _lib.FMPC_E_UNSUPPORTED:
                raise FastMPCError(_lib.FMPC_E_UNSUPPORTED, "RecordedSolves: record_fn enqueued other work than solve calls between two "
                                   "fused steps (or a solve is unsupported) -- record with fuse=False: " + str(e)) from e
            raise
        except BaseException:
            self._lib.fmpc_stretch_end(sp)
            raise
        rc = self._lib.fmpc_stretch_end(sp)
        if rc == _lib.FMPC_E_UNSUPPORTED:
            raise FastMPCError(rc, "RecordedSolves: record_fn enqueued other work than solve calls behind a fused step -- record with fuse=False")
        if rc != _lib.FMPC_OK:
            raise FastMPCError(rc, "fmpc_stretch_end")

    def valid(self):
        return int(self._lib.fmpc_alloc_generation()) == self._gen

    def replay(self):
        if not self.valid():
            raise FastMPCError(_lib.FMPC_E_UNSUPPORTED, "RecordedSolves.replay: device buffers were (re)allocated since the recording -- record again")
        self.graph.replay()
