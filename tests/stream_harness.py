"""Helpers of tests/test_gpu_stream_order.py (no tests, no fixtures): what it takes to look at WHEN the library's work runs
relative to the caller's other work on the same stream.

  Hip             a ctypes binding of the six HIP runtime calls the tests need, resolved through libvoxbox_hip.so's own handle:
                  the runtime the library runs on, also when an earlier test has mapped torch's bundled copy beside it.
  Delay           a batch of vbx_pitch_f64 with the whole candidate list, queued on the context's stream, whose output nobody
                  reads: it keeps the stream busy for milliseconds while the host runs ahead.
  late_producer   one entry point with its input produced LATE on the stream and its outputs consumed at once on the stream,
                  against the same call bracketed by vbx_sync.
  bits_equal      raw-byte equality (NaN payloads count).
"""
import ctypes as C
import math
import os

import numpy as np

HIP_SUCCESS = 0
HIP_ERROR_NOT_READY = 600            # hipErrorNotReady, hip_runtime_api.h
HIP_STREAM_NON_BLOCKING = 1          # hipStreamNonBlocking
HIP_MEMCPY_DEVICE_TO_DEVICE = 3      # hipMemcpyDeviceToDevice, driver_types.h

DELAY_MIN_MS = 10.0                  # the delay is at least this long ...
DELAY_FACTOR = 5.0                   # ... and at least this many times the call under test
DELAY_MAX_REPS = 2000                # (a delay that would need more batches than this fails as vacuous, it is not shortened)


class Hip:
    """hipStreamCreateWithFlags (non-blocking), hipStreamDestroy, hipStreamSynchronize, hipStreamQuery, hipMemcpyAsync (device to
    device) and hipMemsetAsync of the HIP runtime the library itself runs on.  Nothing else is bound."""

    def __init__(self, pkg):
        pkg.load_library()
        # Symbols looked up through the library's OWN handle resolve in its dependency tree: the runtime libvoxbox_hip.so is
        # linked against, whatever else the process has mapped (a test that imported torch has mapped torch's bundled copy
        # too, whose streams the library's runtime does not know).  A handle of our own, so the prototypes stay local.
        L = C.CDLL(pkg.LIB_PATH)
        vp = C.c_void_p
        for name, args in (("hipStreamCreateWithFlags", [C.POINTER(vp), C.c_uint]), ("hipStreamDestroy", [vp]),
                           ("hipStreamSynchronize", [vp]), ("hipStreamQuery", [vp]),
                           ("hipMemcpyAsync", [vp, vp, C.c_size_t, C.c_int, vp]), ("hipMemsetAsync", [vp, C.c_int, C.c_size_t, vp])):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = C.c_int, args
        self.L = L
        # which mapped runtime that is: the one whose mapping holds the resolved function (exactly one does)
        addr = C.cast(L.hipStreamQuery, C.c_void_p).value
        owners = set()
        with open("/proc/self/maps") as f:
            for line in f:
                parts = line.split(None, 5)
                if len(parts) == 6:
                    lo, hi = (int(v, 16) for v in parts[0].split("-"))
                    if lo <= addr < hi:
                        owners.add(parts[5].strip())
        assert len(owners) == 1 and os.path.basename(next(iter(owners))).startswith("libamdhip64.so"), \
            f"hipStreamQuery of the library's runtime resolved into {sorted(owners)}"
        self.path = owners.pop()

    def stream_create(self):
        s = C.c_void_p()
        rc = self.L.hipStreamCreateWithFlags(C.byref(s), HIP_STREAM_NON_BLOCKING)
        assert rc == HIP_SUCCESS and s.value, rc
        return s.value

    def stream_destroy(self, stream):
        assert self.L.hipStreamDestroy(stream) == HIP_SUCCESS

    def stream_sync(self, stream):
        rc = self.L.hipStreamSynchronize(stream)
        assert rc == HIP_SUCCESS, rc

    def stream_query(self, stream):
        """HIP_SUCCESS: everything queued on the stream has finished; HIP_ERROR_NOT_READY: the host is ahead of it."""
        return self.L.hipStreamQuery(stream)

    def copy_async(self, dst, src, nbytes, stream):
        rc = self.L.hipMemcpyAsync(dst, src, nbytes, HIP_MEMCPY_DEVICE_TO_DEVICE, stream)
        assert rc == HIP_SUCCESS, rc

    def memset_async(self, dst, value, nbytes, stream):
        rc = self.L.hipMemsetAsync(dst, value, nbytes, stream)
        assert rc == HIP_SUCCESS, rc


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def first_difference(a, b):
    """(flat byte offset of the first differing byte, number of differing bytes): for messages."""
    x, y = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8), np.frombuffer(np.ascontiguousarray(b).tobytes(), np.uint8)
    if x.size != y.size:
        return -1, abs(x.size - y.size)
    d = np.nonzero(x != y)[0]
    return (int(d[0]), int(d.size)) if d.size else (-1, 0)


class Delay:
    """vbx_pitch_f64 at kmax = VBX_PITCH_MAX_CANDIDATES(frame_len), the slowest kernel per frame, over a fixed batch of the
    synthetic speech; `queue(reps)` puts `reps` such batches on the context's stream and returns without waiting."""
    N, H, SR = 1200, 480, 48000.0

    def __init__(self, vb, pkg, frames=4096):
        self.vb, self.F, self.kmax = vb, frames, pkg.pitch_max_candidates(self.N)
        self.x = vb.synth_speech((frames - 1) * self.H + self.N, sample_offset=11 * 48000)
        self.win = vb.window(pkg.WINDOW_HANNING, self.N)
        self.cand, self.cnt, self.st = vb.empty((frames, self.kmax, 2)), vb.empty(frames, np.int32), vb.empty(frames, np.int32)
        self.batch_ms = None

    def queue(self, reps):
        vb = self.vb
        for _ in range(reps):
            vb._check(vb.L.vbx_pitch_f64(vb.ctx, self.x.ptr, self.F, self.N, self.H, self.win.ptr, self.SR, 0.2, 75.0, 600.0,
                                         self.kmax, self.cand.ptr, self.cnt.ptr, self.st.ptr))

    def timed(self, reps):
        """Milliseconds `reps` batches take, from the context's event timer (the host waits for them)."""
        self.vb.sync()
        self.vb.timer_begin()
        self.queue(reps)
        return self.vb.timer_end()

    def reps_for(self, call_ms):
        """Batches that make the delay comfortably longer than both bounds (1.5 x: the bounds are asserted on a measurement)."""
        if self.batch_ms is None:
            self.queue(1)                                    # first use: tables and workspaces
            self.batch_ms = self.timed(4) / 4.0
        return max(1, int(math.ceil(1.5 * max(DELAY_MIN_MS, DELAY_FACTOR * call_ms) / max(self.batch_ms, 1e-3))))


def late_producer(vb_s, stream, call, inputs, outputs, delay, hip=None, probe=None):
    """The stream contract of one call.  vb_s: a context on the caller-created stream `stream`; call(): issues the entry
    point on vb_s (raises on an error code) and returns without waiting; inputs: [(device buffer the call reads, host array
    of its true content)]; outputs: [device buffer the call writes]; delay: a Delay on vb_s.

    Reference pass: the call bracketed by vbx_sync, cold (it also builds the tables and sizes the workspaces), profiled;
    probe(vb_s), if given, reads the library's vbx_internal_last_* state right after it.  The call is then timed warm and must
    give the same bits again.  Queued pass: x and every output poisoned (0xFF), the snapshots 0xA5, then with NO host wait
    between them: the delay, the producer (a device copy of the true input into x), the call, the consumer (a device copy of
    every output into its snapshot).  Asserted: the delay measured >= DELAY_MIN_MS and >= DELAY_FACTOR x the call (else the
    test is vacuous); the stream is not ready right after queueing (the host ran ahead: the warm call did not block, and the
    producer had not run when the call was issued); after ONE hipStreamSynchronize every snapshot equals the reference pass bit
    for bit and the inputs are intact.  Returns what was measured, the reference outputs and the profile of the reference
    pass."""
    assert hip is not None
    true = [vb_s.to_device(h) for _, h in inputs]
    snaps = [vb_s.empty(o.shape, o.dtype) for o in outputs]
    try:
        for (x, h), t in zip(inputs, true):
            assert x.nbytes >= h.nbytes
            hip.copy_async(x.ptr, t.ptr, h.nbytes, stream)
        for o in outputs:                                    # bytes a call never writes (row padding) read the same in both passes
            vb_s._check(vb_s.L.vbx_memset(vb_s.ctx, o.ptr, 0xFF, o.nbytes))
        vb_s.sync()
        vb_s.profile(True)
        vb_s.profile_reset()
        call()
        vb_s.sync()
        probed = probe(vb_s) if probe is not None else None
        streams, times = vb_s.profile_streams(), vb_s.profile_report()
        vb_s.profile(False)
        ref = [o.numpy() for o in outputs]
        vb_s.sync()
        vb_s.timer_begin()
        call()
        call_ms = vb_s.timer_end()
        vb_s.sync()
        for i, o in enumerate(outputs):
            assert bits_equal(o.numpy(), ref[i]), f"output {i}: two synchronised calls disagree {first_difference(o.numpy(), ref[i])}"
        reps = delay.reps_for(call_ms)
        assert reps <= DELAY_MAX_REPS, f"vacuous: a delay of {reps} batches ({delay.batch_ms:.3f} ms each) for a {call_ms:.3f} ms call"
        delay_ms = delay.timed(reps)
        assert delay_ms >= DELAY_MIN_MS and delay_ms >= DELAY_FACTOR * call_ms, \
            f"vacuous: the delay took {delay_ms:.3f} ms, the call {call_ms:.3f} ms"
        # poison
        for x, _ in inputs:
            vb_s._check(vb_s.L.vbx_memset(vb_s.ctx, x.ptr, 0xFF, x.nbytes))
        for o, s in zip(outputs, snaps):
            vb_s._check(vb_s.L.vbx_memset(vb_s.ctx, o.ptr, 0xFF, o.nbytes))
            vb_s._check(vb_s.L.vbx_memset(vb_s.ctx, s.ptr, 0xA5, s.nbytes))
        vb_s.sync()
        # the queue: nothing below waits for the device until the one synchronisation
        delay.queue(reps)
        for (x, h), t in zip(inputs, true):
            hip.copy_async(x.ptr, t.ptr, h.nbytes, stream)
        call()
        for o, s in zip(outputs, snaps):
            hip.copy_async(s.ptr, o.ptr, o.nbytes, stream)
        state = hip.stream_query(stream)
        hip.stream_sync(stream)
        vb_s.sync()
        assert state == HIP_ERROR_NOT_READY, \
            f"hipStreamQuery gave {state} right after queueing: the host did not run ahead of a {delay_ms:.1f} ms delay"
        for i, s in enumerate(snaps):
            got = s.numpy()
            assert bits_equal(got, ref[i]), \
                f"output {i}: the queued call differs from the synchronised one (first byte, bytes) = {first_difference(got, ref[i])}"
        for i, (x, h) in enumerate(inputs):
            got = np.frombuffer(x.numpy().tobytes()[:h.nbytes], dtype=h.dtype).reshape(h.shape)
            assert bits_equal(got, h), f"input {i} was modified"
        return {"call_ms": round(call_ms, 4), "delay_ms": round(delay_ms, 3), "delay_batches": reps, "ref": ref, "probe": probed,
                "streams": streams, "times": {k: round(v[0], 4) for k, v in times.items()}}
    finally:
        vb_s.sync()
        for d in true + snaps:
            d.free()
