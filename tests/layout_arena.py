"""A fenced arena for layout tests: ONE allocation holds every device buffer of a call, each at a requested residue of
its address modulo 16 and with a fence zone on both sides, so that an access a few elements (or a row) outside a buffer
still lands in memory the test owns, and is noticed.

* outputs and their fences are filled with a canary before the call (a NaN with a recognisable payload for floating-point
  buffers, a fixed word for integer ones); `finish()` asserts that every fence byte, every padding column of a buffer whose
  leading dimension exceeds its row, and every input byte is what it was, and names the buffer and the offset if not;
* inputs are fenced with quiet NaNs (float / double) or -32768 (16-bit PCM): a kernel that USES a sample outside a frame
  produces a NaN (or a value that moves) in its output, which `new_nans()` / `assert_same_bits()` report;
* addresses are plain integers (the package's methods and the C ABI take them as they are).

Two backends with the same layout logic: `HostBackend` (a numpy byte buffer; the helper's own CPU test) and `DeviceBackend`
(vbx_malloc + one upload, one download per case)."""
import ctypes as C

import numpy as np

FENCE_MIN = 4096                       # bytes on each side of every buffer, at least
CANARY_F64 = np.uint64(0x7FF8C0DEC0DEC0DE)      # quiet NaN, payload "c0dec0dec0de"
CANARY_F32 = np.uint32(0x7FC0DEC0)              # quiet NaN, payload "0dec0"
CANARY_I32 = np.uint32(0x5AFEC0DE)
CANARY_I16 = np.uint16(0x5AFE)
PCM_FENCE = -32768                     # a value the test signals never contain
RESIDUES = {8: (0, 8), 4: (0, 4, 8, 12), 2: tuple(range(0, 16, 2))}    # by the size of the element's scalar type


class ArenaViolation(AssertionError):
    pass


def canary_of(dtype):
    """(unsigned view dtype, canary word) of an output element type."""
    dt = np.dtype(dtype)
    if dt == np.float64:
        return np.uint64, CANARY_F64
    if dt == np.float32:
        return np.uint32, CANARY_F32
    if dt == np.int32:
        return np.uint32, CANARY_I32
    if dt == np.int16:
        return np.uint16, CANARY_I16
    if dt == np.complex128:
        return np.uint64, CANARY_F64
    if dt == np.complex64:
        return np.uint32, CANARY_F32
    raise TypeError(dt)


def _input_fence(dtype):
    dt = np.dtype(dtype)
    if dt.kind in "fc":
        return np.array(np.nan, dtype=np.float64 if dt.itemsize >= 8 else np.float32)      # complex: NaN in both halves
    if dt == np.int16:
        return np.array(PCM_FENCE, dtype=np.int16)
    return np.array(CANARY_I32).view(np.int32) if dt.itemsize == 4 else np.array(0x5AFE, dtype=dt)


class HostBackend:
    """The arena in host memory; `view()` lets numpy stand-ins for kernels work on raw addresses."""

    def alloc(self, nbytes):
        self._raw = np.zeros(nbytes + 16, dtype=np.uint8)
        off = (-self._raw.ctypes.data) % 16
        self._buf = self._raw[off:off + nbytes]
        self.base = self._buf.ctypes.data
        return self.base

    def upload(self, image):
        self._buf[:] = image

    def download(self, nbytes):
        return self._buf[:nbytes].copy()

    def view(self, addr, dtype, count):
        dt = np.dtype(dtype)
        off = addr - self.base
        assert 0 <= off and off + count * dt.itemsize <= self._buf.size, "stand-in kernel left the arena"
        return self._buf[off:off + count * dt.itemsize].view(dt)

    def free(self):
        self._raw = self._buf = None


class DeviceBackend:
    def __init__(self, vb):
        self.vb, self.ptr = vb, None

    def alloc(self, nbytes):
        p = C.c_void_p()
        self.vb._check(self.vb.L.vbx_malloc(self.vb.ctx, C.byref(p), nbytes))
        self.ptr = p.value
        assert self.ptr % 16 == 0
        return self.ptr

    def upload(self, image):
        self.vb._check(self.vb.L.vbx_memcpy_h2d(self.vb.ctx, self.ptr, image.ctypes.data, image.nbytes))

    def download(self, nbytes):
        self.vb.sync()
        out = np.empty(nbytes, dtype=np.uint8)
        self.vb._check(self.vb.L.vbx_memcpy_d2h(self.vb.ctx, out.ctypes.data, self.ptr, nbytes))
        return out

    def free(self):
        if self.ptr:
            self.vb.sync()
            self.vb.L.vbx_free(self.vb.ctx, self.ptr)
            self.ptr = None


class _Buf:
    def __init__(self, name, kind, dtype, rows, cols, ld, residue, data):
        self.name, self.kind, self.dtype = name, kind, np.dtype(dtype)
        self.rows, self.cols, self.ld, self.residue, self.data = rows, cols, ld, residue, data
        self.nbytes = ((rows - 1) * ld + cols) * self.dtype.itemsize if rows else 0
        self.off = None


class Arena:
    """a = Arena(backend); a.input(..) / a.output(..) ...; a.place(); <call with a["name"] addresses>; outs = a.finish()"""

    def __init__(self, backend, label=""):
        self.backend, self.label, self.bufs, self.placed = backend, label, {}, False

    def _add(self, b):
        assert not self.placed and b.name not in self.bufs
        # what C gives the element: its own size, for a {re, im} / {frequency, strength} pair the size of one component
        es = b.dtype.itemsize // 2 if b.dtype.kind == "c" else b.dtype.itemsize
        assert b.residue in RESIDUES[es], (b.name, b.residue, b.dtype)
        self.bufs[b.name] = b

    def input(self, name, data, residue=0, inout=False):
        """`data`: the bytes the call reads, any shape (a strided view's gaps and a padded row's padding are the caller's:
        fill them with NaN).  inout=True: the call may rewrite the buffer (in-place entry points); it is returned by finish()."""
        d = np.ascontiguousarray(data)
        self._add(_Buf(name, "inout" if inout else "input", d.dtype, 1, d.size, d.size, residue, d))
        self.bufs[name].shape = d.shape

    def output(self, name, dtype, rows, cols, ld=None, residue=0):
        """[rows, cols] of `dtype` with leading dimension ld >= cols (elements); the ld - cols padding columns are canaries."""
        ld = cols if ld is None else ld
        assert ld >= cols
        self._add(_Buf(name, "output", dtype, rows, cols, ld, residue, None))

    def place(self):
        off, image_parts = 0, []
        for b in self.bufs.values():
            row_bytes = b.ld * b.dtype.itemsize if b.kind == "output" else 0
            b.fence = -(-max(FENCE_MIN, row_bytes) // 16) * 16
            start = off + b.fence
            start += (b.residue - start) % 16
            b.fence_lo = start - off                       # bytes of fence before the buffer (>= b.fence)
            b.off = start
            off = start + b.nbytes
            off += (-off) % 16
            b.end_fence = off + b.fence                    # the fence after it ends here
            off = b.end_fence
        self.nbytes = off
        img = np.zeros(self.nbytes, dtype=np.uint8)
        writable = np.zeros(self.nbytes, dtype=bool)
        lo = 0
        for b in self.bufs.values():
            es = b.dtype.itemsize if b.dtype.kind != "c" else b.dtype.itemsize // 2
            # the element grid of the fill is the buffer's own, so fence and padding hold whole canary elements
            g0 = b.off - ((b.off - lo) // es) * es
            n = (b.end_fence - g0) // es
            if b.kind == "output":
                ut, word = canary_of(b.dtype)
                img[g0:g0 + n * es].view(ut)[:] = word
                for r in range(b.rows):
                    s = b.off + r * b.ld * b.dtype.itemsize
                    writable[s:s + b.cols * b.dtype.itemsize] = True
            else:
                f = _input_fence(b.dtype)
                img[g0:g0 + n * es].view(f.dtype)[:] = f
                img[b.off:b.off + b.nbytes] = b.data.reshape(-1).view(np.uint8)
                if b.kind == "inout":
                    writable[b.off:b.off + b.nbytes] = True
            lo = b.end_fence
        self.image, self.writable = img, writable
        self.base = self.backend.alloc(self.nbytes)
        assert self.base % 16 == 0
        self.backend.upload(img)
        self.placed = True
        return self

    def __getitem__(self, name):
        b = self.bufs[name]
        a = self.base + b.off
        assert a % 16 == b.residue
        return a

    def _where(self, pos):
        """Names the buffer a damaged byte belongs to, and its offset from that buffer."""
        for b in self.bufs.values():
            if b.off - b.fence_lo <= pos < b.end_fence:
                es = b.dtype.itemsize
                if pos < b.off:
                    return f"'{b.name}': {b.off - pos} bytes ({-(-(b.off - pos) // es)} elements) BEFORE its start"
                if pos >= b.off + b.nbytes:
                    d = pos - (b.off + b.nbytes)
                    return f"'{b.name}': byte {d} (element {d // es}) PAST its end"
                e = (pos - b.off) // es
                if b.kind == "output":
                    return f"'{b.name}': padding column {e % b.ld} of row {e // b.ld} (row holds {b.cols} of ld {b.ld})"
                return f"input '{b.name}': element {e} was overwritten"
        return f"byte {pos} of the arena"

    def finish(self, free=True):
        """Downloads the arena, checks fences / padding / inputs, returns {name: array} of the outputs and in/out buffers."""
        got = self.backend.download(self.nbytes)
        bad = np.nonzero((got != self.image) & ~self.writable)[0]
        if free:
            self.backend.free()
        if bad.size:
            spots, seen = [], set()
            for pos in bad:
                w = self._where(int(pos))
                key = w.split(":")[0]
                if key not in seen:
                    seen.add(key)
                    spots.append(w)
            raise ArenaViolation(f"{self.label}: {bad.size} bytes outside the outputs changed -- " + "; ".join(spots[:6]))
        out = {}
        for b in self.bufs.values():
            if b.kind == "output":
                flat = got[b.off:b.off + b.nbytes].view(b.dtype)
                idx = np.arange(b.rows)[:, None] * b.ld + np.arange(b.cols)[None, :]
                out[b.name] = flat[idx].copy()
            elif b.kind == "inout":
                out[b.name] = got[b.off:b.off + b.nbytes].view(b.dtype).reshape(b.shape).copy()
        return out


# ---- comparisons of a layout case with its canonical call ---------------------------------------------------------------

def _words(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64, 16: np.uint64}[a.dtype.itemsize])


def assert_same_bits(label, name, got, want):
    """Bit-for-bit equality (NaN-safe), every element; the message names the first differing element."""
    assert got.shape == want.shape and got.dtype == want.dtype, (label, name, got.shape, want.shape)
    g, w = _words(got), _words(want)
    if not np.array_equal(g, w):
        d = np.argwhere(g != w)
        first = tuple(int(v) for v in d[0])
        raise AssertionError(f"{label}: output '{name}' differs from the canonical call's in {d.shape[0]} words, first at {first}: "
                             f"{got.reshape(g.shape)[first] if got.dtype.kind != 'c' else g[first]!r} != "
                             f"{want.reshape(w.shape)[first] if want.dtype.kind != 'c' else w[first]!r}")


def new_nans(got, want):
    """Indices where `got` holds a NaN and `want` does not (what a used fence sample shows up as)."""
    if got.dtype.kind not in "fc":
        return np.zeros((0, got.ndim), dtype=np.int64)
    return np.argwhere(np.isnan(got) & ~np.isnan(want))


def assert_no_new_nan(label, name, got, want):
    d = new_nans(got, want)
    if d.shape[0]:
        raise AssertionError(f"{label}: output '{name}' holds {d.shape[0]} NaN the canonical call's does not, first at "
                             f"{tuple(int(v) for v in d[0])}: a sample outside a frame (an input fence) was used")


def unwritten(a):
    """Indices of output elements that still hold the canary (the call never wrote them)."""
    ut, word = canary_of(a.dtype)
    v = np.ascontiguousarray(a).view(ut)
    return np.argwhere(v == word)


def assert_written(label, name, a):
    d = unwritten(a)
    if d.shape[0]:
        raise AssertionError(f"{label}: {d.shape[0]} elements of output '{name}' were never written, first at {tuple(int(v) for v in d[0])}")


def gapped_view(frames, stride, fill=np.nan):
    """The 1-D buffer of a Windower view with stride >= frame_len whose frames are the rows of `frames`; gaps hold `fill`."""
    F, N = frames.shape
    assert stride >= N
    out = np.full((F - 1) * stride + N, fill, dtype=frames.dtype)
    for t in range(F):
        out[t * stride:t * stride + N] = frames[t]
    return out


def windows(signal, frame_len, stride, n_frames):
    """Dense [F, N] copy of the Windower view of a 1-D signal (the canonical form of an overlapping view)."""
    return np.stack([signal[t * stride:t * stride + frame_len] for t in range(n_frames)])
