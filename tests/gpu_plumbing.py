"""Device plumbing of the GPU tests: tensors, stream ids, prefilled buffers, the one factory of contexts with the kind of HIP
stream they run on, the flags the runtime reports for a context's streams, a caller that is late on purpose.  No tests here;
torch and lyra_amd are imported inside the functions."""
import os

import numpy as np

FILL = 85   # every byte of a prefilled buffer: what a call must not write still holds it afterwards


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to(_dev())


def _ids(B, max_streams, seed):
    return np.random.default_rng(seed).permutation(max_streams)[:B].astype(np.int32)


def _filled(dev, frames, width, dtype):
    """[frames][width] of `dtype`, every byte FILL: a device tensor on `dev`, a numpy array for dev=None"""
    a = np.full((frames, width * np.dtype(dtype).itemsize), FILL, np.uint8).view(dtype)
    if dev is None:
        return a
    import torch
    return torch.from_numpy(a).to(dev)


def _same(got, want, where, names=("pcm16", "pcm_ext", "is_noise", "is_comfort_noise")):
    """two tuples of per-row outputs, bit for bit; the message names the output (names=None: its index) and the rows"""
    for k, (x, y) in enumerate(zip(got, want)):
        x, y = np.asarray(x), np.asarray(y)
        what = f"output {k}" if names is None else names[k]
        assert np.array_equal(x, y), f"{where}: {what} differs in rows {np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1)).tolist()[:64]}"


def make_ctx(max_streams, mode="xnnpack", rate=None, cng_seed=None, streams=None, **kw):
    """a context on device 0; rate (the encoder's, for DTX) and cng_seed stay the library's defaults when None; **kw: LyraHip's.
    streams: None -- the kind the library picks from max_streams (CU-masked streams, which are blocking streams with respect
    to the NULL stream, up to 1,024); "plain" -- hipStreamNonBlocking priority streams whatever the size, the kind a context
    of 4,096 streams runs on: LYRA_HIP_CU_MASKS=0 for the create call alone, which reads it (api.hip lyra_hip_create)."""
    import lyra_amd
    assert streams in (None, "plain"), streams
    saved = os.environ.get("LYRA_HIP_CU_MASKS")
    if streams == "plain":
        os.environ["LYRA_HIP_CU_MASKS"] = "0"
    try:
        c = lyra_amd.LyraHip(device=0, max_streams=max_streams, requant=mode, **kw)
    finally:
        if streams == "plain":
            if saved is None:
                del os.environ["LYRA_HIP_CU_MASKS"]
            else:
                os.environ["LYRA_HIP_CU_MASKS"] = saved
    if rate is not None:
        c.set_encoder_sample_rate(rate)
    if cng_seed is not None:
        c.set_cng_seed(cng_seed)
    return c


def stream_cases(cases, plain):
    """The values of a parametrize over "<the test's names>,streams": every case of `cases` with streams=None under the id it
    has without the parameter, and the case `plain` once more with streams="plain" ("<id>-plain")."""
    import pytest
    tup = lambda c: c if isinstance(c, tuple) else (c,)                          # noqa: E731
    ident = lambda c: "-".join(str(v) for v in tup(c))                           # noqa: E731
    return [pytest.param(*tup(c), None, id=ident(c)) for c in cases] + [pytest.param(*tup(plain), "plain", id=ident(plain) + "-plain")]


HIP_STREAM_NON_BLOCKING = 1  # hipStreamNonBlocking (hip_runtime_api.h); hipStreamDefault is 0


def _hip_runtime_symbol(name):
    """`name` from the HIP runtime this process has already loaded (torch's), or None: the global scope first, then the
    libamdhip64 that /proc/self/maps lists -- opening a loaded library again gives the loaded one"""
    import ctypes
    try:
        return getattr(ctypes.CDLL(None), name)
    except (AttributeError, OSError):
        pass
    try:
        with open("/proc/self/maps") as f:
            paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    except OSError:
        paths = []
    for p in paths:
        try:
            return getattr(ctypes.CDLL(p), name)
        except (AttributeError, OSError):
            pass
    return None


def stream_flags(c):
    """hipStreamGetFlags of the context's encode-side, decode-side, quantizer and noise streams, in that order; None when the
    loaded runtime does not export the symbol"""
    import ctypes
    fn = _hip_runtime_symbol("hipStreamGetFlags")
    if fn is None:
        return None
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint)]
    noise = c.L.lyra_hip_stream_noise            # (in include/lyra_hip.h; codec.py has no use for it)
    noise.restype, noise.argtypes = ctypes.c_void_p, [ctypes.c_void_p]
    out = []
    for h in (c.stream_handle(), c.stream_handle_decode(), c.stream_handle_quantizer(), noise(c.h)):
        assert h, "a library stream handle is NULL"
        v = ctypes.c_uint(0xFFFFFFFF)
        rc = fn(ctypes.c_void_p(h), ctypes.byref(v))
        assert rc == 0, f"hipStreamGetFlags failed ({rc})"
        out.append(int(v.value))
    return out


def _pinned(a, dtype=None):
    """the array in pinned host memory: a copy from it with non_blocking=True queues on the current stream"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).pin_memory()


class LateStream:
    """A caller that is late on purpose: a torch side stream (not the NULL stream) on which every `upload` is queued behind
    `ms` milliseconds of ordinary torch work (matmuls on a scratch tensor, their number from a timing at construction: bounded
    work, no spinning on host state).  What runs on a library stream without an event on this stream's work reads the
    destination's EARLIER content.  `total_ms`: the work enqueued so far, `BUDGET_MS` what one test case may spend."""
    BUDGET_MS = 500.0
    DIM = 2048

    def __init__(self, ms):
        import time
        import torch
        self.ms = float(ms)
        self.stream = torch.cuda.Stream(device=_dev())
        self.total_ms = 0.0
        self._a = torch.full((self.DIM, self.DIM), 1.0 / self.DIM, dtype=torch.float32, device=_dev())
        self._b = torch.empty_like(self._a)
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            for _ in range(3):                       # (the first matmul loads its kernel)
                torch.mm(self._a, self._a, out=self._b)
            self.stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(8):
                torch.mm(self._a, self._a, out=self._b)
            self.stream.synchronize()
            self.ms_per_matmul = max((time.perf_counter() - t0) * 1e3 / 8, 1e-3)
        self.reps = max(1, int(np.ceil(self.ms / self.ms_per_matmul)))

    def resize(self, ms):
        """`ms` milliseconds of late work per hold from here on, by the timing made at construction"""
        self.ms = float(ms)
        self.reps = max(1, int(np.ceil(self.ms / self.ms_per_matmul)))

    def hold(self):
        """enqueue the late work on the stream (call under `with torch.cuda.stream(self.stream)` or not: it names the stream)"""
        import torch
        self.total_ms += self.reps * self.ms_per_matmul
        assert self.total_ms < self.BUDGET_MS, f"late work of {self.total_ms:.0f} ms in one test case"
        with torch.cuda.stream(self.stream):
            for _ in range(self.reps):
                torch.mm(self._a, self._a, out=self._b)

    def clear_of(self, probe, tries=8):
        """Move to a torch stream whose late work does not hold `probe` back, -> whether one was found.  A process's streams
        share a few hardware queues (GPU_MAX_HW_QUEUES; the four streams of a context lie on four different ones, api.hip
        lyra_hip_create), and a queue runs its entries in order: library work that lands behind the late work on the same
        queue waits for it as if an event had ordered it, and the control would see nothing.  probe(): the call under test and
        a wait for the library's streams alone; the stream is clear if its late work is still pending when probe returns."""
        import torch
        for _ in range(tries):
            self.hold()
            probe()
            pending = not self.stream.query()
            self.stream.synchronize()
            if pending:
                return True
            self.stream = torch.cuda.Stream(device=_dev())
        return False

    def upload(self, dst, host, late=True):
        """dst.copy_(host) from pinned memory on the stream, behind the late work (late=False: behind nothing new)"""
        import torch
        assert host.is_pinned() and dst.is_cuda
        if late:
            self.hold()
        with torch.cuda.stream(self.stream):
            dst.copy_(host, non_blocking=True)


def late_stream(ms):
    return LateStream(ms)


SCRUB16, SCRUB32, SCRUB_F = 0x3333, 0x33333333, -7777.0   # what a host buffer holds once its call has returned


def scrub(*buffers, ids=(), max_streams=0):
    """Overwrite pinned host tensors in place, as a caller that reuses its buffers on return: samples SCRUB16, bytes FILL,
    int32 arrays SCRUB32 (no rate, packet size, bit count, request size or room label a test uses), floats SCRUB_F.  `ids`:
    arrays of stream ids become max_streams - 1 - id -- other ids, still distinct and inside the context: the kernels index
    the per-stream state by id unchecked, so a stale read of an id must show as a wrong result and a wrong state, never as a
    write outside the state (max_streams even: no id stays what it was)."""
    import torch
    pattern = {torch.int16: SCRUB16, torch.uint8: FILL, torch.int32: SCRUB32, torch.float32: SCRUB_F}
    for t in buffers:
        assert t.is_pinned(), "a buffer under test is not in pinned memory"
        t.fill_(pattern[t.dtype])
    for t in ids:
        assert t.is_pinned() and t.dtype == torch.int32 and max_streams % 2 == 0
        t.copy_(max_streams - 1 - t)


class Held:
    """Host-buffer calls on context `c` made while its four library streams wait behind the late caller's work
    (lyra_hip_wait_for_stream: the public way to order library work behind a caller stream): an upload that such a call
    enqueues cannot start before the late work ends, so a call that returns without having waited for it leaves the upload to
    read whatever the caller has put into the buffer since.  call(fn, *buffers, ids=...) holds, asserts that the hold is live,
    runs fn and scrubs the buffers on return.  `returned_early` counts the calls that came back with the late work pending
    (calls that enqueue nothing behind it may: what matters is the result).  live = False: the call and the scrub without the
    hold, for a call's first use, whose allocations and kernel loads no hold of a few milliseconds outlasts."""

    def __init__(self, c, late):
        self.c, self.late, self.calls, self.returned_early, self.live = c, late, 0, 0, True

    def call(self, fn, *buffers, ids=()):
        c, late = self.c, self.late
        if not self.live:
            got = fn()
            scrub(*buffers, ids=ids, max_streams=c.max_streams)
            return got
        late.hold()
        c._chk(c.L.lyra_hip_wait_for_stream(c.h, late.stream.cuda_stream))
        assert not late.stream.query(), "the late work was over before the call was made: nothing held the library back"
        got = fn()
        self.calls += 1
        self.returned_early += int(not late.stream.query())
        scrub(*buffers, ids=ids, max_streams=c.max_streams)
        return got


def late_delay_ms(synchronised_call_s):
    """How long a late caller holds an upload back: 20 times the duration of the same call fully synchronised, at least 2 ms
    and at most 50 ms -- the library's kernels start at once and must have finished inside it, with room for launch jitter."""
    return min(50.0, max(2.0, 20.0 * synchronised_call_s * 1e3))
