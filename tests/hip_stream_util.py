"""The HIP runtime through ctypes, for the tests that hand the library a stream of the caller's (tests/test_borrowed_stream.py).

The streams must come from the SAME runtime libmmdx.so runs on: a second copy of libamdhip64 in the process (a Python wheel that
bundles its own, for one) would hand out streams the library's runtime has never heard of.  So the runtime is opened by the
soname libmmdx.so itself names as a dependency, after the library is loaded -- dlopen() then returns the copy that is already
there -- and hip() checks that the process maps exactly one file of that name.  Nothing here imports torch.

Gate: a host function (hipLaunchHostFunc) that holds its stream until the test opens it -- or until 5 s have passed.  The
timeout is a condition, never a measurement: it is what keeps a mistake in a test from becoming a hang, and a test that sees a gate
time out fails (Gate.open() asserts).  Open every gate in a `finally`, before any device-wide synchronisation and before the
stream is destroyed (Stream.close() opens the gates that are still closed first)."""
import ctypes as C
import re
import threading

from simple_mmd_renderer_amd import _capi as api

SUCCESS = 0
ERROR_NOT_READY = 600                       # hipErrorNotReady
STREAM_NON_BLOCKING = 1                     # hipStreamNonBlocking
CAPTURE_NONE, CAPTURE_ACTIVE, CAPTURE_INVALIDATED = 0, 1, 2      # hipStreamCaptureStatus
GATE_TIMEOUT_S = 5.0

HOST_FN = C.CFUNCTYPE(None, C.c_void_p)     # hipHostFn_t

_hip = None


def runtime_soname() -> str:
    """The soname of the HIP runtime in libmmdx.so's list of dependencies (its .dynstr holds the name)."""
    names = set(re.findall(rb"libamdhip64\.so(?:\.\d+)*", open(api.LIB_PATH, "rb").read()))
    assert len(names) == 1, f"libmmdx.so names {sorted(names)} as its HIP runtime"
    return names.pop().decode()


def mapped_runtimes() -> set:
    """The files called libamdhip64* that this process maps."""
    with open("/proc/self/maps") as f:
        return {line.split()[-1] for line in f if "libamdhip64" in line}


def hip() -> C.CDLL:
    """The runtime libmmdx.so is linked against (loaded by it; this only takes a second handle to it)."""
    global _hip
    if _hip is None:
        api.lib()                                           # libmmdx.so first: it brings its runtime
        before = mapped_runtimes()
        assert len(before) == 1, f"expected the one HIP runtime libmmdx.so loaded, found {sorted(before)}"
        h = C.CDLL(runtime_soname())
        assert mapped_runtimes() == before, f"a second HIP runtime was loaded: {sorted(mapped_runtimes())}"
        for name, args in (("hipStreamCreateWithFlags", [C.POINTER(C.c_void_p), C.c_uint]), ("hipStreamDestroy", [C.c_void_p]),
                           ("hipStreamQuery", [C.c_void_p]), ("hipStreamSynchronize", [C.c_void_p]),
                           ("hipStreamIsCapturing", [C.c_void_p, C.POINTER(C.c_int)]),
                           ("hipLaunchHostFunc", [C.c_void_p, HOST_FN, C.c_void_p]), ("hipSetDevice", [C.c_int]),
                           ("hipGetLastError", [])):
            fn = getattr(h, name)
            fn.restype, fn.argtypes = C.c_int, args
        _hip = h
    return _hip


def _ok(status, what):
    if status != SUCCESS:
        hip().hipGetLastError()
        raise RuntimeError(f"{what}: HIP error {status}")


class Gate:
    """One closed gate on a stream: everything enqueued on the stream behind it waits for open()."""

    def __init__(self, stream: "Stream"):
        self._event = threading.Event()
        self._done = threading.Event()          # set when the host function has returned (by either way out)
        self.timed_out = False
        self.opened = False

        def hold(_):
            self.timed_out = not self._event.wait(GATE_TIMEOUT_S)
            self._done.set()
        self._fn = HOST_FN(hold)                # kept alive with the gate, the gate with its stream
        stream.gates.append(self)
        _ok(hip().hipLaunchHostFunc(stream.ptr, self._fn, None), "hipLaunchHostFunc")

    def release(self) -> None:
        """Let the stream go on (idempotent, never raises: for `finally` blocks)."""
        self.opened = True
        self._event.set()

    def open(self) -> None:
        """release(), and the gate must have held until now."""
        self.release()
        assert self._done.wait(GATE_TIMEOUT_S) and not self.timed_out, \
            "the gate timed out before the test opened it: the stream ran on after 5 s without being told to"


class Stream:
    """A non-blocking stream of the test's own, on `device` (the library never sees the null stream's implicit ordering)."""

    def __init__(self, device: int = 0):
        self.gates = []
        self.device = device
        _ok(hip().hipSetDevice(device), "hipSetDevice")
        p = C.c_void_p()
        _ok(hip().hipStreamCreateWithFlags(C.byref(p), STREAM_NON_BLOCKING), "hipStreamCreateWithFlags")
        self.ptr = p.value

    def query(self) -> int:
        """hipStreamQuery: SUCCESS (idle) or ERROR_NOT_READY (work pending)."""
        st = hip().hipStreamQuery(self.ptr)
        if st not in (SUCCESS, ERROR_NOT_READY):
            _ok(st, "hipStreamQuery")
        return st

    def synchronize(self) -> None:
        _ok(hip().hipStreamSynchronize(self.ptr), "hipStreamSynchronize")

    def capture_status(self) -> int:
        s = C.c_int(-1)
        _ok(hip().hipStreamIsCapturing(self.ptr, C.byref(s)), "hipStreamIsCapturing")
        return s.value

    def gate(self) -> Gate:
        return Gate(self)

    def close(self) -> None:
        if self.ptr:
            for g in self.gates:
                g.release()
            hip().hipStreamSynchronize(self.ptr)
            _ok(hip().hipStreamDestroy(self.ptr), "hipStreamDestroy")
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
