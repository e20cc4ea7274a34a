"""ctypes binding of libseevcn_hip.so (the C-ABI in include/seevcn_hip.h).

There is no CPU fallback: if the library is missing or a symbol is absent, import of any op fails loudly.
Tensors are passed as raw device pointers plus the current torch HIP stream.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SEEVCN_LIB") or os.path.join(_HERE, "lib", "libseevcn_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "seevcn_hip.h")


class SeevcnHipError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}
_PROTOTYPE = re.compile(r"\b(\w[\w ]*?\**)\s*\b(sv_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", re.S)
_SYMBOL = re.compile(r"\b(sv_[a-z0-9_]+)\s*\(")


def parse_declarations(text):
    """name -> (return type, [parameters]) of every `ret sv_name(params);` in the header text `text`, as C text with single spaces
    (`const float* x`).  Raises when a declaration of an sv_* symbol is not of that form."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {name: (" ".join(ret.split()), [] if params.strip() in ("", "void") else [" ".join(p.split()) for p in params.split(",")])
             for ret, name, params in _PROTOTYPE.findall(text)}
    symbols = set(_SYMBOL.findall(text))
    if len(decls) != len(symbols):
        raise SeevcnHipError(f"seevcn_hip.h: {len(symbols)} sv_* symbols, {len(decls)} parsed as prototypes; not parsed: {sorted(symbols - set(decls))}")
    return decls


def _ctype(decl, name):
    """ctypes type of a return type or parameter: `const char*` is a string, every other pointer is void*, scalars by their type name."""
    words = decl.replace("*", " * ").split()
    if words[:3] == ["const", "char", "*"]:
        return ctypes.c_char_p
    if "*" in words:
        return ctypes.c_void_p
    words = [w for w in words if w != "const"]
    if words and words[0] in _SCALARS and len(words) <= 2:               # the type, or the type and the parameter's name
        return _SCALARS[words[0]]
    raise SeevcnHipError(f"seevcn_hip.h: {name}: no ctypes type for `{decl}`")


def parse_prototypes(text):
    """name -> (restype, [argtypes]) of every prototype in the header text `text`; a type this binding does not map is an error."""
    return {name: (_ctype(ret, name), [_ctype(p, name) for p in params]) for name, (ret, params) in parse_declarations(text).items()}


# name -> (restype, argtypes) of every entry: include/seevcn_hip.h is the only place a prototype is written down
with open(HEADER_PATH) as _header:
    SIGNATURES = parse_prototypes(_header.read())

_lib = None


def load():
    """Load the shared library (once) and attach signatures. Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SeevcnHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(or `make -C see-vcn_amd/csrc`). seevcn_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError = ABI mismatch, fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


# switches and entry points that only the measurement build of the library has (csrc/Makefile, target `measure`)
MEASURE_SWITCHES = ("SEEVCN_RS3_DEBUG", "SEEVCN_PLAN_DEBUG", "SEEVCN_WGRAD_DEBUG", "SEEVCN_WGRAD_SKIP", "SEEVCN_DEBUG_SKIP_FINALIZE")


def require_measure_build(who):
    """For measurement tools: exit with one line unless the loaded library is the measurement build."""
    if not load().sv_measure_build():
        raise SystemExit(f"{who}: needs the measurement build of the library (make -C see-vcn_amd/csrc measure, then "
                         f"SEEVCN_LIB=see-vcn_amd/lib/variants/libseevcn_hip_measure.so); {LIB_PATH} is a production build")


_NOT_ON_GPU = "seevcn_amd ops run on the GPU only (got a CPU tensor); there is no CPU fallback"


def check(rc, what):
    if rc != 0:
        msg = load().sv_last_error().decode(errors="replace")
        raise SeevcnHipError(f"{what} failed (code {rc}): {msg}")


def launch(name, *args):
    """Enqueue entry `name` (one whose last parameter is `void* stream`) with `args` on the calling thread's current stream; raise on a
    non-zero status."""
    rc = getattr(_lib or load(), name)(*args, _raw_stream(_get_device()))
    if rc != 0:
        check(rc, name)


def ptr(t):
    """Device pointer of a contiguous GPU tensor (None -> NULL).  Every tensor that reaches a kernel comes through here, so this is where a
    host tensor is refused: passed on, it would be an illegal memory access on the device, not a Python error."""
    if t is None:
        return None
    assert t.is_contiguous(), "seevcn_amd ops need contiguous tensors"
    if not t.is_cuda:
        raise SeevcnHipError(_NOT_ON_GPU)
    return t.data_ptr()


def stream():
    """Raw handle of the calling thread's current stream.  (torch.cuda.current_stream() builds a Stream object through four layers of device
    index helpers: 10 us a call, 74 calls per bench step = 0.7 ms of a host thread that the step is bound by.)"""
    return _raw_stream(_get_device())


_raw_stream = torch._C._cuda_getCurrentRawStream
_get_device = torch._C._cuda_getDevice


import threading as _threading

_sync_hooks = _threading.local()


def _take_checks():
    """The parked checks whose value the CURRENT stream orders (parked on it); checks parked on another stream stay parked -- read here they
    would race with the stream that still computes them (bench.py runs a piece of the trained side, main stream, inside a read of the
    input side, side stream: a lazily built rulebook there must not pick up the input side's pending empty-cluster check)."""
    pending = getattr(_sync_hooks, "checks", None)
    if not pending:
        return []
    cur = stream()
    mine = [c for c in pending if c[0] == cur]
    if mine:
        _sync_hooks.checks = [c for c in pending if c[0] != cur]
    return mine


def host_int(t):
    """int(t.item()) -- a device -> host read that blocks the calling thread until the stream has produced t.  A caller that has other work to
    enqueue meanwhile (bench.py: the trained side of the previous batch) installs a hook with set_sync_hook(); it runs right before the read,
    i.e. after the kernels that produce t were launched, so the wait is spent enqueueing instead of idling.  Checks parked with defer_check()
    on the same stream ride on this read: their values come back in the same copy."""
    return host_ints([t])[0]


def host_ints(tensors):
    """The integers of `tensors` (0-dim / one-element tensors, or longer ones: their elements in order) as one flat Python list with ONE blocking
    device -> host read: one concatenation kernel + one copy (same hook and parked checks as host_int)."""
    hook = getattr(_sync_hooks, "before", None)
    if hook is not None:
        hook()
    pending = _take_checks()
    if not pending and len(tensors) == 1 and tensors[0].numel() == 1:
        return [int(tensors[0].item())]
    flat = [t.reshape(-1) for t in tensors] + [p.reshape(-1) for _, p, _ in pending]
    if len({t.dtype for t in flat}) > 1:
        flat = [t.to(torch.int64) for t in flat]
    vals = torch.cat(flat).tolist()
    n = len(vals) - len(pending)
    for v, (_, _, fn) in zip(vals[n:], pending):
        fn(int(v))
    return [int(v) for v in vals[:n]]


def defer_check(t, fn):
    """Park a validity check on a 0-dim device integer: fn(value) runs (and may raise) at the calling thread's next host_int() or
    flush_checks() ON THE SAME STREAM -- whose order guarantees t is final by then -- instead of costing a blocking read of its own."""
    if getattr(_sync_hooks, "checks", None) is None:
        _sync_hooks.checks = []
    _sync_hooks.checks.append((stream(), t, fn))


def flush_checks():
    """Run the checks parked on the current stream now (one blocking read) -- for call sites that are not followed by a host_int()."""
    pending = _take_checks()
    if pending:
        flat = [p.reshape(-1) for _, p, _ in pending]
        if len({t.dtype for t in flat}) > 1:
            flat = [t.to(torch.int64) for t in flat]
        for v, (_, _, fn) in zip(torch.cat(flat).tolist(), pending):
            fn(int(v))


def set_sync_hook(fn):
    """Install (or with None remove) the calling thread's before-read hook; returns the previous one."""
    prev = getattr(_sync_hooks, "before", None)
    _sync_hooks.before = fn
    return prev


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise SeevcnHipError(_NOT_ON_GPU)


def host_array(ctype, values):
    return (ctype * len(values))(*values)


class Workspace:
    """Grow-only device byte buffers, one set per (device, stream).

    `persistent(name, nbytes)` returns a zero-initialised buffer that the kernels keep zeroed between calls
    (coordinate-index bitmaps); `scratch(name, nbytes)` returns uninitialised bytes.  Every buffer is used inside ONE op call on the
    calling thread's current stream; the key holds that stream's raw handle, so two streams (bench.py runs the input side of batch N + 1
    beside the trained side of batch N) never share a buffer, and a grow-realloc frees a buffer only on the stream that used it.
    """

    def __init__(self):
        self._bufs = {}

    def _get(self, kind, name, nbytes, device, zero):
        if device.type != "cuda":
            raise SeevcnHipError(_NOT_ON_GPU)
        key = (kind, name, device.index, _raw_stream(device.index if device.index is not None else _get_device()))
        buf = self._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            n = int(nbytes * 1.25) + 256 if buf is not None else int(nbytes)
            n = max(n, 256)
            buf = (torch.zeros if zero else torch.empty)(n, dtype=torch.uint8, device=device)
            self._bufs[key] = buf
        return buf

    def persistent(self, name, nbytes, device):
        return self._get("p", name, nbytes, device, True)

    def scratch(self, name, nbytes, device):
        return self._get("s", name, nbytes, device, False)

    def reset(self):
        self._bufs.clear()


workspace = Workspace()
