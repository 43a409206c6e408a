"""ctypes binding of the C-ABI HIP library (include/ppf_hip.h).

There is NO CPU or eager fallback: if the shared library is missing or a call fails, this raises."""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PPF_LIB_PATH") or os.path.join(_HERE, "lib", "libppf_hip.so")      # PPF_LIB_PATH: an alternative build (same-box A/B of two builds)

HEADER = os.path.join(os.path.dirname(_HERE), "include", "ppf_hip.h")

# include/ppf_hip.h is the one place an entry point is declared: the kernels are compiled against it and this binding is parsed from it.
# signature spec per entry point: p = device/host pointer, i = int32, l = int64, L = uint64, f = float, z = size_t, s = hipStream_t
_LETTER = {"int": "i", "int64_t": "l", "uint64_t": "L", "float": "f", "size_t": "z"}
_RET = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}


def _ctype(text):
    return re.sub(r"\s*\*", "*", " ".join(text.split()))              # one spelling: 'const char*'


def parse_header(text):
    """({entry point: spec}, {entry point: ctypes return type}, {PPF_X: value of an integer #define}) of the text of a ppf_hip.h.
    A ppf_stream_t in the LAST position is the stream call() appends ('s'), except in the ppf_stream_* functions, whose streams are
    explicit arguments ('p').  A type without an entry in _LETTER / _RET raises, naming the function: it never defaults."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(PPF_\w+)\s+\(?(-?\d+)\)?\s*$", text, flags=re.M)}
    sigs, rets = {}, {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(ppf_\w+)\s*\(([^()]*)\)\s*;", re.sub(r"^\s*#.*$", "", text, flags=re.M)):
        if _ctype(ret) not in _RET:
            raise ValueError(f"{name}: return type '{_ctype(ret)}' has no ctypes mapping")
        params = [] if params.strip() in ("", "void") else params.split(",")
        spec = ""
        for i, prm in enumerate(params):
            t = _ctype(re.sub(r"\bconst\b|\w+\s*$", "", prm))          # the type without qualifier and parameter name
            if t == "ppf_stream_t":
                spec += "s" if i == len(params) - 1 and not name.startswith("ppf_stream_") else "p"
            elif t.endswith("*"):
                spec += "p"
            elif t in _LETTER:
                spec += _LETTER[t]
            else:
                raise ValueError(f"{name}: parameter '{prm.strip()}' has no ctypes mapping")
        sigs[name], rets[name] = spec, _RET[_ctype(ret)]
    return sigs, rets, defines


with open(HEADER) as _f:
    SIGS, _RESTYPE, DEFINES = parse_header(_f.read())
EXPECTED_ABI = DEFINES["PPF_ABI_VERSION"]              # lib() refuses a library built from a header of another version

_CT = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_int64, "L": ctypes.c_uint64, "f": ctypes.c_float, "s": ctypes.c_void_p, "z": ctypes.c_size_t}
_lib = None
_FAST = {}                     # name -> (bound function, pointer-argument positions, has trailing stream, arity)
_stream_override = []          # raw hipStream_t stack: set by the weight-gradient lane while it enqueues on its own stream


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not found: build it with `python -m protopformer_amd.build` "
                               "(there is no fallback path)")
        _lib = ctypes.CDLL(LIB_PATH)
        got = _lib.ppf_abi_version()
        if got != EXPECTED_ABI:
            _lib = None
            raise RuntimeError(f"{LIB_PATH} was built for ABI version {got}, this binding expects {EXPECTED_ABI}: rebuild it with "
                               "`python -m protopformer_amd.build --force` (a stale library would receive shifted arguments)")
        for name, spec in SIGS.items():
            fn = getattr(_lib, name)
            fn.restype = _RESTYPE[name]
            fn.argtypes = [_CT[c] for c in spec]
            if fn.restype is ctypes.c_int:             # call() reads the return value as a status
                _FAST[name] = (fn, tuple(i for i, c in enumerate(spec) if c == "p"), spec.endswith("s"), len(spec))
    return _lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)     # C entry: ~0.2 us (torch.cuda.current_stream() costs ~8 us)
_dev_index = None


def stream_ptr():
    """Raw hipStream_t the next launch goes to: the weight-gradient lane's while it is enqueueing, else torch's current stream
    on this process's device (one process drives one GPU; the device index is read once)."""
    global _dev_index
    if _stream_override:
        return _stream_override[-1]
    if _raw_stream is None:
        return torch.cuda.current_stream().cuda_stream
    if _dev_index is None:
        _dev_index = torch.cuda.current_device()
    return _raw_stream(_dev_index)


def push_stream(raw):
    _stream_override.append(raw)


def pop_stream():
    _stream_override.pop()


def call(name, *args):
    """Invoke an entry point on the current stream (stream_ptr()); the stream argument is appended automatically
    when the signature ends in 's'."""
    if _lib is None:
        lib()
    fn, ptr_pos, has_stream, arity = _FAST[name]
    if has_stream and len(args) == arity - 1:
        args = args + (stream_ptr(),)
    if len(args) != arity:
        raise TypeError(f"{name}: expected {arity} arguments, got {len(args)}")
    a = list(args)
    for i in ptr_pos:
        x = a[i]
        if x is not None and not isinstance(x, int):
            a[i] = x.data_ptr()
    rc = fn(*a)
    if rc != 0:
        raise RuntimeError(f"{name} failed (rc={rc}): {_lib.ppf_last_error().decode()}")
    if _rec is not None and not _rec.suspended:
        _rec.add_call(name, fn, a, args)


# ------------------------------------------------------------------------------------------------ recorded command lists
# One train step is ~300-800 launches; enqueueing them from Python costs ~20 us each (allocation, shape logic, autograd), which makes
# the small configurations host-bound (HIP graphs do not help on ROCm 7.2: hipGraphLaunch re-enqueues every node from the host at
# the same cost, profiles/r2_graph_timeline.txt).  A Recorder keeps, for ONE eagerly executed step, every library call with its
# converted arguments (raw pointers, sizes, streams) and keeps the tensors alive, so their addresses stay valid; replay() then walks
# the list: one pre-bound ctypes call (~2-3 us) per launch, no Python orchestration, no allocation, no autograd.  What cannot be
# frozen runs as a LIVE Python callable in its place in the list (optimizer scalars, the RCCL collectives of the gradient exchange).
class Recorder:
    CALL, MARK, WAIT, LIVE = 0, 1, 2, 3

    def __init__(self):
        self.cmds, self.keep, self.tickets, self.nslots, self.suspended = [], [], {}, 0, 0
        self.main_stream = stream_ptr() if torch.cuda.is_available() else None      # torch's current stream while the step was recorded

    def add_call(self, name, fn, a, args):
        if name == "ppf_stream_wait_mark":
            slot = self.tickets.get(a[1])
            if slot is not None:              # (a ticket taken before the recording started guards work that is long complete)
                self.cmds.append((Recorder.WAIT, fn, a[0], slot))
            return
        self.cmds.append((Recorder.CALL, fn, tuple(a), name))
        self.keep.append(args)                # the tensors behind the recorded pointers stay allocated


_rec = None


def start_recording():
    global _rec
    if _rec is not None:
        raise RuntimeError("a recording is already in progress")
    _rec = Recorder()
    return _rec


def stop_recording():
    global _rec
    r, _rec = _rec, None
    return r


def stream_mark(raw):
    """Ticket for 'everything enqueued on `raw` so far' (ppf_stream_mark); recorded symbolically: a replay takes a fresh ticket."""
    t = lib().ppf_stream_mark(raw)
    if t < 0:
        raise RuntimeError(_lib.ppf_last_error().decode())
    if _rec is not None and not _rec.suspended:
        _rec.tickets[t] = _rec.nslots
        _rec.cmds.append((Recorder.MARK, raw, _rec.nslots))
        _rec.nslots += 1
    return t


def run_live(fn):
    """Run fn() now; inside a recording it also becomes a LIVE entry of the command list (executed again by every replay, at this
    position): host-side state that changes from step to step (optimizer scalars) and calls outside the library (collectives)."""
    if _rec is None or _rec.suspended:
        return fn()
    _rec.suspended += 1
    try:
        out = fn()
    finally:
        _rec.suspended -= 1
    _rec.cmds.append((Recorder.LIVE, fn))
    return out


def _arm_plan(cmds):
    """{index of a recorded library call: its launch stream} for the calls that are directly followed by ppf_stream_wait_stream(dst, that
    stream): their kernels are launched with a completion event attached (ppf_stream_arm), so the wait does not have to put an event-record
    packet into the producer's queue.  Same-box A/B (profiles/r6_armed_events.txt): deit_small +0.3 %, deit_tiny +0.5 %, cait_xxs24 +0.4 %; main-queue idle
    between kernels 0.87 -> 0.67 ms per deit_small step."""
    plan = {}
    for i, c in enumerate(cmds[:-1]):
        n = cmds[i + 1]
        if c[0] != 0 or n[0] != 0 or n[3] != "ppf_stream_wait_stream" or c[3].startswith("ppf_stream_"):
            continue
        if not _FAST[c[3]][2]:
            continue
        stream = c[2][-1]
        if stream is not None and stream == n[2][1]:
            plan[i] = stream
    return plan


def replay(rec):
    """Enqueue a recorded step again: same kernels, same arguments, same streams and cross-stream dependencies.  The list holds the raw
    streams of the recording; the caller's input copies and the live collectives go to torch's CURRENT stream, so that must be the one the
    step was recorded under."""
    if rec.main_stream is not None and not _stream_override and stream_ptr() != rec.main_stream:
        raise RuntimeError("replay(): the current torch stream differs from the stream the step was recorded on (input copies and "
                           "collectives would not be ordered with the recorded launches); replay under the recording's stream")
    slots = [0] * rec.nslots
    mark = _lib.ppf_stream_mark
    arm_at = getattr(rec, "arm_at", None)
    if arm_at is None:
        arm_at = rec.arm_at = _arm_plan(rec.cmds)
    arm = _FAST["ppf_stream_arm"][0]
    for i, c in enumerate(rec.cmds):
        k = c[0]
        if k == 0:
            if i in arm_at:
                arm(arm_at[i], 1)           # this call's launches carry their completion event: the wait that follows records nothing
            rc = c[1](*c[2])
            if rc != 0:
                if i in arm_at:
                    arm(arm_at[i], 0)       # a failed call leaves no armed stream behind for later eager launches
                raise RuntimeError(f"{c[3]} failed in replay (rc={rc}): {_lib.ppf_last_error().decode()}")
        elif k == 1:
            t = mark(c[1])
            if t < 0:
                raise RuntimeError(f"ppf_stream_mark failed in replay: {_lib.ppf_last_error().decode()}")
            slots[c[2]] = t
        elif k == 2:
            rc = c[1](c[2], slots[c[3]])
            if rc != 0:
                raise RuntimeError(f"ppf_stream_wait_mark failed in replay (rc={rc}): {_lib.ppf_last_error().decode()}")
        else:
            c[1]()
