"""ctypes binding of ``libdeformcontact_hip.so``, derived from the C ABI's header ``include/deformcontact.h``.

There is deliberately NO fallback: if the library is missing or fails to load,
every op raises.  The CPU oracle under ``oracle/`` is test infrastructure and is
never imported from here.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint16, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libdeformcontact_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "deformcontact.h")

_lib = None


class DeformContactLibraryError(RuntimeError):
    pass


# The binding is DERIVED from the header: an entry is its prototype there plus its definition in csrc/ (which the
# compiler checks against the prototype), nothing in Python.  The type names a prototype may use:
_C_TYPES = {"void": None, "int": c_int, "int32_t": c_int32, "int64_t": c_int64, "uint16_t": c_uint16,
            "uint64_t": c_uint64, "float": c_float, "double": c_double, "dc_stream_t": c_void_p}


def _ctype(decl: str, entry: str):
    """The ctypes type of one parameter or return declaration: a scalar by value as itself; ``T *`` a device address
    (``c_void_p``: callers pass ``tensor.data_ptr()``); ``DC_HOST T *`` a host array (``POINTER(T)``); a pointer to
    pointers a host array of device addresses; ``char *`` host text.  Anything else is an error, not a guess."""
    m = re.fullmatch(r"(DC_HOST\s+)?(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(?:\w+)?", decl)
    host, base, stars = (m[1], m[2], m[3].count("*")) if m else (None, None, 0)
    if base == "char" and stars == 1 and not host:
        return c_char_p
    if base not in _C_TYPES or (host and stars != 1) or (base == "void" and (host or not stars)):
        raise DeformContactLibraryError(f"{HEADER_PATH}: {entry}: cannot bind `{decl}`")
    if stars == 0:
        return _C_TYPES[base]
    if stars == 1:
        return POINTER(_C_TYPES[base]) if host else c_void_p
    return POINTER(c_void_p)


def _parse_header(text: str):
    """``({entry: (restype, argtypes)}, {"DC_*": int})`` of the header's ``extern "C"`` block.  Strict: besides comments,
    preprocessor lines and the ``dc_stream_t`` typedef the block may hold only prototypes that map completely."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    block = re.search(r'extern "C" \{(.*)\}', text, flags=re.S)
    if block is None:
        raise DeformContactLibraryError(f'{HEADER_PATH}: no extern "C" block')
    code, defines = [], {}
    for line in block[1].splitlines():
        if line.lstrip().startswith("#"):
            m = re.fullmatch(r"\s*#\s*define\s+(DC_\w+)\s+\(?(-?\d+)\)?\s*", line)
            if m:
                defines[m[1]] = int(m[2])
        else:
            code.append(line)
    signatures = {}
    for stmt in " ".join(" ".join(code).split()).split(";"):
        stmt = stmt.strip()
        m = re.fullmatch(r"([\w *]+?)\b(dc_\w+) ?\(([^()]*)\)", stmt)
        if m is None:
            if stmt in ("", "typedef void *dc_stream_t"):
                continue
            raise DeformContactLibraryError(f"{HEADER_PATH}: not a prototype the binding understands: `{stmt[:160]}`")
        ret, name, params = m[1].strip(), m[2], [p.strip() for p in m[3].split(",")]
        signatures[name] = (None if ret == "void" else _ctype(ret, name),
                            [] if params == ["void"] else [_ctype(p, name) for p in params])
    return signatures, defines


@functools.lru_cache(maxsize=None)
def _header():
    try:
        with open(HEADER_PATH) as f:
            text = f.read()
    except OSError as e:
        raise DeformContactLibraryError(
            f"{HEADER_PATH} not found ({e.strerror}). deformcontact_amd derives its ctypes binding and its limits "
            "from that header: use the package from its source tree.") from e
    return _parse_header(text)


def __getattr__(name):
    if name == "DEFINES":           # {"DC_MAX_SEG": 4, ...}: the header's integer #define DC_* values, parsed on first use
        return _header()[1]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def lib():
    """Load (once) and return the ctypes handle.  Raises loudly when absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise DeformContactLibraryError(
                f"{SO_PATH} not found. Build it with `python -m deformcontact_amd.build` "
                "(hipcc --offload-arch=gfx950). deformcontact_amd has no CPU/PyTorch fallback.")
        try:
            handle = ctypes.CDLL(SO_PATH)
        except OSError as e:  # pragma: no cover
            raise DeformContactLibraryError(f"cannot load {SO_PATH}: {e}") from e
        for name, (res, args) in _header()[0].items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                raise DeformContactLibraryError(
                    f"{SO_PATH} does not export {name}; rebuild the library") from e
            fn.restype, fn.argtypes = res, args
        _lib = handle
        if os.environ.get(COVERAGE_ENV):
            _start_coverage(os.environ[COVERAGE_ENV])
    return _lib


# Launch-site coverage of a whole run ("Launch sites"): with DC_LAUNCH_COVERAGE_FILE set when the
# library loads, every process (children that inherit the variable included) appends the sites it reached, one
# "site \t test id at the first reach" line each, to that file when it exits.
COVERAGE_ENV = "DC_LAUNCH_COVERAGE_FILE"


def _start_coverage(path: str) -> None:
    import atexit
    _lib.dc_launch_coverage(1)

    def _append():
        lines = [f"{site}\t{test}\n" for site, test in launch_reached().items()]
        if lines:
            with open(path, "a") as f:      # one write per process: appends of concurrent children do not interleave
                f.write("".join(lines))
    atexit.register(_append)


def _dump(fn) -> list:
    n = int(fn(None, 0))
    buf = ctypes.create_string_buffer(n + 1)
    fn(buf, n + 1)
    return buf.value.decode().splitlines()


def launch_site_files() -> dict:
    """``{site: source file}`` for every launch site the library was built with (no GPU needed).  A site is
    ``kernel text @ enclosing host function``; a templated launcher gives one site per instantiation."""
    out = {}
    for line in _dump(lib().dc_launch_sites_dump):
        src, _, site = line.partition("\t")
        out[site] = src
    return out


def launch_sites() -> list:
    """Every launch site of the library (see ``launch_site_files``)."""
    return list(launch_site_files())


def launch_coverage(on: bool) -> None:
    """Start / stop adding launched sites to the cumulative reached set (``dc_launch_coverage``)."""
    lib().dc_launch_coverage(1 if on else 0)


def launch_reached() -> dict:
    """``{site: PYTEST_CURRENT_TEST at its first launch}`` for the sites reached while coverage was on."""
    return {site: test for site, test, _ in _reached_rows()}


def _reached_rows():
    return [line.split("\t") for line in _dump(lib().dc_launch_reached_dump)]


def launch_site_counts() -> dict:
    """``{site: launches while coverage was on}`` for the reached sites; the difference around a call names exactly
    the sites that call launched, whatever ran earlier in the process."""
    return {site: int(n) for site, _, n in _reached_rows()}


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().dc_last_error()
        raise DeformContactLibraryError(
            f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def kernel_trace(on: bool) -> None:
    """Start (clearing the log) / stop the library's launch log (``dc_kernel_trace``)."""
    lib().dc_kernel_trace(1 if on else 0)


def kernel_trace_counts() -> dict:
    """``{kernel name: launches}`` recorded since ``kernel_trace(True)``."""
    out = {}
    for line in _dump(lib().dc_kernel_trace_dump):
        name, _, cnt = line.rpartition(" ")
        out[name] = int(cnt)
    return out


def exported_names():
    """Every entry the header declares, in its order (needs the header, not the library)."""
    return list(_header()[0])
