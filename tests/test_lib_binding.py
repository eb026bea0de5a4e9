"""CPU: the ctypes binding is derived from ``include/deformcontact.h`` (``_lib._parse_header``): literal pins of one
signature per parameter class, the parser's refusals, the ``DC_HOST`` markers of the real header, and every Python
constant that states a ``#define DC_*`` limit."""
import ctypes
import re
from ctypes import POINTER, c_char_p, c_float, c_int, c_int64, c_void_p

import pytest

from deformcontact_amd import _lib, attention, graph, neighbors, ops, pointops
from deformcontact_amd.layers import gat_heads, gmm, spline

vp, i64 = c_void_p, c_int64

PINNED = {
    # the hand-written example of INTEGRATION.md section 2
    "dc_spmm_f32": (c_int, [vp] * 4 + [i64, vp, i64, vp, i64, i64, i64, vp]),
    # host int64 arrays between device pointers
    "dc_graph_build_segmented": (c_int, [vp, i64, i64, POINTER(i64), POINTER(i64), c_int] + [vp] * 10),
    # a pointer to pointers, then host arrays
    "dc_graph_build_parts": (c_int, [POINTER(vp), POINTER(i64), POINTER(i64), POINTER(i64), c_int, i64, c_int]
                             + [vp] * 10 + [i64, vp]),
    # host int outputs
    "dc_graph_build_plan": (c_int, [i64, i64, c_int, POINTER(c_int), POINTER(c_int)]),
    # host floats next to device pointers
    "dc_morton_codes": (c_int, [vp, i64, i64, POINTER(c_float), POINTER(c_float), vp, vp]),
    # a float scalar
    "dc_neighbors_fill": (c_int, [vp, i64, i64, vp, vp, i64, i64, vp, c_int, c_float, c_int, c_int, vp, vp, vp, i64, vp]),
    "dc_kernel_trace_dump": (i64, [c_char_p, i64]),
    "dc_kernel_trace": (None, [c_int]),
    "dc_last_error": (c_char_p, []),
    # a device int64_t * stays an address: callers pass tensor.data_ptr()
    "dc_hash_i64": (c_int, [vp, i64, vp, vp]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signatures(name):
    restype, argtypes = _lib._header()[0][name]
    want_res, want_args = PINNED[name]
    assert restype is want_res
    assert len(argtypes) == len(want_args)
    for i, (got, want) in enumerate(zip(argtypes, want_args)):
        assert got is want, f"{name}: argument {i} is {got}, not {want}"
    fn = getattr(_lib.lib(), name)                      # ... and that is what the loaded library carries
    assert fn.restype is want_res and list(fn.argtypes) == want_args


def _parse(body: str):
    return _lib._parse_header('#include <stdint.h>\nextern "C" {\ntypedef void *dc_stream_t;\n#define DC_HOST\n'
                              + body + "\n}\n")


def test_parser_reads_a_small_header():
    sigs, defines = _parse("/* int dc_in_a_comment(int); */\n#define DC_CAP 7\n#define DC_ERR (-2) /* why */\n"
                           "int64_t dc_a(void);\n"
                           "void dc_b(const float *x, DC_HOST const int32_t *h,\n   float *const *ps, double d, "
                           "dc_stream_t stream); // tail\nconst char *dc_c(char *buf, int64_t cap);")
    assert defines == {"DC_CAP": 7, "DC_ERR": -2}
    assert sigs == {"dc_a": (i64, []), "dc_b": (None, [vp, POINTER(ctypes.c_int32), POINTER(vp), ctypes.c_double, vp]),
                    "dc_c": (c_char_p, [c_char_p, i64])}


@pytest.mark.parametrize("body, names", [
    ("int dc_bad(const float *x, size_t n);", ("dc_bad", "size_t n")),                  # an unknown type
    ("int dc_bad(int n, int (*cb)(int));", ("dc_bad", "(*cb)")),                        # a function pointer
    ("int dc_bad(int n, ...);", ("dc_bad", "...")),
    ("int dc_bad(DC_HOST int64_t n);", ("dc_bad", "DC_HOST int64_t n")),                # the marker on a non-pointer
    ("int dc_bad(DC_HOST const int64_t *const *p);", ("dc_bad", "DC_HOST")),            # ... on a pointer to pointers
    ("int dc_bad(DC_HOST void *p);", ("dc_bad", "DC_HOST void")),
    ("int dc_bad(void x);", ("dc_bad", "void x")),
    ("unsigned dc_bad(int n);", ("dc_bad", "unsigned")),
    ("int dc_good(int n);\nint dc_bad(int n, int64_t m", ("dc_bad",)),                  # cut off before the ';'
    ("int dc_bad(int n\nint dc_good(int n);", ("dc_bad",)),
    ("static int helper;", ("static int helper",)),                                     # not a prototype at all
    ("typedef int dc_other_t;", ("dc_other_t",)),                                       # only the one typedef
])
def test_parser_refuses_what_it_cannot_map(body, names):
    with pytest.raises(_lib.DeformContactLibraryError) as e:
        _parse(body)
    for n in names:
        assert n in str(e.value), str(e.value)


def test_missing_header_raises_like_a_missing_library(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "deformcontact.h"))
    with pytest.raises(_lib.DeformContactLibraryError, match="deformcontact.h not found"):
        _lib._header.__wrapped__()


def test_exported_names_need_no_library(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "SO_PATH", str(tmp_path / "absent.so"))
    assert {"dc_version", "dc_spmm_f32", "dc_adam_flat"} <= set(_lib.exported_names())


def test_every_host_marker_sits_on_a_single_star_pointer():
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    marked = re.findall(r"\bDC_HOST\s+([^,()]*)[,)]", text)
    assert len(marked) == 38                           # the #define itself and the conventions comment do not match
    for decl in marked:
        assert re.fullmatch(r"(const )?(int|int32_t|int64_t|float) \*\w+", decl), decl


def test_a_host_array_parameter_still_rejects_a_plain_int():
    """``node_ptr_host`` is bound as ``POINTER(c_int64)``: an address-sized int, which a ``c_void_p`` would take,
    is refused by ctypes before the call."""
    L = _lib.lib()
    host = (ctypes.c_int64 * 2)(0, 3)
    with pytest.raises(ctypes.ArgumentError, match="argument 4"):
        L.dc_graph_build_segmented(None, 0, 3, 4096, host, 1, *([None] * 10))
    assert L.dc_graph_build_segmented(None, 0, 3, host, host, 1, *([None] * 10)) == -1    # (null pointers: DC_EINVAL)


def test_python_constants_are_the_header_defines():
    d = _lib.DEFINES
    assert (d["DC_OK"], d["DC_EINVAL"], d["DC_ELAUNCH"], d["DC_EWORKSPACE"]) == (0, -1, -2, -3)
    assert "DC_HOST" not in d
    assert ops.MAX_SEG == d["DC_MAX_SEG"]
    assert gat_heads.GAT_EDGE_MAX_DIM == ops.GAT_EDGE_MAX_DIM == d["DC_GAT_EDGE_MAX_DIM"]
    assert (gmm.GMM_MAX_K, gmm.GMM_MAX_D) == (d["DC_GMM_MAX_K"], d["DC_GMM_MAX_D"])
    assert (spline.SPLINE_MAX_D, spline.SPLINE_MAX_S, spline.SPLINE_MAX_K) \
        == (d["DC_SPLINE_MAX_D"], d["DC_SPLINE_MAX_S"], d["DC_SPLINE_MAX_K"])
    assert (neighbors.MAX_CAP, neighbors.ND_CHUNK) == (d["DC_NEIGHBORS_MAX_CAP"], d["DC_NEIGHBORS_ND_CHUNK"])
    assert (neighbors._KNN, neighbors._RADIUS) == (d["DC_NEIGHBORS_KNN"], d["DC_NEIGHBORS_RADIUS"])
    assert (graph.GROUP_ALIGN, graph.MAX_PARTS) == (d["DC_GROUP_ALIGN"], d["DC_MAX_PARTS"])
    assert (graph.SEG_MAX_NODES, graph.SEG_MAX_EDGES) == (d["DC_SEG_MAX_NODES"], d["DC_SEG_MAX_EDGES"])
    assert pointops.FPS_RESIDENT_POINTS == d["DC_FPS_RESIDENT_POINTS"] == _lib.lib().dc_fps_resident_points()
    assert attention.FLASH_D == d["DC_ATTN_FLASH_D"]
    assert d["DC_ADAM_STEP_WORDS"] >= 2                   # (dp.FlatAdam sizes its step buffer by it)
