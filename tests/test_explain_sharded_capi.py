"""The collective explain calls at the C boundary (CPU-only: nothing is computed):
both libraries export them, the header declares them with the signature the
binding gives them, and Engine has the methods. A caller detects the feature by
the symbol ms_explain_sharded_device (minisched_gpu.h)."""
import ctypes
import os
import re
import subprocess

from minisched_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "minisched_gpu.h")
NAMES = ("ms_explain_sharded_device", "ms_explain_sharded")


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r" T (ms_\w+)", out))


def test_both_libraries_export_the_symbols():
    assert os.path.exists(_lib.LOOPBACK_LIB_PATH), "make -C mini-kube-scheduler_amd comm-loopback"
    for path in (_lib.LIB_PATH, _lib.LOOPBACK_LIB_PATH):
        assert set(NAMES) <= exported(path), path
        lib = _lib.load(path)
        for name in NAMES:
            assert hasattr(lib, name), (path, name)


def declaration(name):
    """The parameter types of `name` as the header declares them, comments stripped."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert m, f"{name} is not declared"
    return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]


def test_header_and_binding_signatures_agree():
    row, summary = "ms_explain_row *", "ms_explain_summary *"
    assert declaration("ms_explain_sharded_device") == [
        "ms_ctx *ctx", "uint32_t n_pods", "const ms_pod_rec *pods_dev", "uint32_t first", "uint32_t n_nodes",
        row + "rows_dev", summary + "summaries_dev", "void *stream"]
    assert declaration("ms_explain_sharded") == [
        "ms_ctx *ctx", "uint32_t n_pods", "const ms_pod_rec *pods", "uint32_t first", "uint32_t n_nodes",
        row + "rows", summary + "summaries"]
    # pointers as void *, the counts and ordinals as uint32_t: the single-context calls' binding, unchanged
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    assert _lib.SIGNATURES["ms_explain_sharded_device"] == (ctypes.c_int, [vp, u32, vp, u32, u32, vp, vp, vp])
    assert _lib.SIGNATURES["ms_explain_sharded"] == (ctypes.c_int, [vp, u32, vp, u32, u32, vp, vp])
    assert _lib.SIGNATURES["ms_explain_sharded_device"] == _lib.SIGNATURES["ms_explain_device"]
    assert _lib.SIGNATURES["ms_explain_sharded"] == _lib.SIGNATURES["ms_explain"]
    lib = _lib.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == _lib.SIGNATURES[name]


def test_engine_has_the_methods_and_the_abi_is_unchanged():
    assert callable(getattr(_lib.Engine, "explain_sharded", None))
    assert callable(getattr(_lib.Engine, "explain_sharded_device", None))
    assert _lib.load().ms_abi_version() == 7  # additive: detected by the symbol
    src = open(HEADER).read()
    assert re.search(r"#define\s+MS_ABI_VERSION\s+7\b", src)
