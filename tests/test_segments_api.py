"""CPU-side checks of the segment-append boundary (no GPU calls): the header,
the binding list and the built library agree on
srd_batch_append_segments_device, its parameters and their widths, and on
srd_segment's layout (a C translation unit of static assertions and the ctypes
structure); the header says that the call waits twice; and the Python layer
carries the documented names.  csrc/srd_segments.h (the table rule, the unit
cut, the unit descriptor, the streaming kernel's frame and the CRC combine that
the kernels and the host glue run) is checked by a stand-alone host program
under ASan + UBSan, tests/sanitize/segments_check.cpp, which
tests/test_sanitized_rules.py runs."""
import ctypes as C
import inspect
import os
import re
import subprocess

import srd_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "srd_batch_append_segments_device"
# the prototype as the interface fixes it: the source table (host arrays), the segments and the entries' first
# segments (device), then the append's own parameters from the key hashes on
PARAMS = ["ctx", "src_ptrs", "src_lens", "n_src", "d_segs", "n_segs", "d_seg_first", "d_key_hashes", "n", "flags",
          "tail", "d_file", "file_cap", "new_tail", "d_meta_off_out", "stream"]


def _header():
    return open(os.path.join(ROOT, "include", "srd_amd.h")).read()


def test_header_binding_and_library_agree():
    src = _header()
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % NAME, src)
    assert m, NAME
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    assert names == PARAMS
    # the widths the header declares
    width = dict(zip(names, params))
    for k in ("n_src", "n_segs", "n", "tail", "file_cap"):
        assert width[k].startswith("uint64_t "), width[k]
    assert width["flags"].startswith("uint32_t ")
    assert re.sub(r"\s+", " ", width["src_ptrs"]) == "const uint8_t *const *src_ptrs"
    assert re.sub(r"\s+", " ", width["d_segs"]) == "const srd_segment *d_segs"
    assert NAME in srd_amd.EXPORTS
    if not os.path.exists(srd_amd.LIB_PATH):
        srd_amd.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", srd_amd.LIB_PATH], text=True)
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = srd_amd.lib()
    at = L.srd_batch_append_segments_device.argtypes
    assert len(at) == len(PARAMS)
    assert L.srd_batch_append_segments_device.restype is not None
    # the 64-bit values are declared as such (a default int would truncate a tail or a count)
    idx = {k: i for i, k in enumerate(PARAMS)}
    assert [at[idx[k]] for k in ("n_src", "n_segs", "n", "tail", "file_cap")] == [C.c_uint64] * 5
    assert at[idx["flags"]] == C.c_uint32
    assert at[idx["src_lens"]] == C.POINTER(C.c_uint64) and at[idx["new_tail"]] == C.POINTER(C.c_uint64)
    assert at[idx["src_ptrs"]] == C.POINTER(C.c_void_p)
    # the header says what the stream rule costs here, and which interface this is
    doc = src[src.index("sequence of device segments"): m.start()]
    assert "waits twice" in doc and "write_stream_with_key_hash" in doc and "data_store.rs:758-825" in doc


def test_segment_layout(tmp_path):
    """sizeof(srd_segment) == 24 with the fields at 0 / 4 / 8 / 16: the header (a C
    translation unit of static assertions) and the ctypes structure."""
    tu = tmp_path / "seg_layout.c"
    tu.write_text(
        '#include <stddef.h>\n#include "srd_amd.h"\n'
        '_Static_assert(sizeof(srd_segment) == 24, "size");\n'
        '_Static_assert(offsetof(srd_segment, src) == 0, "src");\n'
        '_Static_assert(offsetof(srd_segment, reserved) == 4, "reserved");\n'
        '_Static_assert(offsetof(srd_segment, off) == 8, "off");\n'
        '_Static_assert(offsetof(srd_segment, len) == 16, "len");\n'
        '_Static_assert(sizeof(((srd_segment *)0)->src) == 4 && sizeof(((srd_segment *)0)->reserved) == 4, "u32");\n'
        '_Static_assert(sizeof(((srd_segment *)0)->off) == 8 && sizeof(((srd_segment *)0)->len) == 8, "u64");\n')
    subprocess.check_call(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(tu)])
    S = srd_amd.Segment
    assert C.sizeof(S) == 24
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == \
        [("src", 0, 4), ("reserved", 4, 4), ("off", 8, 8), ("len", 16, 8)]


def test_python_interface_names():
    assert callable(srd_amd.batch_append_segments_device)
    sig = inspect.signature(srd_amd.batch_append_segments_device)
    assert list(sig.parameters)[:11] == ["src_ptrs", "src_lens", "d_segs", "n_segs", "d_seg_first", "d_key_hashes", "n",
                                         "tail", "d_file", "file_cap", "d_meta_off_out"]
    D = srd_amd.DeviceStore
    assert list(inspect.signature(D.batch_write_stream_with_key_hashes).parameters) == ["self", "hashes", "entries"]
    assert list(inspect.signature(D.batch_write_stream).parameters) == ["self", "keys", "entries"]
    assert list(inspect.signature(D.write_stream_with_key_hash).parameters) == ["self", "key_hash", "segments"]
    assert list(inspect.signature(D.write_stream).parameters) == ["self", "key", "segments"]
    for name in ("batch_write_stream_with_key_hashes", "batch_write_stream", "write_stream_with_key_hash", "write_stream"):
        assert "data_store.rs" in getattr(D, name).__doc__, name  # named after the reference method it replaces
