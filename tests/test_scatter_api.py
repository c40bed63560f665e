"""CPU-side checks of the scatter-read boundary (no GPU calls): the header, the
binding list and the built library agree on srd_payload_scatter_device, its 16
parameters and their widths; SRD_SCATTER_BAD_LENGTH is 4 in the header and the
module; the header names the reference's EntryStream and says that the call
waits once; and the Python layer carries the documented names.
csrc/srd_scatter.h with the scatter view of csrc/srd_segments.h (the entry
walk, the unit cut at the destination's residue, the unit descriptor, the
streaming kernel's frame and the CRC combine that the kernels and the host
glue run) is checked by a stand-alone host program under ASan + UBSan,
tests/sanitize/scatter_check.cpp, which tests/test_sanitized_rules.py runs."""
import ctypes as C
import inspect
import os
import re
import subprocess

import srd_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "srd_payload_scatter_device"
# the prototype as the interface fixes it: the gather's ranges, the destination table (host arrays), the segments
# and the queries' first segments (device), the flags, the two output arrays, the stream
PARAMS = ["ctx", "d_file", "file_len", "d_start", "d_end", "n", "dst_ptrs", "dst_lens", "n_dst", "d_segs", "n_segs",
          "d_seg_first", "flags", "d_status", "d_crc_computed", "stream"]


def _header():
    return open(os.path.join(ROOT, "include", "srd_amd.h")).read()


def test_header_binding_and_library_agree():
    src = _header()
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % NAME, src)
    assert m, NAME
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    assert names == PARAMS and len(names) == 16
    # the widths the header declares
    width = dict(zip(names, params))
    for k in ("file_len", "n", "n_dst", "n_segs"):
        assert width[k].startswith("uint64_t "), width[k]
    assert width["flags"].startswith("uint32_t ")
    assert re.sub(r"\s+", " ", width["dst_ptrs"]) == "uint8_t *const *dst_ptrs"
    assert re.sub(r"\s+", " ", width["dst_lens"]) == "const uint64_t *dst_lens"
    assert re.sub(r"\s+", " ", width["d_segs"]) == "const srd_segment *d_segs"
    assert re.sub(r"\s+", " ", width["d_status"]) == "uint8_t *d_status"
    assert re.sub(r"\s+", " ", width["d_crc_computed"]) == "uint32_t *d_crc_computed"
    assert NAME in srd_amd.EXPORTS
    if not os.path.exists(srd_amd.LIB_PATH):
        srd_amd.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", srd_amd.LIB_PATH], text=True)
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = srd_amd.lib()
    at = L.srd_payload_scatter_device.argtypes
    assert len(at) == len(PARAMS) == 16
    assert L.srd_payload_scatter_device.restype is C.c_int
    # the 64-bit values are declared as such (a default int would truncate a length or a count)
    idx = {k: i for i, k in enumerate(PARAMS)}
    assert [at[idx[k]] for k in ("file_len", "n", "n_dst", "n_segs")] == [C.c_uint64] * 4
    assert at[idx["flags"]] == C.c_uint32
    assert at[idx["dst_ptrs"]] == C.POINTER(C.c_void_p) and at[idx["dst_lens"]] == C.POINTER(C.c_uint64)
    for k in ("ctx", "d_file", "d_start", "d_end", "d_segs", "d_seg_first", "d_status", "d_crc_computed", "stream"):
        assert at[idx[k]] == C.c_void_p, k


def test_bad_length_status_value():
    m = re.search(r"#define\s+SRD_SCATTER_BAD_LENGTH\s+(\d+)u", _header())
    assert m and int(m.group(1)) == 4
    assert srd_amd.SCATTER_BAD_LENGTH == 4
    # the gather's statuses keep their values below it
    assert (srd_amd.GATHER_NONE, srd_amd.GATHER_OK, srd_amd.GATHER_BAD_CRC, srd_amd.GATHER_BAD_RANGE) == (0, 1, 2, 3)


def test_header_says_what_the_call_is():
    src = _header()
    m = re.search(r"\bint %s\s*\(" % NAME, src)
    doc = src[src.index("read into a sequence of device segments"): m.start()]
    assert "entry_stream.rs:44-92" in doc and "entry_handle.rs:260-275" in doc
    assert "waits once" in doc and "waits twice" not in doc
    assert "SRD_SCATTER_BAD_LENGTH" in doc and "srd_padded_size(file_len)" in doc
    # the typedef says which table src indexes here
    td = src[src.index("typedef struct {\n  uint32_t src;"): src.index("} srd_segment;")]
    assert "DESTINATION table" in td


def test_python_interface_names():
    sig = inspect.signature(srd_amd.payload_scatter_device)
    assert list(sig.parameters)[:13] == ["d_file", "file_len", "d_start", "d_end", "n", "dst_ptrs", "dst_lens", "d_segs",
                                         "n_segs", "d_seg_first", "flags", "d_status", "d_crc_computed"]
    assert list(inspect.signature(srd_amd.scatter_ranges).parameters) == ["d_file", "file_len", "st", "en", "entries", "ctx"]
    D = srd_amd.DeviceStore
    assert list(inspect.signature(D.batch_read_into_hashed_keys).parameters) == ["self", "hashes", "entries",
                                                                                 "non_hashed_keys"]
    assert inspect.signature(D.batch_read_into_hashed_keys).parameters["non_hashed_keys"].default is None
    assert list(inspect.signature(D.batch_read_into).parameters) == ["self", "keys", "entries"]
    assert list(inspect.signature(D.read_into).parameters) == ["self", "key", "segments"]
    for name in ("batch_read_into_hashed_keys", "batch_read_into", "read_into"):
        assert "entry_stream.rs:76-91" in getattr(D, name).__doc__, name  # named after the reference code it replaces
    assert "entry_stream.rs:76-91" in srd_amd.DeviceIndex.batch_scatter.__doc__
    assert list(inspect.signature(srd_amd.DeviceIndex.batch_scatter).parameters) == ["self", "d_file", "file_len", "hashes",
                                                                                     "entries", "non_hashed_keys"]


def test_scatter_result_rule():
    import numpy as np
    import pytest
    S = srd_amd
    st = np.array([S.GATHER_OK, S.GATHER_BAD_CRC, S.GATHER_NONE, S.GATHER_BAD_RANGE], np.uint8)
    r = S.ScatterResult(st, np.zeros(4, np.uint32))
    assert len(r) == 4
    # GatherResult's rule on the same statuses
    assert r.is_valid_checksum() == [True, False, None, None] == S.GatherResult(None, None, None, st, None).is_valid_checksum()
    with pytest.raises(ValueError):
        S.ScatterResult(np.array([S.GATHER_OK, S.SCATTER_BAD_LENGTH], np.uint8), np.zeros(2, np.uint32)).is_valid_checksum()
