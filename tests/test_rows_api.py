"""CPU-side checks of the rows read's boundary (no GPU calls): the header, the
binding list, the built library and the ctypes argument lists agree on the two
new entries and their 64-bit parameters; SRD_ROWS_TOO_LONG is 5 in the header
and the module and the gather's 0 / 1 / 2 are unchanged; the header says that
the call does not wait and what the reserve call is for; and the Python layer
carries the documented names.  csrc/srd_rows.h over csrc/srd_ttl.h /
srd_table.h / srd_segments.h (the code the kernels and the host glue run) is
checked by a stand-alone host program under ASan + UBSan,
tests/sanitize/rows_check.cpp, which tests/test_sanitized_rules.py runs."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

import srd_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the prototypes as the interface fixes them
PARAMS = {
    "srd_ctx_reserve_rows": ["ctx", "n", "row_cap"],
    "srd_read_rows_device": ["ctx", "d_table", "table_bytes", "d_file", "file_len", "d_hashes", "d_verify_hashes", "n",
                             "d_out", "row_stride", "row_cap", "d_len", "d_status", "d_crc_computed", "d_counts", "flags",
                             "stream"],
}
# the parameters the header declares as 64-bit values (a default int would truncate a length, a stride or a count)
U64 = {"n", "table_bytes", "file_len", "row_stride", "row_cap"}
WIDTH = {"d_hashes": "const uint64_t *", "d_verify_hashes": "const uint64_t *", "d_out": "uint8_t *", "d_len": "uint64_t *",
         "d_status": "uint8_t *", "d_crc_computed": "uint32_t *", "d_counts": "uint64_t *", "d_file": "const uint8_t *"}


def _header():
    return open(os.path.join(ROOT, "include", "srd_amd.h")).read()


def _proto(src, name):
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, src)
    assert m, name
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]
    return [re.sub(r"\s+", " ", p) for p in params]


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_header_binding_and_library_agree(name):
    params = _proto(_header(), name)
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    assert names == PARAMS[name]
    assert name in srd_amd.EXPORTS
    if not os.path.exists(srd_amd.LIB_PATH):
        srd_amd.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", srd_amd.LIB_PATH], text=True)
    assert name in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    fn = getattr(srd_amd.lib(), name)
    at = fn.argtypes
    assert len(at) == len(names)
    assert fn.restype is C.c_int
    for p, k, t in zip(params, names, at):
        if k in U64:
            assert p == "uint64_t " + k and t == C.c_uint64, (p, t)
        elif k == "flags":
            assert p == "uint32_t flags" and t == C.c_uint32
        else:
            assert "*" in p and t == C.c_void_p, (p, t)
            if k in WIDTH:
                assert p == WIDTH[k] + k, p


def test_status_values():
    src = _header()
    m = re.search(r"#define\s+SRD_ROWS_TOO_LONG\s+(\d+)u", src)
    assert m and int(m.group(1)) == srd_amd.ROWS_TOO_LONG == 5
    for i, k in enumerate(("NONE", "OK", "BAD_CRC", "BAD_RANGE")):  # the gather's meaning is kept
        m = re.search(r"#define\s+SRD_GATHER_%s\s+(\d+)u" % k, src)
        assert m and int(m.group(1)) == i == getattr(srd_amd, "GATHER_" + k)
    assert srd_amd.SCATTER_BAD_LENGTH == 4  # (4 stays the scatter's)
    # the rule file carries the same values
    rule = open(os.path.join(ROOT, "rust-simd-r-drive_amd", "csrc", "srd_rows.h")).read()
    assert "ROWS_TOO_LONG = SRD_ROWS_TOO_LONG" in rule and "ROWS_STATUSES = 6" in rule


def test_header_says_what_the_calls_are():
    src = _header()
    doc = src[src.index("---- keyed reads into fixed-size rows"): src.index("int srd_read_rows_device")]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)  # (the comment's line breaks are not part of what it says)
    assert "data_store.rs:1111-1158" in doc and "entry_handle.rs:260-275" in doc
    # the words the other entries use: reads / writes / waits for
    assert "DOES NOT WAIT" in doc and "reads nothing back" in doc and "waits for" in doc
    assert "allocates and frees nothing" in doc and "no synchronous copy" in doc
    assert "returns with everything enqueued" in doc
    assert "No byte outside" in doc and "no zero fill" in doc
    assert "true length" in doc and "nothing enqueued" in doc
    # what the reserve is for, and the capture rule
    res = doc[doc.index("srd_ctx_reserve_rows: the workspace"):]
    assert "do not wait and can be captured" in res and "may synchronise" in res and "srd_ctx_device_bytes" in res
    assert "capturing" in doc and "names srd_ctx_reserve_rows" in doc
    for k in ("16-byte aligned", "multiple of 16", "row_cap == 0", "n >= 2^31", ">= 2^32", "srd_padded_size(file_len)",
              "flags != 0", "n == 0 runs nothing"):
        assert k in doc, k


def test_python_interface_names():
    S = srd_amd
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(S.DeviceIndex.read_rows)[:9] == ["self", "d_file", "file_len", "hashes", "out", "non_hashed_keys", "lens",
                                                "status", "crc"]
    D = S.DeviceStore
    assert sig(D.batch_read_rows_hashed_keys) == ["self", "hashes", "out", "non_hashed_keys", "outs"]
    assert sig(D.batch_read_rows) == ["self", "keys", "out"]
    assert sig(D.reserve_rows) == ["self", "n", "row_cap"]
    assert sig(D.sync) == ["self"] and sig(D.rows_token) == ["self"]
    assert sig(S.Context.reserve_rows) == ["self", "n", "row_cap"]
    for name in ("is_valid_checksum", "payloads", "too_long", "__len__"):
        assert callable(getattr(S.RowsResult, name)), name
    doc = D.batch_read_rows_hashed_keys.__doc__
    assert "capacity" in doc.lower() and "rows_token" in doc and "sync()" in doc
    assert "capturing" in S.DeviceIndex.read_rows.__doc__ and "CURRENT stream" in S.DeviceIndex.read_rows.__doc__


def test_rows_result_waits_lazily_and_once():
    """RowsResult over host stand-ins: nothing is read when it is made, the
    accessors copy status and lens once."""
    import numpy as np
    S = srd_amd
    calls = []

    class T:
        is_cuda = False

        def __init__(self, a, name):
            self.a, self.name, self.shape = a, name, a.shape

        def cpu(self):
            calls.append(self.name)
            return self

        def numpy(self):
            return self.a

    out = np.full((4, 8), 0xA5, np.uint8)
    out[1, :3] = (1, 2, 3)
    out[2, :8] = 7
    r = S.RowsResult(T(out, "out"), T(np.array([0, 3, 8, 99], np.int64), "lens"),
                     T(np.array([S.GATHER_NONE, S.GATHER_OK, S.GATHER_BAD_CRC, S.ROWS_TOO_LONG], np.uint8), "status"),
                     T(np.zeros(4, np.int32), "crc"))
    assert calls == [] and len(r) == 4 and calls == []
    assert r.is_valid_checksum() == [None, True, False, None]
    assert r.too_long() == [(3, 99)]
    assert r.payloads() == [None, bytes((1, 2, 3)), bytes([7] * 8), None]
    assert sorted(calls) == ["lens", "out", "status"]
