"""CPU-side checks of the live-compaction boundary (no GPU calls): the header,
the binding list and the built library agree on srd_compact_live_device, its 10
arguments and srd_compact_stats; the header states what the new table's `used`
count is and how the call synchronises; and the Python layer carries the
documented session methods with their signatures and defaults.  (The change
puts no host-callable arithmetic into a header -- the layout is srd_append.h's,
which tests/sanitize/append_check.cpp checks -- so there is no stand-alone sanitizer
program of its own.)"""
import ctypes as C
import inspect
import os
import re
import subprocess

import srd_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "srd_compact_live_device"


def _header():
    return open(os.path.join(ROOT, "include", "srd_amd.h")).read()


def test_header_binding_and_library_agree():
    src = _header()
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % NAME, src)
    assert m, NAME
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]
    assert len(params) == 10, params
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    assert names == ["ctx", "d_table", "table_bytes", "d_file", "file_len", "d_out", "out_cap", "d_new_table",
                     "new_table_bytes", "stats"]
    # the source store and its table are only read
    assert params[1].startswith("const void") and params[3].startswith("const uint8_t")
    assert NAME in srd_amd.EXPORTS
    if not os.path.exists(srd_amd.LIB_PATH):
        srd_amd.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", srd_amd.LIB_PATH], text=True)
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = srd_amd.lib()
    at = L.srd_compact_live_device.argtypes
    assert len(at) == 10 and L.srd_compact_live_device.restype is C.c_int
    # the 64-bit values are declared as such (a default int would truncate a length or a capacity)
    assert [at[i] for i in (2, 4, 6, 8)] == [C.c_uint64] * 4
    assert at[9] == C.POINTER(srd_amd.CompactStats)


def test_stats_struct_matches_header():
    src = _header()
    m = re.search(r"typedef struct \{([^}]*)\}\s*srd_compact_stats;", src)
    assert m
    fields = re.findall(r"uint64_t\s+(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == ["n_entries", "new_len", "kept_bytes", "n_crc_bad", "first_bad"]
    S = srd_amd.CompactStats
    assert [n for n, _ in S._fields_] == fields and all(t is C.c_uint64 for _, t in S._fields_)
    assert C.sizeof(S) == 40


def test_header_states_used_count_and_synchronisation():
    src = _header()
    a = src.index("a live session compacted on the device")
    doc = " ".join(src[a: src.index("} srd_compact_stats;")].replace(" * ", " ").split())
    assert "its `used` count is n_entries, no slot is deleted" in doc
    assert "On the context stream; synchronises" in doc
    assert "srd_padded_size(new_len) > out_cap" in doc  # which capacity rule the kernels need
    assert "d_out and d_new_table may have been written by then" in doc  # the NULL-byte-only refusal
    assert "data_store.rs:706-749" in doc and "entry_iterator.rs:69-126" in doc and ":587-590" in doc
    # ... and the list of replaced reference interfaces at the top names the entry
    assert NAME in src[: src.index("#ifndef SRD_AMD_H")]


def test_python_interface_names():
    sig = inspect.signature(srd_amd.compact_live_device)
    assert list(sig.parameters) == ["d_table", "table_bytes", "d_file", "file_len", "d_out", "out_cap", "d_new_table",
                                    "new_table_bytes", "ctx"]
    assert sig.parameters["d_out"].default is None  # the planning call
    D = srd_amd.DeviceStore
    sig = inspect.signature(D.compact)
    assert list(sig.parameters) == ["self", "capacity", "allow_bad_crc"]
    assert sig.parameters["capacity"].default is None and sig.parameters["allow_bad_crc"].default is False
    assert list(inspect.signature(D.estimate_compaction_savings).parameters) == ["self"]
    assert list(inspect.signature(D.iter_entries).parameters) == ["self"]
    assert list(inspect.signature(D.reserve).parameters) == ["self", "capacity"]
    doc = " ".join(D.compact.__doc__.split())
    assert "Both buffers" in doc and "held in HBM during the call" in doc
    assert "tombstone on disk" in doc and "disappears from len()" in doc
